// tools/probe/input_kernels.hip -- every kernel with one thread per four pixels of a slot row (dev_slot.h), explicitly instantiated and nothing else: a few
// seconds to compile, so that their registers and instruction counts can be compared between two trees without building the library.
//   F="--offload-arch=gfx950 -O2 ... -Wno-unused-variable"          (HIPCC_FLAGS of __graft_entry__.py without -shared -fPIC)
//   hipcc $F -I cavif_rs_amd/csrc --cuda-device-only -c -Rpass-analysis=kernel-resource-usage tools/probe/input_kernels.hip -o /dev/null
//   hipcc $F -I cavif_rs_amd/csrc --cuda-device-only -S tools/probe/input_kernels.hip -o input_kernels.s && tools/isa_stats.py input_kernels.s
// profiles/input_kernels.md has the figures.
#include <hip/hip_runtime.h>
#include "dev_ingest.h"
#include "dev_deep.h"
#include "dev_jpeg.h"
#include "dev_png.h"
#include "dev_planes.h"
#include "dev_resample.h"
#include "dev_colour.h"
#include "dev_decoded.h"

namespace mi {

#define MI_PROBE_BOTH(kernel, ...) template __global__ void kernel<3>(__VA_ARGS__); template __global__ void kernel<4>(__VA_ARGS__)
MI_PROBE_BOTH(ingest_kernel, const IngestSrc, uint8_t *);
MI_PROBE_BOTH(ingest16_kernel, const Ingest16Src, uint16_t *);
MI_PROBE_BOTH(png_expand_kernel, const uint8_t *, const PngImageDev *, const uint32_t, const uint32_t, uint8_t *);
MI_PROBE_BOTH(png_expand16_kernel, const uint8_t *, const PngImageDev *, const uint32_t, const uint32_t, uint16_t *);
MI_PROBE_BOTH(planes_ingest_kernel, const PlanesSrc, uint8_t *);
MI_PROBE_BOTH(colour_convert_kernel, const ColourDev, uint8_t *, const uint32_t, const uint32_t);
MI_PROBE_BOTH(colour_convert16_kernel, const ColourDev, uint16_t *, const uint32_t, const uint32_t);
MI_PROBE_BOTH(jpeg_colour_kernel, const uint8_t *, const JpegDevGeom, uint8_t *, const size_t);
MI_PROBE_BOTH(jpeg_ycc_kernel, const uint8_t *, const JpegDevGeom, uint8_t *, const size_t);
MI_PROBE_BOTH(resample_v_kernel, const uint32_t *, const uint32_t, const uint32_t, const uint32_t *, const int32_t *, const uint32_t, const uint32_t, const int, uint8_t *);
template __global__ void decoded_kernel<8, 0>(const FrameDev *, const DecodedDst);
template __global__ void decoded_kernel<8, 1>(const FrameDev *, const DecodedDst);
template __global__ void decoded_kernel<10, 0>(const FrameDev *, const DecodedDst);
template __global__ void decoded_kernel<10, 1>(const FrameDev *, const DecodedDst);

}  // namespace mi
