// k4_coder_harness.hip -- TEST INFRASTRUCTURE: the entropy kernel's coder (cavif_rs_amd/csrc/tile_entropy.h, unchanged) on record streams given by the test.
// One workgroup per stream, 64 * (NA + 1) threads: waves 0 .. NA - 1 are the adapters (k4_adapt_sb<NA>), wave NA is the coder (k4_code_sb, re_finish_dev).
// The stage loop of tile_entropy_kernel with the producer replaced by a copy: at step t buffer t is copied in from the stream (the adapters rewrite records in
// place), the adapters turn buffer t - 1 into bounds, the coder codes buffer t - 2, one workgroup barrier per step; three rotating buffers.
// Built twice by tests/helpers/k4_harness.py: hipcc for gfx950 with the product's flags, g++ with the SIMT emulator (tests/emu/).
#include <hip/hip_runtime.h>
#include "../../cavif_rs_amd/csrc/tile_entropy.h"

// per stream: sinfo[8 * s + ...] = first buffer in `bufs`, buffer count, pre-carry capacity, output capacity; bufs[2 * b] = first record, bufs[2 * b + 1] = count
template <int NA>
__global__ __launch_bounds__(64 * (NA + 1)) void k4h_kernel(const uint32_t *recs, const uint32_t *bufs, const uint32_t *sinfo, const uint16_t *cdf_in, int ncdf,
                                                          uint32_t *work, uint32_t rec_cap, uint16_t *pre, uint32_t pre_stride, uint8_t *out, uint32_t out_stride,
                                                          uint32_t *res, uint16_t *cdf_out) {
  constexpr int NT = 64 * (NA + 1);
  extern __shared__ __align__(16) uint8_t k4_smem[];
  const int s = blockIdx.x;
  const uint32_t buf0 = sinfo[8 * s], nbuf = sinfo[8 * s + 1], pre_cap = sinfo[8 * s + 2], out_cap = sinfo[8 * s + 3];
  LDS uint32_t *acc = (LDS uint32_t *)k4_smem;
  LDS uint16_t *cdf = (LDS uint16_t *)(k4_smem + MI_K4_ACC * sizeof(uint32_t));
  const int wave = uni32((int)(threadIdx.x >> 6));
  for (int i = threadIdx.x; i < ncdf; i += NT) cdf[i] = cdf_in[(size_t)s * ncdf + i];
  for (int i = threadIdx.x; i < MI_K4_ACC; i += NT) acc[i] = 0;
  uint32_t *const ring = work + (size_t)s * 3 * rec_cap;
  RangeEncDev ec;
  if (wave == NA) re_init_dev(&ec, pre + (size_t)s * pre_stride, pre_cap, acc);
  __syncthreads();
  for (uint32_t t = 0; t < nbuf + 2; t++) {
    if (t < nbuf) {                                          // "producer": buffer t from the stream, every thread a share
      const uint32_t *src = recs + bufs[2 * (buf0 + t)];
      const uint32_t n = bufs[2 * (buf0 + t) + 1];
      uint32_t *dst = ring + (size_t)(t % 3) * rec_cap;
      for (uint32_t i = threadIdx.x; i < n; i += NT) dst[i] = src[i];
    }
    if (wave < NA) {
      if (t >= 1 && t - 1 < nbuf) k4_adapt_sb<NA>(cdf, ring + (size_t)((t - 1) % 3) * rec_cap, (int)bufs[2 * (buf0 + t - 1) + 1], wave);
    } else {
      if (t >= 2) k4_code_sb(&ec, ring + (size_t)((t - 2) % 3) * rec_cap, (int)bufs[2 * (buf0 + t - 2) + 1]);
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < ncdf; i += NT) cdf_out[(size_t)s * ncdf + i] = cdf[i];
  if (wave == NA) {
    const uint32_t len = re_finish_dev(&ec, out + (size_t)s * out_stride, out_cap);
    if (LANE == 0) { res[2 * s] = len; res[2 * s + 1] = ec.flushed; }
  }
}

// Host side.  Every capacity is checked against its buffer's stride and every record against the table before anything reaches the device: the
// guard zones (stride - capacity) are the caller's, filled with a sentinel and copied in and out with the buffers.  Returns 0, or a negative error.
template <int NA>
static int k4h_run(int nstreams, const uint32_t *recs, uint32_t nrecs, const uint32_t *bufs, uint32_t nbufs, const uint32_t *sinfo, const uint16_t *cdf_in,
                   int ncdf, uint16_t *pre, uint32_t pre_stride, uint8_t *out, uint32_t out_stride, uint32_t *res, uint16_t *cdf_out) {
  if (nstreams <= 0 || ncdf <= 16 || ncdf > 16384) return -1;
  uint32_t rec_cap = 1;
  for (uint32_t b = 0; b < nbufs; b++) {
    if ((uint64_t)bufs[2 * b] + bufs[2 * b + 1] > nrecs) return -2;
    if (bufs[2 * b + 1] > rec_cap) rec_cap = bufs[2 * b + 1];
  }
  for (int s = 0; s < nstreams; s++) {
    const uint32_t *si = sinfo + 8 * s;
    if ((uint64_t)si[0] + si[1] > nbufs || si[2] > pre_stride || si[3] > out_stride) return -3;
  }
  for (uint32_t i = 0; i < nrecs; i++) {
    const uint32_t r = recs[i], off = r & 0xFFFFu;
    if ((r >> 30) == 0u && (r & 0x20000000u) && off + 10 >= (uint32_t)ncdf) return -4;
    if ((r >> 30) == 0u && !(r & 0x20000000u) && (off + ((r >> 20) & 15u) + 1 >= (uint32_t)ncdf || ((r >> 16) & 15u) > ((r >> 20) & 15u))) return -4;
    if ((r >> 30) > 1u) return -4;
  }
  uint32_t *d_recs = nullptr, *d_bufs = nullptr, *d_sinfo = nullptr, *d_work = nullptr, *d_res = nullptr; uint16_t *d_cdf = nullptr, *d_cdf_out = nullptr, *d_pre = nullptr;
  uint8_t *d_out = nullptr;
  const size_t ncdf_all = (size_t)nstreams * ncdf;
  int rc = 0;
#define K4H_OK(x) do { if ((x) != hipSuccess) { rc = -10; goto done; } } while (0)
  K4H_OK(hipMalloc(&d_recs, (size_t)(nrecs ? nrecs : 1) * 4)); K4H_OK(hipMalloc(&d_bufs, (size_t)(nbufs ? nbufs : 1) * 8)); K4H_OK(hipMalloc(&d_sinfo, (size_t)nstreams * 32));
  K4H_OK(hipMalloc(&d_work, (size_t)nstreams * 3 * rec_cap * 4)); K4H_OK(hipMalloc(&d_res, (size_t)nstreams * 8));
  K4H_OK(hipMalloc(&d_cdf, ncdf_all * 2)); K4H_OK(hipMalloc(&d_cdf_out, ncdf_all * 2));
  K4H_OK(hipMalloc(&d_pre, (size_t)nstreams * pre_stride * 2)); K4H_OK(hipMalloc(&d_out, (size_t)nstreams * out_stride));
  if (nrecs) K4H_OK(hipMemcpy(d_recs, recs, (size_t)nrecs * 4, hipMemcpyHostToDevice));
  if (nbufs) K4H_OK(hipMemcpy(d_bufs, bufs, (size_t)nbufs * 8, hipMemcpyHostToDevice));
  K4H_OK(hipMemcpy(d_sinfo, sinfo, (size_t)nstreams * 32, hipMemcpyHostToDevice));
  K4H_OK(hipMemcpy(d_cdf, cdf_in, ncdf_all * 2, hipMemcpyHostToDevice));
  K4H_OK(hipMemcpy(d_pre, pre, (size_t)nstreams * pre_stride * 2, hipMemcpyHostToDevice));
  K4H_OK(hipMemcpy(d_out, out, (size_t)nstreams * out_stride, hipMemcpyHostToDevice));
  K4H_OK(hipMemset(d_res, 0xEE, (size_t)nstreams * 8));
  K4H_OK(hipMemset(d_work, 0, (size_t)nstreams * 3 * rec_cap * 4));
  hipLaunchKernelGGL((k4h_kernel<NA>), dim3(nstreams), dim3(64 * (NA + 1)), MI_K4_ACC * 4 + ((ncdf * 2 + 15) & ~15), 0,
                     d_recs, d_bufs, d_sinfo, d_cdf, ncdf, d_work, rec_cap, d_pre, pre_stride, d_out, out_stride, d_res, d_cdf_out);
  K4H_OK(hipGetLastError());
  K4H_OK(hipDeviceSynchronize());
  K4H_OK(hipMemcpy(pre, d_pre, (size_t)nstreams * pre_stride * 2, hipMemcpyDeviceToHost));
  K4H_OK(hipMemcpy(out, d_out, (size_t)nstreams * out_stride, hipMemcpyDeviceToHost));
  K4H_OK(hipMemcpy(res, d_res, (size_t)nstreams * 8, hipMemcpyDeviceToHost));
  K4H_OK(hipMemcpy(cdf_out, d_cdf_out, ncdf_all * 2, hipMemcpyDeviceToHost));
#undef K4H_OK
done:
  (void)hipFree(d_recs); (void)hipFree(d_bufs); (void)hipFree(d_sinfo); (void)hipFree(d_work); (void)hipFree(d_res); (void)hipFree(d_cdf); (void)hipFree(d_cdf_out);
  (void)hipFree(d_pre); (void)hipFree(d_out);
  return rc;
}

extern "C" int k4h_run_na2(int nstreams, const uint32_t *recs, uint32_t nrecs, const uint32_t *bufs, uint32_t nbufs, const uint32_t *sinfo, const uint16_t *cdf_in,
                           int ncdf, uint16_t *pre, uint32_t pre_stride, uint8_t *out, uint32_t out_stride, uint32_t *res, uint16_t *cdf_out) {
  return k4h_run<2>(nstreams, recs, nrecs, bufs, nbufs, sinfo, cdf_in, ncdf, pre, pre_stride, out, out_stride, res, cdf_out);
}
extern "C" int k4h_run_na4(int nstreams, const uint32_t *recs, uint32_t nrecs, const uint32_t *bufs, uint32_t nbufs, const uint32_t *sinfo, const uint16_t *cdf_in,
                           int ncdf, uint16_t *pre, uint32_t pre_stride, uint8_t *out, uint32_t out_stride, uint32_t *res, uint16_t *cdf_out) {
  return k4h_run<4>(nstreams, recs, nrecs, bufs, nbufs, sinfo, cdf_in, ncdf, pre, pre_stride, out, out_stride, res, cdf_out);
}
