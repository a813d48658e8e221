"""Build and call tests/kernels/k4_coder_harness.hip (the entropy kernel's coder on given record streams) -- test infrastructure only.

Two builds (tests/helpers/kernel_build.py): hipcc with the product's flags (the GPU library) and g++ with the SIMT emulator's shim.  `run` pads every output buffer with a guard zone of sentinels behind the capacity it
passes, and reports whether the zones came back untouched."""
import ctypes as C
import os

from tests.helpers import kernel_build

ROOT = kernel_build.ROOT
KDIR = kernel_build.KDIR
SRC = kernel_build.source('k4_coder_harness.hip')
OUT = kernel_build.OUT
GPU_LIB = kernel_build.target('k4_harness', emu=False)
EMU_LIB = kernel_build.target('k4_harness', emu=True)
GUARD = 64                       # entries of sentinel behind every capacity
SENT8, SENT16 = 0xA7, 0xBEEF


def build(emu, force=False):
    return kernel_build.build(SRC, EMU_LIB if emu else GPU_LIB, emu, force=force)


def build_all(force=False):
    build(emu=False, force=force)
    build(emu=True, force=force)


class Result:
    def __init__(self, data, length, units, nunits, cdf, guards_ok):
        self.data, self.length, self.units, self.nunits, self.cdf, self.guards_ok = data, length, units, nunits, cdf, guards_ok


def run(lib_path, na, streams, pre_caps=None, out_caps=None):
    """Codes every stream (tests.helpers.range_coder_ref.Stream) in its own workgroup of one launch.  Capacities default to what the reference needs
    (+ a margin); the guard zones sit behind them."""
    lib = C.CDLL(lib_path)
    fn = getattr(lib, 'k4h_run_na%d' % na)
    fn.restype = C.c_int
    n = len(streams)
    ncdf = len(streams[0].cdf)
    pre_caps = pre_caps or [len(s.ref.data) + 4 for s in streams]
    out_caps = out_caps or [len(s.ref.data) + 4 for s in streams]
    pre_stride, out_stride = max(pre_caps) + GUARD, max(out_caps) + GUARD
    recs, bufs, sinfo = [], [], []
    for s in streams:
        assert len(s.cdf) == ncdf
        sinfo += [len(bufs) // 2, len(s.splits), 0, 0, 0, 0, 0, 0]
        at = 0
        for sz in s.splits:
            bufs += [len(recs) + at, sz]
            at += sz
        recs += s.records
    for k in range(n):
        sinfo[8 * k + 2], sinfo[8 * k + 3] = pre_caps[k], out_caps[k]
    cdf_in = [v for s in streams for v in s.cdf]
    a_recs = (C.c_uint32 * max(1, len(recs)))(*recs)
    a_bufs = (C.c_uint32 * max(1, len(bufs)))(*bufs)
    a_sinfo = (C.c_uint32 * len(sinfo))(*sinfo)
    a_cdf = (C.c_uint16 * len(cdf_in))(*cdf_in)
    a_pre = (C.c_uint16 * (n * pre_stride))(*([SENT16] * (n * pre_stride)))
    a_out = (C.c_uint8 * (n * out_stride))(*([SENT8] * (n * out_stride)))
    a_res = (C.c_uint32 * (2 * n))()
    a_cdf_out = (C.c_uint16 * len(cdf_in))()
    rc = fn(n, a_recs, len(recs), a_bufs, len(bufs) // 2, a_sinfo, a_cdf, ncdf, a_pre, pre_stride, a_out, out_stride, a_res, a_cdf_out)
    assert rc == 0, 'k4h_run_na%d returned %d' % (na, rc)
    res = []
    for k in range(n):
        length, nunits = a_res[2 * k], a_res[2 * k + 1]
        pre = list(a_pre[k * pre_stride:(k + 1) * pre_stride])
        out = bytes(a_out[k * out_stride:(k + 1) * out_stride])
        # the guard zone: everything past the capacity, and past what the stream may write below it (units and bytes the stream does not have)
        guards_ok = all(v == SENT16 for v in pre[pre_caps[k]:]) and all(b == SENT8 for b in out[out_caps[k]:])
        res.append(Result(out[:length] if length != 0xFFFFFFFF else None, length, pre[:min(nunits, pre_caps[k])], nunits,
                          list(a_cdf_out[k * ncdf:(k + 1) * ncdf]), guards_ok))
    return res


def main(argv):
    """python -m tests.helpers.k4_harness LIB NA NAME...: the named streams of range_coder_ref.all_streams() through LIB, one JSON line per stream (a
    separate process, so that the emulator reads the environment it is started with, MI_EMU_REVERSE among it)."""
    import json
    from tests.helpers import range_coder_ref as R
    lib, na, names = argv[0], int(argv[1]), set(argv[2:])
    streams = [s for s in R.all_streams() if s.name in names]
    for s, r in zip(streams, run(lib, na, streams)):
        print(json.dumps({'name': s.name, 'length': r.length, 'data': r.data.hex() if r.data is not None else None, 'units': r.units, 'nunits': r.nunits,
                          'cdf': r.cdf, 'guards_ok': r.guards_ok}))


if __name__ == '__main__':
    import sys
    sys.path.insert(0, ROOT)
    main(sys.argv[1:])
