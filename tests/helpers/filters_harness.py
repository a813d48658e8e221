"""Build and call tests/kernels/filters_harness.hip (the deblock, CDEF and restoration kernels on given frames, and their __device__ functions on given
rows) -- test infrastructure only.  Built like the K4 harness (tests/helpers/kernel_build.py).

A `Frame` holds what the harness wants of one frame, in numpy arrays with the geometry of the product's plan_geometry / fill_dev.  Buffers the kernels write
start out as sentinels, so `untouched` can tell what a stage had no business writing; the harness itself keeps guard zones around every device buffer and
reports them in `guard_damage`."""
import ctypes as C
import os

import numpy as np

from tests.helpers import kernel_build

ROOT = kernel_build.ROOT
SRC = kernel_build.source('filters_harness.hip')
GPU_LIB = kernel_build.target('filters_harness', emu=False)
EMU_LIB = kernel_build.target('filters_harness', emu=True)
TALLY, PICK, DBK0, DBK1, CDEF, LR_SEARCH, LR = 1, 2, 4, 8, 16, 32, 64
DEBLOCK = TALLY | PICK | DBK0 | DBK1
SENT16, SENT8, SENT32 = 0xA7A7, 0x5A, 0x5A5A5A5A
FT_EDGE, FT_CONSTRAIN, FT_CDEF_TAPS, FT_SGR_SOLVE, FT_RATIO, FT_SUBEXP, FT_PROJECT = range(7)
FT_IN, FT_OUT = 24, 18
CDEF_LIST = [0, 1 * 4 + 0, 2 * 4 + 1, 3 * 4 + 1, 5 * 4 + 2, 7 * 4 + 3, 10 * 4 + 3, 13 * 4 + 3]      # the product's fixed strength list (host_frames.h fill_dev)


def build(emu, force=False):
    return kernel_build.build(SRC, EMU_LIB if emu else GPU_LIB, emu, force=force)


def build_all(force=False):
    build(emu=False, force=force)
    build(emu=True, force=force)


class LrCand(C.Structure):
    _fields_ = [('cost', C.c_longlong), ('xq0', C.c_int), ('xq1', C.c_int)]


P16, P8, PI8, P32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.POINTER(C.c_uint32)


class FhFrame(C.Structure):
    _fields_ = [('w', C.c_int), ('h', C.c_int), ('bd', C.c_int), ('np', C.c_int), ('active', C.c_int),
                ('tune_psnr', C.c_int), ('fast_deblock', C.c_int), ('enable_cdef', C.c_int), ('enable_restoration', C.c_int), ('sgr_full', C.c_int),
                ('lf_sharp', C.c_int), ('cdef_damping', C.c_int),
                ('lf_level', C.c_int * 4), ('cdef_y', C.c_int * 8), ('cdef_uv', C.c_int * 8),
                ('lr_cost', C.c_uint32 * 3), ('pad_', C.c_int),
                ('wq', C.c_longlong * 3), ('rdmult', C.c_longlong),
                ('src', P16 * 3), ('rec', P16 * 3), ('fin', P16 * 3), ('lrp', P16 * 3), ('rec_p0', P16 * 3),
                ('m_txsize', P8), ('m_bsize', P8), ('m_skip', P8),
                ('act', P32), ('svar8', P32),
                ('lf_tally', C.POINTER(C.c_longlong)), ('lf_out', C.POINTER(C.c_int)), ('cdef_idx', PI8),
                ('lr_cand', C.POINTER(LrCand)), ('lr_type', P8), ('lr_set', P8), ('lr_xqd', PI8),
                ('lf_level_out', C.c_int * 4), ('guard_damage', C.c_int)]


def lr_units(size):
    return max(1, (size + 32) // 64)


class Geometry:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.mi_cols, self.mi_rows = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
        self.sb_cols, self.sb_rows = (self.mi_cols + 15) >> 4, (self.mi_rows + 15) >> 4
        self.pw, self.ph = self.sb_cols * 64, self.sb_rows * 64
        self.mi_stride, self.mi_h = self.pw // 4, self.ph // 4
        self.units = lr_units(w) * lr_units(h)


class Frame:
    """One frame of a launch.  src / rec: lists of np planes (ph x pw, uint16); the maps: (mi_h x mi_stride, uint8); act / svar8: (ph / 8 x pw / 8, uint32)."""
    def __init__(self, w, h, bd, np_, src, rec, m_txsize, m_bsize, m_skip, act, svar8, wq, fin=None, rdmult=0, lr_cost=(0, 0, 0), tune_psnr=0, fast_deblock=0,
                 enable_cdef=1, enable_restoration=0, sgr_full=0, lf_level=(0, 0, 0, 0), lf_sharp=0, cdef_damping=3, cdef_y=CDEF_LIST, cdef_uv=CDEF_LIST, active=1,
                 lf_tally=None, lr_cand=None):
        g = self.g = Geometry(w, h)
        self.w, self.h, self.bd, self.np = w, h, bd, np_
        plane = lambda a: np.ascontiguousarray(a, dtype=np.uint16).reshape(g.ph, g.pw).copy()
        sent = lambda: np.full((g.ph, g.pw), SENT16, np.uint16)
        self.src = [plane(a) for a in src[:np_]]
        self.rec = [plane(a) for a in rec[:np_]]
        self.fin = [plane(a) for a in fin[:np_]] if fin is not None else [sent() for _ in range(np_)]
        self.lrp = [sent() for _ in range(np_)]
        self.rec_p0 = [sent() for _ in range(np_)]
        mp = lambda a: np.ascontiguousarray(a, dtype=np.uint8).reshape(g.mi_h, g.mi_stride).copy()
        self.m_txsize, self.m_bsize, self.m_skip = mp(m_txsize), mp(m_bsize), mp(m_skip)
        self.act = np.ascontiguousarray(act, dtype=np.uint32).reshape(g.ph // 8, g.pw // 8).copy()
        self.svar8 = np.ascontiguousarray(svar8, dtype=np.uint32).reshape(g.ph // 8, g.pw // 8).copy()
        self.lf_tally = np.zeros(6 * 65, np.int64) if lf_tally is None else np.ascontiguousarray(lf_tally, dtype=np.int64).reshape(6 * 65).copy()
        self.lf_out = np.full(16, SENT32, np.int32)
        self.cdef_idx = np.full(g.sb_rows * g.sb_cols, SENT8, np.int8)
        nlr = g.units * np_
        self.lr_cand = np.full(nlr * 16 * 2, SENT32 | (SENT32 << 32), np.int64) if lr_cand is None else np.ascontiguousarray(lr_cand, dtype=np.int64).reshape(nlr * 32).copy()
        self.lr_type, self.lr_set, self.lr_xqd = np.full(nlr, SENT8, np.uint8), np.full(nlr, SENT8, np.uint8), np.full(nlr * 2, SENT8, np.int8)
        self.par = dict(active=active, tune_psnr=tune_psnr, fast_deblock=fast_deblock, enable_cdef=enable_cdef, enable_restoration=enable_restoration, sgr_full=sgr_full,
                        lf_sharp=lf_sharp, cdef_damping=cdef_damping, rdmult=rdmult)
        self.lf_level, self.cdef_y, self.cdef_uv, self.lr_cost, self.wq = list(lf_level), list(cdef_y), list(cdef_uv), list(lr_cost), list(wq)
        self.lf_level_out, self.guard_damage = None, None
        self.initial = self._snapshot()

    def _c(self):
        f = FhFrame()
        f.w, f.h, f.bd, f.np = self.w, self.h, self.bd, self.np
        for k, v in self.par.items():
            setattr(f, k, v)
        f.lf_level, f.cdef_y, f.cdef_uv = (C.c_int * 4)(*self.lf_level), (C.c_int * 8)(*self.cdef_y), (C.c_int * 8)(*self.cdef_uv)
        f.lr_cost, f.wq = (C.c_uint32 * 3)(*self.lr_cost), (C.c_longlong * 3)(*self.wq)
        for name in ('src', 'rec', 'fin', 'lrp', 'rec_p0'):
            arr = getattr(self, name)
            setattr(f, name, (P16 * 3)(*[arr[p].ctypes.data_as(P16) if p < self.np else P16() for p in range(3)]))
        for name, t in (('m_txsize', P8), ('m_bsize', P8), ('m_skip', P8), ('act', P32), ('svar8', P32), ('lf_tally', C.POINTER(C.c_longlong)),
                        ('lf_out', C.POINTER(C.c_int)), ('cdef_idx', PI8), ('lr_cand', C.POINTER(LrCand)), ('lr_type', P8), ('lr_set', P8), ('lr_xqd', PI8)):
            setattr(f, name, getattr(self, name).ctypes.data_as(t))
        return f

    def tallies(self):
        """The prefix-summed tallies [3][2][64] of the difference arrays the tally kernel left."""
        return np.cumsum(self.lf_tally.reshape(3, 2, 65)[:, :, :64], axis=2)

    _BUFFERS = ('src', 'rec', 'fin', 'lrp', 'm_txsize', 'm_bsize', 'm_skip', 'act', 'svar8', 'lf_tally', 'lf_out', 'cdef_idx', 'lr_cand', 'lr_type', 'lr_set', 'lr_xqd')

    def _snapshot(self):
        return {k: ([a.copy() for a in getattr(self, k)] if isinstance(getattr(self, k), list) else getattr(self, k).copy()) for k in self._BUFFERS}

    def untouched(self):
        """Every buffer of the frame still holds what it was launched with -- sentinels in everything a stage writes (an idle frame)."""
        for k, was in self.initial.items():
            now = getattr(self, k)
            if not all(np.array_equal(a, b) for a, b in (zip(now, was) if isinstance(now, list) else [(now, was)])):
                return False
        return all(np.array_equal(a, b) for a, b in zip(self.rec_p0, self.initial['rec']))


_libs = {}


def _lib(path):
    if path not in _libs:
        L = C.CDLL(path)
        L.fh_run.argtypes = [C.POINTER(FhFrame), C.c_int, C.c_int]
        L.fh_run.restype = C.c_int
        L.fh_table.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int]
        L.fh_table.restype = C.c_int
        _libs[path] = L
    return _libs[path]


def run(lib_path, frames, stages):
    """One launch per stage of `stages` over all `frames`; their arrays are updated in place."""
    arr = (FhFrame * len(frames))(*[f._c() for f in frames])
    rc = _lib(lib_path).fh_run(arr, len(frames), stages)
    assert rc == 0, 'fh_run returned %d' % rc
    for f, a in zip(frames, arr):
        f.lf_level_out, f.guard_damage = list(a.lf_level_out), a.guard_damage
    return frames


def table(lib_path, op, rows):
    """rows: (n, <= FT_IN) integers -> (n, FT_OUT) int64, one thread per row."""
    rows = np.asarray(rows, dtype=np.int64)
    a = np.zeros((rows.shape[0], FT_IN), np.int64)
    a[:, :rows.shape[1]] = rows
    out = np.zeros((rows.shape[0], FT_OUT), np.int64)
    LL = C.POINTER(C.c_longlong)
    rc = _lib(lib_path).fh_table(op, a.ctypes.data_as(LL), out.ctypes.data_as(LL), rows.shape[0])
    assert rc == 0, 'fh_table returned %d' % rc
    return out


def main(argv):
    """python -m tests.helpers.filters_harness LIB GROUP...: the cases of tests.helpers.filters_cases' groups through LIB against the reference, one JSON line
    per case (a separate process, so that the emulator reads the environment it is started with, MI_EMU_REVERSE among it)."""
    import json
    import time
    from tests.helpers import filters_cases
    for group in argv[1:]:
        t = time.time()
        for name, problems in filters_cases.check_group(argv[0], group):
            print(json.dumps({'group': group, 'name': name, 'problems': problems}), flush=True)
        print(json.dumps({'group': group, 'seconds': round(time.time() - t, 1)}), flush=True)


if __name__ == '__main__':
    import sys
    main(sys.argv[1:])
