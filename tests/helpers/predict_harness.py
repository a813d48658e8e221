"""Build and call tests/kernels/predict_harness.hip (the tile search's intra prediction and distortion functions on given blocks, and its small __device__
functions on given rows) -- test infrastructure only.  Built like the other kernel harnesses (tests/helpers/kernel_build.py).

The block runner returns, per case, the whole LDS arena of the case's wavefront: it started as `fill(seed)`, so what a function wrote outside its defined
output shows.  The device buffers sit between guard zones; `run` fails when one of them, or a buffer the functions only read, changed."""
import ctypes as C
import os

import numpy as np

from tests.helpers import kernel_build

ROOT = kernel_build.ROOT
SRC = kernel_build.source('predict_harness.hip')
GPU_LIB = kernel_build.target('predict_harness', emu=False)
EMU_LIB = kernel_build.target('predict_harness', emu=True)
WAVE, RECT, GDIR4, GDIR8, GNON4, GNON8, CFL, SATD, SATD_WH, SATD_G4, SATD_G8, SSE, PSY = range(13)
PT_STRENGTH, PT_UPSAMPLE, PT_DERIV, PT_SM_WEIGHT, PT_MODE_ANGLE, PT_DECODED = range(6)
PT_IN = 8
# the arena, in uint16 units (the enum of predict_harness.hip); EDGE_OFF and EDGE_LEN(64) of dev_predict.h, GroupPredBuf of dev_group.h
EDGE_OFF, A_G, A_EDGE = 16, 32, 16 + 2 * 64 + 16
A_RA = A_G
A_RL = A_RA + A_EDGE + A_G
A_WA = A_RL + A_EDGE + A_G
A_WL = A_WA + A_EDGE + A_G
A_TMP = A_WL + A_EDGE + A_G
A_TMP_LEN = 2 * 64 + 16
A_PRED = A_TMP + A_TMP_LEN + A_G
A_SRC = A_PRED + 4096 + A_G
A_GP = A_SRC + 4096 + A_G
GP_WA, GP_WL, GP_TMP, GP_PRED, GP_LEN = 0, 48, 96, 128, 192
A_AUX = A_GP + 4 * GP_LEN + A_G
A_AUX_LEN = 2 * 2 * 64
A_LEN = A_AUX + A_AUX_LEN + A_G


def build(emu, force=False):
    return kernel_build.build(SRC, EMU_LIB if emu else GPU_LIB, emu, force=force)


def build_all(force=False):
    build(emu=False, force=force)
    build(emu=True, force=force)


class PhCase(C.Structure):
    _fields_ = [('op', C.c_int), ('bd', C.c_int), ('w', C.c_int), ('h', C.c_int), ('plane_off', C.c_int), ('luma_off', C.c_int),
                ('x', C.c_int), ('y', C.c_int), ('wl', C.c_int), ('hl', C.c_int),
                ('have_left', C.c_int), ('have_above', C.c_int), ('have_ar', C.c_int), ('have_bl', C.c_int), ('ftype', C.c_int), ('alpha', C.c_int),
                ('mode', C.c_int * 4), ('delta', C.c_int * 4), ('data_off', C.c_int), ('aux_off', C.c_int)]


def fill(seed):
    """What the arena holds when a case starts."""
    i = np.arange(A_LEN, dtype=np.uint64)
    return (((i * 2654435761 + (seed & 0xFFFFFFFF) * 40503) & 0xFFFFFFFF) >> 13).astype(np.uint16)


_libs = {}


def _lib(path):
    if path not in _libs:
        L = C.CDLL(path)
        P = C.c_void_p
        L.ph_run.argtypes = [C.POINTER(PhCase), C.c_int, P, C.c_longlong, P, C.c_longlong, P, C.c_longlong, P, P, C.c_uint]
        L.ph_run.restype = C.c_int
        L.ph_table.argtypes = [C.c_int, P, P, C.c_int]
        L.ph_table.restype = C.c_int
        L.ph_arena_len.restype = C.c_int
        assert L.ph_arena_len() == A_LEN, (L.ph_arena_len(), A_LEN)
        _libs[path] = L
    return _libs[path]


def run(lib_path, cases, planes, data, aux=(0,), seed=0):
    """One launch over all `cases` (dicts of PhCase's fields; mode / delta as lists of up to four) -> (arena dumps (n, A_LEN) uint16, results (n, 4) int64)."""
    arr = (PhCase * len(cases))()
    for a, c in zip(arr, cases):
        for k, v in c.items():
            if k in ('mode', 'delta'):
                v = list(v) + [0] * (4 - len(v))
                setattr(a, k, (C.c_int * 4)(*v))
            elif not k.startswith('_'):
                setattr(a, k, int(v))
    planes = np.ascontiguousarray(planes, dtype=np.uint16)
    data = np.ascontiguousarray(data, dtype=np.uint16)
    aux = np.ascontiguousarray(aux, dtype=np.int32)
    dump = np.zeros((len(cases), A_LEN), np.uint16)
    res = np.zeros((len(cases), 4), np.int64)
    rc = _lib(lib_path).ph_run(arr, len(cases), planes.ctypes.data, planes.size, data.ctypes.data, data.size, aux.ctypes.data, aux.size, dump.ctypes.data, res.ctypes.data, seed & 0xFFFFFFFF)
    assert rc == 0, 'ph_run returned %d' % rc
    return dump, res


def table(lib_path, op, rows):
    """rows: (n, <= PT_IN) integers -> (n,) int32, one thread per row."""
    rows = np.asarray(rows, dtype=np.int32)
    a = np.zeros((rows.shape[0], PT_IN), np.int32)
    a[:, :rows.shape[1]] = rows
    out = np.zeros(rows.shape[0], np.int32)
    rc = _lib(lib_path).ph_table(op, a.ctypes.data, out.ctypes.data, rows.shape[0])
    assert rc == 0, 'ph_table returned %d' % rc
    return out


def main(argv):
    """python -m tests.helpers.predict_harness LIB GROUP...: the cases of tests.helpers.predict_cases' groups through LIB against the reference, one JSON line
    per case that disagrees and one per group (a separate process, so that the emulator reads the environment it is started with: MI_EMU_REVERSE, and
    MI_EMU_LDS_POISON, which also seeds the arena's fill)."""
    import json
    import time
    from tests.helpers import predict_cases
    seed = int(os.environ.get('MI_EMU_LDS_POISON', '0'))
    for group in argv[1:]:
        t = time.time()
        rows = predict_cases.check_group(argv[0], group, seed=seed)
        for name, problems in rows:
            if problems:
                print(json.dumps({'group': group, 'name': name, 'problems': problems}), flush=True)
        print(json.dumps({'group': group, 'cases': len(rows), 'seconds': round(time.time() - t, 1)}), flush=True)


if __name__ == '__main__':
    import sys
    main(sys.argv[1:])
