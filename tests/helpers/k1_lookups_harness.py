"""Build and call the checkers of the tile search's branch-free lookups -- test infrastructure only.

tests/kernels/k1_lookups_main.cpp is a stand-alone g++ program (the SIMT emulator's macros, no kernel launch): the product's functions against restatements of
the switch / if forms they replaced, over the whole domain of tests/kernels/k1_lookups_domain.h; it also writes the restatements' values to a file.
tests/kernels/k1_lookups_harness.hip evaluates the product's functions over the same domain on the GPU, one argument per lane."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests.helpers import kernel_build

ROOT = kernel_build.ROOT
SRC = kernel_build.source('k1_lookups_harness.hip')
GPU_LIB = kernel_build.target('k1_lookups_harness', emu=False)
MAIN = kernel_build.source('k1_lookups_main.cpp')


def build(force=False):
    return kernel_build.build(SRC, GPU_LIB, False, force=force)


def build_all(force=False):
    build(force=force)


def run_cpu(workdir):
    """Builds and runs the stand-alone program in `workdir`.  Returns (exit status, its output, the restatements' values)."""
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed for the stand-alone program'
    exe, dump = os.path.join(workdir, 'k1_lookups'), os.path.join(workdir, 'k1_lookups.i32')
    subprocess.check_call([gxx, '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-w', '-I', os.path.join(ROOT, 'tests', 'emu', 'include'),
                           '-I', os.path.join(ROOT, 'include'), MAIN, os.path.join(ROOT, 'tests', 'emu', 'emu_runtime.cpp'), '-o', exe, '-lz', '-lpthread', '-ldl'])
    p = subprocess.run([exe, dump], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    want = np.fromfile(dump, dtype=np.int32) if os.path.exists(dump) else np.zeros(0, np.int32)
    return p.returncode, p.stdout, want


def run_gpu():
    """The product's functions on the GPU over the whole domain: int32 values in the domain's order."""
    L = C.CDLL(build())
    L.k1l_total.restype = C.c_int
    L.k1l_run.argtypes = [C.c_void_p, C.c_int]
    L.k1l_run.restype = C.c_int
    n = L.k1l_total()
    out = np.zeros(n, dtype=np.int32)
    rc = L.k1l_run(out.ctypes.data, n)
    assert rc == 0, 'k1l_run returned %d' % rc
    return out
