"""Builds the kernel harnesses of tests/kernels/ (test infrastructure only): one source, two libraries under tests/kernels/_build/.

hipcc with the product's flags gives the GPU library, g++ with the SIMT emulator's shim (tests/emu/, the same command as tests/emu/__init__.py) its emulated
twin.  Each is stamped with a digest of its sources and flags and rebuilt when stale."""
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KDIR = os.path.join(ROOT, 'tests', 'kernels')
OUT = os.path.join(KDIR, '_build')


def source(name):
    return os.path.join(KDIR, name)


def target(stem, emu):
    return os.path.join(OUT, 'lib%s%s.so' % (stem, '_emu' if emu else ''))


def _sources(src, emu):
    csrc = os.path.join(ROOT, 'cavif_rs_amd', 'csrc')
    srcs = [src] + [os.path.join(csrc, f) for f in sorted(os.listdir(csrc))]
    if emu:
        srcs += [os.path.join(ROOT, 'tests', 'emu', 'emu_runtime.cpp'), os.path.join(ROOT, 'tests', 'emu', 'include', 'hip', 'hip_runtime.h')]
    return srcs


def _command(src, emu, out):
    if emu:
        return ['g++', '-O2', '-g', '-rdynamic', '-fno-extern-tls-init', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-w',
                '-I', os.path.join(ROOT, 'tests', 'emu', 'include'), '-I', os.path.join(ROOT, 'include'), '-x', 'c++',
                src, os.path.join(ROOT, 'tests', 'emu', 'emu_runtime.cpp'), '-o', out, '-lz', '-lpthread', '-ldl']
    import __graft_entry__
    hipcc = 'hipcc' if subprocess.call(['which', 'hipcc'], stdout=subprocess.DEVNULL) == 0 else '/opt/rocm/bin/hipcc'
    return [hipcc] + __graft_entry__.HIPCC_FLAGS + ['-o', out, src]


def _digest(cmd, srcs):
    h = hashlib.sha256(' '.join(os.path.relpath(c, ROOT) if c.startswith(ROOT) else c for c in cmd).encode())
    for s in srcs:
        with open(s, 'rb') as fh:
            h.update(os.path.basename(s).encode() + b'\0' + fh.read())
    return h.hexdigest()


def build(src, out, emu, force=False):
    cmd = _command(src, emu, out)
    want = _digest(cmd, _sources(src, emu))
    stamp = out + '.stamp'
    have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(out) else ''
    if force or have != want:
        os.makedirs(OUT, exist_ok=True)
        subprocess.check_call(cmd)
        with open(stamp, 'w') as fh:
            fh.write(want + '\n')
    return out
