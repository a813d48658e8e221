"""Deep YCbCr input on the CPU: planes_ingest16_kernel (dev_planes.h), the YCbCr branch of frontend_deep_kernel (dev_deep.h) and the input kind
MI_INPUT_YCBCR16 behind them, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/ycc16_cases.py, shared with
tests/test_gpu_ycc16_input.py; every comparison is for equality against the numpy restatement tests/test_ycc16_reference.py checks."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip('PIL.Image')


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'ycc16_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def check(rows, *prefixes):
    """every row passed, and each prefix has the number of rows a complete run prints"""
    from tests.helpers.ycc16_cases import expected_rows
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    want = expected_rows()
    for prefix in prefixes:
        assert len([r for r in rows if r['case'].startswith(prefix)]) == want[prefix], (prefix, [r['case'] for r in rows])


def test_every_sample_value_through_the_ingest_map(emu_env):
    """for each bit count 8..16, full and narrow range, low- and msb-aligned: all 2^bits values in Y, Cb and Cr of a 4:4:4 picture, garbage in the bits that
    do not count -- the reciprocal arithmetic of planes_ingest16_kernel against the integer division of the restatement"""
    check(_run(emu_env, 'values', 600), 'values')


def test_uint16_planes_fill_the_deep_slots(emu_env):
    """planes_ingest16_kernel: 4:4:4, 4:2:2 and 4:2:0, planar and interleaved pairs, into 3- and 4-channel batches, at eight sizes (chroma planes of one and
    two samples' width, partial groups, the 256-pixel run, the workgroup boundary), packed rows, rows padded by 6 bytes, a base 2 bytes off; three images per
    call into slots 1..3 of five, the sentinels in slots 0 and 4 kept; P010, narrow 10 bits, 12 bits and narrow msb-aligned 16 bits in turn"""
    check(_run(emu_env, 'ingest', 900), 'ingest')


def test_strides_of_zero_mean_packed(emu_env):
    check(_run(emu_env, 'defaults', 600), 'defaults')


def test_kind_3_front_end_writes_the_specified_planes(emu_env):
    """frontend_deep_kernel's YCbCr branch: every Y level with neutral chroma, every Cb and Cr level (cut into 64 x 64 tiles here), random slots at eight sizes
    at depths 8 and 10; a 4-channel batch whose fourth sample is 0 uses no alpha"""
    check(_run(emu_env, 'front', 2400), 'front')


def test_deep_ycbcr_does_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order: the kernel tables again"""
    rows = []
    for which in ('ingest', 'values', 'mixed'):
        rows += _run(emu_env, which, 900, MI_EMU_REVERSE='1')
    check(rows, 'ingest', 'values', 'mixed')


def test_files_equal_the_oracle_over_the_restated_planes(emu_env):
    """P010 4:2:0 pictures of 33 x 50 and 37 x 23, full and narrow range, at two settings and both depths: the file is the oracle's frame over the numpy planes
    (its padding replicates the edge), and avifdec decodes it to the reconstruction; 10-bit 4:4:4 at depth 10 is lossless on the way in; 8 bits 4:4:4 give the
    8-bit call's file"""
    check(_run(emu_env, 'files', 1200), 'files oracle', 'files:')


def test_kinds_0_to_3_share_a_batch(emu_env):
    check(_run(emu_env, 'mixed', 900), 'mixed')


def test_deep_ycbcr_is_refused_with_invalid_argument(emu_env):
    """the colour model and alpha rules of the kind, null pointers, subsampling, bits, alignment and range flags, odd pointers and strides, short rows, ranges,
    kinds 4 and -1, set_input_kind(.., 3) before the deep slots exist, mi_batch_convert_colour over a kind-3 slot, a call in flight, planes of mixed sample
    types in Python; a refused call allocates nothing"""
    check(_run(emu_env, 'refused', 600), 'refused', 'accepted')
