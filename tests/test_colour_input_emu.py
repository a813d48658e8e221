"""Colour-managed input on the CPU: colour_convert_kernel and colour_convert16_kernel (dev_colour.h) and mi_batch_convert_colour behind them, inside the
SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/colour_cases.py, shared with tests/test_gpu_colour_input.py; every
comparison is for equality against the numpy restatement tests/test_colour_reference.py checks."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'colour_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def check(rows, *prefixes):
    """every row passed, and each prefix has the number of rows a complete run prints"""
    from tests.helpers.colour_cases import expected_rows
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    want = expected_rows()
    for prefix in prefixes:
        assert len([r for r in rows if r['case'].startswith(prefix)]) == want[prefix], (prefix, [r['case'] for r in rows])


def test_slots_are_converted_in_place(emu_env):
    """1 x 1, 3 x 2, 67 x 5 and 517 x 3, 3 and 4 channels, 8-bit and deep slots, two profiles: the middle slot of three alone (its neighbours keep every
    sample), then a range of two in one launch, which converts the middle slot a second time; the test images; slots of both kinds in one range; the
    identity transform launches nothing (the emulator's launch counter) and a real one over three runs of kinds launches three times"""
    rows = _run(emu_env, 'kernels', 1800)
    check(rows, 'kernels')
    assert len([r for r in rows if r['case'].startswith('launches')]) == 1


def test_converted_slots_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront in the opposite order: the kernel table and the files again"""
    rows = _run(emu_env, 'kernels', 1800, MI_EMU_REVERSE='1') + _run(emu_env, 'files', 900, MI_EMU_REVERSE='1')
    check(rows, 'kernels', 'files png', 'files jpeg', 'files unchanged')


def test_files_are_converted_by_their_own_description(emu_env):
    """PNG files with each chunk combination (iCCP wins over gAMA, sRGB wins over gAMA, gAMA 45455 alone is the identity, gAMA + cHRM, an unsupported and a
    malformed profile leave the upload unmanaged), a 16-bit PNG deep and through its high bytes, a palette PNG with tRNS, JPEG files with one segment, two
    segments in reversed order and a missing segment; the default calls give the bytes of the same files without colour chunks or APP2"""
    check(_run(emu_env, 'files', 900), 'files png', 'files jpeg', 'files unchanged')


def test_managed_source_kinds_beside_the_others(emu_env):
    """mi_ravif_encode_sources with kinds 5, 6 and 7 (33 x 50, RGBA slots): encode_many(managed=True) over a managed PNG, a managed JPEG, files with an unsupported
    and a malformed profile, a host array, a PNG with alpha and gAMA, a 16-bit PNG; the same list without the keyword; kinds 0 to 7 in one run"""
    check(_run(emu_env, 'sources', 1500), 'sources')


def test_conversions_are_refused_with_invalid_argument(emu_env):
    """a YCbCr slot, a range past the capacity, null, a call in flight: MI_INVALID_ARGUMENT, the footprint and the slot unchanged; the Python error types"""
    check(_run(emu_env, 'refused', 600), 'refused')
