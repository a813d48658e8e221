"""-m gpu: deep (16-bit) input on the MI355X through the product library -- the case table of tests/helpers/deep_cases.py (uint16 device arrays, the 16-bit front
end, 16-bit PNG files, files against the oracle, mixed batches, refusals, source kind 4) and the command line's --deep-png.  Nothing is wider than 517 pixels but
the 512 x 384 image that holds every level: the kernels have no size-dependent path beyond the workgroup boundary that width crosses."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
CASES = os.path.join(ROOT, 'tests', 'helpers', 'deep_cases.py')
pytest.importorskip('PIL.Image')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, *prefixes):
    from tests.helpers.deep_cases import expected_rows
    want = expected_rows()
    for prefix in prefixes:
        mine = [r for r in rows if r['case'].startswith(prefix)]
        bad = [r for r in mine if not r['ok']]
        assert not bad, bad
        assert len(mine) == want[prefix], (prefix, [r['case'] for r in mine])


def test_device_arrays_fill_the_deep_slots(table):
    _of(table, 'ingest16')


def test_strides_of_zero_mean_packed(table):
    _of(table, 'defaults')


def test_deep_front_end_writes_the_specified_planes(table):
    _of(table, 'front')


def test_16_bit_png_files_keep_both_bytes(table):
    _of(table, 'png16')


def test_files_equal_the_oracle_over_the_restated_planes(table):
    _of(table, 'files oracle')


def test_kinds_0_1_and_2_share_a_batch(table):
    _of(table, 'mixed')


def test_deep_input_is_refused_with_invalid_argument(table):
    _of(table, 'refused', 'accepted')


def test_sources_of_kind_4_beside_the_others(table):
    _of(table, 'sources')


def test_torch_uint16_tensors_through_encoder_and_batch_encoder():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch')


def _cli_encoder(quality=80.0, speed=4, dirty=False):
    import cavif_rs_amd as m
    aq = min((quality + 100.0) / 2.0, quality + quality / 4.0 + 2.0)           # src/main.rs:115
    return m.Encoder().with_quality(quality).with_alpha_quality(aq).with_speed(speed).with_alpha_color_mode('dirty' if dirty else 'clean')


def test_cli_deep_png_flag(tmp_path):
    """a directory of a 16-bit RGB PNG, a 16-bit RGBA PNG and an 8-bit PNG.  Without --deep-png every file is today's (Encoder.encode_rgba(load_rgba(bytes)): the
    high bytes).  With it the RGB file is the library's deep file and the RGBA file goes deep only together with --dirty-alpha; the 8-bit file never changes."""
    import numpy as np
    import cavif_rs_amd as m
    from tests.helpers import png_cases as P
    from tests.helpers import deep_ref as R
    from tests.helpers.deep_cases import deep_content
    w, h = 37, 23
    s_rgb, s_rgba = deep_content(1, h, w).astype(np.int64), deep_content(2, h, w, 4).astype(np.int64)
    s_rgba[2:9, 3:20, 3] = 1234
    s8 = np.random.default_rng(3).integers(0, 256, (h, w, 3))
    src = tmp_path / 'in'
    src.mkdir()
    files = []
    for name, data in (('rgb16', P.make_png(s_rgb, 16, 2, seed=1)), ('rgba16', P.make_png(s_rgba, 16, 6, seed=2)), ('rgb8', P.make_png(s8, 8, 2, seed=3))):
        p = src / (name + '.png')
        p.write_bytes(data)
        files.append(p)

    def batch_file(e, px):
        """the library's own deep file: a 4-channel batch of one image"""
        b = m.BatchEncoder(e, 1, w, h, 4)
        b.upload(0, px)
        b.encode()
        f = b.get(0).avif_file
        b.close()
        return f
    for dirty in (False, True):
        e = _cli_encoder(dirty=dirty)
        old = [e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file for f in files]
        new = [batch_file(e, s_rgb.astype(np.uint16)), batch_file(e, R.png16_rgba(s_rgba, 6)) if dirty else old[1], old[2]]
        assert new[0] != old[0]
        for flags, want in ((['--deep-png'], new), ([], old)):
            out = tmp_path / ('out%d%d' % (dirty, len(flags)))
            r = subprocess.run([CLI, '-q', '-o', str(out)] + flags + (['--dirty-alpha'] if dirty else []) + [str(f) for f in files], capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr
            for f, w_ in zip(files, want):
                assert (out / (f.stem + '.avif')).read_bytes() == w_, (dirty, flags, f.name)
    assert b'--deep-png' in subprocess.run([CLI], capture_output=True, timeout=60).stderr          # the usage text names the flag
