"""-m gpu: YCbCr input on the MI355X through the product library -- the case table of tests/helpers/ycc_cases.py (JPEG coefficients straight to the file's
own YCbCr, planes in device memory, the front end's YCbCr mode, input kinds, refusals, files against the oracle, mixed runs of all four source kinds) and the
command line's --jpeg-ycbcr.  Nothing is wider than 517 pixels: the kernels have no size-dependent path beyond the workgroup boundary that size crosses."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
CASES = os.path.join(ROOT, 'tests', 'helpers', 'ycc_cases.py')
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
    from tests.helpers.ycc_cases import expected_rows
    want = expected_rows()
    for prefix in prefixes:
        mine = [r for r in rows if r['case'].startswith(prefix)]
        bad = [r for r in mine if not r['ok']]
        assert not bad, bad
        assert len(mine) == want[prefix], (prefix, [r['case'] for r in mine])


def test_jpeg_coefficients_become_the_files_own_ycbcr(table):
    _of(table, 'jpeg_ycc')


def test_device_planes_fill_the_slot(table):
    _of(table, 'planes')


def test_front_end_writes_the_planes_without_the_matrix(table):
    _of(table, 'front')


def test_kind_follows_the_call_that_last_filled_the_slot(table):
    _of(table, 'kinds')


def test_ycbcr_input_is_refused_with_invalid_argument(table):
    _of(table, 'refused', 'accepted')


def test_files_equal_the_oracle_over_the_expected_planes(table):
    _of(table, 'files oracle')


def test_sources_of_all_kinds_in_one_run(table):
    _of(table, 'files sources')


def test_torch_planes_through_encoder_and_batch_encoder():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch')


def _cli_encoder(quality=80.0, speed=4):
    import cavif_rs_amd as m
    aq = min((quality + 100.0) / 2.0, quality + quality / 4.0 + 2.0)           # src/main.rs:115
    return m.Encoder().with_quality(quality).with_alpha_quality(aq).with_speed(speed).with_alpha_color_mode('clean')


def test_cli_jpeg_ycbcr_flag(tmp_path):
    """a directory of two JPEG files (4:2:0 and grey), a keep-RGB JPEG and a PNG: with --jpeg-ycbcr the first two equal Encoder.encode_jpeg(ycbcr=True) and the
    other two go as before; without the flag every file is today's (Encoder.encode_rgba(load_rgba(bytes))); under --color rgb the flag changes nothing"""
    import cavif_rs_amd as m
    from tests.helpers.jpeg_cases import FIXTURES
    names = [('c420_33x50_q30_opt', 'jpg'), ('grey_37x23_q75', 'jpg'), ('rgb_37x23_q95_keeprgb', 'jpg'), ('c444_33x50_q100_noise', 'png')]
    src = tmp_path / 'in'
    src.mkdir()
    files = []
    for name, ext in names:
        p = src / (name + '.' + ext)
        p.write_bytes(open(os.path.join(FIXTURES, name + '.' + ext), 'rb').read())
        files.append(p)
    e = _cli_encoder()
    old = [e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file for f in files]
    new = [e.encode_jpeg(f.read_bytes(), ycbcr=True).avif_file for f in files[:2]] + old[2:]
    assert new[0] != old[0]                                                     # (the grey file's planes are the same on both paths: Y = L, neutral chroma)
    for flags, want in ((['--jpeg-ycbcr'], new), ([], old)):
        out = tmp_path / ('out' + str(len(flags)))
        r = subprocess.run([CLI, '-q', '-o', str(out)] + flags + [str(f) for f in files], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for f, w in zip(files, want):
            assert (out / (f.stem + '.avif')).read_bytes() == w, (flags, f.name)
    rgb = _cli_encoder().with_internal_color_model('rgb')
    out = tmp_path / 'out_rgb'
    r = subprocess.run([CLI, '-q', '--color', 'rgb', '--jpeg-ycbcr', '-o', str(out)] + [str(f) for f in files], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for f in files:
        assert (out / (f.stem + '.avif')).read_bytes() == rgb.encode_rgba(m.load_rgba(f.read_bytes())).avif_file, f.name
    assert b'--jpeg-ycbcr' in subprocess.run([CLI], capture_output=True, timeout=60).stderr          # the usage text names the flag
