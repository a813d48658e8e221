"""-m gpu: PNG input on the MI355X through the product library -- the case table of tests/helpers/png_cases.py (every filter, the geometry around a band
of 64 rows and a chunk of 64 columns, the 15 colour type / depth pairs with tRNS and Adam7, slots and refusals, statuses, mixed streams), full-size files
against mi_png_decode_rgba, the Python layer with and without torch loaded first, and the command line, whose PNG files now reach the encoder as scanlines."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
CASES = os.path.join(ROOT, 'tests', 'helpers', 'png_cases.py')


def _child(which, timeout, *more):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which] + list(more), env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 300)


def _of(rows, prefix, count):
    mine = [r for r in rows if r['case'].startswith(prefix)]
    bad = [r for r in mine if not r['ok']]
    assert not bad, bad
    assert len(mine) == count, [r['case'] for r in mine]


def test_filters_every_type_on_every_row_and_on_the_first(table):
    _of(table, 'filters', 39)


def test_geometry_around_the_band_and_the_column_chunk(table):
    from tests.helpers import png_cases as pc
    _of(table, 'geometry', (len(pc.HEIGHTS) + len(pc.WIDTHS)) * 2 * 2 + 2 + 3 + 2 * 5 * 2)


def test_every_colour_type_depth_trns_and_adam7(table):
    from tests.helpers import png_cases as pc
    assert len(pc.KINDS) == 15
    _of(table, 'kind', len(pc.KIND_SIZES) * 2 * (15 + 6))


def test_slots_mixed_calls_and_refusals(table):
    _of(table, 'slots', 2)
    _of(table, 'refused', 3)


def test_parse_statuses_equal_decode_statuses(table):
    _of(table, 'status', 5)


def test_stream_of_host_jpeg_and_png_sources(table):
    _of(table, 'stream', 3)


def test_python_layer(table):
    _of(table, 'python', 5)


def test_python_layer_with_torch_loaded_first():
    pytest.importorskip('torch')
    _of(_child('python', 300, 'torch'), 'python', 5)


@pytest.mark.parametrize('name', ['rgb8 all Paeth', 'rgba16 random filters', 'rgb8 Adam7 random filters'])
def test_full_size_files_equal_the_host_reader(name):
    """1920 x 1080 through parse_png + BatchEncoder.upload_png + read_input against load_rgba (mi_png_decode_rgba) and the samples the file was made from"""
    import cavif_rs_amd as m
    from tests.helpers import png_cases as pc
    w, h = 1920, 1080
    rng = np.random.default_rng(len(name))
    ctype, depth, kw = {'rgb8 all Paeth': (2, 8, dict(filters=4)), 'rgba16 random filters': (6, 16, dict(seed=1)), 'rgb8 Adam7 random filters': (2, 8, dict(interlace=1, seed=2))}[name]
    # photographic-like content (smooth + noise), so that the predictors' choices vary along a row
    base = np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[..., None] + np.arange(pc.CHANNELS[ctype]) * 977
    s = (base * (1 if depth == 8 else 61) + rng.integers(0, 24 if depth == 8 else 4000, base.shape)) % (1 << depth)
    data = pc.make_png(s, depth, ctype, **kw)
    want = m.load_rgba(data)
    assert np.array_equal(want, pc.expected_rgba(s, depth, ctype))
    p = m.parse_png(data)
    assert (p.width, p.height, p.has_alpha) == (w, h, ctype == 6)
    e = m.Encoder().with_speed(10)
    for ch in (4, 3) if ctype == 2 else (4,):
        b = m.BatchEncoder(e, 2, w, h, ch)
        b.upload_png(1, p)
        got = b.read_input(1)
        b.close()
        assert np.array_equal(got, want[..., :ch]), (name, ch, int((got != want[..., :ch]).sum()))
    p.close()


def _cli_encoder(quality=80.0, speed=4):
    import cavif_rs_amd as m
    aq = min((quality + 100.0) / 2.0, quality + quality / 4.0 + 2.0)           # src/main.rs:115
    return m.Encoder().with_quality(quality).with_alpha_quality(aq).with_speed(speed).with_alpha_color_mode('clean')


@pytest.mark.parametrize('background_exit', [False, True])
def test_cli_converts_a_directory_of_png_and_jpeg_files(tmp_path, background_exit):
    """PNG files of every route (filters, Adam7, palette + tRNS, 16 bit, gray) and JPEG files of two sizes: every output equals
    Encoder.encode_rgba(load_rgba(bytes)), in the one-process mode and with CAVIF_MI_BACKGROUND_EXIT=1"""
    import cavif_rs_amd as m
    from tests.helpers import png_cases as pc
    from tests.helpers.jpeg_cases import FIXTURES
    rng = np.random.default_rng(12)
    files = []
    for i, (ctype, depth, (w, h), kw) in enumerate(((2, 8, (33, 50), dict(filters=4)), (6, 8, (33, 50), dict(seed=1)), (6, 16, (37, 23), dict(interlace=1)), (0, 2, (37, 23), dict()),
                                                    (3, 4, (33, 50), dict(plte=rng.integers(0, 256, 48, dtype=np.uint8).tobytes(), trns=b'\x00\x40\x80')), (2, 8, (200, 130), dict(interlace=1, seed=4)))):
        p = tmp_path / ('p%d.png' % i)
        p.write_bytes(pc.make_png(pc.random_samples(rng, w, h, depth, ctype), depth, ctype, **kw))
        files.append(p)
    for name in ('c420_33x50_q30_opt', 'grey_37x23_q75', 'c444_37x23_q30'):
        p = tmp_path / (name + '.jpg')
        p.write_bytes(open(os.path.join(FIXTURES, name + '.jpg'), 'rb').read())
        files.append(p)
    env = dict(os.environ, CAVIF_MI_BACKGROUND_EXIT='1') if background_exit else {k: v for k, v in os.environ.items() if k != 'CAVIF_MI_BACKGROUND_EXIT'}
    r = subprocess.run([CLI, '-q'] + [str(f) for f in files], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    e = _cli_encoder()
    for f in files:
        assert f.with_suffix('.avif').read_bytes() == e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file, f.name
    # a broken PNG fails alone, with the message it always had
    bad = tmp_path / 'bad.png'
    bad.write_bytes(files[0].read_bytes()[:60])
    r = subprocess.run([CLI, '-f', str(bad), str(files[1])], capture_output=True, timeout=120, env=env)
    assert r.returncode == 1 and b'corrupt image data' in r.stderr and r.stderr.count(b'error:') == 2
