"""-m gpu: device-resident input on the MI355X through the product library -- the case table of tests/helpers/device_input_cases.py (ingest_kernel from
every layout, JPEG coefficients into RGBA and RGB slots, refusals, a mixed batch, mixed streams), the new JPEG path against the old one at sizes the
fixtures do not reach, torch tensors through Encoder and BatchEncoder, and the command line, whose JPEG files now reach the encoder as coefficients."""
import io
import json
import os
import subprocess
import sys
import threading
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
CASES = os.path.join(ROOT, 'tests', 'helpers', 'device_input_cases.py')
Image = pytest.importorskip('PIL.Image')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, prefix, count):
    mine = [r for r in rows if r['case'].startswith(prefix)]
    bad = [r for r in mine if not r['ok']]
    assert not bad, bad
    assert len(mine) == count, [r['case'] for r in mine]


def test_ingest_fills_the_slot_from_every_layout(table):
    from tests.helpers.device_input_cases import SIZES
    _of(table, 'ingest', len(SIZES) * 2 * 3 * 2 * 2 + 3 + 2)


def test_jpeg_coefficients_decode_into_rgba_and_rgb_slots(table):
    from tests.helpers.jpeg_cases import fixture_names
    assert len(fixture_names()) == 31
    _of(table, 'jpeg', 31 + 1 + 5)


def test_uploads_are_refused_with_invalid_argument(table):
    _of(table, 'refused', 6)


def test_strides_of_zero_mean_packed(table):
    _of(table, 'defaults', 4)


def test_batch_of_host_ingested_and_jpeg_images(table):
    _of(table, 'batch', 1)


def test_stream_of_mixed_sources(table):
    _of(table, 'stream', 4)


def test_new_jpeg_path_equals_the_old_one_beyond_the_fixture_sizes():
    """upload_jpeg + read_input against decode_jpeg, the project's own tested path: a 300x20 4:2:0 file (a row wider than one 256-pixel workgroup) and a
    1080p 4:4:4 progressive one, into RGBA and RGB batches"""
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    e = m.Encoder().with_speed(10)
    for (w, h), kw in (((300, 20), dict(quality=90, subsampling=2)), ((1920, 1080), dict(quality=90, subsampling=0, progressive=True))):
        b = io.BytesIO(); Image.fromarray(synth_image(w, h, index=31), 'RGB').save(b, 'JPEG', **kw); data = b.getvalue()
        want = m.decode_jpeg(data)
        c = m.parse_jpeg(data)
        assert (c.width, c.height) == (w, h) and want.shape == (h, w, 4)
        for ch in (4, 3):
            be = m.BatchEncoder(e, 1, w, h, ch)
            be.upload_jpeg(0, c)
            got = be.read_input(0)
            be.close()
            assert np.array_equal(got, want[..., :ch]), (w, h, ch, int((got != want[..., :ch]).sum()))
        c.close()


def test_torch_tensors_through_encoder_and_batch_encoder():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch', 11)


def _cli_encoder(quality=80.0, speed=4):
    import cavif_rs_amd as m
    aq = min((quality + 100.0) / 2.0, quality + quality / 4.0 + 2.0)           # src/main.rs:115
    return m.Encoder().with_quality(quality).with_alpha_quality(aq).with_speed(speed).with_alpha_color_mode('clean')


def test_cli_converts_jpeg_and_png_files_beside_the_decode_pool(tmp_path):
    """four JPEG (one grey, one on stdin) and four PNG files of two sizes: every output equals Encoder.encode_rgba(load_rgba(bytes)); the per-device pool of
    decode contexts behind mi_jpeg_decode_rgba exists before and serves eight threads after, next to the path that no longer uses it"""
    import cavif_rs_amd as m
    from tests.helpers.jpeg_cases import FIXTURES, fixture
    jpegs = ['c420_33x50_q30_opt', 'c444_33x50_q100_noise', 'grey_37x23_q75', 'c444_37x23_q30']
    pngs = ['c422_33x50_q75', 'c420_33x50_q75_exif_com', 'c420_37x23_q100', 'rgb_37x23_q95_keeprgb']
    first = []
    t = threading.Thread(target=lambda: first.append(m.decode_jpeg(fixture(jpegs[0])[0])))
    t.start(); t.join(timeout=60)
    assert first and np.array_equal(first[0], fixture(jpegs[0])[1])
    files = []
    for name, ext in [(n, 'jpg') for n in jpegs] + [(n, 'png') for n in pngs]:
        p = tmp_path / (name + '.' + ext)
        p.write_bytes(open(os.path.join(FIXTURES, name + '.' + ext), 'rb').read())
        files.append(p)
    on_stdin = files.pop(1)
    r = subprocess.run([CLI, '-q'] + [str(f) for f in files] + ['-'], input=on_stdin.read_bytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    e = _cli_encoder()
    for f in files:
        assert f.with_suffix('.avif').read_bytes() == e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file, f.name
    assert r.stdout == e.encode_rgba(m.load_rgba(on_stdin.read_bytes())).avif_file
    # the same two kinds of source through this process's library, where the pool lives
    many = m.encode_many(e, [m.parse_jpeg(fixture(n)[0]) for n in jpegs] + [fixture(n)[1] for n in pngs])
    assert [x.avif_file for x in many] == [e.encode_rgba(fixture(n)[1]).avif_file for n in jpegs + pngs]
    results = [None] * 8

    def run(i):
        results[i] = [m.decode_jpeg(fixture(n)[0]) for n in jpegs[i % 4:] + jpegs[:i % 4]]
    threads = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=60)
    for i in range(8):
        assert results[i] is not None
        for got, n in zip(results[i], jpegs[i % 4:] + jpegs[:i % 4]):
            assert np.array_equal(got, fixture(n)[1]), (i, n)
