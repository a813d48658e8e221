"""-m gpu: JPEG input on the MI355X through the product library -- every fixture of tests/golden/jpeg/ to exactly its expected pixels, two 1080p files
against Pillow's decode on this machine, the decode-context pool under 32 threads, and the command line on JPEG files (directory of mixed inputs,
stdin, an unsupported file among good ones)."""
import io
import os
import subprocess
import threading
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
Image = pytest.importorskip('PIL.Image')


def _cli_encoder(quality=80.0, speed=4, dirty=False, depth=0, color=0):
    import cavif_rs_amd as m
    aq = min((quality + 100.0) / 2.0, quality + quality / 4.0 + 2.0)           # src/main.rs:115
    e = m.Encoder().with_quality(quality).with_alpha_quality(aq).with_speed(speed).with_alpha_color_mode('dirty' if dirty else 'clean')
    if depth:
        e = e.with_bit_depth(depth)
    if color:
        e = e.with_internal_color_model('rgb')
    return e


def _jpeg(img, **kw):
    b = io.BytesIO(); Image.fromarray(img, 'RGB').save(b, 'JPEG', **kw); return b.getvalue()


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGBA'))


def test_every_fixture_decodes_to_libjpegs_pixels():
    import cavif_rs_amd as m
    from tests.helpers.jpeg_cases import fixture_names, fixture
    names = fixture_names()
    assert len(names) >= 24
    bad = []
    for name in names:
        data, want = fixture(name)
        got, via = m.decode_jpeg(data), m.load_rgba(data)
        if got.shape != want.shape or not np.array_equal(got, want) or not np.array_equal(via, want):
            bad.append((name, int((got != want).sum()) if got.shape == want.shape else got.shape))
    assert not bad, bad


def test_1080p_files_equal_pillows_decode_here():
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    from tests.helpers.jpeg_cases import fixture_names, fixture
    for name in fixture_names():                                # is this machine's Pillow the libjpeg the goldens came from?
        data, want = fixture(name)
        if not np.array_equal(_pillow(data), want):
            pytest.skip('the Pillow on this machine does not reproduce the committed expected pixels (%s): its libjpeg is not the one the goldens came from' % name)
    img = synth_image(1920, 1080, index=31)
    for kw in (dict(quality=90, subsampling=2), dict(quality=90, subsampling=0, progressive=True)):
        data = _jpeg(img, **kw)
        got = m.decode_jpeg(data)
        want = _pillow(data)
        assert got.shape == want.shape and np.array_equal(got, want), (kw, int((got != want).sum()))


def test_32_threads_share_the_context_pool():
    """32 threads decode different fixtures through one process at the same moment (more callers than the 8 contexts the pool keeps): same bytes as one by one"""
    import cavif_rs_amd as m
    from tests.helpers.jpeg_cases import fixture_names, fixture
    names = fixture_names()
    work = [fixture(names[i % len(names)]) for i in range(32)]
    results = [None] * 32
    gate = threading.Barrier(32)

    def run(i):
        gate.wait()
        out = []
        for k in range(4):
            data, _ = work[(i + 7 * k) % 32]
            out.append(m.decode_jpeg(data))
        results[i] = out
    threads = [threading.Thread(target=run, args=(i,)) for i in range(32)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=120)
    assert all(r is not None for r in results)
    for i in range(32):
        for k in range(4):
            assert np.array_equal(results[i][k], work[(i + 7 * k) % 32][1]), (i, k)
    m.load_library().mi_release_cached()
    data, want = work[0]
    assert np.array_equal(m.decode_jpeg(data), want)            # the pool refills after a release


def test_cli_converts_a_directory_of_jpeg_and_png_files(tmp_path):
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    files = []
    for i, (w, h) in enumerate([(160, 96), (97, 61), (160, 96), (64, 48), (160, 96), (33, 50)]):
        img = synth_image(w, h, index=50 + i)
        p = tmp_path / ('in%d.%s' % (i, 'png' if i % 3 == 2 else 'jpg'))
        if i % 3 == 2:
            Image.fromarray(img, 'RGB').save(p)
        else:
            p.write_bytes(_jpeg(img, quality=85, subsampling=(2, 1, 0)[i % 3], progressive=bool(i & 1)))
        files.append(p)
    grey = tmp_path / 'grey.jpeg'
    Image.fromarray(synth_image(80, 40, index=60), 'RGB').convert('L').save(grey, 'JPEG', quality=70); files.append(grey)
    out = tmp_path / 'out'
    r = subprocess.run([CLI, '-o', str(out)] + [str(f) for f in files], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    e = _cli_encoder()
    for f in files:
        want = e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file
        assert (out / (f.name.rsplit('.', 1)[0] + '.avif')).read_bytes() == want, f.name
    # stdin JPEG -> stdout, nothing else on stdout
    r = subprocess.run([CLI, '-'], input=files[0].read_bytes(), capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == e.encode_rgba(m.load_rgba(files[0].read_bytes())).avif_file
    # settings reach the JPEG path like the PNG path
    r = subprocess.run([CLI, '-f', '-Q', '50', '-s', '7', '--depth', '8', '-o', str(tmp_path / 'named.avif'), str(files[1])], capture_output=True, timeout=120)
    assert r.returncode == 0 and (tmp_path / 'named.avif').read_bytes() == _cli_encoder(50.0, 7, depth=8).encode_rgba(m.load_rgba(files[1].read_bytes())).avif_file


def test_cli_keeps_going_past_an_unsupported_jpeg(tmp_path):
    """a CMYK file and a cut-off file among good ones fail alone, exit status 1, every other image gets its own file"""
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    e = _cli_encoder()
    names = []
    for i in range(6):
        p = tmp_path / ('im%d.jpg' % i)
        if i == 2:
            Image.new('CMYK', (32, 32), (10, 20, 30, 40)).save(p, 'JPEG')
        elif i == 4:
            p.write_bytes(_jpeg(synth_image(96, 64, index=i), quality=80)[:300])
        else:
            p.write_bytes(_jpeg(synth_image(96 + 32 * (i & 1), 64, index=i), quality=80))
        names.append(str(p))
    r = subprocess.run([CLI] + names, capture_output=True, timeout=120)
    assert r.returncode == 1
    assert b'im2.jpg: error: unsupported image format (this build reads PNG and baseline/progressive 8-bit JPEG)' in r.stderr
    assert b'im4.jpg: error: corrupt image data' in r.stderr and r.stderr.count(b'error: ') == 4
    for i in range(6):
        out = tmp_path / ('im%d.avif' % i)
        if i in (2, 4):
            assert not out.exists()
        else:
            assert out.read_bytes() == e.encode_rgba(m.load_rgba((tmp_path / ('im%d.jpg' % i)).read_bytes())).avif_file
