"""-m gpu: mixed-size batches (mi_batch_set_sizes / _fits / _image_size) through the library under test -- the product library on the MI355X,
or the emulated one through MI_AVIF_LIB as tests/test_gpu_parity.py runs against it.  The tile search, the filters and the entropy coder run on frames of
different sizes in one launch; pictures are coded independently, so every file must equal the oracle's file of that picture alone, byte for byte."""
import os
import numpy as np
import pytest

from tests.helpers import mixed_cases as mc

pytestmark = pytest.mark.gpu
FILL = 0xA5                                              # what a slot holds before the call under test: a pattern no source has throughout


@pytest.fixture(scope='module')
def m():
    import cavif_rs_amd
    return cavif_rs_amd


# ---------------------------------------------------------------- colour frames == oracle
@pytest.mark.parametrize('speed,depth,tiles,passes', mc.COLOUR_SETTINGS)
def test_colour_frames_of_six_sizes_equal_the_oracle(m, oracle, speed, depth, tiles, passes):
    """64x64, 8x8, 129x101, 17x9, 200x72 and 72x136 in a batch made for 6 x 256x192: a single superblock, less than one block, several superblocks in both
    directions, portrait, edges that are no multiples of 8"""
    assert mc.colour_case(m, oracle, speed, depth, tiles, passes) == []


# ---------------------------------------------------------------- alpha
@pytest.mark.parametrize('mode', [1, 0, 2])
def test_alpha_frames_of_four_sizes_equal_the_oracle(m, oracle, mode):
    """an alpha gradient, an opaque picture, 8x8 with alpha and noisy alpha (the cleaner works): files, colour and alpha byte sizes, uses_alpha per picture"""
    assert mc.alpha_case(m, oracle, mode) == []


# ---------------------------------------------------------------- layout
SIZES = [(20, 12), (37, 23), (33, 50), (9, 5), (37, 23)]      # slot sizes of the layout tests (37 x 23 and 33 x 50: JPEG fixtures of those sizes exist)


def _pattern(w, h, ch, k, dtype=np.uint8):
    """slot k's picture before the call under test: the fill with a stripe that names the slot"""
    a = np.full((h, w, ch), FILL if dtype == np.uint8 else 0xA5C3, dtype)
    a[k % h, :, :] = 17 + k
    return a


@pytest.fixture()
def laid_out(m):
    """a 3-channel batch made for 5 x 64x64 laid out for SIZES, every slot holding its pattern"""
    b = m.BatchEncoder(m.Encoder().with_speed(10), 5, 64, 64, 3)
    b.set_sizes(SIZES)
    for k, (w, h) in enumerate(SIZES):
        b.upload(k, _pattern(w, h, 3, k))
    yield b
    b.close()


def _neighbours_keep(b, touched, read=None, dtype=np.uint8):
    for k, (w, h) in enumerate(SIZES):
        if k not in touched:
            got = (read or b.read_input)(k)
            assert got.shape == (h, w, 3) and np.array_equal(got, _pattern(w, h, 3, k, dtype)), 'slot %d changed' % k


def test_layout_offsets_and_sizes(m, laid_out):
    b = laid_out
    assert [b.image_size(k) for k in range(5)] == SIZES
    base = b.device_input(0)
    at = 0
    for k, (w, h) in enumerate(SIZES):
        assert b.device_input(k) - base == at                # sum over the slots in front of it of w * h * channels
        at += w * h * 3
    with pytest.raises(m.AvifError):
        b.device_input(5)


def test_layout_host_upload(m, laid_out):
    b = laid_out
    src = mc.rgb(33, 50)
    b.upload(2, src)
    assert np.array_equal(b.read_input(2), src)
    _neighbours_keep(b, {2})
    # the pinned staging is laid out like the slots: a range of different sizes in one copy
    for k in (1, 2, 3):
        b.pinned_input(k)[...] = 200 + k
    b.upload_async(1, 3)
    for k in (1, 2, 3):
        assert (b.read_input(k) == 200 + k).all()
    _neighbours_keep(b, {1, 2, 3})


def _device_rows(m, which):
    """the cases of mixed_cases.device_cases: pictures in device memory.  The product library takes torch views, and torch has to be imported before the library is
    loaded (a torch wheel brings its own HIP runtime), so they run in a child process; the emulated library's device memory is host memory: numpy views, here"""
    if 'emu' in os.path.basename(m.encoder.library_path()):
        return mc.device_cases(m, mc.host_view)[which]
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, 'tests', 'helpers', 'mixed_cases.py'), root, 'torch'], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.splitlines()[-1])[which]


def test_layout_upload_device_of_a_strided_view(m):
    """a crop of a larger tensor (padded rows) into one slot of a mixed layout: the slot holds the picture, its neighbours their patterns"""
    assert _device_rows(m, 'layout') == []


def test_range_rule(m):
    """a call that describes its pictures with one size needs slots of one size: over two neighbours of different size it is InvalidArgument and nothing is
    written; over two equal neighbours inside a mixed layout it is taken"""
    assert _device_rows(m, 'range') == []


def test_layout_upload_jpeg(m, laid_out):
    from tests.helpers.jpeg_cases import FIXTURES
    b = laid_out
    data = open(os.path.join(FIXTURES, 'c444_37x23_q30.jpg'), 'rb').read()
    c = m.parse_jpeg(data)
    b.upload_jpeg(1, c)
    assert np.array_equal(b.read_input(1), m.decode_jpeg(data)[..., :3])
    _neighbours_keep(b, {1})
    with pytest.raises(m.AvifError) as ex:                      # the slot's size, not the batch's, is what a file must have
        b.upload_jpeg(2, c)
    assert ex.value.code == mc.INVALID
    c.close()


def test_layout_upload_png_handles_of_three_sizes_in_one_call(m, laid_out):
    from tests.helpers import png_cases as pc
    b = laid_out
    rng = np.random.default_rng(3)
    samples = [pc.random_samples(rng, w, h, 8, 2) for w, h in SIZES[1:4]]
    handles = [m.parse_png(pc.make_png(s, 8, 2, seed=i, interlace=i & 1)) for i, s in enumerate(samples)]
    b.upload_png(1, handles)
    for k, s in zip((1, 2, 3), samples):
        assert np.array_equal(b.read_input(k), pc.expected_rgba(s, 8, 2)[..., :3]), 'slot %d' % k
    _neighbours_keep(b, {1, 2, 3})
    with pytest.raises(m.AvifError) as ex:                      # each handle must have its slot's size
        b.upload_png(0, handles)
    assert ex.value.code == mc.INVALID
    for p in handles:
        p.close()


def test_layout_upload16(m, laid_out):
    b = laid_out
    for k, (w, h) in enumerate(SIZES):
        b.upload(k, _pattern(w, h, 3, k, np.uint16))
    rng = np.random.default_rng(4)
    src = rng.integers(0, 65536, (50, 33, 3)).astype(np.uint16)
    b.upload(2, src)
    assert np.array_equal(b.read_input16(2), src) and b.input_kind(2) == 2
    _neighbours_keep(b, {2}, b.read_input16, np.uint16)


# ---------------------------------------------------------------- fit rule
def test_fit_rule_is_derived_from_what_the_batch_reserves(m, oracle):
    """4 x 64x64: 1 x 2048 (its samples fit, its padded plane does not), five pictures, a zero extent; 4 x 128x128: 250 x 120 is larger than the reference and
    fits, and encodes to the oracle's bytes; the footprint never changes"""
    assert mc.fit_rule_case(m, oracle) == []


def test_one_larger_picture_beside_small_ones(m, oracle):
    """the point of the feature in small: a picture of four times the reference's pixels in a batch made for 12 x 64x64, beside two small ones (twelve: the
    pre-carry buffer holds jobs x the largest tile, 3 x 128x128 here)"""
    e = mc.encoder(m, 10)
    images = [mc.rgb(8, 8), mc.rgb(128, 128), mc.rgb(17, 9)]
    b = mc.mixed_batch(m, e, (12, 64, 64), images, 3)
    b.encode()
    for i, im in enumerate(images):
        assert b.get(i).avif_file == oracle.ravif_encode(im, quality=80, speed=10, depth=10)[0]
    b.close()


# ---------------------------------------------------------------- return to uniform
def test_set_count_returns_to_the_uniform_layout(m):
    e = mc.encoder(m, 10)
    uniform = [mc.rgb(72, 40, s) for s in (1, 2, 3)]
    fresh = m.BatchEncoder(e, 3, 72, 40, 3)
    for i, im in enumerate(uniform):
        fresh.upload(i, im)
    fresh.encode()
    want = [fresh.get(i).avif_file for i in range(3)]
    fresh.close()
    b = m.BatchEncoder(e, 3, 72, 40, 3)
    mixed = [mc.rgb(8, 8), mc.rgb(64, 40)]
    b.set_sizes(mc.sizes_of(mixed))
    for i, im in enumerate(mixed):
        b.upload(i, im)
    b.encode()
    b.set_count(3)
    assert [b.image_size(i) for i in range(3)] == [(72, 40)] * 3
    for i, im in enumerate(uniform):
        b.upload(i, im)
    b.encode()
    assert [b.get(i).avif_file for i in range(3)] == want
    b.close()


# ---------------------------------------------------------------- readout
def test_readout_has_each_pictures_own_shape(m):
    from tests.helpers import quality_cases as qc
    from tests.helpers import decoded_cases as dc
    images = mc.alpha_pictures()
    b = mc.mixed_batch(m, mc.encoder(m, 10, 10, quality=60.0, alpha_mode='dirty'), mc.ALPHA_REFERENCE, images, 4)
    b.encode()
    reports = b.measure()
    assert len(reports) == len(images)
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        alpha = b.uses_alpha(i)
        assert all(p.shape == (h, w) for p in b.recon(i) + b.source(i)) and len(b.recon(i)) == 3
        assert (reports[i].width, reports[i].height, reports[i].depth) == (w, h, 10)
        assert qc.triples(reports[i]) == qc.expected_report(b, i, 10, alpha), 'measure()[%d]' % i
        for which in ('recon', 'source'):
            planes = dc.planes_of(b, i, which)
            a = dc.planes_of(b, i, which, alpha=True)[0] if alpha else None
            got = b.decoded(i, which=which)
            assert got.shape == (h, w, 4 if alpha else 3)
            assert np.array_equal(got, dc.restate(planes, 10, 'ycbcr', alpha=a, channels=4 if alpha else 3)), 'decoded(%d, %s)' % (i, which)
    b.close()


# ---------------------------------------------------------------- state
def test_set_sizes_is_refused_while_an_encode_is_in_flight(m):
    images = [mc.rgb(8, 8), mc.rgb(17, 9)]
    b = mc.mixed_batch(m, mc.encoder(m, 10), (2, 64, 64), images, 3)
    b.encode_async()
    with pytest.raises(m.AvifError) as ex:
        b.set_sizes([(8, 8)])
    assert ex.value.code == mc.INVALID
    assert b.fits([(8, 8)])                                     # asking is allowed
    b.wait()
    assert b.image_size(1) == (17, 9) and len(b.get(1).avif_file) > 100
    b.set_sizes([(8, 8)])
    b.close()
