"""tests/helpers/colour_ref.py, the numpy restatement the colour-managed input tests compare against, checked on its own: values worked out by hand, its
identities, LCMS2 (through Pillow's ImageCms) on the 8-bit grid, and a float64 statement of the same transform for the 16-bit path.  No library involved."""
import io

import numpy as np
import pytest

from tests.helpers import colour_cases as K
from tests.helpers import colour_ref as R

# measured on the CPU (profiles/colour_input.md): the largest difference between the 16-bit integer path and its float64 statement over the 16-bit test image,
# for every profile below.  Both sides are deterministic; the 1 the assertion adds covers libm differences between machines.
DEEP_MAX_MEASURED = 1
SMOOTH = K.LCMS_PROFILES + ('identity curve, para 0, para 1',)      # 'para 2, para 4, a short table' has a step: next to it a float64 curve and a table disagree by design


@pytest.fixture(scope='module')
def grid():
    return K.grid8()


@pytest.fixture(scope='module')
def levels():
    return K.levels16()


def test_thresholds_and_tables_by_hand():
    t = K.restated('p3 gamma 2.2')
    # U[k] = ceil(2^24 eotf((2 k - 1) / 510)), worked out in 50-digit decimals: 2546.17, 7638.51, 3591014.45, 16702477.69
    assert [int(t.U[k]) for k in (0, 1, 2, 128, 255)] == [0, 2547, 7639, 3591015, 16702478]
    assert np.all(np.diff(t.U) > 0)
    # a threshold and its predecessor: U[k] is the smallest linear value that gives level k
    for k in (1, 2, 128, 255):
        assert int(t.level8(t.U[k])) == k and int(t.level8(t.U[k] - 1)) == k - 1
    assert int(t.level8(0)) == 0 and int(t.level8(1 << 24)) == 255
    assert int(t.level16(0)) == 0 and int(t.level16(1 << 24)) == 65535 and int(t.level16(2048)) == int(t.out16[1]) == 103    # 65535 * 12.92 / 8192 = 103.36
    # the ends of every input table are exact; an identity curve is round(v / 255 * 2^24): 51 / 255 = 0.2 -> 3355443.2
    assert t.lin8[:, 0].tolist() == [0, 0, 0] and t.lin8[:, 255].tolist() == [1 << 24] * 3 and t.lin16[:, 0].tolist() == [0, 0, 0] and t.lin16[:, 4096].tolist() == [1 << 24] * 3
    ident = R.Transform([('identity',)] * 3)
    assert int(ident.lin8[0][51]) == 3355443 and int(ident.lin16[1][1024]) == 1 << 22
    assert ident.matrix.tolist() == [[1 << 30, 0, 0], [0, 1 << 30, 0], [0, 0, 1 << 30]]


def test_black_white_and_the_primaries_by_hand():
    t = K.restated('p3 gamma 2.2')
    # the matrix: P3 red holds 1.225 of sRGB red and negative green and blue, and so on (the published P3 -> sRGB matrix)
    assert np.allclose(np.array(t.M), [[1.2249, -0.2247, 0.0], [-0.0420, 1.0419, 0.0], [-0.0197, -0.0786, 1.0979]], atol=6e-4)
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    assert t.convert8(px).tolist() == [[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]]          # out-of-gamut primaries clip in linear light
    deep = t.convert16(px.astype(np.uint16) * 257)
    assert deep[0, 0].tolist() == [0, 0, 0] and deep[0, 2].tolist() == [65535, 0, 0] and np.all(deep[0, 1] >= 65533)
    # sRGB primaries with gamma 461 / 256 (1.8 as u8Fixed8): (64 / 255)^1.80078 = 0.08296 -> 1.055 * 0.08296^(1 / 2.4) - 0.055 = 0.3189 -> 81.3 of 255
    # (worked to four digits: the 16-bit sample is held to 2e-4 of full scale)
    g = K.restated('srgb gamma 1.8')
    assert g.convert8(np.full((1, 1, 3), 64, np.uint8)).tolist() == [[[81, 81, 81]]]
    assert abs(int(g.convert16(np.full((1, 1, 3), 64 * 257, np.uint16))[0, 0, 0]) / 65535.0 - 0.3189) < 2e-4
    # sRGB stated as a parametric curve over an identity matrix gives every grey level back
    s = R.Transform([K.SRGB_PARA] * 3)
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(s.convert8(np.stack([v, v, v], -1)[None])[0, :, 0], v)


def test_identities(grid):
    assert R.from_png(0.45455) is None and R.from_png(0.44) is None and R.from_png(0.43) is not None and R.from_png(0.45455, R.SRGB_CHRM) is not None
    assert R.from_png(0.45455, R.SRGB_CHRM).matrix.tolist() == [[1 << 30, 0, 0], [0, 1 << 30, 0], [0, 0, 1 << 30]]
    rng = np.random.default_rng(2)
    v = np.arange(256, dtype=np.uint8)
    w = np.arange(65536, dtype=np.uint16)
    for name in K.PROFILES:
        t = K.restated(name)
        if name in SMOOTH:                                                           # monotone curves stay monotone: grey ramps, every channel
            assert np.all(np.diff(t.convert8(np.stack([v, v, v], -1)[None]).astype(int), axis=1) >= 0), name
            assert np.all(np.diff(t.convert16(np.stack([w, w, w], -1)[None]).astype(int), axis=1) >= 0), name
        rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
        deep = rng.integers(0, 65536, (5, 7, 4), dtype=np.uint16)
        assert np.array_equal(t.convert8(rgba)[..., 3], rgba[..., 3]) and np.array_equal(t.convert8(rgba)[..., :3], t.convert8(rgba[..., :3]))
        assert np.array_equal(t.convert16(deep)[..., 3], deep[..., 3]) and np.array_equal(t.convert16(deep)[..., :3], t.convert16(deep[..., :3]))
        assert np.abs(t.convert8(grid).astype(int) - t.convert_float(grid, 255).astype(int)).max() <= 1, name


@pytest.mark.parametrize('intent', (0, 1))
@pytest.mark.parametrize('name', K.LCMS_PROFILES)
def test_against_lcms2_on_the_8_bit_grid(grid, name, intent):
    """PIL.ImageCms.profileToProfile to ImageCms.createProfile('sRGB'): no sample differs by more than one level, at most 5 % of the samples differ at all"""
    try:
        from PIL import Image, ImageCms
        ImageCms.core.littlecms_version
    except Exception:
        pytest.skip('Pillow was built without littlecms')
    prof = ImageCms.ImageCmsProfile(io.BytesIO(K.profile(name)))
    ref = np.asarray(ImageCms.profileToProfile(Image.fromarray(grid), prof, ImageCms.createProfile('sRGB'), renderingIntent=intent, outputMode='RGB'))
    d = np.abs(ref.astype(int) - K.restated(name).convert8(grid).astype(int))
    share = float((d != 0).mean())
    print('%s, intent %d: max %d, %.2f %% of the samples differ' % (name, intent, d.max(), 100.0 * share))
    assert d.max() <= 1 and share <= 0.05


@pytest.mark.parametrize('name', SMOOTH)
def test_the_16_bit_path_against_float64(levels, grid, name):
    """every grey level, the ramps of pure R, G and B and 4096 random colours against the double matrix and the exact curves; the 8-bit path on v and the 16-bit
    path on 257 v agree within one byte level"""
    t = K.restated(name)
    d = np.abs(t.convert16(levels).astype(int) - t.convert_float(levels, 65535).astype(int))
    print('%s: max %d, mean %.3f' % (name, d.max(), d.mean()))
    assert d.max() <= DEEP_MAX_MEASURED + 1
    assert d.max() < 128                                                             # half an 8-bit step: above it the deep path would add nothing
    wide = t.convert16(grid.astype(np.uint16) * 257).astype(int)
    assert np.abs(t.convert8(grid).astype(int) - (wide + 128) // 257).max() <= 1
