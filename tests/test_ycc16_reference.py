"""The numpy restatement of deep YCbCr input (tests/helpers/ycc16_ref.py) against include/mi_avif.h: the properties the header states about the two sample maps,
checked over every value, values worked out by hand, and the upsampling against the 8-bit restatement of tests/helpers/ycc_cases.py.  No library is loaded:
tests/helpers/ycc16_cases.py compares the kernels with these functions."""
import itertools

import numpy as np
import pytest

from tests.helpers import ycc16_ref as R

pytest.importorskip('PIL.Image')                                                    # ycc_cases reads its fixtures through it
from tests.helpers import ycc_cases as Y8                                           # noqa: E402

M = 65535


@pytest.mark.parametrize('bits', (8, 10))
def test_a_full_range_sample_reaches_the_plane_of_its_own_depth_as_itself(bits):
    v = np.arange(1 << bits)
    assert np.array_equal(R.plane_y(R.canonical(v, bits, False), bits), v)
    assert np.array_equal(R.plane_c(R.canonical(v, bits, True), bits), v)


def test_eight_bits_give_the_planes_of_the_8_bit_path():
    v = np.arange(256)
    t = np.stack([v, v, v[::-1]], -1)[None].astype(np.uint8)
    slot = np.stack([R.canonical(v, 8, False), R.canonical(v, 8, True), R.canonical(v[::-1], 8, True)], -1)[None]
    for depth in (8, 10):
        for got, want in zip(R.planes(slot, depth), Y8.planes_from_triples(t, depth)):
            assert np.array_equal(got, want)
    assert np.array_equal(R.plane_y(R.canonical(v, 8, False), 10), (2046 * v + 255) // 510)
    assert np.array_equal(R.plane_c(R.canonical(v, 8, True), 10), np.clip(512 + (2046 * (v - 128) + 255) // 510, 0, 1023))     # (0 gives -2 before the clamp)


@pytest.mark.parametrize('bits', range(8, 17))
def test_neutral_chroma_gives_half_at_both_depths(bits):
    for narrow in (False, True):
        w = R.canonical(1 << (bits - 1), bits, True, narrow)
        assert w == 32768
        assert R.plane_c(w, 8) == 128 and R.plane_c(w, 10) == 512


def test_narrow_range_values_worked_out_by_hand():
    # Y: (2 * 65535 * (v - 64) + 876) // 1752: 64 -> 876 // 1752 = 0; 940 -> (114817320 + 876) // 1752 = 65535 (114818196 = 65535 * 1752 + 876)
    assert [int(R.canonical(v, 10, False, True)) for v in (64, 940)] == [0, 65535]
    # C: 32768 + (2 * 65535 * (v - 512) + 896) // 1792: 64 -> 32768 + (-58719360 + 896) // 1792 = 32768 - 32767 = 1; 512 -> 32768 + 0;
    # 960 -> 32768 + (58719360 + 896) // 1792 = 32768 + 32768 = 65536, clamped to 65535
    assert [int(R.canonical(v, 10, True, True)) for v in (64, 512, 960)] == [1, 32768, 65535]
    # below black and above white clamp
    assert int(R.canonical(0, 10, False, True)) == 0 and int(R.canonical(1023, 10, False, True)) == M
    assert int(R.canonical(0, 10, True, True)) == 0 and int(R.canonical(1023, 10, True, True)) == M


def test_full_range_values_worked_out_by_hand():
    # 10 bits: Y 1 -> (131070 + 1023) // 2046 = 64; 1023 -> 65535; C 0 -> 32768 + (-67107840 + 1023) // 2046 = 32768 - 32799 < 0 -> 0; 1023 -> 32768 + 32735 = 65503
    assert [int(R.canonical(v, 10, False)) for v in (0, 1, 1023)] == [0, 64, M]
    assert [int(R.canonical(v, 10, True)) for v in (0, 512, 1023)] == [0, 32768, 65503]
    # 16 bits pass unchanged
    v = np.arange(65536)
    assert np.array_equal(R.canonical(v, 16, False), v) and np.array_equal(R.canonical(v, 16, True), v)


def test_samples_are_reduced_to_their_bits_first():
    assert int(R.reduce(0xFFC0, 10, True)) == 1023 and int(R.reduce(0xFC00 | 5, 10, False)) == 5 and int(R.reduce(0xABCD, 16, True)) == 0xABCD
    assert int(R.ingest(0xFFC0, 10, False, True)) == M and int(R.ingest(0xFC00 | 512, 10, True, False)) == 32768


def test_the_two_stage_map_is_the_contract_not_one_direct_rounding():
    """for 14 and 15 bits into depth 10 the two roundings differ from a single one at 54 of 16384 and 128 of 32768 luma values; at every other bit count, and
    at depth 8, they agree everywhere"""
    for bits in range(8, 17):
        v = np.arange(1 << bits)
        P = (1 << bits) - 1
        differ = [int((R.plane_y(R.canonical(v, bits, False), bd) != (2 * ((1 << bd) - 1) * v + P) // (2 * P)).sum()) for bd in (8, 10)]
        assert differ == [0, {14: 54, 15: 128}.get(bits, 0)], (bits, differ)


@pytest.mark.parametrize('hsub,vsub', ((2, 1), (2, 2)))
def test_upsampling_is_the_8_bit_restatement_before_the_final_shift(hsub, vsub):
    """on W = 257 v the sums before the shift are 257 times the 8-bit sums (rounding constant aside), so the 8-bit result follows from them exactly"""
    rng = np.random.default_rng(12)
    r_even, r_odd, s = R.upsample_rounding(vsub)
    for (w, h) in ((5, 4), (9, 5), (37, 23), (130, 3)):
        cw, ch = (w + hsub - 1) // hsub, (h + vsub - 1) // vsub
        c8 = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        sums = R.upsample(257 * c8.astype(np.int64), w, h, hsub, vsub, shift=False)
        r = np.where(np.arange(w) % 2 == 1, r_odd, r_even)[None, :]
        assert ((sums - r) % 257 == 0).all()
        assert np.array_equal((((sums - r) // 257) + r) >> s, Y8.upsample(c8, w, h, hsub, vsub))
        assert np.array_equal(R.upsample(257 * c8.astype(np.int64), w, h, hsub, vsub), sums >> s) and int(sums.max()) <= 16 * M


def test_narrow_planes_are_replicated_and_444_is_copied():
    c = np.array([[100, 60000], [7, 9]])
    for (w, h, hsub, vsub) in ((3, 4, 2, 2), (4, 2, 2, 1), (1, 2, 2, 1)):
        cw, ch = (w + hsub - 1) // hsub, (h + vsub - 1) // vsub
        got = R.upsample(c[:ch, :cw], w, h, hsub, vsub)
        assert np.array_equal(got, c[:ch, :cw][np.arange(h) // vsub][:, np.arange(w) // 2])
        assert np.array_equal(got.astype(np.uint8), Y8.upsample(c[:ch, :cw].astype(np.uint8), w, h, hsub, vsub))
    assert np.array_equal(R.upsample(c, 2, 2, 1, 1), c)


def test_expected_slot_maps_first_and_upsamples_second():
    """a subsampled 8-bit source does not give the 8-bit slot times 257: the rounding of the filter happens on 16-bit values"""
    rng = np.random.default_rng(13)
    w, h = 9, 6
    y, cb, cr = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (3, 5)), rng.integers(0, 256, (3, 5))
    slot = R.expected_slot(y | 0x5500, cb | 0x5500, cr | 0x5500, 8, 2, 2, 4)
    assert slot.shape == (h, w, 4) and slot.dtype == np.uint16 and (slot[..., 3] == M).all()
    assert np.array_equal(slot[..., 0], 257 * y)
    assert np.array_equal(slot[..., 1], R.upsample(R.canonical(cb, 8, True), w, h, 2, 2))
    assert not np.array_equal(slot[..., 1], 257 * Y8.upsample(cb.astype(np.uint8), w, h, 2, 2).astype(np.int64) - 128)
    msb = R.expected_slot(y << 8, cb << 8, cr << 8, 8, 2, 2, 3, msb_aligned=True)
    assert np.array_equal(msb, slot[..., :3])
