"""Cases for the tile search's block heads, partition walker and area copies (tests/test_k1_roundtrips.py through the SIMT emulator, tests/test_gpu_k1_roundtrips.py on
the GPU): small pictures on which the walker meets every situation its memory traffic depends on -- a superblock with no neighbour, partial superblocks (forced
splits at the right and bottom edge; above-right / below-left missing at picture and tile borders), both walkers, 8- and 10-bit, 4:0:0 (the area copy without
chroma planes), two tiles, a second pricing pass with per-tile rate tables -- and on which the search picks trees of many shapes.  TEST INFRASTRUCTURE."""
import numpy as np

# (name, width, height, bit depth, speed, quantizer, 4:0:0, picture kind, configuration overrides by the oracle's field names)
CASES = [
    ('one superblock, no neighbour', 64, 64, 8, 4, 100, False, 0, {}),
    ('partial superblocks 80x48', 80, 48, 10, 4, 110, False, 1, {}),
    ('partial superblocks 136x72', 136, 72, 8, 4, 90, False, 2, {}),
    ('top-down walker 200x120', 200, 120, 10, 4, 100, False, 3, {}),
    ('bottom-up walker 200x120', 200, 120, 8, 2, 100, False, 0, {}),
    ('4:0:0 136x72', 136, 72, 10, 4, 100, True, 1, {}),
    ('two tiles 256x128', 256, 128, 8, 4, 110, False, 2, dict(tiles_override=2, min_tile_size=128)),
    ('two pricing passes 136x72', 136, 72, 8, 4, 100, False, 3, dict(rdo_passes=2)),
]
BS_4X4, BS_8X8, BS_16X16, BS_4X8, BS_8X4 = 0, 1, 2, 5, 6


def picture(w, h, bd, mono, kind):
    """Smooth areas, texture and edges side by side (the style of predict_cases._walker_picture), so that the search picks blocks of many sizes; chroma planes follow
    the luma structure with other phases."""
    yy, xx = np.mgrid[0:h, 0:w]
    rs = np.random.RandomState(11 + kind)
    out = []
    for pl in range(1 if mono else 3):
        p = 128 + 60 * np.sin((xx + 5 * pl) / (9.0 + kind)) + 50 * np.cos((yy + 3 * pl) / 7.0)
        p += np.where((xx // 32 + yy // 32 + kind + pl) % 2 == 0, rs.randint(-70, 71, (h, w)), rs.randint(-4, 5, (h, w)))
        p += np.where(((xx + 2 * yy) // 5) % 7 == 0, 90, 0) * ((xx // 16 + kind) % 3 == 0)
        p += np.where((yy // 4) % 2 == 0, 40, -40) * ((xx // 8 + yy // 8 + kind) % 5 == 0)          # horizontal stripes inside 8x8 nodes: 8x4 blocks pay
        p += np.where((xx // 4) % 2 == 0, 40, -40) * ((xx // 8 + yy // 8 + kind) % 5 == 2)          # vertical ones: 4x8 blocks
        out.append((np.clip(p, 0, 255).astype(np.uint16) << (bd - 8)).astype(np.uint16))
    return out


def oracle_run(oracle, case):
    name, w, h, bd, speed, q, mono, kind, over = case
    pl = picture(w, h, bd, mono, kind)
    cfg = oracle.make_config(w, h, bd, mono, q, speed, **over)
    return pl, oracle.encode_planes(cfg, pl)


def product_kwargs(case):
    name, w, h, bd, speed, q, mono, kind, over = case
    kw = {k: v for k, v in over.items() if k != 'tiles_override'}       # (the overrides used here carry the same names on both sides)
    return dict(bit_depth=bd, quantizer=q, speed=speed, mono=mono, tiles=over.get('tiles_override', 0), **kw)


def shapes_reached(results):
    """What the oracle's final trees hold over the case set: the block-size codes present, and the winners of the 8x8 nodes (by the code at the node's first cell:
    8x8 = NONE, 4x4 = SPLIT, 8x4 = HORZ, 4x8 = VERT)."""
    codes, winners = set(), set()
    for r in results:
        b = r['m_bsize']
        codes |= set(int(v) for v in np.unique(b))
        node = b[0:b.shape[0] - 1:2, 0:b.shape[1] - 1:2]             # nodes that lie inside the picture
        for code, won in ((BS_8X8, 'NONE'), (BS_4X4, 'SPLIT'), (BS_8X4, 'HORZ'), (BS_4X8, 'VERT')):
            if (node == code).any():
                winners.add(won)
    return codes, winners


def check_inputs(results):
    """The condition on the inputs, from the oracle alone: every block shape of the 16x16 class occurs, and each of NONE, SPLIT, HORZ, VERT wins an 8x8 node."""
    codes, winners = shapes_reached(results)
    assert {BS_4X4, BS_8X8, BS_16X16, BS_4X8, BS_8X4} <= codes, 'block-size codes reached: %s' % sorted(codes)
    assert winners == {'NONE', 'SPLIT', 'HORZ', 'VERT'}, '8x8 nodes were won by %s only' % sorted(winners)
