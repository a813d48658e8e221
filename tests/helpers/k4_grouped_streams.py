"""Record streams aimed at the entropy kernel's grouped adapters (k4_adapt_sb of cavif_rs_amd/csrc/tile_entropy.h: an adapter wave's four 16-lane groups adapt
four CDF rows in one step) -- test infrastructure only.  Built from tests/helpers/range_coder_ref.py's records, tables and Stream; run through
tests/helpers/k4_harness.py.  What each stream is for stands at its generator; tests/test_k4_grouped_adapters.py asserts what they reach."""
import random

from tests.helpers import range_coder_ref as R

D = R.DEFS


def row_group(row):
    """tile_entropy.h k4_row_group: the 16-lane group of the row's owner wave (R.row_owner) that adapts it."""
    return (((row // 5 + row // 210) >> 1) + row // 210) & 3


def rows_of(na, wave, group):
    """The real table's (offset, alphabet size) rows that adapter `wave` of `na` adapts in `group`."""
    return [(off, ns) for off, ns in R.ROWS if R.row_owner(off, na) == wave and row_group(off) == group]


def _chunks(n, size):
    """buffer sizes: n records in buffers of `size`, the rest in a last one"""
    return [size] * (n // size) + ([n % size] if n % size else [])


def _sym(rnd, row):
    off, ns = row
    return R.rec_sym(off, rnd.randrange(ns), ns)


def _pick(rnd, rows, prefer=4):
    """a row of the list, alphabets of at least `prefer` symbols first (more entries to get wrong)"""
    big = [r for r in rows if r[1] >= prefer]
    return rnd.choice(big or rows)


def rotation_streams():
    """1. Rows of all four groups of one wave in rotation (ABCDABCD...) over buffers of 1, 15, 16, 17, 63, 64, 65 and 129 records: the groups run out at different
    steps, chunks end in the middle of a rotation."""
    out = []
    rnd = random.Random(7101)
    for na in (2, 4):
        for wave in range(na):
            four = [_pick(rnd, rows_of(na, wave, g)) for g in range(4)]
            splits = [1, 15, 16, 17, 63, 64, 65, 129] * 3
            recs = [_sym(rnd, four[k % 4]) for k in range(sum(splits))]
            s = R.Stream('rotation_na%d_wave%d' % (na, wave), recs, splits=splits)
            s.props['pairs'] = {(na, wave, g) for g in range(4)}
            out.append(s)
    return out


def same_group_streams():
    """2. Several rows of ONE group, interleaved with a row of another group of the same wave: the order across rows inside a group, the change of row on
    every step of a group."""
    out = []
    rnd = random.Random(7202)
    for na in (2, 4):
        for wave in range(na):
            g = (wave + na) & 3
            mates = rows_of(na, wave, g)
            rnd.shuffle(mates)
            mates = mates[:4]
            other = _pick(rnd, rows_of(na, wave, (g + 1) & 3))
            assert len(mates) >= 3, (na, wave, g)
            recs = []
            for k in range(1800):
                recs.append(_sym(rnd, other) if k % 3 == 2 else _sym(rnd, mates[rnd.randrange(len(mates)) if k % 7 else k % len(mates)]))
            s = R.Stream('same_group_na%d_wave%d' % (na, wave), recs, splits=_chunks(len(recs), 257))
            s.props['pairs'] = {(na, wave, g), (na, wave, (g + 1) & 3)}
            out.append(s)
    return out


def chunk_streams():
    """3. One chunk of 64 records of one row (one group runs 64 steps, three run none); one chunk of 64 different rows."""
    rnd = random.Random(7303)
    row = (D['CDF_COEFF_BASE'] + 21 * D['CDF_COEFF_BASE_STRIDE'], 4)
    one = R.Stream('chunk_64_of_one_row', [_sym(rnd, row) for _ in range(64)], splits=[64])
    rows = list(R.ROWS)
    rnd.shuffle(rows)
    many = R.Stream('chunk_64_different_rows', [_sym(rnd, r) for r in rows[:64]], splits=[64])
    more = R.Stream('chunks_64_different_rows_x8', [_sym(rnd, r) for r in rows[64:64 + 512]], splits=[64] * 8)
    return [one, many, more]


def wide_alphabet_streams():
    """4. Alphabets of 15 and 16 symbols (a row of 16 entries + the counter: one more than a group has lanes) packed so that the next row starts right behind the
    counter: a store one entry too wide, or a counter in the wrong place, shows in the final table.  s = 0, nsyms - 1 and values between."""
    rnd = random.Random(7404)
    cdf = R.default_table()
    pos, rows = D['CDF_EOB_PT_16'], []
    for ns in (16, 15, 16, 16, 15, 15, 16, 15):
        assert pos + ns + 1 < R.CDF_TOTAL
        vals = sorted((rnd.randrange(1, 32768) for _ in range(ns - 1)), reverse=True)
        cdf[pos:pos + ns + 1] = vals + [0, rnd.choice((0, 15, 16, 31, 32))]
        rows.append((pos, ns))
        pos += ns + 1
    cdf[pos] = 0x5A5A                                          # the entry behind the last counter: nobody's
    recs = []
    for k in range(2400):
        off, ns = rows[k % len(rows)] if k % 5 else rnd.choice(rows)
        recs.append(R.rec_sym(off, (0, ns - 1, ns // 2, rnd.randrange(ns))[(k // len(rows)) % 4], ns))
    s = R.Stream('alphabets_15_16_packed', recs, cdf=cdf, splits=_chunks(len(recs), 333))
    s.props['rows'] = rows
    s.props['behind'] = pos
    return [s]


def edge_streams():
    """5. Partition-edge bools (has_cols 0 and 1) alternating with adaptive symbols of the SAME partition row inside a chunk: the bool's bound is the row's state at
    that point of the coding order."""
    rnd = random.Random(7505)
    out = []
    recs = []
    for k in range(1536):
        row = R.PEDGE_ROWS[(k // 192) % len(R.PEDGE_ROWS)]
        recs.append(R.rec_pedge(row, (k >> 1) & 1) if k & 1 else R.rec_sym(row, rnd.randrange(10), 10))
    out.append(R.Stream('edges_alternate_one_row', recs, splits=_chunks(len(recs), 448)))
    recs = []
    for k in range(1500):                                       # three partition rows at once, edges and symbols at random, other rows between
        x = rnd.random()
        row = rnd.choice(R.PEDGE_ROWS[:3])
        recs.append(R.rec_pedge(row, rnd.randrange(2)) if x < 0.35 else (R.rec_sym(row, rnd.randrange(10), 10) if x < 0.8 else _sym(rnd, rnd.choice(R.ROWS))))
    out.append(R.Stream('edges_three_rows_mixed', recs, splits=_chunks(len(recs), 200)))
    return out


def mixed_streams():
    """6. Records of every adapter, literal bits and ready bounds mixed: what is not the wave's own comes out untouched (the coder codes them as they are)."""
    rnd = random.Random(7606)
    bounds = (R.rec_bounds(400, 0, 0), R.rec_bounds(512, 256, 1), R.rec_bounds(256, 0, 0), R.rec_bounds(2, 1, 0), R.rec_bounds(512, 300, 3))
    recs = []
    for _ in range(3000):
        x = rnd.random()
        recs.append(_sym(rnd, rnd.choice(R.ROWS)) if x < 0.5 else (R.rec_bit(rnd.randrange(2)) if x < 0.75 else rnd.choice(bounds)))
    splits, left = [], len(recs)
    while left:
        c = min(left, rnd.choice((1, 15, 16, 17, 63, 64, 65, 129, 500)))
        splits.append(c)
        left -= c
    return [R.Stream('mixed_owners_literals_bounds', recs, splits=splits)]


def all_streams():
    return rotation_streams() + same_group_streams() + chunk_streams() + wide_alphabet_streams() + edge_streams() + mixed_streams()


def main(argv):
    """python -m tests.helpers.k4_grouped_streams LIB NA: every stream through LIB, one JSON line per stream (a separate process, so that the emulator reads the
    environment it is started with, MI_EMU_REVERSE among it) -- tests.helpers.k4_harness.main for these streams."""
    import json
    from tests.helpers import k4_harness as H
    lib, na = argv[0], int(argv[1])
    streams = all_streams()
    for s, r in zip(streams, H.run(lib, na, streams)):
        print(json.dumps({'name': s.name, 'length': r.length, 'data': r.data.hex() if r.data is not None else None, 'units': r.units, 'nunits': r.nunits,
                          'cdf': r.cdf, 'guards_ok': r.guards_ok}))


if __name__ == '__main__':
    import sys
    main(sys.argv[1:])
