"""The cases of tests/test_loopfilter_kernels.py: frames and rows built so that the filter stages' hard cases are reached (measured on the reference,
`reach()`), their reference results (tests/helpers/loopfilter_ref.py, computed once per process), and the comparison of a harness run with them
(`check_group`).  Everything is compared exactly.  Test infrastructure only."""
import functools

import numpy as np

from tests.helpers import filters_harness as H
from tests.helpers import loopfilter_ref as R

AC_Q = {8: (60, 66, 71), 10: (240, 264, 281)}                    # luma / U / V AC steps of a mid-range quantiser: only their ratio (the plane weights) matters
RDMULT = 5200
LR_COST = (922, 679, 853)                                          # ceil(-512 log2 p) of the default switchable-restoration CDF (9413, 22581, 32768)
GROUPS = ['deblock_search', 'deblock_pick', 'deblock_apply', 'table_edge', 'cdef', 'cdef_lists', 'table_cdef', 'lr', 'lr_decide', 'table_lr', 'launch']


def plane_weights(bd, np_):
    q = AC_Q[bd]
    return [((q[0] * q[0]) << 12) // (q[p] * q[p]) if p < np_ else 0 for p in range(3)]


class Case:
    def __init__(self, name, w, h, bd, np_, src, rec, fin=None, tx=None, bs=None, skip=None, oracle=True, **par):
        self.name, self.w, self.h, self.bd, self.np = name, w, h, bd, np_
        self.g = H.Geometry(w, h)
        z = np.zeros((self.g.mi_h, self.g.mi_stride), np.uint8)
        self.src, self.rec, self.fin = src, rec, fin
        self.tx, self.bs, self.skip = (z if tx is None else tx), (z if bs is None else bs), (z if skip is None else skip)
        self.oracle, self.par = oracle, par
        self.tune_psnr = par.get('tune_psnr', 0)
        self.act, self.svar8 = R.activity(self.g, bd, src[0], self.tune_psnr)
        self.wq = plane_weights(bd, np_)

    def frame(self, **over):
        par = dict(self.par)
        par.update(over)
        return H.Frame(self.w, self.h, self.bd, self.np, self.src, self.rec, self.tx, self.bs, self.skip, self.act, self.svar8, self.wq, fin=self.fin,
                       rdmult=RDMULT, lr_cost=LR_COST, **par)


def _diff(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return ['%s: shape %s, reference %s' % (name, got.shape, want.shape)]
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        return ['%s: %d entries differ, first at %s: %s, reference %s' % (name, len(bad), at, got[at], want[at])]
    return []


# ---------------------------------------------------------------- deblocking: maps and content
def build_maps(g, rects, seed):
    """(m_txsize, m_bsize): `rects` = (column, row, side in mi, block size code, transform size code) of the large blocks; every 8x8 area they leave is an 8x8
    block (8x8 or 4x4 transforms), four 4x4 blocks, two 4x8 or two 8x4 blocks, so that all of these meet each other in both orders and directions."""
    rng = np.random.default_rng(seed)
    tx = np.zeros((g.mi_h, g.mi_stride), np.uint8)
    bs = np.zeros((g.mi_h, g.mi_stride), np.uint8)
    done = np.zeros((g.mi_h, g.mi_stride), bool)
    for (c, r, n, b, t) in rects:
        assert c % n == 0 and r % n == 0 and not done[r:r + n, c:c + n].any()
        tx[r:r + n, c:c + n], bs[r:r + n, c:c + n], done[r:r + n, c:c + n] = t, b, True
    for r in range(0, g.mi_rows, 2):
        for c in range(0, g.mi_cols, 2):
            if not done[r, c]:
                b, t = [(1, 1), (1, 0), (0, 0), (5, 5), (6, 6)][int(rng.integers(0, 5))]
                tx[r:r + 2, c:c + 2], bs[r:r + 2, c:c + 2] = t, b
    return tx, bs


MAPS = {(136, 72): [(0, 0, 16, 4, 4), (16, 0, 8, 3, 3), (24, 0, 4, 2, 2), (28, 0, 4, 2, 1), (24, 4, 4, 2, 2), (28, 4, 4, 2, 2), (20, 8, 4, 2, 2), (20, 12, 4, 2, 2), (16, 12, 4, 2, 2),
                    (24, 8, 8, 3, 3)],
        (70, 38): [(0, 0, 8, 3, 2), (8, 0, 4, 2, 2), (12, 0, 4, 2, 1), (8, 4, 4, 2, 2)],
        (66, 34): [(0, 0, 8, 3, 2), (8, 0, 4, 2, 2), (12, 0, 4, 2, 1), (8, 4, 4, 2, 2)],
        (24, 16): [(0, 0, 4, 2, 2)]}
LINE_KINDS = 8


def craft_line(rng, fsz, plane, bd, kind):
    """16 samples p7 .. p0, q0 .. q7 around an edge that aim at one of the filter's decisions."""
    s8 = bd - 8
    one, mx = 1 << s8, (1 << bd) - 1
    low = lambda n=None: rng.integers(0, one, n)                  # at depth 10: the two low bits
    p, q = np.zeros(8, np.int64), np.zeros(8, np.int64)
    base = int(rng.integers(30, 220)) << s8
    if kind == 0:                                                 # smooth
        p[:] = base + rng.integers(-2 * one, 2 * one + 1, 8)
        q[:] = base + rng.integers(-2 * one, 2 * one + 1, 8)
    elif kind == 1:                                               # a step between two flat sides
        p[:] = base + low(8)
        q[:] = base + int(rng.integers(-45, 46)) * one + low(8)
    elif kind == 2:                                               # one mask term at its limit, or one step past it, for a level
        lvl = int(rng.integers(1, 64))
        term, over = int(rng.integers(0, 7)), int(rng.integers(0, 2)) * int(rng.integers(1, one + 1))
        sg = 1 if base < (128 << s8) else -1
        p[:] = q[:] = base
        d = (lvl << s8) + over
        if term == 0:
            p[1:] = base + sg * d
        elif term == 1:
            q[1:] = base + sg * d
        elif term == 2:
            p[2:] = base + sg * d
        elif term == 3:
            q[2:] = base + sg * d
        elif term == 4:
            p[3:] = base + sg * d
        elif term == 5:
            q[3:] = base + sg * d
        else:                                                     # |p0 - q0| * 2 + |p1 - q1| / 2 against blimit = 3 lvl + 4
            want, d = ((3 * lvl + 4) << s8) + over, 0
            while 2 * d + d // 2 < want:                          # a plain step d: |p0 - q0| = |p1 - q1| = d
                d += 1
            q[:] = base + sg * d
    elif kind == 3:                                               # flat / flat2: every sample within one step of p0, one of them exactly at or just past it
        p[:] = base + rng.integers(-one, one + 1, 8)
        q[:] = base + rng.integers(-one, one + 1, 8)
        p[0] = base
        q[0] = base + int(rng.integers(-one, one + 1))
        i, over = int(rng.integers(1, 7)), int(rng.integers(0, 2))
        if rng.integers(0, 2):
            p[i] = p[0] + (one + over) * (1 if rng.integers(0, 2) else -1)
        else:
            q[i] = q[0] + (one + over) * (1 if rng.integers(0, 2) else -1)
    elif kind == 4:                                               # high edge variance: |p1 - p0| or |q1 - q0| at a threshold or one past it
        t, over = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        p[:] = base
        q[:] = base + int(rng.integers(-8, 9)) * one
        if rng.integers(0, 2):
            p[1:] = p[0] + ((t << s8) + over) * (1 if rng.integers(0, 2) else -1)
        else:
            q[1:] = q[0] + ((t << s8) + over) * (1 if rng.integers(0, 2) else -1)
    elif kind == 5:                                               # the narrow filter's clamps: samples at the ends of the range
        recipe = int(rng.integers(0, 4))
        a = [[2, 60, 0, 0], [0, 0, 2, 60], [0, 0, 3, 3 - int(rng.integers(0, 4))], [3, 3 - int(rng.integers(0, 4)), 0, 0]][recipe]      # p0, p1, q0, q1 in 8-bit steps
        v = np.array(a, np.int64) * one + low(4) * int(rng.integers(0, 2))
        if rng.integers(0, 2):
            v = mx - v
        p[0], p[1:], q[0], q[1:] = v[0], v[1], v[2], v[3]
    elif kind == 6:
        p[:] = q[:] = 0 if rng.integers(0, 2) else mx
    else:                                                         # a wide step with both sides noisy: masks off at low levels, on at high ones
        p[:] = base + rng.integers(-6 * one, 6 * one + 1, 8)
        q[:] = base + int(rng.integers(-30, 31)) * one + rng.integers(-6 * one, 6 * one + 1, 8)
    return np.clip(np.concatenate([p[::-1], q]), 0, mx)


def deblock_content(g, bd, np_, tx, bs, orient, seed):
    """Planes whose every edge line of pass `orient` is a crafted line (the other pass sees what that leaves); the source is the reconstruction plus noise."""
    rng = np.random.default_rng(seed)
    s8, mx = bd - 8, (1 << bd) - 1
    rec, src = [], []
    for plane in range(np_):
        a = (np.repeat(np.repeat(rng.integers(40, 200, (g.ph // 8, g.pw // 8)), 8, 0), 8, 1) << s8) + rng.integers(0, 3 << s8, (g.ph, g.pw))
        k = plane
        for (x, y, fsz) in R.edge_lines(g, plane, orient, tx, bs):
            half = fsz // 2
            for i in range(4):
                line = craft_line(rng, fsz, plane, bd, k % LINE_KINDS)[8 - half:8 + half]
                k += 1
                if orient == 0:
                    a[y + i, x - half:x + half] = line
                else:
                    a[y - half:y + half, x + i] = line
        rec.append(a.astype(np.uint16))
        src.append(np.clip(a + rng.integers(-6 << s8, (6 << s8) + 1, a.shape), 0, mx).astype(np.uint16))
    return src, rec


@functools.lru_cache(None)
def deblock_cases():
    out = []
    for (w, h, bd, np_, orient) in ((136, 72, 8, 3, 0), (136, 72, 10, 3, 1), (136, 72, 10, 1, 0), (70, 38, 10, 3, 0), (70, 38, 8, 3, 1), (70, 38, 8, 1, 0),
                                     (66, 34, 8, 3, 0), (66, 34, 10, 3, 1)):       # 66 x 34: the last mi column and row start at x = 68 >= w, y = 36 >= h -- their edges are dropped
        g = H.Geometry(w, h)
        tx, bs = build_maps(g, MAPS[(w, h)], seed=w + bd)
        src, rec = deblock_content(g, bd, np_, tx, bs, orient, seed=w * 7 + bd + np_)
        out.append(Case('dbk_%dx%d_bd%d_np%d_%s' % (w, h, bd, np_, 'vh'[orient]), w, h, bd, np_, src, rec, tx=tx, bs=bs))
    return out


@functools.lru_cache(None)
def deblock_ref(name):
    c = {c.name: c for c in deblock_cases()}[name]
    stats = {}
    t = R.deblock_tallies(c.g, c.bd, c.np, c.src, c.rec, c.tx, c.bs, stats)
    lv = R.pick_levels(t, c.np)
    rec0 = R.deblock_pass(c.g, c.bd, c.np, c.rec, c.tx, c.bs, lv, 0, 0)
    rec1 = R.deblock_pass(c.g, c.bd, c.np, rec0, c.tx, c.bs, lv, 0, 1)
    return dict(tally=t, levels=lv, rec0=rec0, rec1=rec1, stats=stats)


def _frame_common(f, name):
    out = []
    if f.guard_damage:
        out.append('%s: %d guard bytes changed' % (name, f.guard_damage))
    return out


def check_deblock_search(lib):
    for c in deblock_cases():
        ref = deblock_ref(c.name)
        f = H.run(lib, [c.frame()], H.DEBLOCK)[0]
        pr = _frame_common(f, c.name) + _diff('tallies', f.tallies()[:c.np], ref['tally'][:c.np])
        pr += _diff('lf_level', f.lf_level_out, ref['levels']) + _diff('lf_out', f.lf_out[:4], ref['levels'])
        for p in range(c.np):
            pr += _diff('rec after pass 0, plane %d' % p, f.rec_p0[p], ref['rec0'][p]) + _diff('rec after pass 1, plane %d' % p, f.rec[p], ref['rec1'][p])
            pr += _diff('src plane %d' % p, f.src[p], c.src[p])
        if not (all((a == H.SENT16).all() for a in f.fin + f.lrp) and (f.cdef_idx == H.SENT8).all() and (f.lf_out[4:] == np.int32(H.SENT32)).all()):
            pr.append('a buffer deblocking does not own changed')
        yield c.name, pr


# the pick on written tallies: name -> (tallies [3][2][64] as sparse {(plane, pass, level): value}, np, fast_deblock, lf_level in, expected levels)
def pick_cases():
    return [('tie_lowest_wins', {(0, 0, 9): -50, (0, 0, 30): -50, (0, 1, 40): -7, (0, 1, 41): -7, (1, 0, 5): -3, (1, 1, 5): -3, (1, 0, 6): -6, (2, 1, 20): -1, (2, 0, 21): -1}, 3, 0, (0, 0, 0, 0)),
            ('all_non_negative', {(0, 0, 3): 5, (0, 1, 63): 1, (1, 0, 7): 9, (2, 1, 1): 0}, 3, 0, (7, 7, 7, 7)),
            ('chroma_forced_to_0', {(0, 0, 10): 4, (1, 0, 12): -100, (1, 1, 12): -100, (2, 0, 33): -5}, 3, 0, (0, 0, 0, 0)),
            ('minima_at_1_and_63', {(0, 0, 1): -9, (0, 0, 2): -8, (0, 1, 63): -9, (0, 1, 62): -8, (1, 0, 1): -4, (1, 1, 1): 1, (2, 0, 63): 2, (2, 1, 63): -3}, 3, 0, (0, 0, 0, 0)),
            ('chroma_sum_of_passes', {(0, 0, 20): -1, (1, 0, 10): -10, (1, 1, 10): 11, (1, 0, 11): 4, (1, 1, 11): -5, (2, 0, 50): -(1 << 40), (2, 1, 50): (1 << 40) - 1}, 3, 0, (0, 0, 0, 0)),
            ('mono', {(0, 0, 17): -2, (0, 1, 48): -2, (1, 0, 5): -99}, 1, 0, (0, 0, 0, 0)),
            ('fast_deblock_passes_through', {(0, 0, 9): -50, (1, 0, 3): -50}, 3, 1, (21, 22, 23, 24))]


def check_deblock_pick(lib):
    g = H.Geometry(24, 16)
    z = np.zeros((g.ph, g.pw), np.uint16)
    frames, want = [], []
    for name, sparse, np_, fast, lv_in in pick_cases():
        t = np.zeros((3, 2, 64), np.int64)
        for k, v in sparse.items():
            t[k] = v
        d = np.zeros((3, 2, 65), np.int64)
        d[:, :, :64] = np.diff(t, axis=2, prepend=0)
        d[:, :, 64] = -t[:, :, 63]
        c = Case(name, 24, 16, 8, np_, [z] * 3, [z] * 3)
        frames.append(c.frame(fast_deblock=fast, lf_level=lv_in, lf_tally=d))
        want.append(list(lv_in) if fast else R.pick_levels(t, np_))
    H.run(lib, frames, H.PICK)
    for (name, *_), f, lv in zip(pick_cases(), frames, want):
        yield 'pick_' + name, _frame_common(f, name) + _diff('lf_level', f.lf_level_out, lv) + _diff('lf_out', f.lf_out[:4], lv)


APPLY_LEVELS = [(l, 0) for l in (1, 15, 16, 17, 31, 32, 47, 48, 63)] + [(l, s) for l in (15, 32, 63) for s in (1, 4, 5, 7)]


def check_deblock_apply(lib):
    """The filter at given levels and sharpness (the product sets sharpness 0; the kernel reads the field).  Not expressible through the oracle's frame-level
    entry points: reference against kernel only."""
    for c in [c for c in deblock_cases() if c.name in ('dbk_70x38_bd10_np3_v', 'dbk_70x38_bd8_np3_h', 'dbk_66x34_bd8_np3_v')]:      # (66 x 34: edges at x >= w, y >= h dropped)
        frames = [c.frame(lf_level=(l, max(1, l - 3), l, max(1, l - 1)), lf_sharp=s) for l, s in APPLY_LEVELS]
        H.run(lib, frames, H.DBK0 | H.DBK1)
        for (l, s), f in zip(APPLY_LEVELS, frames):
            lv = (l, max(1, l - 3), l, max(1, l - 1))
            rec0 = R.deblock_pass(c.g, c.bd, c.np, c.rec, c.tx, c.bs, lv, s, 0)
            rec1 = R.deblock_pass(c.g, c.bd, c.np, rec0, c.tx, c.bs, lv, s, 1)
            pr = _frame_common(f, c.name)
            for p in range(c.np):
                pr += _diff('rec after pass 0, plane %d' % p, f.rec_p0[p], rec0[p]) + _diff('rec after pass 1, plane %d' % p, f.rec[p], rec1[p])
            yield 'apply_%s_level%d_sharp%d' % (c.name, l, s), pr


# ---------------------------------------------------------------- the table runner: filter_edge_sample_dev
@functools.lru_cache(None)
def edge_rows():
    """48 lines per (size, plane, depth, level): all kinds of crafted lines, the all-zero and the all-maximum line among them; a third of them at sharpness level % 8."""
    rng = np.random.default_rng(77)
    rows = []
    for fsz in (4, 8, 16):
        for plane in (0, 1):
            for bd in (8, 10):
                for lvl in range(1, 64):
                    for k in range(48):
                        line = craft_line(rng, fsz, plane, bd, k % LINE_KINDS)
                        if k == 46:
                            line[:] = 0
                        if k == 47:
                            line[:] = (1 << bd) - 1
                        half = fsz // 2
                        line[:8 - half] = 0
                        line[8 + half:] = 0
                        rows.append(list(line) + [fsz, plane, lvl, lvl % 8 if k % 3 == 0 else 0, bd])
    return np.array(rows, np.int64)


def edge_rows_ref(rows, stats=None):
    out = np.zeros((rows.shape[0], 16), np.int64)
    keys = rows[:, 16:21]
    for key in np.unique(keys, axis=0):
        sel = (keys == key).all(axis=1)
        fsz, plane, lvl, sharp, bd = (int(v) for v in key)
        out[sel] = R.filter_lines(rows[sel, :16], np.full(int(sel.sum()), fsz), plane, lvl, sharp, bd, stats if sharp == 0 and lvl else None)
    return out


def check_table_edge(lib):
    rows = edge_rows()
    got = H.table(lib, H.FT_EDGE, rows)[:, :16]
    yield 'table_filter_edge_sample', _diff('filtered lines (%d rows)' % len(rows), got, edge_rows_ref(rows))


# ---------------------------------------------------------------- CDEF
CDEF_KINDS = 16


def _stripe_index(d, i, j):
    """The line of direction d through (i, j): 7.15.2's partial-sum index."""
    return [i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j][d]


def cdef_block_content(rng, kind, bd):
    s8, mx = bd - 8, (1 << bd) - 1
    one = 1 << s8
    base = int(rng.integers(60, 190)) << s8
    ii, jj = np.mgrid[0:8, 0:8]
    if kind < 8:                                                   # stripes along direction `kind`
        k = np.vectorize(lambda i, j: _stripe_index(kind, i, j))(ii, jj)
        return base + (int(rng.integers(12, 50)) << s8) * ((k >> 1) & 1)
    if kind == 8:                                                  # flat: direction 0, variance 0
        return np.full((8, 8), base)
    if kind == 9:                                                  # two samples one 8-bit step off a flat block: variance 0, a direction all the same
        a = np.full((8, 8), base)
        a[2, 5] += one
        a[3, 5] += one
        return a
    if kind == 10:                                                 # full-swing stripes: var >> 6 at its cap
        d = 2 + 4 * (base & 1)
        k = np.vectorize(lambda i, j: _stripe_index(d, i, j))(ii, jj)
        return mx * ((k >> 2) & 1)
    if kind == 11:                                                 # faint stripes: var >> 6 of 0 and 1
        d = int(rng.integers(0, 8))
        k = np.vectorize(lambda i, j: _stripe_index(d, i, j))(ii, jj)
        return base + (int(rng.integers(1, 4)) << s8) * ((k >> 1) & 1)
    if kind == 12:                                                 # a cross: directions 2 and 6 cost the same, the order decides
        return base + (30 << s8) * ((ii == 3) | (jj == 3))
    if kind == 13:                                                 # differences in the low bits only (depth 10): flat to the direction search
        return base + rng.integers(0, one, (8, 8))
    if kind == 14:
        return rng.integers(0, mx + 1, (8, 8))
    return np.where((ii // 2 + jj // 2) & 1, mx, 0)                # 0 next to the maximum


def cdef_content(g, bd, np_, seed):
    """rec planes of per-block patterns (chroma: other blocks' patterns), strongly different samples wherever a tap must not be fetched, and a skip map with
    segment bits above bit 0."""
    rng = np.random.default_rng(seed)
    mx = (1 << bd) - 1
    rec = []
    for p in range(np_):
        a = np.where(rng.integers(0, 2, (g.ph, g.pw)) > 0, mx, 0)                     # outside the mi area: 0 / maximum noise
        n = 3 * p
        for r in range(0, g.mi_rows, 2):
            for c in range(0, g.mi_cols, 2):
                a[4 * r:4 * r + 8, 4 * c:4 * c + 8] = cdef_block_content(rng, n % CDEF_KINDS, bd)
                n += 1 + 4 * p
        rec.append(np.clip(a, 0, mx).astype(np.uint16))
    skip = np.zeros((g.mi_h, g.mi_stride), np.uint8)
    for r in range(0, g.mi_rows, 2):
        for c in range(0, g.mi_cols, 2):
            u = rng.random()
            cells = [0, 0, 0, 0] if u < 0.6 else ([1, 1, 1, 1] if u < 0.75 else list(rng.integers(0, 2, 4)))
            skip[r:r + 2, c:c + 2] = np.array(cells, np.uint8).reshape(2, 2) | (rng.integers(0, 8, (2, 2)) << 1).astype(np.uint8)
    return rec, skip


def _winner_source(c_rec, g, bd, np_, skip, winners):
    """A source that makes strength index winners[sb] the cheapest of superblock sb: the reconstruction filtered at that strength."""
    rng = np.random.default_rng(5)
    src = [a.copy() for a in c_rec]
    act = np.full((g.ph // 8, g.pw // 8), 16384, np.uint32)
    for sb, idx in enumerate(winners):
        code = H.CDEF_LIST[idx]
        _, fin, _ = R.cdef_frame(g, bd, np_, c_rec, c_rec, skip, act, act, [4096] * 3, 1, 1, 3, [code] * 8, [code] * 8, only_sb=sb)
        sr, sc = sb // g.sb_cols, sb % g.sb_cols
        for p in range(np_):
            src[p][64 * sr:64 * sr + 64, 64 * sc:64 * sc + 64] = fin[p][64 * sr:64 * sr + 64, 64 * sc:64 * sc + 64]
    for p in range(np_):                                           # a little noise, so that the other strengths' costs are not trivially ordered
        src[p] = np.clip(src[p].astype(np.int64) + (rng.integers(0, 40, src[p].shape) == 0), 0, (1 << bd) - 1).astype(np.uint16)
    return src


# Superblocks in which only blocks touching one side or one corner of the frame are filtered, on a noisy source: the strengths' costs lie close together, so what
# the search fetches for a tap outside the frame decides the index.  Samples beyond the mi area differ from their neighbours by about a strength, where constrain()
# passes most of a difference on (a far-off sample would be constrained away).  frame -> superblock -> (what, the 8x8 blocks as (mi row, mi column))
BORDER_BLOCKS = {'a': {0: ('top-left corner', [(0, 0)]), 1: ('top side', [(0, c) for c in range(18, 30, 2)]), 2: ('top-right corner', [(0, 32)]),
                       4: ('bottom side', [(16, c) for c in range(18, 30, 2)]), 3: ('psychovisual', [(16, c) for c in range(2, 14, 2)])},     # (3: see reach())
                 'b': {0: ('left side', [(r, 0) for r in range(2, 14, 2)]), 2: ('right side', [(r, 32) for r in range(2, 14, 2)]),
                       3: ('bottom-left corner', [(16, 0)]), 5: ('bottom-right corner', [(16, 32)])}}

BORDER_PAIR = (5, 6)                                              # the two strength indices whose costs are made to meet
BORDER_BLEND = {'a': {0: 573, 1: 509, 2: 643, 4: 511, 3: 527}, 'b': {0: 498, 2: 500, 3: 501, 5: 563}}      # how many 1024ths of a superblock's samples come from the second one


@functools.lru_cache(None)
def _border_base(which, bd, seed):
    g = H.Geometry(136, 72)
    rng = np.random.default_rng(seed)
    s8, mx = bd - 8, (1 << bd) - 1
    ii, jj = np.mgrid[0:8, 0:8]
    rec, src = [], []
    for p in range(3):
        a = (128 << s8) + rng.integers(-14 << s8, (14 << s8) + 1, (g.ph, g.pw))
        for r in range(0, g.mi_rows, 2):
            for c in range(0, g.mi_cols, 2):
                d = int(rng.integers(0, 8))
                k = np.vectorize(lambda i, j: _stripe_index(d, i, j))(ii, jj)
                a[4 * r:4 * r + 8, 4 * c:4 * c + 8] = (128 << s8) + (int(rng.integers(4, 9)) << s8) * ((k >> 1) & 1)
        src.append(np.clip(a + rng.integers(-1 << s8, (1 << s8) + 1, a.shape), 0, mx).astype(np.uint16))
        rec.append(np.clip(a + rng.integers(-5 << s8, (5 << s8) + 1, a.shape), 0, mx).astype(np.uint16))      # the reconstruction is the noisy one: filtering pays
    skip = (1 | (rng.integers(0, 8, (g.mi_h, g.mi_stride)) << 1)).astype(np.uint8)
    for what, blocks in BORDER_BLOCKS[which].values():
        for (r, c) in blocks:
            skip[r:r + 2, c:c + 2] &= 0xFE
    flat = np.full((g.ph // 8, g.pw // 8), 16384, np.uint32)
    fins = {sb: [R.cdef_frame(g, bd, 3, rec, rec, skip, flat, flat, [4096] * 3, 1, 1, 3, [H.CDEF_LIST[i]] * 8, [H.CDEF_LIST[i]] * 8, only_sb=sb)[1] for i in BORDER_PAIR]
            for sb in BORDER_BLOCKS[which]}
    order = {sb: np.random.default_rng(seed + sb).permutation(len(BORDER_BLOCKS[which][sb][1]) * 3 * 64) for sb in BORDER_BLOCKS[which]}
    return g, rec, src, skip, fins, order


def cdef_border_case(which, bd, seed, blend=None):
    """136 x 72, a noisy reconstruction of striped blocks.  In each listed superblock every source sample is the reconstruction filtered at one of the two
    strengths of BORDER_PAIR (by the reference, outside taps skipped): BORDER_BLEND 1024ths of the samples, in a fixed random order, at the second.  Both cost about
    the same and less than any other, so a few border samples filtered from a wrongly fetched tap change the winner (the reach test checks that on the reference,
    per side and corner; in one more superblock the psychovisual boost decides between the two)."""
    g, rec, src, skip, fins, order = _border_base(which, bd, seed)
    blend = blend or BORDER_BLEND[which]
    src = [a.copy() for a in src]
    for sb, (what, blocks) in BORDER_BLOCKS[which].items():
        second = (np.argsort(order[sb]) < (len(order[sb]) * blend[sb]) // 1024).reshape(len(blocks), 3, 8, 8)
        for n, (r, c) in enumerate(blocks):
            for p in range(3):
                x, y = fins[sb][0][p][4 * r:4 * r + 8, 4 * c:4 * c + 8], fins[sb][1][p][4 * r:4 * r + 8, 4 * c:4 * c + 8]
                src[p][4 * r:4 * r + 8, 4 * c:4 * c + 8] = np.where(second[n, p], y, x)
    return Case('cdef_border_%s_bd%d' % (which, bd), 136, 72, bd, 3, src, rec, skip=skip)


@functools.lru_cache(None)
def cdef_border_cases():
    return [cdef_border_case('a', 8, 101), cdef_border_case('b', 10, 102)]


@functools.lru_cache(None)
def cdef_cases():
    out = list(cdef_border_cases())
    for (w, h, bd, tune, winners) in ((136, 72, 8, 0, (1, 2, 3, 4, 5, 6)), (72, 40, 10, 0, (7, 0)), (136, 72, 10, 1, (6, 5, 4, 3, 2, 1)), (72, 40, 8, 1, (0, 7))):
        g = H.Geometry(w, h)
        rec, skip = cdef_content(g, bd, 3, seed=w + bd)
        out.append(Case('cdef_%dx%d_bd%d_tune%d' % (w, h, bd, tune), w, h, bd, 3, _winner_source(rec, g, bd, 3, skip, winners), rec, skip=skip, tune_psnr=tune))
    g = H.Geometry(72, 40)
    rng = np.random.default_rng(11)
    rec, skip = cdef_content(g, 8, 1, seed=3)
    skip[:, 16:18] |= 1                                            # the second superblock: every block skipped
    out.append(Case('cdef_72x40_mono_sb_all_skipped', 72, 40, 8, 1, [np.clip(rec[0].astype(np.int64) + rng.integers(-9, 10, rec[0].shape), 0, 255).astype(np.uint16)], rec, skip=skip))
    rec, skip = cdef_content(g, 10, 3, seed=4)
    src = [np.where(rng.integers(0, 3, a.shape) == 0, 1024, np.clip(a.astype(np.int64) + rng.integers(-30, 31, a.shape), 0, 1023)).astype(np.uint16) for a in rec]
    out.append(Case('cdef_72x40_bd10_source_1024', 72, 40, 10, 3, src, rec, skip=skip))
    out.append(Case('cdef_72x40_bd10_disabled', 72, 40, 10, 3, src, rec, skip=skip, enable_cdef=0))
    return out


@functools.lru_cache(None)
def cdef_list_cases():
    """All 64 (primary, secondary) codes: eight lists of eight, luma and chroma lists in opposite order, damping 3 and 6 -- at depths 8 and 10.  Not expressible
    through the oracle's frame-level entry point (fixed list, damping 3): reference against kernel only."""
    out = []
    g = H.Geometry(72, 40)
    for bd in (8, 10):
        rng = np.random.default_rng(bd)
        rec, skip = cdef_content(g, bd, 3, seed=20 + bd)
        src = [np.clip(a.astype(np.int64) + rng.integers(-12 << (bd - 8), (12 << (bd - 8)) + 1, a.shape), 0, (1 << bd) - 1).astype(np.uint16) for a in rec]
        for k in range(8):
            codes = list(range(8 * k, 8 * k + 8))
            out.append(Case('cdef_list%d_bd%d' % (k, bd), 72, 40, bd, 3, src, rec, skip=skip, oracle=False, tune_psnr=k & 1, cdef_y=codes, cdef_uv=codes[::-1],
                            cdef_damping=3 if k % 2 == 0 else 6))
    return out


@functools.lru_cache(None)
def cdef_ref(name):
    c = {c.name: c for c in cdef_cases() + cdef_list_cases()}[name]
    stats = {}
    idx, fin, costs = R.cdef_frame(c.g, c.bd, c.np, c.src, c.rec, c.skip, c.act, c.svar8, c.wq, c.tune_psnr, c.par.get('enable_cdef', 1), c.par.get('cdef_damping', 3),
                                   c.par.get('cdef_y', H.CDEF_LIST), c.par.get('cdef_uv', H.CDEF_LIST), stats)
    return dict(idx=idx, fin=fin, costs=costs, stats=stats)


def _check_cdef_frame(c, f):
    ref = cdef_ref(c.name)
    mw, mh = c.g.mi_cols * 4, c.g.mi_rows * 4
    pr = _frame_common(f, c.name) + _diff('cdef_idx', f.cdef_idx, ref['idx'])
    for p in range(c.np):
        pr += _diff('fin plane %d' % p, f.fin[p][:mh, :mw], ref['fin'][p][:mh, :mw]) + _diff('rec plane %d' % p, f.rec[p], c.rec[p])
        outside = f.fin[p].copy()
        outside[:mh, :mw] = H.SENT16
        if not (outside == H.SENT16).all() or not (f.lrp[p] == H.SENT16).all():
            pr.append('plane %d: fin outside the mi area, or lrp, changed' % p)
    return pr


def check_cdef(lib):
    for c in cdef_cases():
        yield c.name, _check_cdef_frame(c, H.run(lib, [c.frame()], H.CDEF)[0])


def check_cdef_lists(lib):
    cases = cdef_list_cases()
    for k in range(0, len(cases), 8):                              # the eight lists of a depth in one launch
        frames = H.run(lib, [c.frame() for c in cases[k:k + 8]], H.CDEF)
        for c, f in zip(cases[k:k + 8], frames):
            yield c.name, _check_cdef_frame(c, f)


@functools.lru_cache(None)
def cdef_rows():
    rng = np.random.default_rng(9)
    con = [(d, t, dmp) for t in (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 60, 63) for dmp in (2, 3, 4, 5, 6, 7, 8) for d in list(range(-70, 71)) + [-1023, -512, -255, 255, 512, 1023]]
    taps = []
    for n in range(6000):
        cs = int(rng.integers(0, 2)) * 2
        mx = (1 << (8 + cs)) - 1
        x = int(rng.integers(0, mx + 1))
        spread = int(rng.choice([3, 20, 200, 1023]))
        t = [int(v) for v in np.clip(x + rng.integers(-spread, spread + 1, 12), 0, mx)]
        if n % 50 == 0:
            x, t = (0, [mx] * 12) if n % 100 else (mx, [0] * 12)
        pri = int(rng.integers(0, 16)) << cs
        if n % 3 == 0:
            pri = (pri * int(rng.integers(4, 17)) + 8) >> 4        # a luma strength after the variance adjustment: any value
        sec = int(rng.choice([0, 1, 2, 4])) << cs
        taps.append([x] + t + [pri, sec, int(rng.integers(3, 7)) + cs - int(rng.integers(0, 2)), cs])
    return np.array(con, np.int64), np.array(taps, np.int64)


def check_table_cdef(lib):
    con, taps = cdef_rows()
    got = H.table(lib, H.FT_CONSTRAIN, con)[:, 0]
    yield 'table_constrain', _diff('constrain', got, [R.constrain(int(d), int(t), int(m)) for d, t, m in con])
    got = H.table(lib, H.FT_CDEF_TAPS, taps)
    want = [R.cdef_filter_sample(int(r[0]), [int(v) for v in r[1:13]], int(r[13]), int(r[14]), int(r[15]), int(r[16])) for r in taps]
    yield 'table_cdef_taps', _diff('cdef_apply_taps', got[:, 0], want) + _diff('cdef_finish(cdef_pri_sum + cdef_sec_sum)', got[:, 1], want)


# ---------------------------------------------------------------- loop restoration
def lr_plane(rng, g, bd, kind):
    """(fin, rec, src) of one plane; rec (the deblocked rows a stripe boundary takes) is unrelated to fin, so a row from the wrong plane shows."""
    mx = (1 << bd) - 1
    s8 = bd - 8
    yy, xx = np.mgrid[0:g.ph, 0:g.pw]
    if kind == 'random':
        fin = np.clip((np.repeat(np.repeat(rng.integers(30, 220, (g.ph // 4, g.pw // 4)), 4, 0), 4, 1) << s8) + rng.integers(-14 << s8, (14 << s8) + 1, (g.ph, g.pw)), 0, mx)
    elif kind == 'far':                                            # moderate noise (the filters smooth it) under a source far away: sums past 2^30
        fin = np.clip((128 << s8) + (xx << s8) // 2 + rng.integers(-18 << s8, (18 << s8) + 1, (g.ph, g.pw)), 0, mx)
    elif kind == 'flat':                                           # z == 0
        fin = np.full((g.ph, g.pw), 133 << s8)
    elif kind == 'checker':                                        # z >= 255 everywhere
        fin = np.where((yy + xx) & 1, mx, 0)
    else:                                                          # 'ramp' / 'equal': slopes that walk z through the table's upper end
        k = (12 + (yy // 2) % 48) << s8
        t = (xx * k) % (2 * mx)
        fin = np.where(t > mx, 2 * mx - t, t)
    rec = np.clip(mx - fin + rng.integers(-20 << s8, (20 << s8) + 1, fin.shape), 0, mx)
    src = fin if kind == 'equal' else mx - fin if kind == 'far' else np.clip(fin + rng.integers(-10 << s8, (10 << s8) + 1, fin.shape) + (rng.integers(0, 4, fin.shape) == 0) * (6 << s8), 0, mx)
    return fin.astype(np.uint16), rec.astype(np.uint16), src.astype(np.uint16)


LR_FRAMES = [(17, 9, 8, 3, 1, ('random', 'ramp', 'checker')), (95, 95, 10, 3, 0, ('random', 'checker', 'equal')), (96, 96, 8, 1, 1, ('ramp',)),
             (95, 120, 10, 1, 1, ('far',)), (130, 57, 8, 3, 0, ('checker', 'random', 'ramp')), (95, 120, 8, 3, 0, ('equal', 'random', 'flat')),
             (130, 57, 10, 1, 1, ('ramp',))]


@functools.lru_cache(None)
def lr_cases():
    out = []
    for (w, h, bd, np_, full, kinds) in LR_FRAMES:
        g = H.Geometry(w, h)
        rng = np.random.default_rng(w * 3 + h + bd)
        planes = [lr_plane(rng, g, bd, k) for k in kinds]
        out.append(Case('lr_%dx%d_bd%d_np%d_%s_%s' % (w, h, bd, np_, 'full' if full else 'reduced', '_'.join(kinds)), w, h, bd, np_, [p[2] for p in planes],
                        [p[1] for p in planes], fin=[p[0] for p in planes], enable_restoration=1, sgr_full=full))
    return out


@functools.lru_cache(None)
def lr_ref(name):
    c = {c.name: c for c in lr_cases()}[name]
    stats = {}
    args = (c.g, c.bd, c.np, c.src, c.rec, c.fin, c.act, c.wq, RDMULT, LR_COST, c.par['sgr_full'])
    cands = R.lr_search(*args, stats)
    types, sets, xqd, lrp = R.lr_decide(*args, cands, stats)
    return dict(cands=cands, types=types, sets=sets, xqd=xqd, lrp=lrp, stats=stats)


def _cands_of(f, np_, units, nsets):
    """[plane][unit][set index] = (cost, xq0, xq1) from the frame's LrCand array."""
    a = f.lr_cand.reshape(np_ * units, 16, 2)
    x = a[:, :, 1]
    xq0, xq1 = ((x & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000, x >> 32
    return [[[(int(a[p * units + u, s, 0]), int(xq0[p * units + u, s]), int(xq1[p * units + u, s])) for s in range(nsets)] for u in range(units)] for p in range(np_)]


def _check_lr_outputs(c, f, types, sets, xqd, lrp):
    pr = _diff('lr_type', f.lr_type, types) + _diff('lr_set', f.lr_set, sets) + _diff('lr_xqd', f.lr_xqd, xqd)
    for p in range(c.np):
        pr += _diff('lrp plane %d' % p, f.lrp[p][:c.h, :c.w], lrp[p][:c.h, :c.w])
        outside = f.lrp[p].copy()
        outside[:c.h, :c.w] = H.SENT16
        if not (outside == H.SENT16).all():
            pr.append('lrp plane %d changed outside w x h' % p)
        pr += _diff('fin plane %d' % p, f.fin[p], c.fin[p]) + _diff('rec plane %d' % p, f.rec[p], c.rec[p])
    return pr


def check_lr(lib):
    for c in lr_cases():
        ref = lr_ref(c.name)
        f = H.run(lib, [c.frame()], H.LR_SEARCH | H.LR)[0]
        nsets = 16 if c.par['sgr_full'] else 4
        pr = _frame_common(f, c.name) + _diff('LrCand (cost, xq0, xq1) per plane, unit, set', _cands_of(f, c.np, c.g.units, nsets), ref['cands'])
        yield c.name, pr + _check_lr_outputs(c, f, ref['types'], ref['sets'], ref['xqd'], ref['lrp'])


@functools.lru_cache(None)
def lr_decide_cases():
    """lr_kernel alone on written candidates, 19 units: every set applied once, weights at every clamp end, an exact tie with RESTORE_NONE, two equal sets."""
    base = {c.name: c for c in lr_cases()}
    picks = [(10, 0, 95), (14, 31, 95), (0, -96, -32), (1, 31, 95), (2, -96, 95), (3, 31, -32), (4, 5, 60), (5, -20, 95), (6, 31, 0), (7, -96, 70), (8, 0, 0), (9, 12, 90),
             (11, 0, -32), (12, 0, 95), (13, 0, 64), (15, -96, 95), ('tie', 3, 77), ('equal', 9, 50), ('tie', -96, 95)]
    out, k = [], 0
    for name, w, h in (('lr_96x96_bd8_np1_full_ramp', 96, 96), ('lr_130x57_bd8_np3_reduced_checker_random_ramp', 130, 57), ('lr_95x95_bd10_np3_reduced_random_checker_equal', 95, 95),
                       ('lr_95x120_bd8_np3_reduced_equal_random_flat', 95, 120)):
        c = base[name]
        n = c.g.units * c.np
        units = picks[k:k + n]
        k += n
        none = []
        for p in range(c.np):
            for ui in range(c.g.units):
                x0, x1, y0, y1 = R.unit_rect(w, h, ui // R.lr_units(w), ui % R.lr_units(w))
                sse = int(((c.fin[p][y0:y1, x0:x1].astype(np.int64) - c.src[p][y0:y1, x0:x1]) ** 2).sum())
                none.append(R.lr_cost_of(sse, R.lr_unit_act(c.g, c.act, (x0, x1, y0, y1)), c.wq[p], LR_COST[0], RDMULT))
        cands = []
        for (what, q0, q1), nc in zip(units, none):
            row = [(nc + 1000 + s, 1, 1) for s in range(16)]
            if what == 'tie':
                row[5] = (nc, q0, q1)
            elif what == 'equal':
                row[4], row[11] = (nc - 5, q0, q1), (nc - 5, q1, q0)
            else:
                row[what] = (nc - 1, q0, q1)
            cands.append(row)
        out.append((c, [cands[p * c.g.units:(p + 1) * c.g.units] for p in range(c.np)]))
    assert k == len(picks)
    return out


def check_lr_decide(lib):
    for c, cands in lr_decide_cases():
        packed = np.array([[[cost, (q0 & 0xFFFFFFFF) | (q1 << 32)] for (cost, q0, q1) in row] for per in cands for row in per], np.int64)
        f = H.run(lib, [c.frame(sgr_full=1, lr_cand=packed)], H.LR)[0]
        types, sets, xqd, lrp = R.lr_decide(c.g, c.bd, c.np, c.src, c.rec, c.fin, c.act, c.wq, RDMULT, LR_COST, 1, cands)
        yield 'decide_' + c.name, _frame_common(f, c.name) + _check_lr_outputs(c, f, types, sets, xqd, lrp) + _diff('lr_cand', f.lr_cand, packed.reshape(-1))


@functools.lru_cache(None)
def lr_rows():
    rng = np.random.default_rng(31)
    solve, ratio = [], []
    for n in range(4000):
        mag = int(rng.choice([8, 20, 29, 30, 31, 36, 44]))
        h00, h11 = int(rng.integers(1, 1 << mag)), int(rng.integers(1, 1 << mag))
        lim = int((h00 * h11) ** 0.5)
        mode = n % 5
        h01 = int(rng.integers(-lim // 2, lim // 2 + 1)) if mode < 3 else (lim + int(rng.integers(0, 3)) if mode == 3 else int(rng.integers(-3, 4)))   # mode 3: det <= 0 or barely above
        c0, c1 = int(rng.integers(-(1 << mag), 1 << mag)), int(rng.integers(-(1 << mag), 1 << mag))
        if n % 7 == 0:                                            # a ratio near +-4
            c0 = 4 * h00 + int(rng.integers(-2, 3))
        r0, r1 = [(2, 1), (2, 1), (0, 1), (2, 0)][n % 4]
        solve.append([h00, h11, h01, c0, c1, r0, r1])
    for n in range(3000):
        det = int(rng.integers(1, 1 << int(rng.choice([6, 20, 40, 53, 54, 55, 60]))))
        if det >= 1 << 54 and n % 2:
            det = (1 << 54) + int(rng.integers(0, 4))
        kind = n % 6
        num = [int(rng.integers(-5 * det, 5 * det + 1)), 4 * det, 4 * det - 1, -4 * det, -4 * det + 1, (2 * int(rng.integers(-400, 400)) + 1) * det // 256][kind]
        if abs(num) < 1 << 62:
            ratio.append([num, det])
    sub = [[v, lo, hi, ref] for (lo, hi, refs) in ((-96, 32, (-32, -96, 31, 0)), (-32, 96, (31, -32, 95, 40))) for ref in refs for v in range(lo, hi)]
    proj = [[cd, f0, f1, r0, r1, w0, w1, mx] for mx in (255, 1023) for cd in (0, 1, mx - 1, mx) for f0 in (0, 9, 16 * mx) for f1 in (0, 16 * mx - 5, 16 * mx)
            for (r0, r1) in ((2, 1), (0, 1), (2, 0)) for w0 in (-96, 0, 31) for w1 in (-32, 40, 95)]
    return [np.array(a, np.int64) for a in (solve, ratio, sub, proj)]


def check_table_lr(lib):
    solve, ratio, sub, proj = lr_rows()
    got = H.table(lib, H.FT_SGR_SOLVE, solve)[:, :2]
    yield 'table_lr_sgr_solve', _diff('xqd', got, [R.sgr_solve(*[int(v) for v in r]) for r in solve])
    got = H.table(lib, H.FT_RATIO, ratio)[:, 0]
    yield 'table_lr_ratio_q7', _diff('ratio', got, [R.ratio_q7(int(a), int(b)) for a, b in ratio])
    got = H.table(lib, H.FT_SUBEXP, sub)[:, :2]
    yield 'table_lr_subexp_code', _diff('(bit count, bit string)', got, [R.subexp_code(*[int(v) for v in r]) for r in sub])
    got = H.table(lib, H.FT_PROJECT, proj)[:, 0]
    yield 'table_lr_project', _diff('sample', got, [R.project(*[int(v) for v in r]) for r in proj])


# ---------------------------------------------------------------- the launch shape
def check_launch(lib):
    """One launch of all stages over a 136 x 72 frame, a 24 x 16 frame and an idle one: the small frame (whose workgroups beyond its own cells, superblocks and
    units return early) and the large one come out as when launched alone, the idle one is not touched."""
    big = deblock_cases()[0]
    g = H.Geometry(24, 16)
    rng = np.random.default_rng(2)
    tx, bs = build_maps(g, MAPS[(24, 16)], seed=1)
    src, rec = deblock_content(g, 8, 3, tx, bs, 0, seed=8)
    small = Case('small', 24, 16, 8, 3, src, rec, tx=tx, bs=bs, skip=(rng.integers(0, 4, (g.mi_h, g.mi_stride)) == 0).astype(np.uint8))
    stages = H.DEBLOCK | H.CDEF | H.LR_SEARCH | H.LR
    mk = lambda c, **kw: c.frame(enable_restoration=1, sgr_full=0, **kw)
    together = H.run(lib, [mk(big), mk(small), mk(big, active=0, lf_tally=np.full(6 * 65, H.SENT32 | (H.SENT32 << 32), np.int64))], stages)      # (the idle frame's tallies start as sentinels too)
    alone = [H.run(lib, [mk(big)], stages)[0], H.run(lib, [mk(small)], stages)[0]]
    for name, a, b in (('launch_large_frame', together[0], alone[0]), ('launch_small_frame', together[1], alone[1])):
        pr = _frame_common(a, name) + _frame_common(b, name + ' alone') + _diff('lf_level', a.lf_level_out, b.lf_level_out)
        for field in ('lf_tally', 'lf_out', 'cdef_idx', 'lr_cand', 'lr_type', 'lr_set', 'lr_xqd'):
            pr += _diff(field, getattr(a, field), getattr(b, field))
        for field in ('rec', 'rec_p0', 'fin', 'lrp'):
            for p in range(3):
                pr += _diff('%s plane %d' % (field, p), getattr(a, field)[p], getattr(b, field)[p])
        if not (a.lf_level_out[0] or a.lf_level_out[1]) or (a.cdef_idx == H.SENT8).any() or (a.lr_type == H.SENT8).any():
            pr.append('a stage did not run')
        yield name, pr
    idle = together[2]
    pr = _frame_common(idle, 'idle')
    if not idle.untouched() or idle.lf_level_out != [0, 0, 0, 0] or (idle.lr_cand != np.int64(H.SENT32 | (H.SENT32 << 32))).any() or any(_diff('rec', idle.rec[p], big.rec[p]) for p in range(3)):
        pr.append('the idle frame was touched')
    yield 'launch_idle_frame', pr


CHECKS = {'deblock_search': check_deblock_search, 'deblock_pick': check_deblock_pick, 'deblock_apply': check_deblock_apply, 'table_edge': check_table_edge,
          'cdef': check_cdef, 'cdef_lists': check_cdef_lists, 'table_cdef': check_table_cdef, 'lr': check_lr, 'lr_decide': check_lr_decide, 'table_lr': check_table_lr,
          'launch': check_launch}


def check_group(lib, group):
    return list(CHECKS[group](lib))


# ---------------------------------------------------------------- the oracle's stages on a case (av1o_test_loop_filters)
def oracle_run(L, c, stages):
    import ctypes as C
    fn = L.av1o_test_loop_filters
    fn.restype = C.c_int
    P = C.c_void_p
    fn.argtypes = [C.POINTER(C.c_int), C.c_int64] + [C.POINTER(P)] * 4 + [P] * 11
    g = c.g
    cp = lambda arrs: [np.ascontiguousarray(a).copy() for a in arrs]
    src, rec = cp(c.src), cp(c.rec)
    fin = cp(c.fin) if c.fin is not None else [np.zeros((g.ph, g.pw), np.uint16) for _ in range(c.np)]
    lrp = [np.zeros((g.ph, g.pw), np.uint16) for _ in range(c.np)]
    ptrs = lambda arrs: (P * 3)(*[a.ctypes.data for a in arrs] + [None] * (3 - len(arrs)))
    skip = np.ascontiguousarray(c.skip & 1)                       # the oracle keeps the segment id in a map of its own
    par = (C.c_int * 13)(c.w, c.h, c.bd, c.np, c.tune_psnr, c.par.get('fast_deblock', 0), c.par.get('enable_cdef', 1), c.par.get('enable_restoration', 0),
                         c.par.get('sgr_full', 0), *AC_Q[c.bd], stages)
    nlr = g.units * c.np
    tally, lv, idx = np.zeros((3, 2, 64), np.int64), np.zeros(4, np.int32), np.full(g.sb_rows * g.sb_cols, 99, np.int8)
    act, svar8 = np.zeros_like(c.act), np.zeros_like(c.svar8)
    lt, ls, lx = np.zeros(nlr, np.uint8), np.zeros(nlr, np.uint8), np.zeros(nlr * 2, np.int8)
    tx, bs = np.ascontiguousarray(c.tx), np.ascontiguousarray(c.bs)
    rc = fn(par, RDMULT, ptrs(src), ptrs(rec), ptrs(fin), ptrs(lrp), tx.ctypes.data, bs.ctypes.data, skip.ctypes.data, tally.ctypes.data, lv.ctypes.data, idx.ctypes.data,
            act.ctypes.data, svar8.ctypes.data, lt.ctypes.data, ls.ctypes.data, lx.ctypes.data)
    assert rc == 0
    return dict(rec=rec, fin=fin, lrp=lrp, tally=tally, levels=list(lv), idx=idx, act=act, svar8=svar8, types=lt, sets=ls, xqd=lx)


def reference_against_oracle(L, group):
    """(name, problems) for the cases of `group` that the oracle's frame-level entry points can express."""
    if group == 'deblock_search':
        for c in deblock_cases():
            ref, o = deblock_ref(c.name), oracle_run(L, c, 1)
            pr = _diff('tallies', o['tally'][:c.np], ref['tally'][:c.np]) + _diff('levels', o['levels'], ref['levels']) + _diff('act', o['act'], c.act) + _diff('svar8', o['svar8'], c.svar8)
            yield c.name, pr + [d for p in range(c.np) for d in _diff('deblocked plane %d' % p, o['rec'][p], ref['rec1'][p])]
    if group == 'cdef':
        for c in cdef_cases():
            ref, o = cdef_ref(c.name), oracle_run(L, c, 2)
            mw, mh = c.g.mi_cols * 4, c.g.mi_rows * 4
            pr = _diff('cdef_idx', o['idx'], ref['idx']) + _diff('act', o['act'], c.act) + _diff('svar8', o['svar8'], c.svar8)
            yield c.name, pr + [d for p in range(c.np) for d in _diff('fin plane %d' % p, o['fin'][p][:mh, :mw], ref['fin'][p][:mh, :mw])]
    if group == 'lr':
        for c in lr_cases():
            ref, o = lr_ref(c.name), oracle_run(L, c, 4)
            pr = _diff('lr_type', o['types'], ref['types']) + _diff('lr_set', o['sets'], ref['sets']) + _diff('lr_xqd', o['xqd'], ref['xqd'])
            yield c.name, pr + [d for p in range(c.np) for d in _diff('lrp plane %d' % p, o['lrp'][p][:c.h, :c.w], ref['lrp'][p][:c.h, :c.w])]


# ---------------------------------------------------------------- what the cases reach, measured on the reference alone
def _merge(into, st):
    for k, v in st.items():
        if isinstance(v, set):
            into.setdefault(k, set()).update(v)
        else:
            into[k] = into.get(k, 0) + v


@functools.lru_cache(None)
def reach():
    out = {'deblock_frames': {8: {}, 10: {}}, 'deblock_rows': {8: {}, 10: {}}, 'cdef': {8: {}, 10: {}}, 'lr': {8: {}, 10: {}}}
    for c in deblock_cases():
        st = out['deblock_frames'][c.bd]
        _merge(st, deblock_ref(c.name)['stats'])
        for plane in range(c.np):
            for pass_ in range(2):
                m = c.tx if plane == 0 else c.bs
                for (x, y, fsz) in R.edge_lines(c.g, plane, pass_, c.tx, c.bs):
                    cur = R.tx_extent(int(m[y // 4, x // 4]), plane, pass_)
                    prev = R.tx_extent(int(m[y // 4, x // 4 - 1] if pass_ == 0 else m[y // 4 - 1, x // 4]), plane, pass_)
                    st.setdefault('neighbours', set()).add((plane > 0, pass_, prev, cur))
                    st.setdefault('sizes', set()).add((plane > 0, fsz))
    for c in deblock_cases():                                     # edges the frame's size drops: what the edge loop would find if the whole mi area were on screen
        full = H.Geometry(c.w, c.h)
        full.w, full.h = full.mi_cols * 4, full.mi_rows * 4
        for plane in range(c.np):
            for pass_ in range(2):
                gone = set(R.edge_lines(full, plane, pass_, c.tx, c.bs)) - set(R.edge_lines(c.g, plane, pass_, c.tx, c.bs))
                st = out['deblock_frames'][c.bd]
                st['dropped_x'] = st.get('dropped_x', 0) + sum(x >= c.w for x, y, _ in gone)
                st['dropped_y'] = st.get('dropped_y', 0) + sum(y >= c.h for x, y, _ in gone)
                st.setdefault('dropped_pass_plane', set()).update((pass_, plane > 0) for _ in gone)
    rows = edge_rows()
    for bd in (8, 10):
        edge_rows_ref(rows[rows[:, 20] == bd], out['deblock_rows'][bd])
    for c in cdef_cases() + cdef_list_cases():
        st = out['cdef'][c.bd]
        ref = cdef_ref(c.name)
        _merge(st, ref['stats'])
        if c.oracle:
            st.setdefault('winners_tune%d' % c.tune_psnr, set()).update(int(v) for v in ref['idx'])
    for c, which in zip(cdef_border_cases(), 'ab'):               # the counterfactual: were taps outside the frame fetched, which superblocks would choose otherwise
        a = (c.g, c.bd, c.np, c.src, c.rec, c.skip, c.act, c.svar8, c.wq, c.tune_psnr, 1, 3, H.CDEF_LIST, H.CDEF_LIST)
        for sb, (what, blocks) in BORDER_BLOCKS[which].items():
            if what == 'psychovisual':                            # ... and one where the luma distortion's variance boost decides: plain activity-weighted SSE chooses otherwise
                plain = a[:9] + (1,) + a[10:]
                out['cdef']['psy_decides'] = bool(R.cdef_frame(*a, only_sb=sb)[0][sb] != R.cdef_frame(*plain, only_sb=sb)[0][sb])
            elif R.cdef_frame(*a, only_sb=sb)[0][sb] != R.cdef_frame(*a, only_sb=sb, outside_available=True)[0][sb]:
                out['cdef'].setdefault('outside_tap_decides', set()).add(what)
    for c in lr_cases():
        st = out['lr'][c.bd]
        _merge(st, lr_ref(c.name)['stats'])
        for ui in range(c.g.units):
            x0, x1, y0, y1 = R.unit_rect(c.w, c.h, ui // R.lr_units(c.w), ui % R.lr_units(c.w))
            stripes = len({(y + 8) // 64 for y in range(y0, y1)})
            st.setdefault('chunks', set()).add(stripes * ((x1 - x0 + 63) // 64))
            st.setdefault('last_stripe_rows', set()).add(y1 - max(y0, ((y1 - 1 + 8) // 64) * 64 - 8))
    for c, cands in lr_decide_cases():
        st = {}
        R.lr_decide(c.g, c.bd, c.np, c.src, c.rec, c.fin, c.act, c.wq, RDMULT, LR_COST, 1, cands, st)
        out['lr'].setdefault('decide', set()).update(st['lr_sets'])
    return out
