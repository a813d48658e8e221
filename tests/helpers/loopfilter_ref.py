"""A plain reference of the frame-level filter stages, written from the AV1 specification: 7.14 (loop filter: edge loop, filter size, masks, narrow and
wide filters), 7.15 (CDEF: direction, filter), 7.17 (self-guided restoration with the stripe rule of get_source_sample) and 5.11.58 (the weights' code).  numpy int64 / Python integers.
It has none of the kernels' shortcuts: the level search runs the real filter on every edge line at every level 1..63, the CDEF search filters every block
at all eight strengths, ratios are exact rationals.  The encoder-side distortion (Tune::Psychovisual) is restated with exact integers
(tests/test_independent_checks.py checks the boost formula against floating point).  Test infrastructure only."""
import math
from fractions import Fraction

import numpy as np

I64 = np.int64


# ---------------------------------------------------------------- geometry (4:4:4, 64x64 superblocks)
def tx_extent(code, plane, pass_):
    """Samples a transform of size `code` (0..4 = 4 << code square, 5 = 4 wide x 8 tall, 6 = 8 wide x 4 tall) spans across the edge direction: its width for
    vertical edges (pass 0), its height for horizontal ones.  Chroma follows the block: its largest transform, 32x32 for a 64x64 block (get_tx_size)."""
    if code <= 4:
        return 32 if (plane and code == 4) else 4 << code
    wide, tall = (4, 8) if code == 5 else (8, 4)
    return wide if pass_ == 0 else tall


def edge_lines(g, plane, pass_, m_txsize, m_bsize):
    """7.14.2 for an intra frame: every 4-sample-long edge piece -> (x, y of its first q0 sample, filter size)."""
    m = m_txsize if plane == 0 else m_bsize
    out = []
    for r in range(g.mi_rows):
        for c in range(g.mi_cols):
            x, y = 4 * c, 4 * r
            if x >= g.w or y >= g.h:                              # onScreen
                continue
            if (pass_ == 0 and c == 0) or (pass_ == 1 and r == 0):    # the picture's own edge
                continue
            cur = tx_extent(int(m[r, c]), plane, pass_)
            if (x if pass_ == 0 else y) % cur:                    # not a transform edge
                continue
            prev = tx_extent(int(m[r, c - 1] if pass_ == 0 else m[r - 1, c]), plane, pass_)
            base = min(cur, prev)                                 # 7.14.3
            out.append((x, y, min(16, base) if plane == 0 else min(8, base)))
    return out


def gather_lines(plane_arr, lines, pass_):
    """(N, 16) samples p7 .. p0, q0 .. q7 of the 4 lines of every edge piece; samples beyond the filter's reach are 0 (never read)."""
    n = len(lines) * 4
    L = np.zeros((n, 16), I64)
    pos = np.zeros((n, 3), I64)
    k = 0
    for (x, y, fsz) in lines:
        half = fsz // 2 if fsz < 16 else 8
        for i in range(4):
            xx, yy = (x, y + i) if pass_ == 0 else (x + i, y)
            if pass_ == 0:
                L[k, 8 - half:8 + half] = plane_arr[yy, xx - half:xx + half]
            else:
                L[k, 8 - half:8 + half] = plane_arr[yy - half:yy + half, xx]
            pos[k] = (xx, yy, fsz)
            k += 1
    return L, pos


# ---------------------------------------------------------------- 7.14.6: the sample filtering process, on (N, 16) lines at once
def filter_lines(L, fsz, plane, lvl, sharp, bd, stats=None):
    """L: (N, 16) int64, p_i = L[:, 7 - i], q_i = L[:, 8 + i]; fsz: (N,) filter sizes.  Returns the filtered lines."""
    L = np.asarray(L, I64)
    fsz = np.asarray(fsz, I64)
    P = lambda i: L[:, 7 - i]
    Q = lambda i: L[:, 8 + i]
    out = L.copy()
    if lvl == 0:
        return out
    shift = 2 if sharp > 4 else (1 if sharp > 0 else 0)                     # 7.14.6.2
    limit = min(max(lvl >> shift, 1), 9 - sharp) if sharp > 0 else max(1, lvl >> shift)
    blimit = 2 * (lvl + 2) + limit
    thresh = lvl >> 4
    s8 = bd - 8
    limit_bd, blimit_bd, thresh_bd, one = limit << s8, blimit << s8, thresh << s8, 1 << s8
    ab = np.abs
    hev = (ab(P(1) - P(0)) > thresh_bd) | (ab(Q(1) - Q(0)) > thresh_bd)     # 7.14.6.2 hevMask
    flen = np.where(fsz == 4, 4, np.where(plane != 0, 6, np.where(fsz == 8, 8, 16)))
    m4 = (ab(P(1) - P(0)) <= limit_bd) & (ab(Q(1) - Q(0)) <= limit_bd) & (ab(P(0) - Q(0)) * 2 + ab(P(1) - Q(1)) // 2 <= blimit_bd)
    m6 = (ab(P(2) - P(1)) <= limit_bd) & (ab(Q(2) - Q(1)) <= limit_bd)
    m8 = (ab(P(3) - P(2)) <= limit_bd) & (ab(Q(3) - Q(2)) <= limit_bd)
    mask = m4 & ((flen < 6) | m6) & ((flen < 8) | m8)
    f6 = (ab(P(1) - P(0)) <= one) & (ab(Q(1) - Q(0)) <= one) & (ab(P(2) - P(0)) <= one) & (ab(Q(2) - Q(0)) <= one)
    f8 = (ab(P(3) - P(0)) <= one) & (ab(Q(3) - Q(0)) <= one)
    flat = (fsz >= 8) & f6 & ((flen < 8) | f8)
    flat2 = (fsz >= 16) & np.logical_and.reduce([(ab(P(i) - P(0)) <= one) & (ab(Q(i) - Q(0)) <= one) for i in (4, 5, 6)])
    # 7.14.6.3 narrow filter
    lo, hi, off = -(1 << (bd - 1)), (1 << (bd - 1)) - 1, 0x80 << s8
    c = lambda v: np.clip(v, lo, hi)
    ps1, ps0, qs0, qs1 = P(1) - off, P(0) - off, Q(0) - off, Q(1) - off
    filt0 = np.where(hev, c(ps1 - qs1), 0)
    filt = c(filt0 + 3 * (qs0 - ps0))
    f1, f2 = c(filt + 4) >> 3, c(filt + 3) >> 3
    narrow = mask & ((fsz == 4) | ~flat)
    nq0, np0 = c(qs0 - f1) + off, c(ps0 + f2) + off
    fo = (f1 + 1) >> 1
    nq1, np1 = c(qs1 - fo) + off, c(ps1 + fo) + off
    out[:, 8] = np.where(narrow, nq0, out[:, 8])
    out[:, 7] = np.where(narrow, np0, out[:, 7])
    out[:, 9] = np.where(narrow & ~hev, nq1, out[:, 9])
    out[:, 6] = np.where(narrow & ~hev, np1, out[:, 6])
    # 7.14.6.4 wide filters: (log2Size, n, n2) = luma 8: (3, 3, 0), chroma 6: (3, 2, 1), luma 16: (4, 6, 1)
    wide = mask & ~narrow
    use16 = wide & (fsz == 16) & flat2
    for sel, log2size, n, n2 in ((wide & ~use16 & (plane == 0), 3, 3, 0), (wide & ~use16 & (plane != 0), 3, 2, 1), (use16, 4, 6, 1)):
        if not sel.any():
            continue
        for i in range(-n, n):
            t = np.zeros(L.shape[0], I64)
            for j in range(-n, n + 1):
                p = min(max(i + j, -(n + 1)), n)
                t += L[:, 8 + p] * (2 if abs(j) <= n2 else 1)
            out[:, 8 + i] = np.where(sel, (t + (1 << (log2size - 1))) >> log2size, out[:, 8 + i])
    if stats is not None:
        dev = lambda idx: np.maximum.reduce([np.maximum(ab(P(i) - P(0)), ab(Q(i) - Q(0))) for i in idx])
        terms = [(ab(P(1) - P(0)), limit_bd, flen >= 4), (ab(Q(1) - Q(0)), limit_bd, flen >= 4), (ab(P(0) - Q(0)) * 2 + ab(P(1) - Q(1)) // 2, blimit_bd, flen >= 4),
                 (ab(P(2) - P(1)), limit_bd, flen >= 6), (ab(Q(2) - Q(1)), limit_bd, flen >= 6), (ab(P(3) - P(2)), limit_bd, flen >= 8), (ab(Q(3) - Q(2)), limit_bd, flen >= 8)]
        fails = [(v > lim) & on for v, lim, on in terms]
        nfail = np.sum(fails, axis=0)
        hm = np.maximum(ab(P(1) - P(0)), ab(Q(1) - Q(0)))
        f3 = np.where(flen >= 8, dev((1, 2, 3)), dev((1, 2)))
        extra = [('mask_term%d_fails_alone' % j, fails[j] & (nfail == 1)) for j in range(7)]
        extra += [('mask_term%d_at_limit' % j, mask & terms[j][2] & (terms[j][0] == terms[j][1])) for j in range(7)]
        extra += [('flat_in', (fsz >= 8) & mask & flat & (f3 == one)), ('flat_out', (fsz >= 8) & mask & ~flat & (f3 == one + 1)),
                  ('flat2_in', wide & (fsz == 16) & flat2 & (dev((4, 5, 6)) == one)), ('flat2_out', wide & (fsz == 16) & ~flat2 & (dev((4, 5, 6)) == one + 1)),
                  ('hev_t%d_on' % thresh, mask & hev & (hm == thresh_bd + 1)), ('hev_t%d_off' % thresh, mask & ~hev & (hm == thresh_bd))]
        for k, v in extra:
            stats[k] = stats.get(k, 0) + int(v.sum())
        for k, v in (('mask_off', ~mask), ('narrow_hev', narrow & hev), ('narrow_nohev', narrow & ~hev), ('wide8', wide & ~use16 & (plane == 0)),
                     ('wide6', wide & ~use16 & (plane != 0)), ('wide16', use16), ('flat_not_flat2', wide & (fsz == 16) & ~flat2),
                     ('clamp_q0_lo', narrow & (qs0 - f1 < lo)), ('clamp_q0_hi', narrow & (qs0 - f1 > hi)),
                     ('clamp_p0_lo', narrow & (ps0 + f2 < lo)), ('clamp_p0_hi', narrow & (ps0 + f2 > hi)),
                     ('clamp_q1_lo', narrow & ~hev & (qs1 - fo < lo)), ('clamp_q1_hi', narrow & ~hev & (qs1 - fo > hi)),
                     ('clamp_p1_lo', narrow & ~hev & (ps1 + fo < lo)), ('clamp_p1_hi', narrow & ~hev & (ps1 + fo > hi)),
                     ('clamp_filt', narrow & ((np.abs(filt0 + 3 * (qs0 - ps0)) > hi) | (hev & (np.abs(ps1 - qs1) > hi)) | (filt + 4 > hi)))):
            stats[k] = stats.get(k, 0) + int(v.sum())
    return out


def deblock_tallies(g, bd, np_, src, rec, m_txsize, m_bsize, stats=None):
    """Brute force: tally[plane][pass][l] = the SSE change of the frame when every edge line of (plane, pass) is filtered at level l, sharpness 0, judged on
    the unfiltered reconstruction."""
    t = np.zeros((3, 2, 64), I64)
    for plane in range(np_):
        for pass_ in range(2):
            lines = edge_lines(g, plane, pass_, m_txsize, m_bsize)
            if not lines:
                continue
            R, pos = gather_lines(rec[plane].astype(I64), lines, pass_)
            S, _ = gather_lines(src[plane].astype(I64), lines, pass_)
            base = (R - S) ** 2
            for l in range(1, 64):
                F = filter_lines(R, pos[:, 2], plane, l, 0, bd, stats)
                t[plane, pass_, l] = int(((F - S) ** 2 - base).sum())
    return t


def pick_levels(t, np_):
    """The level choice from the tallies: the lowest level of the smallest SSE per luma pass, one level per chroma plane over both passes; chroma levels are not
    coded (5.9.11) when both luma levels are 0."""
    lv = [int(np.argmin(t[0, 0])), int(np.argmin(t[0, 1])), 0, 0]
    for plane in range(1, np_):
        lv[plane + 1] = int(np.argmin(t[plane, 0] + t[plane, 1]))
    if lv[0] == 0 and lv[1] == 0:
        lv[2] = lv[3] = 0
    return lv


def deblock_pass(g, bd, np_, rec, m_txsize, m_bsize, levels, sharp, pass_):
    """7.14.1 for one pass over all planes, in place on copies; returns the new planes."""
    out = []
    for plane in range(np_):
        a = rec[plane].astype(I64).copy()
        lvl = levels[pass_] if plane == 0 else levels[plane + 1]
        lines = edge_lines(g, plane, pass_, m_txsize, m_bsize) if lvl else []
        if lines:
            L, pos = gather_lines(a, lines, pass_)
            F = filter_lines(L, pos[:, 2], plane, lvl, sharp, bd)
            seen = np.zeros(a.shape, bool)
            for k in range(L.shape[0]):
                for j in np.nonzero(F[k] != L[k])[0]:
                    xx, yy = (pos[k, 0] + j - 8, pos[k, 1]) if pass_ == 0 else (pos[k, 0], pos[k, 1] + j - 8)
                    assert not seen[yy, xx], 'two edges of one pass change the same sample'
                    seen[yy, xx] = True
                    a[yy, xx] = F[k, j]
        out.append(a.astype(np.uint16))
    return out


# ---------------------------------------------------------------- Tune::Psychovisual, exact integers
def cell_var(s, q, n, bd):
    """64 x the per-sample variance of an 8x8 cell (n = 8) on the 8-bit scale."""
    assert n == 8
    v = q - ((s * s + 32) >> 6)
    return max(v, 0) >> (2 * (bd - 8))


def psy_boost_q14(sv, dv):
    num = 4033 * (sv + dv + 16384)
    den = math.isqrt(4033 * 4033 + sv * dv)
    return (num + den // 2) // den


def activity(g, bd, src0, tune_psnr):
    """Per 8x8 cell of the padded luma source: (activity scale Q14, variance)."""
    a = src0.astype(I64).reshape(g.ph // 8, 8, g.pw // 8, 8)
    s, q = a.sum(axis=(1, 3)), (a * a).sum(axis=(1, 3))
    var = np.zeros(s.shape, np.uint32)
    act = np.zeros(s.shape, np.uint32)
    for cy in range(s.shape[0]):
        for cx in range(s.shape[1]):
            v = cell_var(int(s[cy, cx]), int(q[cy, cx]), 8, bd)
            var[cy, cx] = v
            act[cy, cx] = 16384 if tune_psnr else psy_boost_q14(v, v)
    return act, var


def luma_dist(block, srcb, svar, act, bd, tune_psnr):
    sse = int(((block - srcb) ** 2).sum())
    if tune_psnr:
        return (sse * act + 8192) >> 14
    d = (sse * psy_boost_q14(svar, cell_var(int(block.sum()), int((block * block).sum()), 8, bd)) + 8192) >> 14
    return (d * act + 8192) >> 14


# ---------------------------------------------------------------- 7.15: CDEF
CDEF_DIRS = [[(-1, 1), (-2, 2)], [(0, 1), (-1, 2)], [(0, 1), (0, 2)], [(0, 1), (1, 2)], [(1, 1), (2, 2)], [(1, 0), (2, 1)], [(1, 0), (2, 0)], [(1, 0), (2, -1)]]
DIV_TABLE = [0, 840, 420, 280, 210, 168, 140, 120, 105]


def cdef_direction(block, bd):
    """7.15.2: (yDir, var) of an 8x8 luma block; `costs` too, for the reach test."""
    cost = [0] * 8
    partial = [[0] * 15 for _ in range(8)]
    for i in range(8):
        for j in range(8):
            x = (int(block[i, j]) >> (bd - 8)) - 128
            partial[0][i + j] += x
            partial[1][i + j // 2] += x
            partial[2][i] += x
            partial[3][3 + i - j // 2] += x
            partial[4][7 + i - j] += x
            partial[5][3 - i // 2 + j] += x
            partial[6][j] += x
            partial[7][i // 2 + j] += x
    for i in range(8):
        cost[2] += partial[2][i] ** 2
        cost[6] += partial[6][i] ** 2
    cost[2] *= DIV_TABLE[8]
    cost[6] *= DIV_TABLE[8]
    for i in range(7):
        cost[0] += (partial[0][i] ** 2 + partial[0][14 - i] ** 2) * DIV_TABLE[i + 1]
        cost[4] += (partial[4][i] ** 2 + partial[4][14 - i] ** 2) * DIV_TABLE[i + 1]
    cost[0] += partial[0][7] ** 2 * DIV_TABLE[8]
    cost[4] += partial[4][7] ** 2 * DIV_TABLE[8]
    for d in (1, 3, 5, 7):
        for j in range(5):
            cost[d] += partial[d][3 + j] ** 2
        cost[d] *= DIV_TABLE[8]
        for j in range(3):
            cost[d] += (partial[d][j] ** 2 + partial[d][10 - j] ** 2) * DIV_TABLE[2 * j + 2]
    best, ydir = 0, 0
    for d in range(8):
        if cost[d] > best:
            best, ydir = cost[d], d
    return ydir, (best - cost[(ydir + 4) & 7]) >> 10, cost


def constrain(diff, thr, damping):
    if not thr:
        return 0
    adj = max(0, damping - (thr.bit_length() - 1))
    mag = abs(diff)
    v = min(max(thr - (mag >> adj), 0), mag)
    return -v if diff < 0 else v


def cdef_filter_sample(x, taps, pri, sec, damping, cs):
    """7.15.3 for one sample: taps = 12 values or None (CdefAvailable = 0), in the order k = 0, 1 x sign -, + x (primary, secondary, secondary); neither the
    sum nor the bounds depend on the order."""
    s, mx, mn = 0, x, x
    odd = (pri >> cs) & 1
    for n, t in enumerate(taps):
        if t is None:
            continue
        k, q = n // 6, n % 3
        w = ((3, 3) if odd else (4, 2))[k] if q == 0 else (2, 1)[k]
        s += w * constrain(t - x, pri if q == 0 else sec, damping)
        mx, mn = max(mx, t), min(mn, t)
    return min(max(x + ((8 + s - (1 if s < 0 else 0)) >> 4), mn), mx)


def constrain_v(diff, thr, damping):
    if not thr:
        return np.zeros_like(diff)
    adj = max(0, damping - (thr.bit_length() - 1))
    mag = np.abs(diff)
    return np.sign(diff) * np.minimum(np.maximum(thr - (mag >> adj), 0), mag)


def cdef_block(g, plane_arr, x0, y0, pri, sec, damping, dir_, cs, outside_available=False):
    """The filtered 8x8 block at (x0, y0) of the plane (7.15.3, all 64 samples at once): a tap outside the frame's mi area is not available -- it adds nothing
    to the sum and does not move the bounds.  outside_available (the reach test's counterfactual, never the reference): such a tap is taken from the padded plane
    instead, wrapping around it at the top and the left."""
    fw, fh = g.mi_cols * 4, g.mi_rows * 4
    X = plane_arr[y0:y0 + 8, x0:x0 + 8]
    ys, xs = np.mgrid[y0:y0 + 8, x0:x0 + 8]
    s, mx, mn = np.zeros((8, 8), I64), X.copy(), X.copy()
    odd = (pri >> cs) & 1
    for k in range(2):
        for sg in (-1, 1):
            for q, d2 in enumerate((dir_, (dir_ - 2) & 7, (dir_ + 2) & 7)):
                yy, xx = ys + sg * CDEF_DIRS[d2][k][0], xs + sg * CDEF_DIRS[d2][k][1]
                ok = (yy >= 0) & (yy < fh) & (xx >= 0) & (xx < fw)
                t = plane_arr[np.clip(yy, 0, fh - 1), np.clip(xx, 0, fw - 1)]
                if outside_available:
                    ok, t = np.ones_like(ok), plane_arr[yy % plane_arr.shape[0], xx % plane_arr.shape[1]]
                w = ((3, 3) if odd else (4, 2))[k] if q == 0 else (2, 1)[k]
                s += np.where(ok, w * constrain_v(t - X, pri if q == 0 else sec, damping), 0)
                mx, mn = np.where(ok, np.maximum(mx, t), mx), np.where(ok, np.minimum(mn, t), mn)
    return np.clip(X + ((8 + s - (s < 0)) >> 4), mn, mx)


def cdef_strengths(code, plane, var, bd, cdef_damping):
    """7.15.1: (priStr, secStr, damping, use the luma direction?) of a strength code (pri << 2 | sec) for a block of variance `var`."""
    cs = bd - 8
    pri, sec = (code >> 2) << cs, code & 3
    sec = (4 if sec == 3 else sec) << cs
    use_dir = pri != 0                                            # dir = (priStr == 0) ? 0 : yDir, before the variance adjustment
    damping = cdef_damping + cs - (1 if plane else 0)
    if plane == 0:
        vs = min((var >> 6).bit_length() - 1, 12) if (var >> 6) else 0
        pri = (pri * (4 + vs) + 8) >> 4 if var else 0
    return pri, sec, damping, use_dir


def cdef_frame(g, bd, np_, src, rec, m_skip, act, svar8, wq, tune_psnr, enable_cdef, cdef_damping, cdef_y, cdef_uv, stats=None, only_sb=None, outside_available=False):
    """The search over the eight strengths per 64x64 block (cost = activity-weighted, psychovisual distortion x the plane's weight, summed over the
    blocks that are filtered at all) and the filter at the winner (only_sb: that superblock alone).  Returns (cdef_idx, fin planes over the mi area, costs per superblock)."""
    cs = bd - 8
    R = [rec[p].astype(I64) for p in range(np_)]
    S = [src[p].astype(I64) for p in range(np_)]
    fin = [a.copy() for a in R]
    idx_out = np.full(g.sb_rows * g.sb_cols, -1, np.int8)
    all_costs = {}
    skip = (m_skip & 1).astype(bool)
    for sr in range(g.sb_rows):
        for sc in range(g.sb_cols):
            if not enable_cdef or (only_sb is not None and only_sb != sr * g.sb_cols + sc):
                continue
            blocks = []
            for r in range(sr * 16, min(sr * 16 + 16, g.mi_rows), 2):
                for c in range(sc * 16, min(sc * 16 + 16, g.mi_cols), 2):
                    if skip[r, c] and skip[r + 1, c] and skip[r, c + 1] and skip[r + 1, c + 1]:
                        continue
                    d, v, costs = cdef_direction(R[0][4 * r:4 * r + 8, 4 * c:4 * c + 8], bd)
                    blocks.append((r, c, d, v))
                    if stats is not None:
                        stats.setdefault('dirs', set()).add(d)
                        stats.setdefault('var>>6', set()).add(min(v >> 6, 4096))
                        if v == 0 and d not in (0, 4):
                            stats['var0_dir'] = stats.get('var0_dir', 0) + 1
                        if sorted(costs)[-1] == sorted(costs)[-2] and max(costs) > 0:
                            stats['dir_tie'] = stats.get('dir_tie', 0) + 1
            if not blocks:
                continue
            cost = [0] * 8
            filtered, done = {}, {}
            for idx in range(8):
                for (r, c, d, v) in blocks:
                    x0, y0 = 4 * c, 4 * r
                    for p in range(np_):
                        pri, sec, damping, use_dir = cdef_strengths(cdef_y[idx] if p == 0 else cdef_uv[idx], p, v, bd, cdef_damping)
                        key = (r, c, p, pri, sec, damping, d if use_dir else 0)
                        if key not in done:                       # (a list may repeat a strength: the same block, the same distortion)
                            if pri == 0 and sec == 0:
                                blk = R[p][y0:y0 + 8, x0:x0 + 8]
                            else:
                                blk = cdef_block(g, R[p], x0, y0, pri, sec, damping, d if use_dir else 0, cs, outside_available)
                            sb = S[p][y0:y0 + 8, x0:x0 + 8]
                            a = int(act[r // 2, c // 2])
                            if p == 0:
                                e = luma_dist(blk, sb, int(svar8[r // 2, c // 2]), a, bd, tune_psnr)
                            else:
                                e = (int(((blk - sb) ** 2).sum()) * a + 8192) >> 14
                            done[key] = (blk, e)
                        blk, e = done[key]
                        if stats is not None and p == 0 and pri == 0 and sec:
                            stats['pri0_sec'] = stats.get('pri0_sec', 0) + 1
                        filtered[(idx, r, c, p)] = blk
                        cost[idx] += (e * wq[p]) >> 5
            best = min(range(8), key=lambda i: (cost[i], i))
            idx_out[sr * g.sb_cols + sc] = best
            all_costs[(sr, sc)] = cost
            for (r, c, d, v) in blocks:
                for p in range(np_):
                    fin[p][4 * r:4 * r + 8, 4 * c:4 * c + 8] = filtered[(best, r, c, p)]
    return idx_out, [a.astype(np.uint16) for a in fin], all_costs


# ---------------------------------------------------------------- 7.17: loop restoration, self-guided filter, 64x64 units in every plane
SGR_PARAMS = [(2, 12, 1, 4), (2, 15, 1, 6), (2, 18, 1, 8), (2, 21, 1, 9), (2, 24, 1, 10), (2, 29, 1, 11), (2, 36, 1, 12), (2, 45, 1, 13), (2, 56, 1, 14),
              (2, 68, 1, 15), (0, 0, 1, 5), (0, 0, 1, 8), (0, 0, 1, 11), (0, 0, 1, 14), (2, 30, 0, 0), (2, 75, 0, 0)]     # Sgr_Params: r0, eps0, r1, eps1
REDUCED_SETS = [1, 3, 6, 11]


def lr_units(size):
    return max((size + 32) // 64, 1)                              # count_units_in_frame(64, size)


def unit_rect(W, H, ur, uc):
    """Samples whose unitRow = Min(unitRows - 1, (y + 8) / 64) and unitCol = Min(unitCols - 1, x / 64) are (ur, uc): x0, x1, y0, y1 (exclusive ends)."""
    ucols, urows = lr_units(W), lr_units(H)
    return uc * 64, (W if uc == ucols - 1 else uc * 64 + 64), max(0, ur * 64 - 8), (H if ur == urows - 1 else ur * 64 + 56)


def source_window(cdef, dbk, W, H, xs, ys, stripe_start, stripe_end, stats=None):
    """get_source_sample over the coordinate lists xs, ys: the CDEF output inside the stripe, the deblocked frame in the two rows above and below it."""
    xs = np.clip(np.asarray(xs), 0, W - 1)
    rows = []
    for y in ys:
        y = min(max(int(y), 0), H - 1)
        if y < stripe_start:
            rows.append(dbk[max(stripe_start - 2, y), xs])
        elif y > stripe_end:
            rows.append(dbk[min(stripe_end + 2, y), xs])
        else:
            rows.append(cdef[y, xs])
        if stats is not None and (y < stripe_start or y > stripe_end):
            stats['dbk_rows'] = stats.get('dbk_rows', 0) + 1
    return np.array(rows, I64)


def box_filter(cdef, dbk, W, H, bd, x0, y0, w, h, r, eps, pass_, stripe_start, stripe_end, stats=None):
    """7.17.3 for the w x h region at (x0, y0) of one stripe -> F (h, w), from the definition: every (A, B) entry sums its own (2r + 1)^2 box."""
    n = (2 * r + 1) ** 2
    n2e = n * n * eps
    s = ((1 << 20) + n2e // 2) // n2e
    one_by_n = ((1 << 12) + n // 2) // n
    win = source_window(cdef, dbk, W, H, range(x0 - 1 - r, x0 + w + 1 + r), range(y0 - 1 - r, y0 + h + 1 + r), stripe_start, stripe_end, stats)
    a = np.zeros((h + 2, w + 2), I64)
    b = np.zeros((h + 2, w + 2), I64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            c = win[dy:dy + h + 2, dx:dx + w + 2]
            a += c * c
            b += c
    rnd = lambda v, k: (v + (1 << (k - 1))) >> k if k else v
    a = rnd(a, 2 * (bd - 8))
    d = rnd(b, bd - 8)
    p = np.maximum(0, a * n - d * d)
    z = rnd(p * s, 20)
    a2 = np.where(z >= 255, 256, np.where(z == 0, 1, ((z << 8) + z // 2) // (z + 1)))
    A = a2
    B = rnd((256 - a2) * b * one_by_n, 12)
    if stats is not None:
        stats.setdefault('z', set()).update(int(v) for v in np.unique(np.minimum(z, 256)))
    F = np.zeros((h, w), I64)
    cd = cdef[y0:y0 + h, x0:x0 + w].astype(I64)
    for i in range(h):
        shift = 4 if (pass_ == 0 and ((y0 + i) & 1)) else 5        # (i & 1) of the 4-row blocks the specification walks: the row's own parity
        va = np.zeros(w, I64)
        vb = np.zeros(w, I64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if pass_ == 0:
                    wt = (6 if dx == 0 else 5) if ((y0 + i + dy) & 1) else 0
                else:
                    wt = 4 if (dx == 0 or dy == 0) else 3
                va += wt * A[i + 1 + dy, 1 + dx:1 + dx + w]
                vb += wt * B[i + 1 + dy, 1 + dx:1 + dx + w]
        F[i] = rnd(va * cd[i] + vb, 8 + shift - 4)
    return F


def unit_filters(cdef, dbk, W, H, bd, rect, set_, stats=None):
    """(flt0, flt1) of a unit for a parameter set, stripe by stripe (StripeNum = (y + 8) / 64)."""
    x0, x1, y0, y1 = rect
    r0, e0, r1, e1 = SGR_PARAMS[set_]
    out = [np.zeros((y1 - y0, x1 - x0), I64), np.zeros((y1 - y0, x1 - x0), I64)]
    ys = y0
    while ys < y1:
        stripe = (ys + 8) // 64
        start = stripe * 64 - 8
        ye = min(y1, start + 64)
        for pass_, (r, e) in enumerate(((r0, e0), (r1, e1))):
            if r:
                out[pass_][ys - y0:ye - y0] = box_filter(cdef, dbk, W, H, bd, x0, ys, x1 - x0, ye - ys, r, e, pass_, start, start + 63, stats)
        ys = ye
    return out


def sgr_solve(h00, h11, h01, c0, c1, r0, r1, stats=None):
    """The least-squares weights of (flt0 - u, flt1 - u) against (src - u) in Q7, as the encoder defines them: the five sums are first scaled down together
    (floor) until the largest magnitude is below 2^30, then the ratios are exact, rounded half away from zero, and clamped to what the syntax codes."""
    m = max(abs(v) for v in (h00, h11, h01, c0, c1))
    sh = 0
    while (m >> sh) >= (1 << 30):
        sh += 1
    h00, h11, h01, c0, c1 = (v >> sh for v in (h00, h11, h01, c0, c1))
    xq0 = xq1 = 0
    regime = 'single'
    if r0 == 0:
        if h11 > 0:
            xq1 = ratio_q7(c1, h11)
    elif r1 == 0:
        if h00 > 0:
            xq0 = ratio_q7(c0, h00)
    else:
        det = h00 * h11 - h01 * h01
        regime = 'det<=0' if det <= 0 else ('det>=2^54' if det >= 1 << 54 else 'det')
        if det > 0:
            xq0, xq1 = ratio_q7(h11 * c0 - h01 * c1, det), ratio_q7(h00 * c1 - h01 * c0, det)
    x0 = min(max(xq0, -96), 31)
    x1 = min(max(128 - x0 - xq1, -32), 95)
    if r0 == 0:
        x0 = 0                                                    # not coded: read_lr_unit leaves 0
    if r1 == 0:
        x1 = 95                                                   # not coded: Clip3(-32, 95, 128 - xqd0)
    if stats is not None:
        stats.setdefault('solve', set()).update({regime, 'sh>0' if sh else 'sh=0'})
        stats.setdefault('xqd0', set()).add(x0)
        stats.setdefault('xqd1', set()).add(x1)
    return x0, x1


def lr_unit_act(g, act, rect):
    x0, x1, y0, y1 = rect
    cells = act[y0 >> 3:((y1 - 1) >> 3) + 1, x0 >> 3:((x1 - 1) >> 3) + 1].astype(I64)
    return (int(cells.sum()) + cells.size // 2) // cells.size


def lr_cost_of(sse, unit_act, wq, rate, rdmult):
    return ((((sse * unit_act + 8192) >> 14) * wq) >> 5) + ((rate * rdmult + 256) >> 9)


def lr_apply(cd, flt, set_, x0, x1, bd):
    r0, _, r1, _ = SGR_PARAMS[set_]
    u = cd << 4
    v = x1 * u + x0 * (flt[0] if r0 else u) + (128 - x0 - x1) * (flt[1] if r1 else u)
    return np.clip((v + 1024) >> 11, 0, (1 << bd) - 1)


def lr_search(g, bd, np_, src, rec, fin, act, wq, rdmult, lr_cost, sgr_full, stats=None):
    """Every candidate of every (plane, unit): cands[plane][unit][set index] = (cost, xqd0, xqd1)."""
    W, H = g.w, g.h
    ucols, urows = lr_units(W), lr_units(H)
    sets = list(range(16)) if sgr_full else REDUCED_SETS
    cands = []
    for p in range(np_):
        cdef, dbk, s = fin[p].astype(I64), rec[p].astype(I64), src[p].astype(I64)
        per_unit = []
        for ui in range(ucols * urows):
            rect = unit_rect(W, H, ui // ucols, ui % ucols)
            x0, x1, y0, y1 = rect
            cd, sv = cdef[y0:y1, x0:x1], s[y0:y1, x0:x1]
            ua = lr_unit_act(g, act, rect)
            row = []
            for set_ in sets:
                r0, _, r1, _ = SGR_PARAMS[set_]
                flt = unit_filters(cdef, dbk, W, H, bd, rect, set_, stats)
                u = cd << 4
                e = (sv << 4) - u
                f0 = flt[0] - u if r0 else np.zeros_like(u)
                f1 = flt[1] - u if r1 else np.zeros_like(u)
                sums = [int((f0 * f0).sum()), int((f1 * f1).sum()), int((f0 * f1).sum()), int((f0 * e).sum()), int((f1 * e).sum())]
                xq0, xq1 = sgr_solve(*sums, r0, r1, stats)
                sse = int(((lr_apply(cd, flt, set_, xq0, xq1, bd) - sv) ** 2).sum())
                rate = lr_cost[2] + 4 * 512 + (512 * subexp_bits(xq0, -96, 32, -32) if r0 else 0) + (512 * subexp_bits(xq1, -32, 96, 31) if r1 else 0)
                row.append((lr_cost_of(sse, ua, wq[p], rate, rdmult), xq0, xq1))
            per_unit.append(row)
        cands.append(per_unit)
    return cands


def lr_decide(g, bd, np_, src, rec, fin, act, wq, rdmult, lr_cost, sgr_full, cands, stats=None):
    """RESTORE_NONE against the candidates (a candidate must be strictly cheaper; the first of equal candidates wins), and the filter at the winner.
    Returns lr_type, lr_set, lr_xqd as flat lists over (plane, unit) and the restored planes (defined inside w x h only)."""
    W, H = g.w, g.h
    ucols, urows = lr_units(W), lr_units(H)
    sets = list(range(16)) if sgr_full else REDUCED_SETS
    types, csets, xqd, out = [], [], [], []
    for p in range(np_):
        cdef, dbk, s = fin[p].astype(I64), rec[p].astype(I64), src[p].astype(I64)
        o = cdef.copy()
        for ui in range(ucols * urows):
            rect = unit_rect(W, H, ui // ucols, ui % ucols)
            x0, x1, y0, y1 = rect
            cd, sv = cdef[y0:y1, x0:x1], s[y0:y1, x0:x1]
            best = lr_cost_of(int(((cd - sv) ** 2).sum()), lr_unit_act(g, act, rect), wq[p], lr_cost[0], rdmult)
            t, bs, b0, b1 = 0, 0, 0, 0
            for si, (cost, q0, q1) in enumerate(cands[p][ui][:len(sets)]):
                if cost < best:
                    best, t, bs, b0, b1 = cost, 1, sets[si], q0, q1
            if stats is not None:
                stats.setdefault('lr_sets', set()).add((t, bs))
            types.append(t)
            csets.append(bs)
            xqd += [b0, b1]
            if t:
                o[y0:y1, x0:x1] = lr_apply(cd, unit_filters(cdef, dbk, W, H, bd, rect, bs), bs, b0, b1, bd)
        out.append(o.astype(np.uint16))
    return types, csets, xqd, out


# ---------------------------------------------------------------- restoration's scalar pieces
def ratio_q7(num, det):
    """128 num / det for det > 0, rounded half away from zero; at or beyond +-4 it saturates to +-512.  A denominator of 2^54 or more is halved together with
    the numerator (floor) until it is below: part of the encoder's definition (the products stay inside 64 bits); from there on the ratio is exact."""
    while det >= (1 << 54):
        det >>= 1
        num >>= 1
    q = Fraction(num, det)
    if abs(q) >= 4:
        return -512 if q < 0 else 512
    r = math.floor(abs(q) * 128 + Fraction(1, 2))
    return -r if q < 0 else r


def subexp_code(v, lo, hi_excl, ref, k=4):
    """(count, value) of the bits that decode_signed_subexp_with_ref_bool(lo, hi_excl, k, ref) reads to return v (5.11.58 and the processes it calls).  The value the decoder must
    read is found by trying every one against the specification's inverse_recenter; the bit count then follows the branches of decode_subexp_bool."""
    mx, x, r = hi_excl - lo, v - lo, ref - lo

    def inv_recenter_target(r_, mx_):
        # decode_unsigned_subexp_with_ref_bool: v = decode_subexp; if (r << 1) <= mx: inverse_recenter(r, v) else mx - 1 - inverse_recenter(mx - 1 - r, v)
        for t in range(mx_):
            def inverse_recenter(rr, vv):
                if vv > 2 * rr:
                    return vv
                if vv & 1:
                    return rr - ((vv + 1) >> 1)
                return rr + (vv >> 1)
            got = inverse_recenter(r_, t) if (r_ << 1) <= mx_ else mx_ - 1 - inverse_recenter(mx_ - 1 - r_, t)
            if got == x:
                return t
        raise AssertionError('no code for the value')
    t = inv_recenter_target(r, mx)
    # decode_subexp_bool(numSyms = mx, k), run backwards: the bits it must be fed, most significant first
    i, mk, bits = 0, 0, []
    lit = lambda val, n: [(val >> (n - 1 - j)) & 1 for j in range(n)]
    while True:
        b2 = k + i - 1 if i else k
        a = 1 << b2
        if mx <= mk + 3 * a:                                      # ns(numSyms - mk): w - 1 bits v; v < m is the value, else one more bit: (v << 1) - m + extra_bit
            n = mx - mk
            w = n.bit_length()
            m = (1 << w) - n
            val = t - mk
            if val < m:
                bits += lit(val, w - 1)
            else:
                bits += lit((val + m) >> 1, w - 1) + [(val + m) & 1]
            break
        if t >= mk + a:                                           # subexp_more_bools = 1
            bits.append(1)
            i += 1
            mk += a
        else:
            bits += [0] + lit(t - mk, b2)                         # subexp_bits: L(b2)
            break
    return len(bits), int(''.join(map(str, bits)) or '0', 2)


def subexp_bits(v, lo, hi_excl, ref, k=4):
    return subexp_code(v, lo, hi_excl, ref, k)[0]


def project(cdef, f0, f1, r0, r1, w0, w1, mx):
    """7.17.2's projection of one sample from the two box filter outputs (Q4) with weights w0, w1 (Q7)."""
    u = cdef << 4
    w2 = 128 - w0 - w1
    v = w1 * u + w0 * (f0 if r0 else u) + w2 * (f1 if r1 else u)
    return min(max((v + 1024) >> 11, 0), mx)
