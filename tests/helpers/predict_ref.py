"""Intra prediction, block availability and block distortion written from the text of the AV1 specification (7.11.2 with 7.11.2.2 - 7.11.2.12, 7.11.5, the
BlockDecoded bookkeeping of 5.11.3 / 7.11.2) in plain Python integers -- test infrastructure only.  It follows the specification's own steps and names, not the
kernels' or the oracle's code: edges are arrays indexed from -2 as AboveRow / LeftCol are, the strength and upsample decisions are tables, the Hadamard
transforms are matrix products.  tests/test_predict_kernels.py pins it by the oracle before any kernel is judged by it.

Every function takes an optional `stats` dict in which it counts the decisions it took (what the reach test measures)."""
import numpy as np

DC_PRED, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED, D67_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED = range(13)
MODE_TO_ANGLE = {V_PRED: 90, H_PRED: 180, D45_PRED: 45, D135_PRED: 135, D113_PRED: 113, D157_PRED: 157, D203_PRED: 203, D67_PRED: 67}
DIRECTIONAL = sorted(MODE_TO_ANGLE)
# Dr_Intra_Derivative, one entry per two degrees
DR_INTRA_DERIVATIVE = [0, 1023, 0, 547, 372, 0, 0, 273, 215, 0, 178, 151, 0, 132, 116, 0, 102, 0, 90, 80, 0, 71, 64, 0, 57, 51, 0, 45, 0, 40, 35, 0, 31, 27, 0, 23, 19, 0, 15, 0, 11, 0, 7, 3]
SM_WEIGHTS = {
    2: [255, 149, 85, 64],
    3: [255, 197, 146, 105, 73, 50, 37, 32],
    4: [255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16],
    5: [255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8],
    6: [255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
        65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4]}
INTRA_EDGE_KERNEL = [[0, 4, 8, 4, 0], [0, 5, 6, 5, 0], [2, 4, 4, 4, 2]]
# 7.11.2.9 as a table: per filter type, (largest w + h of the class, [(smallest |delta|, strength)] in rising order)
EDGE_STRENGTH = {0: [(8, [(56, 1)]), (12, [(40, 1)]), (16, [(40, 1)]), (24, [(8, 1), (16, 2), (32, 3)]), (32, [(1, 1), (4, 2), (32, 3)]), (1 << 30, [(1, 3)])],
                 1: [(8, [(40, 1), (64, 2)]), (16, [(20, 1), (48, 2)]), (24, [(4, 3)]), (1 << 30, [(1, 3)])]}


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def round2(x, n):
    return x if n == 0 else (x + (1 << (n - 1))) >> n


def round2_signed(x, n):
    return round2(x, n) if x >= 0 else -round2(-x, n)


def dr_intra_derivative(angle):
    v = DR_INTRA_DERIVATIVE[angle >> 1]
    assert v, 'no derivative for the angle %d' % angle
    return v


def edge_filter_strength(w, h, filter_type, delta):
    d, strength = abs(delta), 0
    for largest, steps in EDGE_STRENGTH[filter_type]:
        if w + h <= largest:
            for least, s in steps:
                if d >= least:
                    strength = s
            break
    return strength


def edge_upsample_selection(w, h, filter_type, delta):
    d = abs(delta)
    if d <= 0 or d >= 40:
        return 0
    return int(w + h <= 8) if filter_type else int(w + h <= 16)


class Edge:
    """AboveRow or LeftCol: indices -2 .. 2 * 64 + 64."""
    OFF = 16

    def __init__(self):
        self.v = [None] * (self.OFF + 2 * 64 + 64 + 16)

    def __getitem__(self, i):
        v = self.v[i + self.OFF]
        assert v is not None, 'edge sample %d read before it was written' % i
        return v

    def __setitem__(self, i, v):
        self.v[i + self.OFF] = int(v)

    def copy(self):
        e = Edge()
        e.v = list(self.v)
        return e

    def run(self, lo, hi):
        return [self[i] for i in range(lo, hi)]


def geometry(w, h):
    """(mi_cols, mi_rows, pw, ph) of a w x h picture: whole 8x8 blocks in the mi grid, whole superblocks in the padded plane."""
    mi_cols, mi_rows = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    return mi_cols, mi_rows, ((mi_cols + 15) >> 4) * 64, ((mi_rows + 15) >> 4) * 64


def prepare_edges(frame, mi_cols, mi_rows, bd, x, y, w, h, have_left, have_above, have_above_rt, have_below_lft, stats=None):
    """7.11.2, the edge preparation: AboveRow[-1 .. w + h - 1] and LeftCol[-1 .. w + h - 1] of the block at (x, y) of CurrFrame = frame[row][column]."""
    max_x, max_y = mi_cols * 4 - 1, mi_rows * 4 - 1
    above, left = Edge(), Edge()
    n = w + h
    _bump(stats, 'avail_L%d_A%d_AR%d_BL%d' % (have_left, have_above, have_above_rt, have_below_lft))
    if not have_above and have_left:
        for i in range(n):
            above[i] = frame[y][x - 1]
    elif not have_above and not have_left:
        for i in range(n):
            above[i] = (1 << (bd - 1)) - 1
    else:
        above_limit = min(max_x, x + (2 * w if have_above_rt else w) - 1)
        _bump(stats, 'above_limit_is_max_x' if max_x < x + (2 * w if have_above_rt else w) - 1 else 'above_limit_is_run')
        if max_x < x + w - 1:
            _bump(stats, 'above_limit_inside_block')
        for i in range(n):
            above[i] = frame[y - 1][min(above_limit, x + i)]
    if not have_left and have_above:
        for i in range(n):
            left[i] = frame[y - 1][x]
    elif not have_left and not have_above:
        for i in range(n):
            left[i] = (1 << (bd - 1)) + 1
    else:
        left_limit = min(max_y, y + (2 * h if have_below_lft else h) - 1)
        _bump(stats, 'left_limit_is_max_y' if max_y < y + (2 * h if have_below_lft else h) - 1 else 'left_limit_is_run')
        if max_y < y + h - 1:
            _bump(stats, 'left_limit_inside_block')
        for i in range(n):
            left[i] = frame[min(left_limit, y + i)][x - 1]
    if have_above and have_left:
        above[-1] = frame[y - 1][x - 1]
    elif have_above:
        above[-1] = frame[y - 1][x]
    elif have_left:
        above[-1] = frame[y][x - 1]
    else:
        above[-1] = 1 << (bd - 1)
    left[-1] = above[-1]
    return above, left


def intra_edge_filter(buf, sz, strength):
    """7.11.2.12 on buf[-1 .. sz - 2]."""
    if strength == 0:
        return
    edge = [buf[i - 1] for i in range(sz)]
    for i in range(1, sz):
        s = 0
        for j in range(5):
            k = min(max(i - 2 + j, 0), sz - 1)
            s += INTRA_EDGE_KERNEL[strength - 1][j] * edge[k]
        buf[i - 1] = (s + 8) >> 4


def intra_edge_upsample(buf, num_px, bd, stats=None, which=''):
    """7.11.2.11 on buf[-2 .. 2 * num_px - 2]."""
    dup = [0] * (num_px + 3)
    dup[0] = buf[-1]
    for i in range(-1, num_px):
        dup[i + 2] = buf[i]
    dup[num_px + 2] = buf[num_px - 1]
    buf[-2] = dup[0]
    for i in range(num_px):
        s = round2(-dup[i] + 9 * dup[i + 1] + 9 * dup[i + 2] - dup[i + 3], 4)
        if s < 0:
            _bump(stats, 'upsample_clamp_lo_%s' % which)
        if s > (1 << bd) - 1:
            _bump(stats, 'upsample_clamp_hi_%s' % which)
        buf[2 * i - 1] = min(max(s, 0), (1 << bd) - 1)
        buf[2 * i] = dup[i + 2]


def directional(above, left, mi_cols, mi_rows, bd, x, y, w, h, have_left, have_above, p_angle, filter_type, stats=None):
    """7.11.2.4 with enable_intra_edge_filter = 1: the prediction (h rows of w) of angle p_angle from copies of the edges."""
    max_x, max_y = mi_cols * 4 - 1, mi_rows * 4 - 1
    a, l = above.copy(), left.copy()
    if p_angle != 90 and p_angle != 180:
        if 90 < p_angle < 180 and w + h >= 24:
            v = round2(l[0] * 5 + a[-1] * 6 + a[0] * 5, 4)
            if v != a[-1]:
                _bump(stats, 'corner_filter_changes')
            a[-1] = l[-1] = v
        if have_above:
            strength = edge_filter_strength(w, h, filter_type, p_angle - 90)
            num_px = min(w, max_x - x + 1) + (h if p_angle < 90 else 0) + 1
            _bump(stats, 'strength_above_%d' % strength)
            if max_x - x + 1 < w:
                _bump(stats, 'num_px_above_truncated')
            intra_edge_filter(a, num_px, strength)
        if have_left:
            strength = edge_filter_strength(w, h, filter_type, p_angle - 180)
            num_px = min(h, max_y - y + 1) + (w if p_angle > 180 else 0) + 1
            _bump(stats, 'strength_left_%d' % strength)
            if max_y - y + 1 < h:
                _bump(stats, 'num_px_left_truncated')
            intra_edge_filter(l, num_px, strength)
    upsample_above = edge_upsample_selection(w, h, filter_type, p_angle - 90)
    if upsample_above:
        intra_edge_upsample(a, w + (h if p_angle < 90 else 0), bd, stats, 'above_bd%d' % bd)
    upsample_left = edge_upsample_selection(w, h, filter_type, p_angle - 180)
    if upsample_left:
        intra_edge_upsample(l, h + (w if p_angle > 180 else 0), bd, stats, 'left_bd%d' % bd)
    _bump(stats, 'upsample_above_%d' % upsample_above)
    _bump(stats, 'upsample_left_%d' % upsample_left)
    dx = dy = 0
    if p_angle < 90:
        dx = dr_intra_derivative(p_angle)
    elif 90 < p_angle < 180:
        dx = dr_intra_derivative(180 - p_angle)
    if 90 < p_angle < 180:
        dy = dr_intra_derivative(p_angle - 90)
    elif p_angle > 180:
        dy = dr_intra_derivative(270 - p_angle)
    pred = [[0] * w for _ in range(h)]
    used = set()
    for i in range(h):
        for j in range(w):
            if p_angle < 90:
                idx = (i + 1) * dx
                base = (idx >> (6 - upsample_above)) + (j << upsample_above)
                shift = ((idx << upsample_above) >> 1) & 0x1F
                max_base_x = (w + h - 1) << upsample_above
                if base < max_base_x:
                    v = round2(a[base] * (32 - shift) + a[base + 1] * shift, 5)
                else:
                    _bump(stats, 'base_ge_max_base_x')
                    v = a[max_base_x]
            elif 90 < p_angle < 180:
                idx = (j << 6) - (i + 1) * dx
                base = idx >> (6 - upsample_above)
                if base >= -(1 << upsample_above):
                    shift = ((idx << upsample_above) >> 1) & 0x1F
                    v = round2(a[base] * (32 - shift) + a[base + 1] * shift, 5)
                    used.add('above')
                    if base == -(1 << upsample_above):
                        _bump(stats, 'base_at_switch_limit')
                else:
                    idx = (i << 6) - (j + 1) * dy
                    base = idx >> (6 - upsample_left)
                    shift = ((idx << upsample_left) >> 1) & 0x1F
                    v = round2(l[base] * (32 - shift) + l[base + 1] * shift, 5)
                    used.add('left')
            elif p_angle > 180:
                idx = (j + 1) * dy
                base = (idx >> (6 - upsample_left)) + (i << upsample_left)
                shift = ((idx << upsample_left) >> 1) & 0x1F
                v = round2(l[base] * (32 - shift) + l[base + 1] * shift, 5)
            elif p_angle == 90:
                v = a[j]
            else:
                v = l[i]
            pred[i][j] = v
    if used == {'above', 'left'}:
        _bump(stats, 'above_left_switch_in_block')
    return pred


def non_directional(above, left, bd, w, h, have_left, have_above, mode, stats=None):
    """7.11.2.2 (Paeth), 7.11.2.5 (DC), 7.11.2.6 (smooth) on the raw edges."""
    log2w, log2h = w.bit_length() - 1, h.bit_length() - 1
    pred = [[0] * w for _ in range(h)]
    if mode == PAETH_PRED:
        for i in range(h):
            for j in range(w):
                base = above[j] + left[i] - above[-1]
                p_left, p_top, p_top_left = abs(base - left[i]), abs(base - above[j]), abs(base - above[-1])
                if p_left <= p_top and p_left <= p_top_left:
                    pred[i][j] = left[i]
                    _bump(stats, 'paeth_left')
                elif p_top <= p_top_left:
                    pred[i][j] = above[j]
                    _bump(stats, 'paeth_top')
                else:
                    pred[i][j] = above[-1]
                    _bump(stats, 'paeth_top_left')
                ties = (p_left == p_top) + (p_top == p_top_left) + (p_left == p_top_left)
                if ties == 3:
                    _bump(stats, 'paeth_tie3' if len({left[i], above[j], above[-1]}) > 1 else 'paeth_tie3_equal')
                elif ties == 1 and len({left[i], above[j], above[-1]}) == 3:
                    _bump(stats, 'paeth_tie2_%s' % ('lt' if p_left == p_top else ('t_tl' if p_top == p_top_left else 'l_tl')))
    elif mode == DC_PRED:
        s, div = 0, 0
        if have_left and have_above:
            s, div = sum(above[k] for k in range(w)) + sum(left[k] for k in range(h)), w + h
            avg = (s + ((w + h) >> 1)) // (w + h)
        elif have_left:
            s, div = sum(left[k] for k in range(h)), h
            avg = (s + (h >> 1)) >> log2h
        elif have_above:
            s, div = sum(above[k] for k in range(w)), w
            avg = (s + (w >> 1)) >> log2w
        else:
            avg = 1 << (bd - 1)
        if div and (s + (div >> 1)) % div == 0:
            _bump(stats, 'dc_exact_half_L%d_A%d_%dx%d' % (have_left, have_above, w, h))
        _bump(stats, 'dc_L%d_A%d' % (have_left, have_above))
        if avg in (0, (1 << bd) - 1):
            _bump(stats, 'dc_extreme_%d' % (avg != 0))
        pred = [[avg] * w for _ in range(h)]
    else:
        wx, wy = SM_WEIGHTS[log2w], SM_WEIGHTS[log2h]
        for i in range(h):
            for j in range(w):
                if mode == SMOOTH_PRED:
                    pred[i][j] = round2(wy[i] * above[j] + (256 - wy[i]) * left[h - 1] + wx[j] * left[i] + (256 - wx[j]) * above[w - 1], 9)
                elif mode == SMOOTH_V_PRED:
                    pred[i][j] = round2(wy[i] * above[j] + (256 - wy[i]) * left[h - 1], 8)
                else:
                    assert mode == SMOOTH_H_PRED
                    pred[i][j] = round2(wx[j] * left[i] + (256 - wx[j]) * above[w - 1], 8)
    return pred


def predict(frame, mi_cols, mi_rows, bd, x, y, w, h, have_left, have_above, have_above_rt, have_below_lft, mode, angle_delta, filter_type, stats=None):
    """The intra prediction process for one block: (AboveRow, LeftCol, pred)."""
    above, left = prepare_edges(frame, mi_cols, mi_rows, bd, x, y, w, h, have_left, have_above, have_above_rt, have_below_lft, stats)
    if mode in MODE_TO_ANGLE:
        pred = directional(above, left, mi_cols, mi_rows, bd, x, y, w, h, have_left, have_above, MODE_TO_ANGLE[mode] + 3 * angle_delta, filter_type, stats)
    else:
        pred = non_directional(above, left, bd, w, h, have_left, have_above, mode, stats)
    return above, left, pred


def predict_cfl(luma, bd, x, y, w, h, alpha, dc_pred, stats=None):
    """7.11.5 at 4:4:4 with the whole luma block available: the chroma prediction from the DC prediction and the reconstructed luma."""
    log2w, log2h = w.bit_length() - 1, h.bit_length() - 1
    l = [[int(luma[y + i][x + j]) << 3 for j in range(w)] for i in range(h)]
    luma_avg = round2(sum(sum(r) for r in l), log2w + log2h)
    pred = [[0] * w for _ in range(h)]
    for i in range(h):
        for j in range(w):
            prod = alpha * (l[i][j] - luma_avg)
            if prod != 0 and abs(prod) % 64 == 32:
                _bump(stats, 'cfl_half_%s' % ('pos' if prod > 0 else 'neg'))
            v = dc_pred[i][j] + round2_signed(prod, 6)
            if v < 0:
                _bump(stats, 'cfl_clamp_lo')
            if v > (1 << bd) - 1:
                _bump(stats, 'cfl_clamp_hi')
            pred[i][j] = min(max(v, 0), (1 << bd) - 1)
    return pred


# ---------------------------------------------------------------- BlockDecoded
NONE, HORZ, VERT, SPLIT = 'NONE', 'HORZ', 'VERT', 'SPLIT'


def walk_tile(mi_row_start, mi_row_end, mi_col_start, mi_col_end, partition, stats=None):
    """Decodes the partition tree `partition(r, c, size4) -> NONE | HORZ | VERT | SPLIT` of one tile superblock by superblock (64x64, in raster order), every
    superblock in the quadtree's coding order, keeping BlockDecoded as the specification defines it (clear_block_decoded_flags at each superblock, the block's
    cells set once it is decoded).  Yields (r, c, w4, h4, shape, answers): `answers` maps every cell of the ring around the block that lies inside the tile to
    the flag the map holds when the block is predicted; shape is 0 for a square, 1 for the 8x4 and 2 for the 4x8 halves of an 8x8 node."""
    out = []
    for sr in range(mi_row_start, mi_row_end, 16):
        for sc in range(mi_col_start, mi_col_end, 16):
            decoded = {}
            sb_w4, sb_h4 = mi_col_end - sc, mi_row_end - sr
            for yy in range(-1, 17):
                for xx in range(-1, 17):
                    decoded[(sr + yy, sc + xx)] = int((yy < 0 and xx < sb_w4) or (xx < 0 and yy < sb_h4))
            decoded[(sr + 16, sc - 1)] = 0

            def block(r, c, w4, h4, shape):
                answers = {}
                for pr in range(r - 1, r + h4 + 1):
                    for pc in range(c - 1, c + w4 + 1):
                        inside = r <= pr < r + h4 and c <= pc < c + w4
                        if not inside and mi_row_start <= pr < mi_row_end and mi_col_start <= pc < mi_col_end:
                            answers[(pr, pc)] = decoded[(pr, pc)]
                out.append((r, c, w4, h4, shape, answers))
                for pr in range(r, r + h4):
                    for pc in range(c, c + w4):
                        decoded[(pr, pc)] = 1

            def node(r, c, size4):
                if r >= mi_row_end or c >= mi_col_end:
                    return
                p, half = partition(r, c, size4), size4 >> 1
                if p == NONE or size4 == 1:
                    block(r, c, size4, size4, 0)
                elif p == HORZ:
                    block(r, c, size4, half, 1)
                    block(r + half, c, size4, half, 1)
                elif p == VERT:
                    block(r, c, half, size4, 2)
                    block(r, c + half, half, size4, 2)
                else:
                    for dr, dc in ((0, 0), (0, half), (half, 0), (half, half)):
                        node(r + dr, c + dc, half)
            node(sr, sc, 16)
    return out


# ---------------------------------------------------------------- distortion
def hadamard(n):
    h = np.array([[1]], dtype=np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


H4, H8 = hadamard(4), hadamard(8)


def satd(src, pred, w, h, stats=None):
    """Sum of |H D H^T|: one 4x4 Hadamard per 4x4 cell for the 4x4, 8x4 and 4x8 blocks, one 8x8 Hadamard per 8x8 cell on the scale of four 4x4 ones
    ((s + 2) >> 2) for everything larger."""
    d = np.asarray(src, dtype=np.int64).reshape(h, w) - np.asarray(pred, dtype=np.int64).reshape(h, w)
    total = 0
    if w >= 8 and h >= 8:
        for by in range(0, h, 8):
            for bx in range(0, w, 8):
                s = int(np.abs(H8 @ d[by:by + 8, bx:bx + 8] @ H8.T).sum())
                total += (s + 2) >> 2
    else:
        for by in range(0, h, 4):
            for bx in range(0, w, 4):
                total += int(np.abs(H4 @ d[by:by + 4, bx:bx + 4] @ H4.T).sum())
    return total


def sse(a, b):
    d = np.asarray(a, dtype=np.int64).ravel() - np.asarray(b, dtype=np.int64).ravel()
    return int((d * d).sum())
