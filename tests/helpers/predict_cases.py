"""The constructed cases of tests/test_predict_kernels.py -- test infrastructure only: blocks for the tile search's intra prediction and distortion functions
(tests/kernels/predict_harness.hip), their expected results from tests/helpers/predict_ref.py, and the comparison of a whole LDS arena with what it may hold.

Groups: edges (availability, frame geometry, the raw edges), directional (all 56 angles in the wave, 16-lane-row and rectangular forms), nondirectional, cfl,
availability (decoded_before against the BlockDecoded walk), satd, distortion (SSE and the psychovisual distortion), tables."""
import functools
import itertools

import numpy as np

from tests.helpers import predict_harness as H
from tests.helpers import predict_ref as R

GROUPS = ['edges', 'directional', 'nondirectional', 'cfl', 'availability', 'satd', 'distortion', 'tables']
ORACLE_GROUPS = ['edges', 'directional', 'nondirectional', 'cfl', 'availability', 'satd', 'distortion']
ANGLES = [(m, d) for m in R.DIRECTIONAL for d in range(-3, 4)]                      # the 56 prediction angles
SIZES = [2, 3, 4, 5, 6]                                                              # log2 of 4 .. 64
NONDIR = [R.DC_PRED, R.PAETH_PRED, R.SMOOTH_PRED, R.SMOOTH_V_PRED, R.SMOOTH_H_PRED]
CFL_ALPHA_MAX = 16                                                                   # the product's alphas: +-1 .. +-16 (CflAlphaU / V = 1 + cfl_alpha)


# ---------------------------------------------------------------- planes
def _plane(w, h, bd, kind):
    """A padded plane (ph x pw) of a w x h picture.  Everything outside the mi grid holds the complement of its neighbour inside, so that a sample fetched from
    beyond maxX / maxY changes a result."""
    mi_cols, mi_rows, pw, ph = R.geometry(w, h)
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:ph, 0:pw]
    if kind == 'rand':                       # every bit of the depth in use
        p = np.random.RandomState(1000 + w * 7 + h * 3 + bd).randint(0, mx + 1, (ph, pw))
    elif kind == 'alt':                      # 0 0 max max along both axes: the upsample's -a + 9b + 9c - d leaves the range at both ends
        p = np.where(((xx + yy) >> 1) & 1, mx, 0)
    elif kind == 'steps':                    # steps of three samples: the three edge filter kernels give three different edges
        p = np.where(((xx // 3) + (yy // 3)) & 1, mx - 5, 9)
    elif kind == 'paeth':                    # small differences around one value: |base - x| ties of every kind
        p = (mx >> 1) + np.array([4, -8, 2, -4, 8, -2, 1, -16])[(xx * 5 + yy * 3) % 8]
    elif kind == 'half1':                    # DC from one edge: the sum of a run of n samples is n / 2 above a multiple of n (the rounding term decides)
        p = 100 + ((xx + yy) & 1)
    elif kind == 'half2':                    # DC from both edges of a block at (64, 64): the sum is n above a multiple of 2 n
        p = 100 + (yy < 64)
    elif kind == 'zero':
        p = np.zeros((ph, pw), np.int64)
    elif kind == 'full':
        p = np.full((ph, pw), mx)
    elif kind == 'luma':                     # chroma from luma: a block average with a fraction, differences that make alpha * ac an odd multiple of 32
        p = (mx >> 1) + ((xx * 3 + yy * 5) % 23) * (1 << (bd - 8)) - 11 + ((xx ^ yy) & 1) * (mx >> 2)
    elif kind == 'luma_hi':                  # a bright block on black and a black block on bright: alpha * ac beyond the clamp at both ends
        p = np.where((xx // 2 + yy) % 5 == 0, mx, 0) if (w + h) & 1 else np.where((xx // 2 + yy) % 5 == 0, 0, mx)
    else:
        raise KeyError(kind)
    p = np.clip(p, 0, mx).astype(np.uint16)
    inside = (xx < mi_cols * 4) & (yy < mi_rows * 4)
    return np.where(inside, p, (mx - p.astype(np.int64)).astype(np.uint16)).astype(np.uint16)


class Planes:
    """The planes of a launch in one buffer."""
    def __init__(self):
        self.off, self.arr, self.total = {}, {}, 0

    def get(self, w, h, bd, kind):
        k = (w, h, bd, kind)
        if k not in self.off:
            self.arr[k] = _plane(w, h, bd, kind)
            self.off[k] = self.total
            self.total += self.arr[k].size
        return self.off[k], self.arr[k]

    def buffer(self):
        return np.concatenate([self.arr[k].ravel() for k in sorted(self.off, key=self.off.get)]) if self.off else np.zeros(1, np.uint16)


def _case(P, op, pic, bd, kind, x, y, wl, hl, hl_, ha, ar, bl, mode, delta=(0,), ftype=0, alpha=0, luma='luma'):
    w, h = pic
    off, _ = P.get(w, h, bd, kind)
    loff = P.get(w, h, bd, luma)[0] if op == H.CFL else off
    return dict(op=op, bd=bd, w=w, h=h, plane_off=off, luma_off=loff, x=x, y=y, wl=wl, hl=hl, have_left=hl_, have_above=ha, have_ar=ar, have_bl=bl, ftype=ftype, alpha=alpha,
                mode=list(mode), delta=list(delta), data_off=0, aux_off=0, _kind=kind, _luma=luma)


def _name(c):
    return 'op%d bd%d %s %dx%d at (%d,%d) of %dx%d L%dA%dAR%dBL%d mode%s delta%s ft%d alpha%d' % (
        c['op'], c['bd'], c['_kind'], 1 << c['wl'], 1 << c['hl'], c['x'], c['y'], c['w'], c['h'], c['have_left'], c['have_above'], c['have_ar'], c['have_bl'],
        c['mode'], c['delta'], c['ftype'], c['alpha'])


BIG = (128, 128)                              # a picture in which a 64x64 block at (64, 64) has every neighbour
POS = {(1, 1): (64, 64), (1, 0): (64, 0), (0, 1): (0, 64), (0, 0): (0, 0)}      # (have_left, have_above) -> position: inside, first row, first column, origin
GROUP_OP = {(True, 2): H.GDIR4, (True, 3): H.GDIR8, (False, 2): H.GNON4, (False, 3): H.GNON8}


def _angle(m, d):
    return R.MODE_TO_ANGLE[m] + 3 * d


def _dir_rows(angles):
    """The 56 angles dealt to the four 16-lane rows of a wave: full waves of four different angles, and waves whose rows 0 and 2 (1 and 3) are dead (pa = 90)."""
    pas = [_angle(m, d) for m, d in angles]
    rows = [pas[i:i + 4] for i in range(0, len(pas), 4)]
    for i in range(0, len(pas), 8):
        q = pas[i:i + 8:2]
        rows.append([90, q[0], 90, q[1]])
        rows.append([q[2], 90, q[3], 90])
    return rows


def edges_cases(P):
    """Availability in all combinations, the frame's end inside a block on each edge, the limit of the above-right and below-left runs binding and not binding."""
    out = []
    probe = [(R.V_PRED, 0), (R.H_PRED, 0), (R.D45_PRED, 0), (R.D203_PRED, 0), (R.D135_PRED, 0), (R.D67_PRED, -3), (R.D203_PRED, 3), (R.PAETH_PRED, 0), (R.DC_PRED, 0), (R.SMOOTH_PRED, 0)]
    for bd in (8, 10):
        for wl in SIZES:
            n = 1 << wl
            for (hl_, ha), (x, y) in POS.items():
                for ar, bl in itertools.product((0, 1), repeat=2):
                    if (ar and not ha) or (bl and not hl_):
                        continue
                    for m, d in probe:
                        out.append(_case(P, H.WAVE, BIG, bd, 'rand', x, y, wl, wl, hl_, ha, ar, bl, [m], [d]))
            # 68 x 36: the mi grid ends at 72 x 40.  A block at x = 64 has 8 columns left, one at y = 32 has 8 rows left; above-right / below-left claimed and not
            geo = [((68, 36), 64, 16), ((68, 36), 16, 32), ((68, 36), 64, 32)] if n <= 32 else []
            # 72 x 104: a 64x64 block at (64, 64) has 8 columns and 40 rows left; 72 x 40: one 64x64 block over the whole picture, no neighbour
            geo += [((72, 104), 64, 64), ((72, 104), 0, 64), ((72, 104), 64, 0)] if n == 64 else []
            for pic, x, y in geo:
                if x + n > R.geometry(*pic)[2] or y + n > R.geometry(*pic)[3]:
                    continue
                for ar, bl in ((0, 0), (1, 1)):
                    for m, d in probe:
                        out.append(_case(P, H.WAVE, pic, bd, 'rand', x, y, wl, wl, int(x > 0), int(y > 0), ar and y > 0, bl and x > 0, [m], [d], ftype=1 if m == R.D135_PRED else 0))
            if n == 64:
                out += [_case(P, H.WAVE, (72, 40), bd, 'rand', 0, 0, wl, wl, 0, 0, 0, 0, [m], [d]) for m, d in probe]
        # the rectangular form: 8x4 and 4x8 in every availability, and at the frame's end (12 x 12: the mi grid ends at 16 x 16; 68 x 36 as above)
        for wl, hl in ((3, 2), (2, 3)):
            for (hl_, ha), (x, y) in POS.items():
                for ar, bl in itertools.product((0, 1), repeat=2):
                    if (ar and not ha) or (bl and not hl_):
                        continue
                    for m, d in probe:
                        out.append(_case(P, H.RECT, BIG, bd, 'rand', x, y, wl, hl, hl_, ha, ar, bl, [m], [d]))
            for pic, x, y in (((68, 36), 68, 16), ((68, 36), 16, 36), ((68, 36), 68, 36), ((68, 36), 64, 32)):
                for ar, bl in ((0, 0), (1, 1)):
                    for m, d in probe:
                        out.append(_case(P, H.RECT, pic, bd, 'rand', x, y, wl, hl, 1, 1, ar, bl, [m], [d]))
        # the 16-lane-row forms on the same availability and geometry
        for wl in (2, 3):
            where = [(BIG, x, y, hl_, ha, ar, bl) for (hl_, ha), (x, y) in POS.items() for ar, bl in itertools.product((0, 1), repeat=2) if not (ar and not ha) and not (bl and not hl_)]
            where += [((68, 36), x, y, 1, 1, ar, ar) for x, y in ((68, 16), (16, 36), (68, 36)) for ar in (0, 1)]
            for pic, x, y, hl_, ha, ar, bl in where:
                out.append(_case(P, GROUP_OP[(True, wl)], pic, bd, 'rand', x, y, wl, wl, hl_, ha, ar, bl, [45, 212, 135, 90]))
                out.append(_case(P, GROUP_OP[(True, wl)], pic, bd, 'rand', x, y, wl, wl, hl_, ha, ar, bl, [180, 58, 203, 113], ftype=1))
                out.append(_case(P, GROUP_OP[(False, wl)], pic, bd, 'rand', x, y, wl, wl, hl_, ha, ar, bl, [R.DC_PRED, R.PAETH_PRED, R.SMOOTH_PRED, -1]))
    return out


def directional_cases(P):
    out = []
    for bd in (8, 10):
        for ft in (0, 1):
            for wl in SIZES:
                for kind in ('rand', 'alt', 'steps') if wl <= 3 else ('rand', 'steps') if wl == 4 else ('rand',):
                    out += [_case(P, H.WAVE, BIG, bd, kind, 64, 64, wl, wl, 1, 1, 1, 1, [m], [d], ftype=ft) for m, d in ANGLES]
            for wl, hl in ((3, 2), (2, 3)):
                for kind in ('rand', 'alt', 'steps'):
                    out += [_case(P, H.RECT, BIG, bd, kind, 64, 64, wl, hl, 1, 1, 1, 1, [m], [d], ftype=ft) for m, d in ANGLES]
            for wl in (2, 3):
                for kind in ('rand', 'alt', 'steps'):
                    out += [_case(P, GROUP_OP[(True, wl)], BIG, bd, kind, 64, 64, wl, wl, 1, 1, 1, 1, rows, ftype=ft) for rows in _dir_rows(ANGLES)]
    return out


def nondirectional_cases(P):
    out = []
    for bd in (8, 10):
        for (hl_, ha), (x, y) in POS.items():
            for kind in ('rand', 'paeth', 'zero', 'full', 'half1', 'half2'):
                for wl in SIZES:
                    out += [_case(P, H.WAVE, BIG, bd, kind, x, y, wl, wl, hl_, ha, 0, 0, [m]) for m in NONDIR]
                for wl, hl in ((3, 2), (2, 3)):
                    out += [_case(P, H.RECT, BIG, bd, kind, x, y, wl, hl, hl_, ha, 0, 0, [m]) for m in NONDIR]
                for wl in (2, 3):                                      # four different modes per wave, and waves with idle rows (mode < 0) between live ones
                    for rows in ([R.DC_PRED, R.PAETH_PRED, R.SMOOTH_PRED, R.SMOOTH_V_PRED], [R.SMOOTH_H_PRED, -1, R.DC_PRED, -1], [-1, R.PAETH_PRED, -1, R.SMOOTH_H_PRED],
                                 [R.SMOOTH_V_PRED, R.SMOOTH_PRED, -1, R.PAETH_PRED]):
                        out.append(_case(P, GROUP_OP[(False, wl)], BIG, bd, kind, x, y, wl, wl, hl_, ha, 0, 0, rows))
    return out


def cfl_cases(P):
    out = []
    alphas = [-CFL_ALPHA_MAX, -9, -4, -1, 1, 3, 8, CFL_ALPHA_MAX]
    for bd in (8, 10):
        for wl in SIZES[:4]:                                            # chroma from luma exists up to 32x32
            for (hl_, ha), (x, y) in POS.items():
                for luma, kind in (('luma', 'rand'), ('luma_hi', 'zero'), ('luma_hi', 'full'), ('luma', 'paeth')):
                    for a in alphas:
                        out.append(_case(P, H.CFL, BIG if luma == 'luma' else (127, 128), bd, kind, x, y, wl, wl, hl_, ha, 0, 0, [R.DC_PRED], alpha=a, luma=luma))
                    if luma == 'luma_hi':
                        out += [_case(P, H.CFL, BIG, bd, kind, x, y, wl, wl, hl_, ha, 0, 0, [R.DC_PRED], alpha=a, luma=luma) for a in (-CFL_ALPHA_MAX, CFL_ALPHA_MAX)]
    return out


PRED_GROUPS = {'edges': edges_cases, 'directional': directional_cases, 'nondirectional': nondirectional_cases, 'cfl': cfl_cases}


@functools.lru_cache(maxsize=None)
def prediction_cases(group):
    P = Planes()
    return PRED_GROUPS[group](P), P


# ---------------------------------------------------------------- expected results of a prediction case
def _frame(P, c, which='plane'):
    return P.arr[(c['w'], c['h'], c['bd'], c['_kind'] if which == 'plane' else c['_luma'])]


_ref_cache = {}


def reference(P, c, stats=None):
    """{'above', 'left', 'preds': [(h x w list or None) per row]} of one prediction case; cached when no statistics are asked for."""
    key = (c['op'], c['bd'], c['w'], c['h'], c['_kind'], c['_luma'], c['x'], c['y'], c['wl'], c['hl'], c['have_left'], c['have_above'], c['have_ar'], c['have_bl'], c['ftype'],
           c['alpha'], tuple(c['mode']), tuple(c['delta']))
    if stats is None and key in _ref_cache:
        return _ref_cache[key]
    fr = _frame(P, c).astype(np.int64)
    mi_cols, mi_rows, _, _ = R.geometry(c['w'], c['h'])
    w, h, bd = 1 << c['wl'], 1 << c['hl'], c['bd']
    geo = (mi_cols, mi_rows, bd, c['x'], c['y'], w, h, c['have_left'], c['have_above'])
    above, left = R.prepare_edges(fr, mi_cols, mi_rows, bd, c['x'], c['y'], w, h, c['have_left'], c['have_above'], c['have_ar'], c['have_bl'], stats)
    out = dict(above=above, left=left, preds=[], dc=None)
    if c['op'] in (H.WAVE, H.RECT):
        m, d = c['mode'][0], c['delta'][0]
        out['preds'] = [R.directional(above, left, *geo, _angle(m, d), c['ftype'], stats) if m in R.MODE_TO_ANGLE else R.non_directional(above, left, bd, w, h, c['have_left'], c['have_above'], m, stats)]
    elif c['op'] in (H.GDIR4, H.GDIR8):
        out['preds'] = [R.directional(above, left, *geo, pa, c['ftype'], stats) for pa in c['mode']]
    elif c['op'] in (H.GNON4, H.GNON8):
        out['preds'] = [None if m < 0 else R.non_directional(above, left, bd, w, h, c['have_left'], c['have_above'], m, stats) for m in c['mode']]
    elif c['op'] == H.CFL:
        out['dc'] = R.non_directional(above, left, bd, w, h, c['have_left'], c['have_above'], R.DC_PRED, stats)
        out['preds'] = [R.predict_cfl(_frame(P, c, 'luma').astype(np.int64), bd, c['x'], c['y'], w, h, c['alpha'], out['dc'], stats)]
    if stats is None:
        _ref_cache[key] = out
    return out


def _is_directional(c):
    return c['op'] in (H.GDIR4, H.GDIR8) or (c['op'] in (H.WAVE, H.RECT) and c['mode'][0] in R.MODE_TO_ANGLE)


def expected_arena(c, ref, start):
    """(the arena a case must leave, the entries that are compared): the defined output is the raw edges [-1 .. w + h - 1] and pred[0 .. w * h); the working
    copies of the edges (from [-2], as far as an upsampled edge reaches) and the filter's scratch are a directional prediction's to use and are not compared;
    everything else must still hold what the case started with."""
    exp, cmp_ = start.copy(), np.ones(H.A_LEN, bool)
    w, h = 1 << c['wl'], 1 << c['hl']
    n = w + h
    for base, e in ((H.A_RA, ref['above']), (H.A_RL, ref['left'])):
        exp[base + H.EDGE_OFF - 1: base + H.EDGE_OFF + n] = e.run(-1, n)
    flat = lambda p: np.asarray(p, dtype=np.uint16).ravel()
    if c['op'] in (H.WAVE, H.RECT, H.CFL):
        exp[H.A_PRED: H.A_PRED + w * h] = flat(ref['preds'][0])
        if c['op'] == H.CFL:
            exp[H.A_SRC: H.A_SRC + w * h] = flat(ref['dc'])
        if _is_directional(c):
            for base in (H.A_WA, H.A_WL):             # (edges are upsampled up to w + h = 16)
                cmp_[base + H.EDGE_OFF - 2: base + H.EDGE_OFF + (2 * n if n <= 16 else n)] = False
            cmp_[H.A_TMP: H.A_TMP + H.A_TMP_LEN] = False
    else:
        for g, p in enumerate(ref['preds']):
            gb = H.A_GP + g * H.GP_LEN
            if p is not None:
                exp[gb + H.GP_PRED: gb + H.GP_PRED + w * h] = flat(p)
            if _is_directional(c):
                cmp_[gb: gb + H.GP_PRED] = False
    return exp, cmp_


_REGIONS = [('raw above', H.A_RA, H.A_EDGE), ('raw left', H.A_RL, H.A_EDGE), ('working above', H.A_WA, H.A_EDGE), ('working left', H.A_WL, H.A_EDGE), ('filter scratch', H.A_TMP, H.A_TMP_LEN),
            ('pred', H.A_PRED, 4096), ('src', H.A_SRC, 4096)] + [('row %d buffers' % g, H.A_GP + g * H.GP_LEN, H.GP_LEN) for g in range(4)] + [('cells', H.A_AUX, H.A_AUX_LEN)]


def where(i):
    for name, base, ln in _REGIONS:
        if base <= i < base + ln:
            return '%s[%d]' % (name, i - base - (H.EDGE_OFF if 'above' in name or 'left' in name else 0))
    return 'guard[%d]' % i


def compare_arena(exp, cmp_, got):
    bad = np.nonzero(cmp_ & (exp != got))[0]
    return ['%s: %d, expected %d' % (where(i), got[i], exp[i]) for i in bad[:4]] + (['... %d entries differ' % len(bad)] if len(bad) > 4 else [])


def check_predictions(lib_path, group, seed=0):
    cases, P = prediction_cases(group)
    dump, _ = H.run(lib_path, cases, P.buffer(), np.zeros(1, np.uint16), seed=seed)
    start = H.fill(seed)
    rows, wave = [], {}
    for c, got in zip(cases, dump):
        ref = reference(P, c)
        problems = compare_arena(*expected_arena(c, ref, start), got)
        if c['op'] == H.WAVE and _is_directional(c):
            wave[(c['bd'], c['_kind'], c['w'], c['h'], c['x'], c['y'], c['wl'], c['have_left'], c['have_above'], c['have_ar'], c['have_bl'], c['ftype'], _angle(c['mode'][0], c['delta'][0]))] = got
        rows.append((c, problems))
    if group == 'directional':               # every 16-lane-row result also equals the wave form's on the same edges
        for (c, problems), got in zip(rows, dump):
            if c['op'] in (H.GDIR4, H.GDIR8):
                nn = 1 << (2 * c['wl'])
                for g, pa in enumerate(c['mode']):
                    wv = wave[(c['bd'], c['_kind'], c['w'], c['h'], c['x'], c['y'], c['wl'], c['have_left'], c['have_above'], c['have_ar'], c['have_bl'], c['ftype'], pa)]
                    gb = H.A_GP + g * H.GP_LEN + H.GP_PRED
                    if not np.array_equal(got[gb: gb + nn], wv[H.A_PRED: H.A_PRED + nn]):
                        problems.append('row %d (angle %d) differs from the wave form' % (g, pa))
    return [(_name(c), problems) for c, problems in rows]


# ---------------------------------------------------------------- availability: decoded_before against the BlockDecoded walk
def _mixed(r, c, s):
    if s == 16:
        return R.SPLIT
    k = ((r >> 3) * 5 + (c >> 3) * 3) % 4
    if s == 8:
        return [R.NONE, R.SPLIT, R.SPLIT, R.SPLIT][k]
    if s == 4:
        return R.NONE if (r + c) % 12 == 0 else R.SPLIT
    if s == 2:
        return [R.NONE, R.HORZ, R.VERT, R.SPLIT][((r >> 1) + (c >> 1) * 3) % 4]
    return R.NONE


TREES = {'all 4x4': lambda r, c, s: R.SPLIT, 'all 8x8': lambda r, c, s: R.NONE if s == 2 else R.SPLIT, 'all 8x4': lambda r, c, s: R.HORZ if s == 2 else R.SPLIT,
         'all 4x8': lambda r, c, s: R.VERT if s == 2 else R.SPLIT, 'all 16x16': lambda r, c, s: R.NONE if s == 4 else R.SPLIT,
         'all 32x32': lambda r, c, s: R.NONE if s == 8 else R.SPLIT, 'all 64x64': lambda r, c, s: R.NONE, 'mixed': _mixed}
TILE = (16, 48, 32, 80)                       # 2 x 3 superblocks, not at the frame's origin: mi rows 16 .. 47, mi columns 32 .. 79


@functools.lru_cache(maxsize=None)
def availability_rows():
    """[(tree, r, c, w4, h4, shape, pr, pc, the map's flag)] for every cell of the ring around every block of every tree that lies in the tile -- among them the
    cells the callers ask about: (r - 1, c + w4) and (r + h4, c - 1) of the block, of its transform sub-blocks (the cells right of and below the block) and of a
    rectangular block's 4x4 cells."""
    rows = []
    for name, tree in TREES.items():
        for r, c, w4, h4, shape, answers in R.walk_tile(*TILE, tree):
            rows += [(name, r, c, w4, h4, shape, pr, pc, v) for (pr, pc), v in sorted(answers.items())]
    return rows


def check_availability(lib_path):
    rows = availability_rows()
    got = H.table(lib_path, H.PT_DECODED, [(r, c, shape, pr, pc) for _, r, c, _, _, shape, pr, pc, _ in rows])
    bad = {}
    for (name, r, c, w4, h4, shape, pr, pc, v), g in zip(rows, got):
        if int(g) != v:
            bad.setdefault(name, []).append('block (%d,%d) %dx%d shape %d, cell (%d,%d): %d, the map holds %d' % (r, c, w4 * 4, h4 * 4, shape, pr, pc, g, v))
    # dev_blk64.h writes the answers for a 64x64 block as literals: above-right available whenever it lies in the tile, below-left never
    lit = [(r, c, pr, pc, v) for name, r, c, w4, h4, shape, pr, pc, v in rows if name == 'all 64x64' and ((pr, pc) == (r - 1, c + 16) or (pr, pc) == (r + 16, c - 1))]
    for r, c, pr, pc, v in lit:
        if v != int(pr < r):
            bad.setdefault('all 64x64', []).append('64x64 block (%d,%d), cell (%d,%d): the literal of dev_blk64.h says %d, the map holds %d' % (r, c, pr, pc, int(pr < r), v))
    return [(name, bad.get(name, [])[:6]) for name in TREES] + [('64x64 literal reached', [] if len(lit) >= 4 else ['only %d cells' % len(lit)])]


# ---------------------------------------------------------------- distortion
def _diff_blocks(n_w, n_h, bd, rs):
    """(src, pred) pairs of a w x h block: random, all +-max, checkerboards, one 8x8 cell non-zero among zero cells."""
    mx, nn = (1 << bd) - 1, n_w * n_h
    yy, xx = np.mgrid[0:n_h, 0:n_w]
    out = [(rs.randint(0, mx + 1, nn), rs.randint(0, mx + 1, nn)), (np.full(nn, mx), np.zeros(nn, np.int64)), (np.zeros(nn, np.int64), np.full(nn, mx)),
           (np.where((xx + yy) & 1, mx, 0).ravel(), np.where((xx + yy) & 1, 0, mx).ravel()), (np.where(xx & 1, mx, 0).ravel(), np.where(yy & 1, mx, 0).ravel())]
    if n_w >= 16 and n_h >= 16:
        for cy, cx in {(0, 0), (0, n_w // 8 - 1), (n_h // 8 - 1, 0), (n_h // 8 - 1, n_w // 8 - 1), (1, 0)}:
            s = np.full((n_h, n_w), mx >> 1)
            s[cy * 8: cy * 8 + 8, cx * 8: cx * 8 + 8] += rs.randint(-3, 4, (8, 8)) + np.eye(8, dtype=np.int64)[::-1] * 2          # a sum with (s + 2) >> 2 off the multiple of 4
            out.append((s.ravel(), np.full(nn, mx >> 1)))
    return [(np.asarray(s, np.int64), np.asarray(p, np.int64)) for s, p in out]


def _impulse_pairs(bd):
    """Two impulses at every pair of positions of one 8x8 cell that lie in opposite halves (rows 0-3 against rows 4-7: the mirrored stage of satd8_lane; columns
    0-3 against 4-7: its last stage), with equal and with opposite signs."""
    mx = (1 << bd) - 1
    out = []
    for a in range(64):
        for b in range(a + 1, 64):
            if ((a >> 3) < 4) != ((b >> 3) < 4) or ((a & 7) < 4) != ((b & 7) < 4):
                sign = 1 if (a * 7 + b) % 3 else -1
                s = np.full(64, mx >> 1)
                s[a] += 37 + (a % 5)
                s[b] += sign * (91 + (b % 7))
                out.append((s, np.full(64, mx >> 1)))
    return out


@functools.lru_cache(maxsize=None)
def distortion_cases(group):
    """(cases, data, what each case holds): satd = satd_dev, satd_group<4|8>, satd_wh; distortion = sse_dev and psy_dist_wave."""
    rs = np.random.RandomState(77)
    cases, data, meta = [], [], []

    def put(*blocks):
        off = sum(len(d) for d in data)
        data.extend(np.asarray(b, np.int64) for b in blocks)
        return off

    def add(op, wl, hl, bd, blocks):
        cases.append(dict(op=op, bd=bd, w=8, h=8, plane_off=0, luma_off=0, x=0, y=0, wl=wl, hl=hl, have_left=0, have_above=0, have_ar=0, have_bl=0, ftype=0, alpha=0,
                          mode=[0], delta=[0], data_off=put(*blocks), aux_off=0))
        meta.append((op, 1 << wl, 1 << hl, bd, blocks))
    for bd in (8, 10):
        if group == 'satd':
            for wl in SIZES:
                for s, p in _diff_blocks(1 << wl, 1 << wl, bd, rs):
                    add(H.SATD, wl, wl, bd, [s, p])
            pairs = _impulse_pairs(bd)
            for s, p in pairs[:: 1 if bd == 8 else 3]:
                add(H.SATD, 3, 3, bd, [s, p])
            for i in range(0, len(pairs) - 3, 4 if bd == 8 else 12):                       # the same pairs, four predictions per wave against one source
                add(H.SATD_G8, 3, 3, bd, [pairs[i][1]] + [pairs[i + g][0] for g in range(4)])
            for wl, hl in ((3, 2), (2, 3)):
                for s, p in _diff_blocks(1 << wl, 1 << hl, bd, rs):
                    add(H.SATD_WH, wl, hl, bd, [s, p])
            for wl, op in ((2, H.SATD_G4), (3, H.SATD_G8)):
                blocks = _diff_blocks(1 << wl, 1 << wl, bd, rs)
                for i in range(len(blocks)):                                                  # row g holds the prediction of block i + g: every row another value
                    add(op, wl, wl, bd, [blocks[i][0]] + [blocks[(i + g) % len(blocks)][1] for g in range(4)])
        else:
            for wl, hl in ((2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5), (6, 5), (6, 6)):     # nn = 16 .. 4096: 1024 and below in 32 bits, above in 64
                for s, p in _diff_blocks(1 << wl, 1 << hl, bd, rs):
                    add(H.SSE, wl, hl, bd, [s, p])
            for wl in SIZES:
                for s, p in _diff_blocks(1 << wl, 1 << wl, bd, rs)[:1] + _diff_blocks(1 << wl, 1 << wl, bd, rs)[3:]:
                    q = np.clip(s + rs.randint(-40, 41, s.size), 0, (1 << bd) - 1)                # a reconstruction near the source as well as a far one
                    add(H.PSY, wl, wl, bd, [s, q])
                    add(H.PSY, wl, wl, bd, [s, p])
    return cases, np.concatenate(data), meta


def _psy_oracle(L, meta):
    """The oracle's psychovisual distortion of every PSY case, and the cells' variances and activities it derives from the source."""
    import ctypes as C
    fn = L.av1o_test_psy_dist
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    out = {}
    for i, (op, w, h, bd, blocks) in enumerate(meta):
        if op == H.PSY:
            s, q = (np.ascontiguousarray(b, dtype=np.uint16) for b in blocks)
            sv, act = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
            d = fn(s.ctypes.data, q.ctypes.data, w, bd, sv.ctypes.data, act.ctypes.data)
            assert d >= 0
            nc = 1 if w == 4 else (w // 8) ** 2
            out[i] = (int(d), sv[:nc].copy(), act[:nc].copy())
    return out


def check_distortion(lib_path, group, seed=0):
    cases, data, meta = distortion_cases(group)
    psy, aux = {}, [np.zeros(1, np.int64)]
    if group == 'distortion':                 # psy_dist_wave is compared with the oracle only (its Q14 boost is checked against floats in tests/test_independent_checks.py)
        from tests.helpers import oracle
        psy = _psy_oracle(oracle.lib(), meta)
        for i, (d, sv, act) in psy.items():
            cases[i]['aux_off'] = sum(len(a) for a in aux)
            aux += [sv.astype(np.int64), act.astype(np.int64)]
    dump, res = H.run(lib_path, cases, np.zeros(1, np.uint16), data, aux=np.concatenate(aux), seed=seed)
    start = H.fill(seed)
    rows = []
    for i, ((op, w, h, bd, blocks), got, r) in enumerate(zip(meta, dump, res)):
        exp, cmp_ = start.copy(), np.ones(H.A_LEN, bool)
        nn = w * h
        exp[H.A_SRC: H.A_SRC + nn] = blocks[0]
        if op in (H.SATD_G4, H.SATD_G8):
            want = [R.satd(blocks[0], blocks[1 + g], w, h) for g in range(4)]
            for g in range(4):
                exp[H.A_GP + g * H.GP_LEN + H.GP_PRED: H.A_GP + g * H.GP_LEN + H.GP_PRED + nn] = blocks[1 + g]
        else:
            exp[H.A_PRED: H.A_PRED + nn] = blocks[1]
            want = [psy[i][0] if op == H.PSY else R.sse(*blocks) if op == H.SSE else R.satd(blocks[0], blocks[1], w, h), 0, 0, 0]
        if op == H.PSY:
            cmp_[H.A_AUX: H.A_AUX + H.A_AUX_LEN] = False          # the harness's own staging of the cells
        problems = compare_arena(exp, cmp_, got)
        if [int(v) for v in r] != want:
            problems.append('result %s, expected %s' % ([int(v) for v in r], want))
        rows.append(('op%d %dx%d bd%d case %d' % (op, w, h, bd, i), problems))
    return rows


# ---------------------------------------------------------------- tables
def check_tables(lib_path):
    rows = []
    args = [(w, h, ft, d) for w, h in ((4, 4), (8, 4), (4, 8), (8, 8), (16, 16), (32, 32), (64, 64), (8, 16), (16, 8), (16, 32), (4, 16)) for ft in (0, 1) for d in range(-135, 136)]
    for op, fn, name in ((H.PT_STRENGTH, R.edge_filter_strength, 'edge_strength_dev'), (H.PT_UPSAMPLE, R.edge_upsample_selection, 'edge_upsample_sel_dev')):
        got = H.table(lib_path, op, args)
        bad = ['%s%s: %d, expected %d' % (name, a, g, fn(*a)) for a, g in zip(args, got) if int(g) != fn(*a)]
        rows.append((name, bad[:6]))
    angles = sorted({a for m, d in ANGLES for pa in [_angle(m, d)] for a in (pa, 180 - pa, pa - 90, 270 - pa) if 0 < a < 90})
    got = H.table(lib_path, H.PT_DERIV, [(a,) for a in angles])
    rows.append(('dr_deriv_dev', ['angle %d: %d, expected %d' % (a, g, R.dr_intra_derivative(a)) for a, g in zip(angles, got) if int(g) != R.dr_intra_derivative(a)][:6]))
    args = [(l, i) for l in SIZES for i in range(1 << l)]
    got = H.table(lib_path, H.PT_SM_WEIGHT, args)
    rows.append(('sm_weights_dev', ['%s: %d, expected %d' % (a, g, R.SM_WEIGHTS[a[0]][a[1]]) for a, g in zip(args, got) if int(g) != R.SM_WEIGHTS[a[0]][a[1]]][:6]))
    got = H.table(lib_path, H.PT_MODE_ANGLE, [(m,) for m in R.DIRECTIONAL])
    rows.append(('mode_angle_of', ['mode %d: %d, expected %d' % (m, g, R.MODE_TO_ANGLE[m]) for m, g in zip(R.DIRECTIONAL, got) if int(g) != R.MODE_TO_ANGLE[m]]))
    return rows


def check_group(lib_path, group, seed=0):
    """[(case, problems)] of one group through the library `lib_path`."""
    if group in PRED_GROUPS:
        return check_predictions(lib_path, group, seed)
    if group == 'availability':
        return check_availability(lib_path)
    if group in ('satd', 'distortion'):
        return check_distortion(lib_path, group, seed)
    assert group == 'tables', group
    return check_tables(lib_path)


# ---------------------------------------------------------------- the BlockDecoded walk against the oracle's walker
def _walker_picture(kind):
    """192 x 128 luma samples (2 x 3 superblocks, one tile): smooth areas, texture and edges side by side, so that a search picks blocks of many sizes."""
    h, w = 128, 192
    yy, xx = np.mgrid[0:h, 0:w]
    rs = np.random.RandomState(11 + kind)
    p = 128 + 60 * np.sin(xx / (9.0 + kind)) + 50 * np.cos(yy / 7.0)
    p += np.where((xx // 64 + yy // 64 + kind) % 2 == 0, rs.randint(-70, 71, (h, w)), rs.randint(-4, 5, (h, w)))
    p += np.where(((xx + 2 * yy) // 5) % 7 == 0, 90, 0) * ((xx // 32 + kind) % 3 == 0)
    return np.clip(p, 0, 255).astype(np.uint16)


WALKER_RUNS = [dict(part_min=s, part_max=s) for s in (4, 8, 16, 32, 64)] + [dict(speed=1, quantizer=40), dict(speed=1, quantizer=100, kind=1), dict(speed=2, quantizer=70, kind=2),
                                                                            dict(speed=1, quantizer=160, kind=3)]


def walker_against_oracle(L, stats=None):
    """The oracle searches pictures of one tile of 2 x 3 superblocks -- with the partition size forced (uniform trees of every size) and free (the trees its
    rate-distortion search picks, 8x4 and 4x8 halves among them) -- while it records every above-right / below-left flag it reads off its m_decoded map.  The
    reference walks the tree the encode ended with; at every block of that tree, and at every transform sub-block of it that asks about a cell outside the block,
    the flags the oracle read must be the ones the reference's map holds -- in every trial in which the oracle visited that block, not only the last."""
    from tests.helpers import oracle
    rows, stats = [], {} if stats is None else stats
    for run in WALKER_RUNS:
        run = dict(run)
        asked = sorted(run.items())
        pic = _walker_picture(run.pop('kind', 0))
        cfg = oracle.make_config(pic.shape[1], pic.shape[0], 8, mono=True, quantizer=run.pop('quantizer', 80), speed=run.pop('speed', 4), **run)
        buf = np.zeros((1 << 20, 9), np.int32)
        L.av1o_test_avail_trace(buf.ctypes.data, len(buf))
        try:
            out = oracle.encode_planes(cfg, [pic])
            n = L.av1o_test_avail_trace_count()
        finally:
            L.av1o_test_avail_trace(None, 0)
        name = 'walker %s (partitions %d..%d)' % (asked, cfg.part_min, cfg.part_max)
        problems = []
        if out['tiles'] != (1, 1) or n > len(buf):
            rows.append((name, ['tiles %s, %d trace entries' % (out['tiles'], n)]))
            continue
        bsize = out['m_bsize']
        mi_rows, mi_cols = bsize.shape

        def partition(r, c, size4):
            code = int(bsize[r, c])
            if size4 == 2 and code in (5, 6):
                return R.VERT if code == 5 else R.HORZ
            return R.NONE if code <= 4 and (1 << code) == size4 else R.SPLIT
        blocks = {}
        for r, c, w4, h4, shape, answers in R.walk_tile(0, mi_rows, 0, mi_cols, partition):
            blocks[(r, c, w4, h4)] = answers
            stats[('tree', w4, h4)] = stats.get(('tree', w4, h4), 0) + 1
        seen = set()
        dims = lambda code: (1 << code, 1 << code) if code <= 4 else ((1, 2) if code == 5 else (2, 1))
        for kind, r, c, code, ar, bl, br, bc, bcode in buf[:n].tolist():
            w4, h4 = dims(code)
            if kind == 0:
                if (r, c, w4, h4) not in blocks:
                    continue                                       # a trial that did not end in the tree
                seen.add((r, c, w4, h4))
                ans, cells = blocks[(r, c, w4, h4)], [((r - 1, c + w4), ar), ((r + h4, c - 1), bl)]
            else:
                blk = (br, bc) + dims(bcode)
                if blk not in blocks:
                    continue                                       # a sub-block of a trial block that is not in the tree
                inside = lambda pr, pc: blk[0] <= pr < blk[0] + blk[3] and blk[1] <= pc < blk[1] + blk[2]
                ans, cells = blocks[blk], [(cell, v) for cell, v in (((r - 1, c + w4), ar), ((r + h4, c - 1), bl)) if not inside(*cell)]
            for cell, v in cells:
                want = ans.get(cell, 0)                            # a cell outside the tile is not available
                stats[('oracle', kind, want)] = stats.get(('oracle', kind, want), 0) + 1
                if v != want and len(problems) < 6:
                    problems.append('kind %d block (%d,%d) %dx%d, cell %s: the oracle read %d, the reference map holds %d' % (kind, r, c, w4 * 4, h4 * 4, cell, v, want))
        if seen != set(blocks):
            problems.append('%d blocks of the tree were never visited' % len(set(blocks) - seen))
        rows.append((name, problems))
    # what the runs reach: every block shape in a tree, and both answers for blocks and for sub-blocks
    missing = [k for k in [('tree', 1, 1), ('tree', 2, 2), ('tree', 4, 4), ('tree', 8, 8), ('tree', 16, 16), ('tree', 1, 2), ('tree', 2, 1)] + [('oracle', k, v) for k in (0, 1) for v in (0, 1)]
               if not stats.get(k)]
    rows.append(('walker runs reach every shape and answer', ['never reached: %s' % (k,) for k in missing]))
    return rows


# ---------------------------------------------------------------- the reference against the oracle
def reference_against_oracle(L, group):
    """[(case, problems)]: the reference's results against the oracle's on every case of `group` the oracle can express -- the prediction of every block (the raw
    edges through the predictions that copy them: V, H and Paeth rows), chroma from luma, SATD and SSE.  The psychovisual distortion has no reference of its own."""
    import ctypes as C
    rows = []
    if group == 'availability':
        return walker_against_oracle(L)
    if group in PRED_GROUPS:
        fn = L.av1o_test_predict
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4
        cases, P = prediction_cases(group)
        seen = set()
        for c in cases:
            ref = reference(P, c)
            plane, luma = np.ascontiguousarray(_frame(P, c)), np.ascontiguousarray(_frame(P, c, 'luma')) if c['op'] == H.CFL else None
            for g, p in enumerate(ref['preds']):
                if p is None:
                    continue
                if c['op'] in (H.GDIR4, H.GDIR8):      # a row's angle as a mode and a delta
                    m, d = next((m, d) for m, d in ANGLES if _angle(m, d) == c['mode'][g])
                else:
                    m, d = (c['mode'][g], 0) if c['op'] in (H.GNON4, H.GNON8) else (c['mode'][0], c['delta'][0])
                par = [c['w'], c['h'], c['bd'], c['x'], c['y'], c['wl'], c['hl'], c['have_left'], c['have_above'], c['have_ar'], c['have_bl'], m, d, c['ftype'], int(c['op'] == H.CFL), c['alpha']]
                key = (c['_kind'], c['_luma'], tuple(par))
                if key in seen:
                    continue
                seen.add(key)
                dst = np.zeros((1 << c['hl'], 1 << c['wl']), np.uint16)
                rc = fn(np.asarray(par, np.int32).ctypes.data, (luma if luma is not None else plane).ctypes.data, plane.ctypes.data, dst.ctypes.data)
                problems = ['the oracle refuses the case (%d)' % rc] if rc else []
                if not rc and not np.array_equal(dst, np.asarray(p, np.uint16)):
                    i, j = np.argwhere(dst != np.asarray(p, np.uint16))[0]
                    problems.append('pred[%d][%d]: reference %d, oracle %d' % (i, j, p[i][j], dst[i, j]))
                rows.append((_name(c) + ' row %d' % g, problems))
        return rows
    fn = L.av1o_test_distortion
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for i, (op, w, h, bd, blocks) in enumerate(distortion_cases(group)[2]):
        if op == H.PSY:
            continue
        s = np.ascontiguousarray(blocks[0], dtype=np.uint16)
        for g in range(len(blocks) - 1):
            p = np.ascontiguousarray(blocks[1 + g], dtype=np.uint16)
            want = R.sse(s, p) if op == H.SSE else R.satd(s, p, w, h)
            got = fn(s.ctypes.data, p.ctypes.data, w, h, int(op == H.SSE))
            rows.append(('op%d %dx%d bd%d case %d row %d' % (op, w, h, bd, i, g), [] if got == want else ['reference %d, oracle %d' % (want, got)]))
    return rows


# ---------------------------------------------------------------- what the cases reach, measured on the reference alone
@functools.lru_cache(maxsize=None)
def reach():
    st = {}
    for group in PRED_GROUPS:
        cases, P = prediction_cases(group)
        for c in cases:
            reference(P, c, st)
    # the three filter kernels on an edge of the 'steps' plane
    edge = _plane(128, 128, 10, 'steps')[63, 64:64 + 33].astype(np.int64)
    outs = set()
    for s in (1, 2, 3):
        e = R.Edge()
        for i, v in enumerate(edge):
            e[i - 1] = v
        R.intra_edge_filter(e, 33, s)
        outs.add(tuple(e.run(-1, 32)))
    st['steps_plane_distinct_strengths'] = len(outs)
    av = {}
    for name, r, c, w4, h4, shape, pr, pc, v in availability_rows():
        if shape and (pr >> 1, pc >> 1) == (r >> 1, c >> 1):
            av[(shape, v)] = av.get((shape, v), 0) + 1
        if (pr, pc) in ((r - 1, c + w4), (r + h4, c - 1)):
            av[('block', (pr, pc) == (r - 1, c + w4), v)] = av.get(('block', (pr, pc) == (r - 1, c + w4), v), 0) + 1
    st['availability'] = av
    return st
