"""Child-process side of the quality-metric tests (TEST INFRASTRUCTURE): the case table, a numpy restatement of the metric specification and the
runs over the library under test (tests/test_quality_emu.py: the SIMT-emulated build; tests/test_gpu_quality.py: the product library), one JSON line per case.

    python tests/helpers/quality_cases.py ROOT sizes|settings|alpha|source|refusals|search|measured|all|large|torch

The expected integers come from the restatement below, applied to the planes the library hands out (BatchEncoder.source / .recon); every comparison is for
equality and no case is excused.  tests/test_quality_reference.py holds the restatement itself against known answers.
"""
import ctypes as C
import math
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import emit      # noqa: E402

# w x h: one window; no window (sse still exact); partial 4 x 4 cells at the edge; one 64 x 64 tile of the kernel; windows that straddle its tile edge (one tile
# plus 3 samples and more, on either axis); several tiles both ways
SIZES = ((8, 8), (7, 9), (16, 5), (9, 8), (12, 11), (64, 64), (67, 70), (130, 66), (200, 136))
DEPTHS = (8, 10)
SEARCH = dict(size=(64, 48), lo=60, hi=67)
INVALID = 4
ONE = 1 << 30


# ---------------------------------------------------------------- the specification, restated
def ssim_constants(bd):
    return (26634, 239708) if bd == 8 else (428658, 3857925)


def window_sums(s, r):
    """S, R, SS, RR, SR (int64, one entry per window) of the 8 x 8 windows at (4 i, 4 j) that lie inside the planes; None when there is none"""
    s, r = s.astype(np.int64), r.astype(np.int64)
    h, w = s.shape
    if w < 8 or h < 8:
        return None

    def win(a):
        return np.lib.stride_tricks.sliding_window_view(a, (8, 8))[::4, ::4].sum(axis=(2, 3))
    return win(s), win(r), win(s * s), win(r * r), win(s * r)


def restate_plane(s, r, bd):
    """(sse, ssim_sum, ssim_windows) of one plane: Python integers"""
    d = s.astype(np.int64) - r.astype(np.int64)
    sse = int((d * d).sum())
    sums = window_sums(s, r)
    h, w = s.shape
    windows = ((w - 8) // 4 + 1) * ((h - 8) // 4 + 1) if w >= 8 and h >= 8 else 0
    if sums is None:
        return sse, 0, 0
    S, R, SS, RR, SR = sums
    assert S.size == windows
    c1, c2 = ssim_constants(bd)
    fa, fb, fc, fd = 2 * S * R + c1, 128 * SR - 2 * S * R + c2, S * S + R * R + c1, 64 * SS - S * S + 64 * RR - R * R + c2
    assert max(int(np.abs(x).max()) for x in (fa, fb, fc, fd)) < 1 << 53
    n = fa.astype(np.float64) * fb.astype(np.float64)
    m = fc.astype(np.float64) * fd.astype(np.float64)
    q = n / m
    fixed = np.floor(q * 1073741824.0 + 0.5).astype(np.int64)
    return sse, int(fixed.sum()), windows


def textbook_mean_ssim(s, r, bd):
    """the mean over the same windows of SSIM written the usual way, in float64: means, biased variances and covariance of the 64 samples"""
    S, R, SS, RR, SR = (x.astype(np.float64) for x in window_sums(s, r))
    peak = float((1 << bd) - 1)
    k1, k2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    mu_s, mu_r = S / 64, R / 64
    var_s, var_r, cov = SS / 64 - mu_s * mu_s, RR / 64 - mu_r * mu_r, SR / 64 - mu_s * mu_r
    v = (2 * mu_s * mu_r + k1) * (2 * cov + k2) / ((mu_s * mu_s + mu_r * mu_r + k1) * (var_s + var_r + k2))
    return float(v.mean())


def expected_report(b, i, bd, alpha):
    """[(sse, ssim_sum, windows) per colour plane], the alpha plane's triple or None"""
    col = [restate_plane(s, r, bd) for s, r in zip(b.source(i), b.recon(i))]
    al = restate_plane(b.source(i, alpha=True)[0], b.recon(i, alpha=True)[0], bd) if alpha else None
    return col, al


def triples(q):
    return [(p.sse, p.ssim_sum, p.ssim_windows) for p in q.planes], (None if q.alpha is None else (q.alpha.sse, q.alpha.ssim_sum, q.alpha.ssim_windows))


def psnr_db(sse, n, bd):
    return math.inf if sse == 0 else 10.0 * math.log10(float((1 << bd) - 1) ** 2 * n / sse)


def content(seed, h, w, c=3):
    """a diagonal ramp under noise: lossy at every quality the cases use"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 3 + y * 5) % 256)[..., None] + rng.integers(-40, 41, (h, w, c))
    return np.clip(base, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- the library under test
class Lib:
    def __init__(self, root):
        import cavif_rs_amd as m
        self.m, self.L = m, m.load_library()


def measured_batch(m, enc, images, channels=3):
    h, w = images[0].shape[:2]
    b = m.BatchEncoder(enc, len(images), w, h, channels)
    for i, im in enumerate(images):
        b.upload(i, im)
    b.encode()
    return b, b.measure()


def check_images(b, reports, bd, alphas):
    """every image's report against the restatement; returns (all equal, the expected triples)"""
    ok, want = True, []
    for i, q in enumerate(reports):
        exp = expected_report(b, i, bd, alphas[i])
        want.append(exp)
        ok = ok and triples(q) == exp and (q.width, q.height, q.depth) == (b.w, b.h, bd)
    return ok, want


def run_sizes(lib, sizes=SIZES):
    m = lib.m
    for (w, h) in sizes:
        for bd in DEPTHS:
            e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd)
            b, rep = measured_batch(m, e, [content(w * 1000 + h + bd, h, w)])
            ok, want = check_images(b, rep, bd, [False])
            col = want[0][0]
            windows = ((w - 8) // 4 + 1) * ((h - 8) // 4 + 1) if w >= 8 and h >= 8 else 0
            emit('size %dx%d %d bit' % (w, h, bd), ok and all(t[2] == windows for t in col) and sum(t[0] for t in col) > 0 and len(col) == 3,
                 got=triples(rep[0])[0], want=col)
            b.close()


def speed_without_lrf(m, quality):
    q = m.quality_to_quantizer(quality)
    for speed in range(10, 0, -1):
        if not m.tweaks_from_preset(speed, q)['lrf']:
            return speed
    return None


def run_settings(lib):
    m = lib.m
    w, h = 72, 40
    quality = 60
    no_lrf = speed_without_lrf(m, quality)
    lrf4 = m.tweaks_from_preset(4, m.quality_to_quantizer(quality))['lrf']
    cases = [('speed 4 (lrp is the reconstruction)', m.Encoder().with_speed(4).with_bit_depth(10), 10, bool(lrf4)),
             ('speed %s without loop restoration (fin is the reconstruction)' % no_lrf, m.Encoder().with_speed(no_lrf or 10).with_bit_depth(8), 8, no_lrf is not None),
             ('RGB colour model', m.Encoder().with_speed(10).with_bit_depth(10).with_internal_color_model('rgb'), 10, True),
             ('rdo_passes = 2', m.Encoder().with_speed(10).with_bit_depth(8).with_rdo_passes(2), 8, True)]
    for k, (name, e, bd, precondition) in enumerate(cases):
        b, rep = measured_batch(m, e.with_quality(quality), [content(77 + k, h, w)])
        ok, want = check_images(b, rep, bd, [False])
        emit('setting: ' + name, ok and precondition and sum(t[0] for t in want[0][0]) > 0, got=triples(rep[0])[0], want=want[0][0])
        b.close()


def alpha_images(w, h):
    """three different RGBA pictures, the middle one opaque"""
    out = []
    for i in range(3):
        px = content(300 + i, h, w, 4)
        px[..., 3] = 255 if i == 1 else np.clip(px[..., 3].astype(np.int64) + 60 * i, 0, 255)
        out.append(px)
    return out


def run_alpha(lib):
    m = lib.m
    w, h, bd = 40, 24, 10
    e = m.Encoder().with_speed(10).with_quality(60).with_alpha_quality(50).with_bit_depth(bd)
    imgs = alpha_images(w, h)
    b, rep = measured_batch(m, e, imgs, 4)
    alphas = [True, False, True]
    ok, want = check_images(b, rep, bd, alphas)
    distinct = len({repr(x) for x in want}) == 3 and want[0][1] != want[2][1]
    emit('alpha: three RGBA images, one opaque', ok and [q.alpha is not None for q in rep] == alphas and distinct and want[0][1][0] > 0, got=[triples(q) for q in rep], want=want)
    first = [triples(q) for q in rep]
    b.set_count(2)
    refused = b._L.mi_batch_measure(b._h)                                           # the planes on the device belong to a run of three
    b.encode()
    rep = b.measure()
    ok, want = check_images(b, rep, bd, alphas[:2])
    emit('alpha: the same batch after set_count(2)', ok and len(rep) == 2 and refused == INVALID and [triples(q) for q in rep] == first[:2], got=[triples(q) for q in rep], want=want)
    b.close()


def run_source(lib):
    m = lib.m
    w, h = 12, 11
    for bd in DEPTHS:
        e = m.Encoder().with_speed(10).with_bit_depth(bd).with_alpha_color_mode('dirty')
        px = content(40 + bd, h, w, 4)
        px[..., 3] = np.random.default_rng(bd).integers(0, 256, (h, w))
        b3, _ = measured_batch(m, e, [px[..., :3]])
        want = np.array([[m.rgb_to_ycbcr(tuple(int(v) for v in px[y, x, :3]), bd) for x in range(w)] for y in range(h)], np.uint16)
        src = b3.source(0)
        ok = len(src) == 3 and all(np.array_equal(src[p], want[..., p]) for p in range(3))
        b3.close()
        b4, rep = measured_batch(m, e, [px], 4)
        a = px[..., 3].astype(np.uint16)
        ok = ok and rep[0].alpha is not None and np.array_equal(b4.source(0, alpha=True)[0], a if bd == 8 else (a << 2) | (a >> 6))
        b4.close()
        emit('source planes %d bit' % bd, ok)


def run_refusals(lib):
    m, L = lib.m, lib.L
    from cavif_rs_amd.encoder import _ImageQuality
    w, h = 16, 8
    e = m.Encoder().with_speed(10)
    b = m.BatchEncoder(e, 2, w, h, 3)
    q = _ImageQuality()
    for i in range(2):
        b.upload(i, content(5 + i, h, w))
    emit('refused: measure and get_quality before any encode', [L.mi_batch_measure(b._h), L.mi_batch_get_quality(b._h, 0, C.byref(q))] == [INVALID] * 2)
    b.encode_async()
    st = L.mi_batch_measure(b._h)
    b.wait()
    emit('refused: measure between encode_async and wait', st == INVALID)
    before = L.mi_batch_get_quality(b._h, 0, C.byref(q))
    ok = L.mi_batch_measure(b._h) == 0 and L.mi_batch_get_quality(b._h, 1, C.byref(q)) == 0
    b.encode()
    after = L.mi_batch_get_quality(b._h, 0, C.byref(q))
    emit('refused: get_quality before a measure and after a new encode without one', ok and [before, after] == [INVALID] * 2, statuses=[before, after])
    ok = L.mi_batch_measure(b._h) == 0
    emit('refused: an index out of range', ok and [L.mi_batch_get_quality(b._h, 2, C.byref(q)), L.mi_batch_get_quality(b._h, -1, C.byref(q))] == [INVALID] * 2)
    src = (C.POINTER(C.c_uint16) * 3)()
    emit('refused: null pointers', [L.mi_batch_measure(None), L.mi_batch_get_quality(None, 0, C.byref(q)), L.mi_batch_get_quality(b._h, 0, None),
                                    L.mi_batch_get_source(None, 0, 0, src), L.mi_batch_get_source(b._h, 0, 0, None)] == [INVALID] * 5 and
         math.isnan(L.mi_quality_psnr_db(None)) and math.isnan(L.mi_quality_ssim_db(None)))
    b.close()


def bisect(table, target, lo, hi):
    """Encoder.encode_to_target restated over a table quality -> metric: (quality, reached, tried)"""
    tried = [(hi, table[hi])]
    if table[hi] < target:
        return hi, False, tried
    l, h = lo, hi
    while l < h:
        mid = (l + h) // 2
        if (mid, table[mid]) not in tried:
            tried.append((mid, table[mid]))
        if table[mid] >= target:
            h = mid
        else:
            l = mid + 1
    return h, True, tried


def run_search(lib):
    m = lib.m
    (w, h), lo, hi = SEARCH['size'], SEARCH['lo'], SEARCH['hi']
    e = m.Encoder().with_speed(10)
    px = content(99, h, w)
    direct = {q: e.with_quality(q).encode_measured(px) for q in range(lo, hi + 1)}
    for metric in ('ssim', 'psnr'):
        table = {q: (r.ssim_db if metric == 'ssim' else r.psnr_db) for q, (_, r) in direct.items()}
        vals = sorted(table.values())
        targets = {'inside': (vals[3] + vals[4]) / 2, 'above metric(hi)': table[hi] + 0.5, 'below metric(lo)': min(vals) - 0.5}
        for name, target in targets.items():
            got = e.encode_to_target(px, target, metric=metric, lo=lo, hi=hi)
            q, reached, tried = bisect(table, target, lo, hi)
            ok = (got.quality, got.reached, got.tried) == (q, reached, tried) and len(tried) <= 8
            ok = ok and got.image.avif_file == e.with_quality(got.quality).encode_rgb(px).avif_file and got.quality_report == direct[got.quality][1]
            if name == 'above metric(hi)':
                ok = ok and not got.reached and got.quality == hi
            if name == 'below metric(lo)':
                ok = ok and got.reached and got.quality == lo
            emit('search: %s, target %s' % (metric, name), ok, target=target, quality=got.quality, tried=got.tried, table=table)
    try:
        e.encode_to_target(content(1, 9, 7), 10.0, metric='ssim')
        raised = False
    except ValueError:
        raised = True
    emit('search: ssim on a 7x9 picture raises', raised)


def run_measured(lib):
    m = lib.m
    e = m.Encoder().with_speed(10).with_quality(70)
    ok = True
    for c in (3, 4):
        px = content(11 + c, 24, 40, c)
        img, rep = e.encode_measured(px)
        b, batch = measured_batch(m, e, [px], c)
        ok = ok and img.avif_file == (e.encode_rgb if c == 3 else e.encode_rgba)(px).avif_file and rep == batch[0] and (rep.alpha is not None) == (c == 4)
        # the host conversions against the C helpers and against the restated definitions
        cq = rep._c()
        for mine, theirs in ((rep.psnr_db, lib.L.mi_quality_psnr_db(C.byref(cq))), (rep.ssim_db, lib.L.mi_quality_ssim_db(C.byref(cq))),
                             (rep.psnr_db, psnr_db(sum(rep.sse), 3 * 24 * 40, 10)), (rep.ssim, rep.ssim_sum[0] / ONE / rep.ssim_windows[0])):
            ok = ok and math.isclose(mine, theirs, rel_tol=1e-12)
        b.close()
    emit('measured: encode_measured gives the file of encode_rgb / encode_rgba and the batch path\'s report', ok)


def run_large(lib):
    """the product library only: one 1920 x 1080 image (addresses at full size)"""
    from cavif_rs_amd.synth import synth_image
    m = lib.m
    e = m.Encoder().with_speed(10).with_quality(60)
    b, rep = measured_batch(m, e, [synth_image(1920, 1080, index=1)])
    ok, want = check_images(b, rep, 10, [False])
    emit('large: 1920x1080', ok and want[0][0][0][2] == 479 * 269, got=triples(rep[0])[0], want=want[0][0])
    b.close()


def run_torch(lib):
    """the product library only: the report of a torch-tensor input equals that of the same pixels uploaded from the host"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10).with_quality(60)
    for c in (3, 4):
        px = content(500 + c, 70, 67, c)
        img_t, rep_t = e.encode_measured(torch.from_numpy(px).cuda())
        img_h, rep_h = e.encode_measured(px)
        emit('torch: encode_measured of a %d-channel tensor' % c, rep_t == rep_h and img_t.avif_file == img_h.avif_file and sum(rep_h.sse) > 0)


RUNS = {'sizes': run_sizes, 'settings': run_settings, 'alpha': run_alpha, 'source': run_source, 'refusals': run_refusals, 'search': run_search, 'measured': run_measured}


def main():
    root, which = sys.argv[1], sys.argv[2]
    if which == 'torch':
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else which.split(',')):
        if name == 'torch':
            run_torch(lib)
        elif name == 'large':
            run_large(lib)
        elif name.startswith('sizes:'):                                             # one size of the table by its index
            run_sizes(lib, (SIZES[int(name[6:])],))
        else:
            RUNS[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
