"""How an adapter wave's four 16-lane groups share its CDF rows (tile_entropy.h k4_row_group): the oracle's symbol histogram per row offset and tile
(AV1O_SYM_HIST, as tools/k4_row_balance.py) on the same three picture kinds; candidate group functions are compared by the share of a tile's adaptive
symbols that the busiest (wave, group) pair carries, for two and for four adapter waves (k4_row_owner stays as it is).  The ratio of that share to the
busiest adapter's share today is the predicted ratio of serial adapter steps (the histogram ignores order and chunking: a lower bound on the steps).
CPU only.   python tools/k4_group_balance.py [--search]"""
import sys, numpy as np
sys.path.insert(0, '.')
from tools.k4_row_balance import hist
from tests.helpers import oracle
from cavif_rs_amd.synth import synth_image

ROWS = np.arange(65536, dtype=np.uint32)
owner = lambda r, na: (r // 5 + r // 210) & (na - 1)

def cands():
    q = lambda r: r // 5 + r // 210
    out = {}
    for s in (1, 2, 3):
        out['(q >> %d) & 3' % s] = lambda r, s=s: (q(r) >> s) & 3
    for m in (3, 5, 7, 9, 11, 13):
        for s in (2, 3, 4):
            out['((q * %d) >> %d) & 3' % (m, s)] = lambda r, m=m, s=s: ((q(r) * m) >> s) & 3
    for d in (20, 40, 42, 84, 105, 210, 420):
        for s in (1, 2):
            out['((q >> %d) + row / %d) & 3' % (s, d)] = lambda r, d=d, s=s: ((q(r) >> s) + r // d) & 3
    for d in (3, 7, 10, 15):
        out['(row / %d) & 3' % d] = lambda r, d=d: (r // d) & 3
    return out

def shares(h, group, na):
    """mean over tiles of: busiest adapter's share, busiest (adapter, group)'s share"""
    o, g = owner(ROWS, na), group(ROWS) & 3
    tot = h.sum(axis=1).astype(np.float64)
    wave = np.stack([(h * (o == a)).sum(axis=1) for a in range(na)], 1)
    pair = np.stack([(h * ((o == a) & (g == k))).sum(axis=1) for a in range(na) for k in range(4)], 1)
    ok = tot > 0
    return (wave.max(axis=1)[ok] / tot[ok]).mean(), (pair.max(axis=1)[ok] / tot[ok]).mean()

# tile_entropy.h k4_row_group (tests/helpers/k4_grouped_streams.py mirrors it)
K4_ROW_GROUP = '((q >> 1) + row / 210) & 3'

if __name__ == '__main__':
    oracle.build(); oracle.lib()
    sets = {'config-5 like (1280x832, speed 1, q80, 10-bit)': hist(synth_image(1280, 832, index=5), quality=80, speed=1, depth=10),
            'config-4 like (1920x1080, speed 4, q80, 10-bit)': hist(synth_image(1920, 1080, index=0), quality=80, speed=4, depth=10),
            'config-3 like (1024x1024 RGBA, speed 4, q80)': hist(synth_image(1024, 1024, index=3, alpha=True), quality=80, alpha_quality=90, speed=4)}
    C = cands()
    table = []
    for name, f in C.items():
        worst, line = 0.0, []
        for h in sets.values():
            for na in (2, 4):
                w, p = shares(h, f, na)
                line.append((w, p)); worst = max(worst, p / w)
        table.append((worst, name, line))
    table.sort()
    pick = table if '--search' in sys.argv else [t for t in table if t[1] == K4_ROW_GROUP]
    print('picture kinds:', ' | '.join(sets))
    print('per kind and NA = 2, 4: busiest adapter share % -> busiest (adapter, group) share %;  worst ratio over the six')
    for worst, name, line in pick[:16]:
        print('%-32s %s   worst ratio %.3f' % (name, '  '.join('%4.1f -> %4.1f' % (100 * w, 100 * p) for w, p in line), worst))
