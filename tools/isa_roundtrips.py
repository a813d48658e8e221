#!/usr/bin/env python3
"""tools/isa_roundtrips.py FILE.s [name filter ...]: the dependent memory round trips of the tile search's functions, counted in the compiled code.

A round trip is an `s_waitcnt` that names `vmcnt` and follows at least one flat_ / global_ / scratch_ / buffer_ load since the previous such wait: a point where
the wave stands until memory has answered.  Instructions are taken in text order (no control flow is followed) and a function is split into segments at its
`s_barrier`s: the first segment of a block search is its head, which every wave of the workgroup waits out.  Per function: the round trips per segment and in
all, and the counts of scratch_load / scratch_store / v_readlane / v_writelane (what spilled wave-uniform state costs around the calls).

Without a file it prints the command that writes the listing (the product's flags, the headline configuration's instantiations only, device code as text)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_FILTERS = ['try_block', 'tile_search_kernel']
LOAD = re.compile(r'^(flat|global|scratch|buffer)_load')
LABEL = re.compile(r'^([A-Za-z_$][\w$.]*):')


def compile_command(out='mi_avif_k1.s'):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    flags = [f for f in HIPCC_FLAGS if f != '-shared']
    return ['hipcc'] + flags + ['-Wno-pass-failed', '-DMI_FAST_BUILD', '--cuda-device-only', '-S', '-o', out, os.path.join('cavif_rs_amd', 'csrc', 'mi_avif.hip'), '-Iinclude']


def demangle(names):
    try:
        p = subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-cxxfilt'] if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-cxxfilt') else ['c++filt'],
                           input='\n'.join(names), capture_output=True, text=True, check=True)
        out = p.stdout.splitlines()
        return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}
    except Exception:
        return {n: n for n in names}


def functions(path):
    """(name, instruction lines) per function: from a global label that a `.type NAME,@function` announced to its `.Lfunc_end`."""
    funcs, announced, cur, body = [], set(), None, []
    with open(path) as fh:
        for line in fh:
            s = line.strip()
            if s.startswith('.type') and '@function' in s:
                announced.add(s.split()[1].split(',')[0])
                continue
            m = LABEL.match(s)
            if m and m.group(1) in announced and cur is None:
                cur, body = m.group(1), []
                continue
            if cur is not None:
                if s.startswith('.Lfunc_end'):
                    funcs.append((cur, body))
                    cur = None
                elif s and not s.startswith(('.', ';')) and not LABEL.match(s):
                    body.append(s.split(';')[0].strip())
    return funcs


def count(body):
    segs, trips, pending = [], 0, False
    c = {'scratch_load': 0, 'scratch_store': 0, 'v_readlane': 0, 'v_writelane': 0}
    for ins in body:
        op = ins.split()[0]
        for key in c:
            if op.startswith(key):
                c[key] += 1
        if LOAD.match(op):
            pending = True
        elif op == 's_waitcnt' and 'vmcnt' in ins:
            if pending:
                trips += 1
            pending = False
        elif op == 's_barrier':
            segs.append(trips)
            trips = 0
    segs.append(trips)
    return segs, c


def report(path, filters):
    funcs = [(n, b) for n, b in functions(path)]
    names = demangle([n for n, _ in funcs])
    rows = []
    for n, b in funcs:
        d = names[n]
        if not any(f in d for f in filters):
            continue
        segs, c = count(b)
        rows.append((d, segs, c))
    for d, segs, c in rows:
        short = re.sub(r'^(void|long long) ', '', d).split('(')[0]
        print('%s\n  round trips: %d before the first barrier, %d in all; per barrier segment: %s' % (short, segs[0], sum(segs), ' '.join(str(s) for s in segs)))
        print('  scratch_load %d  scratch_store %d  v_readlane %d  v_writelane %d' % (c['scratch_load'], c['scratch_store'], c['v_readlane'], c['v_writelane']))
    return rows


if __name__ == '__main__':
    print('# listing: ' + ' '.join(compile_command()))
    if len(sys.argv) < 2:
        sys.exit(0)
    report(sys.argv[1], sys.argv[2:] or DEFAULT_FILTERS)
