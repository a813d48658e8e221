"""Mixed-size batches without a GPU: the cases of tests/helpers/mixed_cases.py -- frames of different sizes in one launch of the tile search, the filters and the
entropy coder -- through the emulated library (tests/emu/), in child processes as tests/test_emu_kernels.py runs its own.  Bytes equal the oracle's."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# job -> (cases of tests/emu/mixed_cases.py, extra environment); the speed-1 colour case is most of the time, so it runs beside the others
_JOBS = {'colour1': ('colour1', {}), 'rest': ('colour4,alpha,fit,stream', {}), 'colour1_reverse': ('colour1', {'MI_EMU_REVERSE': '1'}),
         'rest_reverse': ('colour4,alpha,fit,stream', {'MI_EMU_REVERSE': '1'})}


@pytest.fixture(scope='module')
def jobs(oracle):
    from tests import emu
    env = emu.env()
    script = os.path.join(ROOT, 'tests', 'emu', 'mixed_cases.py')
    procs = {j: subprocess.Popen([sys.executable, script, ROOT, which], env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for j, (which, extra) in _JOBS.items()}
    out = {}
    for j, p in procs.items():
        try:
            stdout, stderr = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            p.kill()
            stdout, stderr = p.communicate()
        out[j] = (p.returncode, [json.loads(l) for l in stdout.splitlines() if l.startswith('{')], stderr)
    return out


def _check(jobs, names, cases):
    rows = []
    for j in names:
        rc, r, stderr = jobs[j]
        assert rc == 0 and r, (j, r, stderr[-2000:])
        rows += r
    assert sorted(r['case'] for r in rows) == sorted(cases), rows
    assert all(r['ok'] for r in rows), [r for r in rows if not r['ok']]


CASES = ['colour1', 'colour4', 'alpha', 'fit', 'stream']


def test_emulated_mixed_batches_equal_the_oracle(jobs):
    """colour frames of six sizes in one launch at speeds 4 and 1, colour + alpha frames under the cleaner, the fit rule, one encode_many mixed run"""
    _check(jobs, ['colour1', 'rest'], CASES)


def test_emulated_mixed_batches_do_not_depend_on_lane_order(jobs):
    """the same once more with the emulator's lanes and waves running in reverse order (MI_EMU_REVERSE)"""
    _check(jobs, ['colour1_reverse', 'rest_reverse'], CASES)
