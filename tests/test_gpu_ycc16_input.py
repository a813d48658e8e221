"""-m gpu: deep YCbCr input on the MI355X through the product library -- the case table of tests/helpers/ycc16_cases.py (every sample value through the ingest
map, uint16 planes into deep slots, the kind-3 front end, files against the oracle, mixed batches, refusals) and uint16 torch tensors through the Python entry
points.  Nothing is wider than 517 pixels but the 256 x 256 pictures that hold every value: the kernels have no size-dependent path beyond the workgroup
boundary that width crosses."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'ycc16_cases.py')
pytest.importorskip('PIL.Image')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, *prefixes):
    from tests.helpers.ycc16_cases import expected_rows
    want = expected_rows()
    for prefix in prefixes:
        mine = [r for r in rows if r['case'].startswith(prefix)]
        bad = [r for r in mine if not r['ok']]
        assert not bad, bad
        assert len(mine) == want[prefix], (prefix, [r['case'] for r in mine])


def test_every_sample_value_through_the_ingest_map(table):
    _of(table, 'values')


def test_uint16_planes_fill_the_deep_slots(table):
    _of(table, 'ingest')


def test_strides_of_zero_mean_packed(table):
    _of(table, 'defaults')


def test_kind_3_front_end_writes_the_specified_planes(table):
    _of(table, 'front')


def test_files_equal_the_oracle_over_the_restated_planes(table):
    _of(table, 'files oracle', 'files:')


def test_kinds_0_to_3_share_a_batch(table):
    _of(table, 'mixed')


def test_deep_ycbcr_is_refused_with_invalid_argument(table):
    _of(table, 'refused', 'accepted')


def test_torch_uint16_planes_through_encoder_and_batch_encoder():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch')
