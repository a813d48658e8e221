"""The tile search's lookups on row-uniform small integers (dr_deriv_dev, edge_strength_dev, edge_upsample_sel_dev, dr_dxdy_dev, dr_dxdy_uni, sm_weights_dev of dev_predict.h;
txtype_to_sym of dev_common.h) are straight-line code on packed immediates.  Here each is compared with a restatement of the switch / if form it replaced
(tests/kernels/k1_lookups_main.cpp), exhaustively: angles -10..280 for the derivative and for a row's (dx, dy) in both its forms (packed immediates; the table
read with a scalar load for wave-uniform angles, dr_dxdy_uni), every directional mode x angle delta for the same, (w, h) in {4, 8, 16, 32, 64}^2 x filter
type x delta -135..135 for filter strength and upsampling, every (tx set, transform type), every smooth weight.
On the CPU the stand-alone program compares both forms; on the GPU one launch evaluates the new forms with one argument per lane (different arguments in
every lane of a row and every row of a wave) and the values are compared with the restatements' exactly."""
import numpy as np
import pytest

from tests.helpers import k1_lookups_harness as H

N_DERIV, N_EDGE, N_ROW, N_TXSYM, N_SMW = 291, 25 * 2 * 271, 56, 48, 124
TOTAL = N_DERIV + 2 * N_EDGE + 2 * (N_ROW + N_DERIV) + N_TXSYM + N_SMW


@pytest.fixture(scope='module')
def cpu(tmp_path_factory):
    return H.run_cpu(str(tmp_path_factory.mktemp('k1_lookups')))


def test_new_forms_equal_the_earlier_forms_over_the_whole_domain(cpu):
    status, text, want = cpu
    assert status == 0, text
    assert 'checked %d mismatches 0' % TOTAL in text, text
    assert 'per operation: %d %d %d %d %d %d %d %d %d' % (N_DERIV, N_EDGE, N_EDGE, N_ROW, N_DERIV, N_ROW, N_DERIV, N_TXSYM, N_SMW) in text, text
    assert want.size == TOTAL


def test_the_restatements_are_the_spec_tables(cpu):
    """the reference itself: a few values of the restatements against the AV1 specification's tables, so that a slip copied into both forms would show"""
    _, _, want = cpu
    deriv = {a: int(want[a + 10]) for a in range(-10, 281)}
    assert sum(1 for v in deriv.values() if v) == 27 and deriv[3] == 1023 and deriv[45] == 64 and deriv[87] == 3 and deriv[14] == 273 and deriv[0] == 0 and deriv[90] == 0
    row = want[N_DERIV + 2 * N_EDGE:][:N_ROW].reshape(8, 7)                 # modes V, H, D45, D135, D113, D157, D203, D67 x delta -3..3
    assert row[0, 3] == 0 and row[1, 3] == 0                                # V and H: no derivative
    assert row[2, 3] == 64 and row[3, 3] == (64 | 64 << 16) and row[5, 3] == (151 | 27 << 16) and row[6, 3] == 27 << 16 and row[7, 3] == 27
    assert row[0, 2] == 3 and row[0, 4] == (3 | 1023 << 16)                 # 87 and 93 degrees


@pytest.mark.gpu
def test_gpu_values_equal_the_earlier_forms_with_a_different_argument_in_every_lane(cpu):
    status, text, want = cpu
    assert status == 0, text
    got = H.run_gpu()
    assert got.size == want.size == TOTAL
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, 'first differing arguments %s: got %s, expected %s' % (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
