"""-m gpu: the cases of tests/helpers/k1_roundtrip_cases.py through the product library -- block heads fetched as one batch per wave role, the walker's area copies,
the candidate evaluated last kept in the frame -- against the oracle, stream and reconstruction byte for byte.  (The emulator has no EXEC mask: what a divergent
region does to later code shows here only.)"""
import numpy as np
import pytest

from tests.helpers import k1_roundtrip_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def refs(oracle):
    out = [K.oracle_run(oracle, c) for c in K.CASES]
    K.check_inputs([r for _, r in out])              # the condition on the inputs, from the oracle alone, before anything is compared
    return out


@pytest.mark.parametrize('i', range(len(K.CASES)), ids=[c[0] for c in K.CASES])
def test_product_equals_oracle(refs, i):
    import cavif_rs_amd as m
    pl, r = refs[i]
    obu, rec = m.encode_planes(pl, **K.product_kwargs(K.CASES[i]))
    assert obu == r['obu']
    assert len(rec) == len(r['recon'])
    for a, b in zip(rec, r['recon']):
        assert np.array_equal(a, b)


def test_avif_file_equals_oracle(oracle):
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    img = synth_image(136, 72, index=7)
    got = m.Encoder().with_quality(70).with_speed(4).with_bit_depth(10).encode_rgb(img)
    assert got.avif_file == oracle.ravif_encode(img, quality=70, speed=4, depth=10)[0]
