"""kzg::commit_batch / kzg::open_batch of the host mirror through keaki_amd/keaki.py: equal to the loops over commit / open on both sides of
COMMIT_BATCH_MIN, polynomials of unequal lengths, and PolynomialTooLarge raised first."""
import numpy as np
import pytest

from conftest_helpers import rand_fr_ints
from test_gpu_parity import mont

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def setup(oc):
    from keaki_amd import keaki as K
    s = K.KZGSetup.setup(mont(oc, [0x1234567890abcdef1122334455667788 % R])[0], 300)
    yield K, s
    s.close()


def _polys(oc, m, lengths, seed):
    return [mont(oc, rand_fr_ints(lengths[j % len(lengths)], seed + j)) for j in range(m)]


def test_commit_and_open_batch_equal_the_loops(oc, setup):
    K, s = setup
    mn = K.commit_batch_min()
    assert mn >= 1
    for m in sorted({1, max(1, mn - 1), mn, mn + 1, 9}):
        polys = _polys(oc, m, [300, 1, 33, 257], 10 * m)
        polys[-1] = np.concatenate([polys[-1], np.zeros((2, 4), np.uint64)])[:300]       # trailing zeros are not part of a polynomial
        zs = mont(oc, rand_fr_ints(m, 99 + m))
        coms, proofs = K.commit_batch(s, polys), K.open_batch(s, polys, zs)
        for j in range(m):
            assert np.array_equal(coms[j], K.commit(s, polys[j])), "commit %d of %d" % (j, m)
            assert np.array_equal(proofs[j], K.open(s, polys[j], zs[j])), "open %d of %d" % (j, m)
    assert K.commit_batch(s, []).shape == (0, 8)


def test_polynomial_too_large_is_raised_first(oc, setup):
    K, s = setup
    ok, long = mont(oc, rand_fr_ints(5, 1)), mont(oc, rand_fr_ints(301, 2))
    with pytest.raises(K.KZGError) as e:                     # KZGError::PolynomialTooLarge(degree, max_degree)
        K.commit_batch(s, [ok, long, ok])
    assert e.value == K.KZGError(301, 300)
    assert K.commit_batch(s, [ok, long[:300], ok]).shape == (3, 8)
    # open: the QUOTIENT's length counts (301 coefficients leave 300 terms: fits), 302 do not
    assert K.open_batch(s, [ok, long], mont(oc, [5, 6])).shape == (2, 8)
    with pytest.raises(K.KZGError):
        K.open_batch(s, [ok, mont(oc, rand_fr_ints(302, 3))], mont(oc, [5, 6]))
