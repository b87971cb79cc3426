"""CPU suite: the formula keaki_amd/csrc/kzg_multi.hip restates, in Python integers (tests/kzg_set_model.py). Z, the weights and I are checked
against their definitions; schoolbook long division of p - I by Z is exact and equals the partial-fraction sum coefficient by coefficient; the top
k - 1 coefficients vanish. n <= 200, k <= 12."""
import pytest

import kzg_set_model as M
from conftest import rand_fr_ints

R = M.R
OMEGA8 = pow(5, (R - 1) // 8, R)


def structured_points(k):
    """0, 1, r - 1, then eighth roots of unity, then small integers: distinct"""
    pts = [0, 1, R - 1] + [pow(OMEGA8, i, R) for i in (1, 2, 3, 5, 6, 7)] + [2, 3, 5]
    assert len(set(pts)) == len(pts)
    return pts[:k]


CASES = [(n, k, kind) for kind in ("random", "structured") for n, k in
         [(1, 1), (1, 3), (2, 2), (3, 2), (5, 5), (6, 5), (12, 12), (13, 12), (32, 7), (33, 8), (64, 9), (65, 1), (100, 12), (200, 12), (200, 2), (199, 11)]]


def make(n, k, kind):
    r = rand_fr_ints(n + k, 77 * n + k)
    p = r[:n]
    if kind == "structured":
        p = [0 if i % 5 == 0 else (R - 1 if i % 7 == 0 else c) for i, c in enumerate(p)]
        p[-1] = p[-1] or 1
    zs = r[n:] if kind == "random" else structured_points(k)
    assert len(set(zs)) == k
    return p, zs


@pytest.mark.parametrize("n,k,kind", CASES)
def test_set_polynomials(n, k, kind):
    p, zs = make(n, k, kind)
    zc, cs = M.vanishing(zs), M.weights(zs)
    assert len(zc) == k + 1 and zc[-1] == 1
    assert all(M.poly_eval(zc, z) == 0 for z in zs)
    x = rand_fr_ints(1, 5)[0]
    prod = 1
    for z in zs:
        prod = prod * (x - z) % R
    assert M.poly_eval(zc, x) == prod
    dz = [(i * c) % R for i, c in enumerate(zc)][1:]                      # Z'
    assert all(c * M.poly_eval(dz, z) % R == 1 for c, z in zip(cs, zs))
    if k >= 2:
        assert sum(cs) % R == 0                                           # the x^(k-1) coefficient of sum_j c_j Z / (x - z_j) = 1
    ys = [M.poly_eval(p, z) for z in zs]
    ic = M.interpolant(zs, ys)
    assert len(ic) == k and all(M.poly_eval(ic, z) == y for z, y in zip(zs, ys))


@pytest.mark.parametrize("n,k,kind", CASES)
def test_long_division_equals_partial_fractions(n, k, kind):
    p, zs = make(n, k, kind)
    q_ld, ys = M.quotient_long_division(p, zs)                            # asserts exactness
    q_pf = M.quotient_partial_fractions(p, zs)
    assert len(q_ld) == len(q_pf) == n - 1
    assert q_ld == q_pf
    top = max(0, n - 1 - (k - 1))
    assert not any(q_pf[top:]), "the top k - 1 coefficients must vanish"
    if n <= k:
        assert not any(q_pf)
    # the relation the verifier checks, at a random evaluation point in place of tau
    tau = rand_fr_ints(1, 9)[0]
    ic = M.interpolant(zs, ys)
    lhs = (M.poly_eval(p, tau) - M.poly_eval(ic, tau)) % R
    assert lhs == M.poly_eval(q_ld, tau) * M.poly_eval(M.vanishing(zs), tau) % R


def test_single_point_is_the_ordinary_quotient():
    p = rand_fr_ints(50, 3)
    z = rand_fr_ints(1, 4)[0]
    q, v = M.divide_linear(p, z)
    assert M.weights([z]) == [1]
    assert M.quotient_partial_fractions(p, [z]) == q and M.quotient_long_division(p, [z]) == (q, [v])


def test_aggregation_of_single_proofs():
    """pi_S = sum_j c_j pi_j in the exponent, also when tau is one of the points (Z(tau) = 0)"""
    p = rand_fr_ints(40, 11)
    zs = rand_fr_ints(6, 12)
    for tau in (rand_fr_ints(1, 13)[0], zs[2]):
        single = [M.poly_eval(M.divide_linear(p, z)[0], tau) for z in zs]
        agg = sum(c * s for c, s in zip(M.weights(zs), single)) % R
        assert agg == M.set_proof_dl(p, zs, tau)
