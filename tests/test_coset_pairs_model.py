"""CPU suite: the model of the per-item coset check (tests/coset_pairs_model.py) is right about what it states, and the inputs of the GPU tests
(tests/test_gpu_coset_pairs.py, tests/test_gpu_verify_cosets_each.py) do what they are named for."""
import pytest

import coset_pairs_model as P
import coset_verify_model as M
import fk_coset_model as FM
from conftest import rand_fr_ints

R = P.R
TAU = rand_fr_ints(1, 20261021)[0]


def vector(log2d, log2l, seed):
    r = 1 << (log2d - log2l)
    rnd = rand_fr_ints(r + (1 << log2d), seed)
    return M.vector_case(TAU, rnd[r:], log2d, log2l, rnd[:r])[0]


@pytest.mark.parametrize("log2d,log2l", [(4, 1), (6, 2), (6, 6), (5, 0), (7, 3)])
def test_pairs_satisfy_the_coset_check_of_valid_items(log2d, log2l):
    """dl(A_k) = c_k(tau) - I_k(tau) = q_k (tau^l - h_k^l): the predicate of verify_multi on coset k (coset_verify_model.Case.single)"""
    c = vector(log2d, log2l, 40 + log2d)
    tl = pow(TAU, c.l, R)
    for k in range(c.n):
        a, ck = P.pair_dl(c, k)
        assert ck == pow(c.h[k], c.l, R)
        assert (a - c.q[k] * (tl - ck)) % R == 0 and c.single(k)
        assert P.lhs_dl(c, k) == tl * c.q[k] % R and P.status(c, k) == 0
    assert P.statuses(c) == [0] * c.n


corrupt = P.corrupt


@pytest.mark.parametrize("kind", ["value", "proof", "shift", "swap"])
def test_every_corruption_of_the_gpu_tests_flips_exactly_its_items(kind):
    c = vector(6, 2, 77)
    k, k2 = 5, 11
    b = corrupt(c, kind, k, k2)
    want = [1 if i == k or (kind == "swap" and i == k2) else 0 for i in range(c.n)]
    assert P.statuses(b) == want
    assert [0 if b.single(i) else 1 for i in range(c.n)] == want          # the verdict of verify_multi item by item
    assert not b.verdict()                                                  # and verify_cosets rejects the batch


def test_gamma_combination_of_the_items_is_the_batch_equation():
    """sum_k gamma_k (dl(L_k) - tau^l q_k) = dl(L) - tau^l dl(R) of verify_cosets, valid items or not"""
    for c in (vector(5, 2, 3), corrupt(vector(5, 2, 3), "value", 2), corrupt(vector(6, 3, 4), "proof", 0)):
        per_item = sum(g * (P.lhs_dl(c, k) - c.tau_l * c.q[k]) for k, g in enumerate(c.gamma)) % R
        L, Rr = c.sums()
        assert per_item == (L - c.tau_l * Rr) % R


def test_values_from_coefficients_inverts_the_interpolant():
    for l in (1, 2, 4, 16):
        a = rand_fr_ints(l + 1, 900 + l)
        h, a = a[0], a[1:]
        y = P.values_from_coeffs(h, a)
        assert M.interpolant_coset(h, y) == a
        c = P.case_from_rows(TAU, 12345, h, P.neg_rows_to_coeffs(a))
        assert c.a(0) == a and P.pair_dl(c, 0)[0] == (12345 - FM.poly_eval(a, TAU)) % R


@pytest.mark.parametrize("wb", P.CR_WB_CANDIDATES)
def test_signed_digit_walk(wb):
    half, W = 1 << (wb - 1), P.cr_windows(wb)
    for v in rand_fr_ints(50, wb) + list(P.digit_rows(wb).values()) + [1, R - 2, (1 << 253) + 1]:
        ds = P.digits(v, wb)
        assert len(ds) == W and P.from_digits(ds, wb) == v and all(-half < d <= half for d in ds)
    fam = {k: P.digits(v, wb) for k, v in P.digit_rows(wb).items()}
    full = 253 // wb
    assert fam["zero"] == [0] * W
    assert fam["half"][:full] == [half] * full and not any(fam["half"][full:])
    # raw digit half + 1 -> negative digit -(half - 1) and a carry; every later raw digit is half + 2; the carry leaves the last one as +1
    assert fam["half_plus_1"][0] == -(half - 1) and fam["half_plus_1"][1:full] == [-(half - 2)] * (full - 1) and fam["half_plus_1"][full] == 1
    assert fam["carry_to_top"] == [-1] + [0] * (W - 2) + [1]
    assert fam["r_minus_1"][W - 1] != 0 and P.from_digits(fam["r_minus_1"], wb) == R - 1


def test_branch_families_meet_the_branches_they_name():
    wb = P.cr_wb(1)
    assert wb == 13
    steps, total = P.walk(P.branch_family("double_mid_walk", TAU, wb), TAU, wb)
    assert any(acc == e and acc for acc, e in steps)                         # equal operands: the doubling branch
    assert total == (10 * TAU + (3 << wb) * TAU) % R
    steps, total = P.walk(P.branch_family("identity_mid_walk", TAU, wb), TAU, wb)
    i = [n for n, (acc, e) in enumerate(steps) if acc and (acc + e) % R == 0]
    assert i and i[0] + 1 < len(steps) and steps[i[0] + 1][0] == 0           # opposite operands, the identity, and the walk goes on from it
    assert total == (3 << wb) * TAU % R
    for name, rel in (("slices_equal", 1), ("slices_opposite", R - 1)):
        rows = P.branch_family(name, TAU, wb)
        s0, s1 = P.walk(rows[:1], TAU, wb, 0)[1], P.walk(rows[1:], TAU, wb, 1)[1]
        assert s0 and s0 == rel * s1 % R
    assert P.cr_slices(1, 1, 4) == 2 and P.cr_slices(1, 1, 1) == 1            # the lane thresholds the GPU test sets to reach both forms
