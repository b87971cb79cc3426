"""CPU suite: the big-integer model of kzg set_pairs / verify_sets_each (tests/set_pairs_model.py) against independent arithmetic -- Lagrange
interpolation and the product form of Z for the pairs, verify_multi's predicate for the verdicts -- and the signed-digit walk of the G2 row kernel
at the digit edges: the carry rule, the slices, and the group-law branches a structured tau makes the walk meet."""
import pytest

import set_pairs_model as P
import verify_sets_model as M
from conftest_helpers import rand_fr_ints

R = P.R
KS = [1, 2, 3, 5, 8, 9, 17, 64]


def make_case(n, k, seed, shared=False, tau=None):
    degree = k + 2
    r = rand_fr_ints(1 + n + n * k + (degree + 1) * (1 if shared else n), seed)
    tau = r[0] if tau is None else tau
    gammas, zs, rest = r[1:1 + n], [r[1 + n + i * k:1 + n + (i + 1) * k] for i in range(n)], r[1 + n + n * k:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(tau, polys, zs, gammas)


def lagrange_at(zs, ys, x):
    out = 0
    for j, (zj, yj) in enumerate(zip(zs, ys)):
        num = den = 1
        for t, zt in enumerate(zs):
            if t != j:
                num = num * (x - zt) % R
                den = den * (zj - zt) % R
        out = (out + yj * num % R * M.inv(den)) % R
    return out


@pytest.mark.parametrize("k", KS)
def test_pairs_against_lagrange_and_the_product_form(k):
    c = make_case(3, k, 500 + k)
    for i in range(c.n):
        a, z2 = P.pair_dl(c, i)
        prod = 1
        for z in c.z[i]:
            prod = prod * (c.tau - z) % R
        assert z2 == prod
        assert a == (P.com_of(c, i) - lagrange_at(c.z[i], c.y[i], c.tau)) % R
        assert (a - c.q[i] * z2) % R == 0                      # a valid item: the equation holds
        ri, rz = P.rows(c, i)
        assert len(ri) == M.kp_of(k) and len(rz) == k and all(v == 0 for v in ri[k:])
        assert sum(v * pow(c.tau, t, R) for t, v in enumerate(ri)) % R == (-lagrange_at(c.z[i], c.y[i], c.tau)) % R
        assert (sum(v * pow(c.tau, t, R) for t, v in enumerate(rz)) + pow(c.tau, k, R)) % R == z2    # monic: the top coefficient is not stored
    if k == 1:
        for i in range(c.n):
            assert P.pair_dl(c, i) == ((P.com_of(c, i) - c.y[i][0]) % R, (c.tau - c.z[i][0]) % R)


@pytest.mark.parametrize("k", [1, 2, 5, 9])
def test_verdicts_follow_verify_multi_and_mark_exactly_the_corrupted_items(k):
    c = make_case(6, k, 900 + k)
    assert P.statuses(c) == [0] * 6 and c.verdict()
    for kind, i, j in (("proof", 0, 0), ("value", 5, k - 1), ("point", 2, 0), ("com", 3, 0)):
        d = P.corrupt(c, kind, i, j)
        want = [1 if t == i else 0 for t in range(6)]
        assert P.statuses(d) == want, kind
        assert [0 if d.single(t) else 1 for t in range(6)] == want, kind
        assert not d.verdict()
    s = make_case(4, k, 77 + k, shared=True)
    assert P.statuses(s) == [0] * 4 and len(s.com) == 1


def test_the_identity_rule_case_by_case():
    tau = rand_fr_ints(1, 4242)[0]
    # a constant polynomial opened at a set that holds tau: A = c - c = 0, Z2 = 0, any proof
    for q, a_zero, z_zero, want in ((5, True, True, 0), (0, True, False, 0), (5, True, False, 1), (0, False, False, 1), (5, False, True, 1), (0, False, True, 1)):
        zs = [tau, 3] if z_zero else [7, 3]
        y = [11, 11] if a_zero else [12, 11]       # the value at the first point decides A where that point is tau
        c = M.Case(tau, 2, [11], [zs], [y], [q], [1])
        a, z2 = P.pair_dl(c, 0)
        assert (a == 0) == a_zero and (z2 == 0) == z_zero
        assert P.status(c, 0) == want, (q, a_zero, z_zero)
        # the rule decides what the equation decides
        assert want == (0 if (a - q * z2) % R == 0 else 1)


@pytest.mark.parametrize("wb", [8, 10, 13])
def test_the_carry_rule_at_the_digit_edges(wb):
    half = 1 << (wb - 1)
    for v in P.edge_scalars(wb) + rand_fr_ints(20, wb):
        ds = P.digits(v, wb)
        assert len(ds) == P.sr_windows(wb) and P.from_digits(ds, wb) == v
        assert all(-half < d <= half for d in ds)
    assert P.digits(half, wb)[:2] == [half, 0]                            # the half stays positive: no carry
    assert P.digits(half + 1, wb)[:2] == [-(half - 1), 1]                # the first negative digit, with a carry
    assert P.digits((1 << wb) - 1, wb)[:2] == [-1, 1]
    assert P.digits(((1 << wb) - 1) + (half << wb), wb)[:3] == [-1, -(half - 1), 1]   # the carry lifts a half over the edge
    top = P.sr_windows(wb) - 1
    chain = P.digits((1 << (wb * top)) - 1, wb)                          # all ones below the top window: the carry runs the whole way up
    assert chain == [-1] + [0] * (top - 1) + [1]
    assert P.digits(0, wb) == [0] * (top + 1)
    assert P.digits(R - 1, wb)[-1] > 0


@pytest.mark.parametrize("wb", [8, 10, 13])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9])
def test_the_walk_sums_to_z_of_tau_in_any_number_of_slices(k, wb):
    c = make_case(2, k, 31 * k + wb)
    for i in range(c.n):
        want = P.pair_dl(c, i)[1]
        _, zc = P.rows(c, i)
        S = 1
        while S <= M.kp_of(k):
            ev, got = P.walk(zc, c.g2_powers, wb, S)
            assert got == want, (S,)
            assert P.event_kinds(ev)["equal"] == 0 and P.event_kinds(ev)["opposite"] == 0      # a random tau meets nothing
            S *= 2


@pytest.mark.parametrize("wb", [8, 13])
def test_structured_tau_makes_the_walk_meet_the_group_law_branches(wb):
    k = 4
    # tau = 1: all bases equal. Coefficients chosen as digits: equal entries double, opposite ones cancel
    g2 = [1] * (k + 1)
    ev, got = P.walk(P.branch_coeffs(wb), g2, wb)
    kinds = P.event_kinds(ev)
    assert kinds["equal"] >= 1 and kinds["opposite"] >= 1 and got == (sum(P.branch_coeffs(wb)) + 1) % R
    # the same through real point sets (k = 2, where Z_0 = z_0 z_1 and Z_1 = -(z_0 + z_1) are solved for): -d meets d; and Z = X^2 + X doubles g2 at the top
    d, pts = P.opposite_pair(wb)
    zc = M.KM.vanishing(pts)
    assert zc == [d, (1 << wb) - d, 1] and len(set(pts)) == 2
    ev, got = P.walk(zc[:2], [1, 1, 1], wb)
    assert P.event_kinds(ev)["opposite"] == 1 and got == ((1 << wb) + 1) % R
    ev, got = P.walk(M.KM.vanishing([R - 1, 0])[:2], [1, 1, 1], wb)
    assert P.event_kinds(ev)["equal"] == 1 and got == 2
    # tau = 0: every base but the first is the identity; its entries are skipped
    g0 = [1] + [0] * k
    ev, got = P.walk([9, 8, 7, 6], g0, wb)
    assert got == 9 and all(e % R for _, e in ev[:-1])
    # tau inside the point set: Z(tau) = 0
    tau = rand_fr_ints(1, 99)[0]
    c = M.Case(tau, 2, [4], [[tau, 5]], [[4, 4]], [123], [1])
    _, zc = P.rows(c, 0)
    assert P.walk(zc, c.g2_powers, wb)[1] == 0 and P.pair_dl(c, 0) == (0, 0) and P.status(c, 0) == 0
