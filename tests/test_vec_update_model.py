"""The scalar model of vec_update (tests/vec_update_model.py) against recommitting: the update formulas of keaki_amd/csrc/vec_update.hip on
scalars in the exponent, for every SRS the GPU tests use and the pass split they take their list lengths from."""
import os
import re

import pytest

import structured_inputs as S
import vec_update_model as M
from conftest_helpers import rand_fr_ints

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def taus(d):
    w = M.omega(d)
    return [("random", S.secrets()["random"]), ("zero", 0), ("one", 1)] + [("omega^%d" % t, pow(w, t, R)) for t in sorted({1 % d, d // 2, d - 1})]


def check(d, tau, changes, seed, k_pass=0):
    srs = S.powers(tau, d)
    evals = rand_fr_ints(d, seed)
    com, proofs = M.commit_and_open(srs, evals)
    new = list(evals)
    for i, dl in changes:
        new[i] = (new[i] + dl) % R
    assert M.update(srs, d, com, proofs, changes, k_pass) == M.commit_and_open(srs, new)


@pytest.mark.parametrize("d", [1, 2, 4, 16])
def test_update_equals_recommit(d):
    rnd = rand_fr_ints(4 * d + 8, 100 + d)
    for name, tau in taus(d):
        check(d, tau, [(0, rnd[0])], 1)
        check(d, tau, [(d - 1, rnd[1])], 2)
        check(d, tau, [(i, rnd[2 + i]) for i in range(d)], 3)                                     # all positions
        check(d, tau, [(d // 2, rnd[0]), (d // 2, rnd[1]), (0, rnd[2]), (d // 2, R - rnd[0])], 4)   # duplicates add
        check(d, tau, [(i % d, rnd[i]) for i in range(2 * d + 3)], 5)
        check(d, tau, [(0, 0), (d - 1, R - 1)], 6)


@pytest.mark.parametrize("d", [4, 16])
def test_degenerate_deltas(d):
    tau = S.secrets()["random"]
    srs = S.powers(tau, d)
    for i in (0, d - 1):
        evals = [0] * d
        evals[i] = 12345
        com, proofs = M.commit_and_open(srs, evals)
        assert M.update(srs, d, com, proofs, [(i, 12345)]) == (2 * com % R, [2 * p % R for p in proofs])      # delta = v: everything doubles
        assert M.update(srs, d, com, proofs, [(i, R - 12345)]) == (0, [0] * d)                                # delta = -v: everything vanishes
        assert M.update(srs, d, 0, [0] * d, [(i, 12345)]) == (com, proofs)                                    # from the all-zero vector
        assert M.update(srs, d, com, proofs, [(i, 77), (i, R - 77)]) == (com, proofs)


@pytest.mark.parametrize("d", [2, 16])
def test_tables_have_their_closed_forms(d):
    """a_i = A(tau) / (tau - w^i), u_i = (L_i(tau) - 1) / (tau - w^i) and c_i a_i = L_i(tau) wherever tau is off the domain; on it a_i = 0 but for one"""
    w = M.omega(d)
    tau = S.secrets()["random"]
    a, u, pw, e = M.tables(S.powers(tau, d), d)
    A = (pow(tau, d, R) - 1) % R
    for i in range(d):
        x = pow(w, i, R)
        inv = pow(tau - x, -1, R)
        li = x * pow(d, -1, R) % R * A % R * inv % R
        assert a[i] == A * inv % R and u[i] == (li - 1) * inv % R and pw[i] * x % R == 1
        assert i == 0 or e[i] * (x - 1) % R == 1
    a, _, _, _ = M.tables(S.powers(pow(w, 1, R), d), d)
    assert [bool(x) for x in a] == [i == 1 for i in range(d)]


def test_pass_split():
    assert M.passes(0) == [] and M.passes(1) == [(0, 1)] and M.passes(M.UPD_K_PASS + 1) == [(0, M.UPD_K_PASS), (M.UPD_K_PASS, 1)]
    assert M.passes(7, 3) == [(0, 3), (3, 3), (6, 1)] and M.passes(3, 3) == [(0, 3)] and M.passes(4, 3) == [(0, 3), (3, 1)]
    assert M.passes(20, 99) == M.passes(20, 0) == M.passes(20)                  # out of range: the built-in size
    assert M.pass_edge_ks(3) == [1, 2, 3, 4, 7]
    for k in M.pass_edge_ks(3):
        check(16, S.secrets()["random"], [(5 * t % 16, 1000 + t) for t in range(k)], 9, k_pass=3)
    hdr = open(os.path.join(ROOT, "keaki_amd", "csrc", "internal.h")).read()
    assert int(re.search(r"constexpr uint32_t UPD_K_PASS = (\d+);", hdr).group(1)) == M.UPD_K_PASS
