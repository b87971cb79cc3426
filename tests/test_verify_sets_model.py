"""CPU suite: the combination keaki_hip_kzg_verify_sets evaluates, restated over Z_r with tau known (tests/verify_sets_model.py), so that every
group element is its discrete log. The GPU tests (tests/test_gpu_verify_sets.py) take their expected sums from this model; here the model itself
is pinned: against the per-item predicate, against verify_batch's combination at k = 1, and its Z, weights and I against tests/kzg_set_model.py."""
import os
import random
import re

import pytest

import kzg_set_model as KM
import verify_sets_model as VM

R = VM.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed, n, k, shared=False, deg=None):
    rnd = random.Random(seed)
    tau = rnd.randrange(2, R)
    deg = (k + 3) if deg is None else deg
    polys = [[rnd.randrange(R) for _ in range(deg)] for _ in range(1 if shared else n)]
    zs = [rnd.sample(range(1, 1 << 62), k) for _ in range(n)]
    gammas = [rnd.randrange(1, R) for _ in range(n)]
    return VM.valid_case(tau, polys, zs, gammas), rnd


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 17, 64])
@pytest.mark.parametrize("shared", [False, True])
def test_valid_items_balance_for_any_gammas(k, shared):
    c, rnd = _case(100 + k, 5 if k < 64 else 2, k, shared)
    assert all(c.single(i) for i in range(c.n))
    assert c.verdict()
    for g in ([0] * c.n, [1] * c.n, [rnd.randrange(R) for _ in range(c.n)]):
        d = c.copy()
        d.gamma = g
        assert d.verdict()


@pytest.mark.parametrize("k", [1, 2, 3, 9])
def test_one_value_point_or_proof_off_by_one_is_rejected(k):
    c, rnd = _case(200 + k, 4, k)
    for what in ("y", "z", "q"):
        i, j = rnd.randrange(c.n), rnd.randrange(k)
        d = c.copy()
        if what == "y":
            d.y[i][j] = (d.y[i][j] + 1) % R
        elif what == "z":
            d.z[i][j] = (d.z[i][j] + 1) % R
        else:
            d.q[i] = (d.q[i] + 1) % R
        assert not d.single(i), what
        assert all(d.single(t) for t in range(d.n) if t != i)
        assert not d.verdict(), what


def test_verdict_is_the_gamma_weighted_sum_of_the_single_predicates():
    """-dl(L) + sum_t tau^t dl(R_t) = sum_i gamma_i (q_i Z_i(tau) - c_i + I_i(tau)): the identity the call rests on, on INVALID items too"""
    c, rnd = _case(7, 5, 4)
    for i in range(c.n):
        c.y[i][0] = rnd.randrange(R)
        c.q[i] = rnd.randrange(R)
    s = c.sums()
    lhs = (-s[0] + sum(pow(c.tau, t, R) * s[t] for t in range(1, c.k + 1))) % R
    rhs = 0
    for i in range(c.n):
        zt, it = KM.poly_eval(c.Z(i), c.tau), KM.poly_eval(c.I(i), c.tau)
        rhs = (rhs + c.gamma[i] * (c.q[i] * zt - c.com[i] + it)) % R
    assert lhs == rhs


@pytest.mark.parametrize("shared", [False, True])
def test_k1_is_verify_batch(shared):
    """Z = X - z: -gamma Z_0 = gamma z, J_0 = sum gamma y, [tau^0]_1 = g1 -- L and R_1 are verify_batch's L and R"""
    c, _ = _case(11, 6, 1, shared)
    c.y[2][0] = (c.y[2][0] + 5) % R            # the equality is one of sums, not of verdicts
    l, r = VM.batch_sums(c.com, [row[0] for row in c.z], [row[0] for row in c.y], c.q, c.gamma)
    assert c.sums() == [l, r]
    assert c.rows()[0] == [g * z[0] % R for g, z in zip(c.gamma, c.z)] and c.rows()[1] == c.gamma


def test_row_layout_and_the_sign_of_row_zero():
    c, _ = _case(13, 3, 5)
    rows, flat = c.rows(), c.rows_flat()
    assert len(rows) == c.k + 1 and len(flat) == (c.k + 1) * c.n
    for i in range(c.n):
        zc = KM.vanishing(c.z[i])
        assert zc[c.k] == 1
        assert flat[0 * c.n + i] == (-c.gamma[i] * zc[0]) % R
        for t in range(1, c.k):
            assert flat[t * c.n + i] == c.gamma[i] * zc[t] % R
        assert flat[c.k * c.n + i] == c.gamma[i]


def test_set_polynomials_are_kzg_set_models():
    c, _ = _case(17, 3, 6)
    for i in range(c.n):
        zc, ic, w = c.Z(i), c.I(i), KM.weights(c.z[i])
        assert zc == KM.vanishing(c.z[i]) and all(KM.poly_eval(zc, z) == 0 for z in c.z[i])
        assert [KM.poly_eval(ic, z) for z in c.z[i]] == c.y[i]
        # the weights are 1 / Z'(z_j), and I is the weighted sum of the quotients Z / (X - z_j)
        dz = [(t * zc[t]) % R for t in range(1, len(zc))]
        assert all(wj * KM.poly_eval(dz, z) % R == 1 for wj, z in zip(w, c.z[i]))
        acc = [0] * c.k
        for z, y, wj in zip(c.z[i], c.y[i], w):
            q, rem = KM.divide_linear(zc, z)
            assert rem == 0
            acc = [(a + y * wj % R * b) % R for a, b in zip(acc, q)]
        assert acc == ic


def test_degenerate_inputs():
    c, _ = _case(19, 3, 4, deg=3)                # degree < k: p = I, the proof is the identity
    assert c.q == [0, 0, 0] and c.verdict()
    e = VM.valid_case(5, [[1, 2, 3]], [], [])    # n = 0
    assert e.n == 0 and e.verdict() and e.sums() == [0, 0]
    d, _ = _case(23, 4, 3)
    d.z, d.y, d.q, d.com = [d.z[0]] * 4, [d.y[0]] * 4, [d.q[0]] * 4, [d.com[0]] * 4        # one item four times, four gammas
    assert d.verdict()


def test_tiling_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "keaki_amd", "csrc", "kzg_sets.hip")).read()
    assert int(re.search(r"constexpr u32 VS_THREADS = (\d+);", src).group(1)) == VM.VS_THREADS
    assert int(re.search(r"constexpr u32 VS_INV = (\d+);", src).group(1)) == VM.VS_INV
    hdr = open(os.path.join(ROOT, "include", "keaki_hip.h")).read()
    assert int(re.search(r"KEAKI_VERIFY_SETS_K_MAX = (\d+)", hdr).group(1)) == VM.K_MAX
    assert [VM.tile_items(k) for k in (1, 2, 3, 8, 9, 17, 64)] == [256, 128, 64, 32, 16, 8, 4]
