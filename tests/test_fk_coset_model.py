"""CPU suite: the model of the FK23 coset openings (tests/fk_coset_model.py) against itself and against the models that were there before.
(a) the proofs by long division == (b) the device pipeline in discrete-log space, for d = 4 .. 64 and every l <= d; l = 1 is open_fk; r = 1 gives 0;
(c) the host split plan holds its invariants and restates the constants of csrc/fk_coset_plan.h."""
import os
import random
import re

import pytest

import fk_coset_model as M
import fk_shard_model as FS
import kzg_set_model as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poly(rng, d, F):
    return [rng.randrange(F.q) for _ in range(d)]


def test_roots_are_the_domain_generators():
    for log2n in (1, 5, 28):
        w = M.omega(1 << log2n)
        assert pow(w, 1 << log2n, M.R) == 1 and pow(w, 1 << (log2n - 1), M.R) == M.R - 1
    assert M.omega(64, M.F_SMALL) == FS.root(64)


def test_coset_quotient_is_schoolbook_long_division():
    rng = random.Random(11)
    for d, l in ((8, 1), (8, 2), (8, 8), (16, 4), (12, 4), (5, 8)):
        p = [rng.randrange(M.R) for _ in range(d)]
        c = rng.randrange(M.R)
        quot, rem = KS.long_division(p, [(-c) % M.R] + [0] * (l - 1) + [1])
        assert M.quotient_coset(p, l, c) == quot and len(quot) == max(d - l, 0)


def test_coset_points_are_the_index_blocks():
    d, l = 32, 4
    r, w = d // l, M.omega(32)
    for i in range(r):
        c = pow(M.omega(r), i, M.R)
        idx = M.coset_indices(d, l, i)
        assert idx == [i + t * r for t in range(l)]
        assert all(pow(pow(w, k, M.R), l, M.R) == c for k in idx)


@pytest.mark.parametrize("log2d", [2, 3, 4, 5, 6])
def test_long_division_equals_the_toeplitz_route(log2d):
    rng = random.Random(100 + log2d)
    d = 1 << log2d
    for log2l in range(log2d + 1):
        tau = rng.randrange(2, M.R)
        srs = [pow(tau, k, M.R) for k in range(d)]
        p = _poly(rng, d, M.FR)
        want = M.proofs_direct(p, log2d, log2l, tau)
        assert M.proofs_toeplitz(srs, p, log2d, log2l) == want, (log2d, log2l)
        # every split of the terms gives the same sums
        l, n2 = 1 << log2l, 2 << (log2d - log2l)
        for g in (1, 2, 4):
            for min_lanes in (1, 4 * n2, 1 << 20):
                assert M.proofs_toeplitz(srs, p, log2d, log2l, plan=M.split_plan(n2, l, g, min_lanes)) == want, (log2d, log2l, g, min_lanes)


def test_set_proof_of_the_coset_is_the_same_quotient():
    """pi_i is what the set opening of the l coset points commits to (kzg_set_model: (p - I) / Z)"""
    rng = random.Random(5)
    log2d, log2l, tau = 4, 2, 0x1234567
    d, l = 1 << log2d, 1 << log2l
    p = _poly(rng, d, M.FR)
    got = M.proofs_direct(p, log2d, log2l, tau)
    w = M.omega(d)
    for i in range(d // l):
        zs = [pow(w, k, M.R) for k in M.coset_indices(d, l, i)]
        assert KS.set_proof_dl(p, zs, tau) == got[i]


def test_l_equal_one_is_open_fk():
    rng = random.Random(7)
    F = M.F_SMALL
    for log2d in (1, 3, 5):
        d = 1 << log2d
        srs, p = _poly(rng, d, F), _poly(rng, d, F)
        assert M.proofs_toeplitz(srs, p, log2d, 0, F) == FS.open_fk_plain(srs, p, log2d)


def test_one_coset_gives_the_identity():
    rng = random.Random(9)
    for log2d in (0, 3, 6):
        d = 1 << log2d
        p = _poly(rng, d, M.FR)
        assert M.proofs_direct(p, log2d, log2d, 12345) == [0]
        assert M.proofs_toeplitz([pow(12345, k, M.R) for k in range(d)], p, log2d, log2d) == [0]


def test_lane_q_reads_hat_a_at_the_bit_reversed_position():
    """the convention the raw entry fixes: hat_a natural order with (2r)^-1 folded in, hat_s at position q = index brev(q)"""
    log2d, log2l, tau = 4, 1, 987654321
    d, l, r = 16, 2, 8
    rng = random.Random(3)
    srs, p = [pow(tau, k, M.R) for k in range(d)], _poly(rng, d, M.FR)
    hs, ha = M.hat_s_rows(srs, log2d, log2l), M.hat_a_rows(p, log2d, log2l)
    w = M.omega(2 * r)
    for j in range(l):
        full = M.dft([srs[(r - 1 - k) * l + j] for k in range(r)] + [0] * r, w)
        assert hs[j] == [full[M.bitrev(q, 4)] for q in range(2 * r)]
        plain = M.dft([0] * r + [p[u * l + j] for u in range(r)], w)
        assert [x * 2 * r % M.R for x in ha[j]] == plain


def test_split_plan():
    src = open(os.path.join(ROOT, "keaki_amd", "csrc", "fk_coset_plan.h")).read()
    assert int(re.search(r"constexpr uint32_t FKC_G = (\d+);", src).group(1)) == M.FKC_G
    assert int(re.search(r"constexpr uint32_t FKC_SPLIT_MIN_LANES = (\d+);", src).group(1)) == M.FKC_SPLIT_MIN_LANES
    for log2l in range(11):
        l = 1 << log2l
        for log2n2 in range(1, 22):
            n2 = 1 << log2n2
            for g in (0, 1, 2, 4):
                for ml in (0, 1, 1 << 10, 1 << 31):
                    G, S, groups = M.split_plan(n2, l, g, ml)
                    assert G == min(g or 4, l) and G * S * groups == l and groups >= 1 and S & (S - 1) == 0
                    lim = ml or M.FKC_SPLIT_MIN_LANES
                    # no split beyond need, and none that leaves a lane less than a full group
                    assert S == 1 or n2 * S // 2 < lim
                    assert n2 * S >= lim or l // (2 * S) < G
    # the shapes of the GPU suite fall on both sides: unsplit and split
    assert M.split_plan(16, 2)[1] == 1 and M.split_plan(128, 16)[1] == 4 and M.split_plan(32, 64)[1] == 16
    assert M.split_plan(1 << 17, 64)[1] == 1 and M.split_plan(1 << 16, 64)[1] == 2 and M.split_plan(1 << 15, 64)[1] == 4
