"""GPU suite: the stages of the pairing on CHOSEN inputs, through the hooks that already exist (final_exp_batch, miller_loop_batch,
pairing_batch). No device code of its own. Where tests/test_gpu_tower_ops.py holds single tower functions to Python integers, this file runs
the whole final exponentiation on the structured elements a random Miller output never is (one, -1, unit vectors, every word at p - 1,
subfield elements), and whole pairings on points with known logs, so that the expected GT element is a power of e(G1, G2) computed without a
Miller loop. Every case runs in both kernel forms (`pair_wide_max` 0: one lane pair per item; 1 << 20: twelve lanes per item), the Miller
cases also with and without the second wave (`pair_two_waves`), on a private context."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 1 << 20], ids=["lane_pairs", "twelve_lanes"])
def h(request):
    from keaki_amd.hip import KeakiHip
    ctx = KeakiHip(0)
    ctx.set_option("pair_wide_max", request.param)
    yield ctx
    ctx.close()


def f_mont(py, fs):
    """Fq12 values -> n x 48 uint64, Montgomery limbs (2^256) in the order c0.c0.c0 ... c1.c2.c1: what final_exp_batch takes"""
    return np.array([[l for f6 in f for f2 in f6 for x in f2 for l in py.to_mont_limbs(x, py.P)] for f in fs], dtype=np.uint64)


def gt_bytes(py, f):
    return np.frombuffer(py.gt_serialize(f), dtype=np.uint8)


@pytest.fixture(scope="module")
def chosen(py):
    """(tag, f, expected GT bytes): the structured elements of tests/tower_ref.py except zero -- as the kernel's words, so 'all p-1' is p - 1 in
    every 2^261-form word of the accumulator -- every coefficient -1, and elements of Fq, Fq2, Fq6 and of the pure-w part"""
    rng = random.Random(0x5747)
    out = [(t, tr.f12_of(s)) for t, s in tr.structured(with_zero=False)]
    out.append(("every coefficient -1", tr.f12_of([tr.enc(py.P - 1)] * 12)))
    for _ in range(3):
        out += [(t, tr.f12_of(s)) for t, s in tr.subfields(rng)]
    # one plus a unit vector of the w part: the sparsest elements the easy part does not kill
    out += [("one + unit%d" % i, tr.f12_of([a + b for a, b in zip(tr.stored(py.F12_ONE), tr.unit(i))])) for i in range(6, 12)]
    assert 30 <= len(out) <= 50
    return [(t, f, gt_bytes(py, py.final_exponentiation(f))) for t, f in out]


def test_final_exponentiation_of_chosen_elements(h, py, chosen):
    one = gt_bytes(py, py.F12_ONE)
    # what the reference says about these inputs (checked here, not assumed): Fq6 is fixed by f -> f^(p^6), so its elements and -1 die in the easy part
    for t, f, want in chosen:
        if t in ("one", "-1", "in Fq", "in Fq2", "in Fq6") or (t.startswith("unit") and int(t[4:]) < 6):
            assert np.array_equal(want, one), t
    pure_w = [(t, f, want) for t, f, want in chosen if t == "pure w"]
    assert len(pure_w) == 3 and np.array_equal(pure_w[0][2], gt_bytes(py, py.final_exponentiation_naive(pure_w[0][1])))
    # (a pure-w element changes sign under f -> f^(p^6), and -1 dies under p^2 + 1: one again. The elements that do NOT end in one are the mixed ones)
    assert all(np.array_equal(want, one) for _, _, want in pure_w)
    assert sum(not np.array_equal(want, one) for _, _, want in chosen) >= 8
    # the same elements at different rows, lanes and slot columns: batch sizes 1, 3, 4, 5, 33, each starting somewhere else in the list
    n = len(chosen)
    for m, start in ((1, 0), (3, 1), (4, 4), (5, 8), (33, 13), (n, 0)):
        idx = [(start + i) % n for i in range(m)]
        got = h.final_exp_batch(f_mont(py, [chosen[i][1] for i in idx]))
        for row, i in zip(got, idx):
            assert np.array_equal(row, chosen[i][2]), "final_exp_batch, batch of %d: element [%s] (item %d)" % (m, chosen[i][0], idx.index(i))


@pytest.fixture(scope="module")
def known_logs(py, oc):
    """scalars a, b; a G1 and b G2 as Montgomery limbs; GT bytes of e(G1, G2)^(a b) for every (a, b)"""
    r = py.R
    s = [1, 2, r - 1, r - 2, (r + 1) // 2, 1 << 128, random.Random(0x6c6f67).randrange(1, r)]
    p = oc.g1_from_ints([py.g1_mul(py.G1_GEN, a) for a in s])
    q = oc.g2_from_ints([py.g2_mul(py.G2_GEN, b) for b in s])
    e = tr.gt_generator()
    powers = {}
    for a in s:
        for b in s:
            k = a * b % r
            if k not in powers:
                powers[k] = gt_bytes(py, py.f12_pow(e, k))
    # a b = 1 and a b = -1 occur: e(G1, G2) itself and its conjugate
    assert np.array_equal(powers[1], gt_bytes(py, e)) and np.array_equal(powers[r - 1], gt_bytes(py, py.f12_conj(e))) and 2 * ((r + 1) // 2) % r == 1
    return s, p, q, powers


def test_bilinearity_with_known_logs(h, py, oc, rand_fr, known_logs):
    s, p, q, powers = known_logs
    r, n = py.R, len(s)
    pairs = [(i, j) for i in range(n) for j in range(n)]          # 49 pairings
    P, Q = np.stack([p[i] for i, _ in pairs]), np.stack([q[j] for _, j in pairs])
    want = np.stack([powers[s[i] * s[j] % r] for i, j in pairs])
    try:
        for two_waves in (1, 0):
            h.set_option("pair_two_waves", two_waves)
            # Q per item: lines on the fly
            got = h.pairing_batch(P, Q)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, "pairing_batch(a G1, b G2), two_waves %d: (a, b) index %s" % (two_waves, [pairs[k] for k in bad[:4]])
            # Q broadcast (stride 0): every item reads the same b G2
            for j in range(n):
                got = h.pairing_batch(p, q[j])
                for i in range(n):
                    assert np.array_equal(got[i], powers[s[i] * s[j] % r]), "pairing_batch(a G1, fixed b G2), two_waves %d: (a, b) index %s" % (two_waves, (i, j))
            # the Miller loop alone, finished by the oracle's final exponentiation
            f_dev = h.miller_loop_batch(P, Q)
            for k, (i, j) in enumerate(pairs):
                e = oc.final_exp_raw(f_dev[k])
                assert oc.fq_from_mont(e.reshape(-1, 4)).tobytes() == want[k].tobytes(), "miller_loop_batch, two_waves %d: (a, b) index %s" % (two_waves, (i, j))
            # TABULATED lines (the fixed second slot g2): the per-item pairing of an encapsulation, kept alive by `encap_gt`, is
            # e(r_i (C - v_i g1), g2) = e(G1, G2)^(r_i (c - v_i)) for C = c G1. v = c - 1 leaves the exponent r_i; v = c the identity in the first slot
            c = s[-1]
            h.set_option("encap_gt", 1 << 30)
            mont = lambda v: oc.fr_to_mont(oc.ints_to_limbs(v))
            _, gt, _ = h.encap_batch(p[-1], q[1], mont(rand_fr(n + 1, 77)), mont([(c - 1) % r] * n + [c]), mont(s + [5]), 32)
            for i in range(n):
                assert np.array_equal(gt[i], powers[s[i]]), "encap_batch on tabulated lines, two_waves %d: r index %d" % (two_waves, i)
            assert np.array_equal(gt[n], gt_bytes(py, py.F12_ONE))
    finally:
        h.set_option("pair_two_waves", 1)
        h.set_option("encap_gt", -1)


def test_identities_at_the_edges_of_a_wave(h, py, oc, rand_fr):
    """P = 0, Q = 0 and both, at the first and the last item of a wave (32 items as lane pairs, 4 as rows of twelve lanes) and in a ragged
    tail: GT one there -- the arithmetic on zeros runs and is discarded -- and the neighbours keep their values"""
    n = 38
    g1, g2 = oc.generators()
    P = oc.g1_mul_batch(g1, oc.fr_to_mont(oc.ints_to_limbs(rand_fr(n, 901))), threads=8)
    Q = oc.g2_mul_batch(g2, oc.fr_to_mont(oc.ints_to_limbs(rand_fr(n, 902))), threads=8)
    p0, q0, both = (0, 32), (3, 31), (4, 37)
    for i in p0 + both:
        P[i] = 0
    for i in q0 + both:
        Q[i] = 0
    ident = sorted(p0 + q0 + both)
    want = oc.pairing_batch(P, Q, threads=8)
    one = gt_bytes(py, py.F12_ONE)
    assert all(np.array_equal(want[i], one) for i in ident) and not any(np.array_equal(want[i], one) for i in range(n) if i not in ident)
    one_mont = f_mont(py, [py.F12_ONE])[0]
    try:
        for two_waves in (1, 0):
            h.set_option("pair_two_waves", two_waves)
            for m in (n, 33, 5, 4, 1):
                got = h.pairing_batch(P[:m], Q[:m])
                bad = np.nonzero((got != want[:m]).any(axis=1))[0]
                assert bad.size == 0, "pairing_batch with identities, two_waves %d, %d items: items %s" % (two_waves, m, bad[:6].tolist())
            f_dev = h.miller_loop_batch(P, Q)
            for i in range(n):
                if i in ident:
                    assert np.array_equal(f_dev[i], one_mont), "miller_loop_batch, two_waves %d: identity item %d is not one" % (two_waves, i)
                else:
                    e = oc.final_exp_raw(f_dev[i])
                    assert oc.fq_from_mont(e.reshape(-1, 4)).tobytes() == want[i].tobytes(), "miller_loop_batch, two_waves %d: item %d" % (two_waves, i)
            # Q broadcast (stride 0): P = 0 among the items, and a broadcast Q = 0
            assert np.array_equal(h.pairing_batch(P, Q[1]), oc.pairing_batch(P, Q[1], threads=8))
            assert np.array_equal(h.pairing_batch(P[:5], Q[3]), np.tile(one, (5, 1)))
    finally:
        h.set_option("pair_two_waves", 1)
