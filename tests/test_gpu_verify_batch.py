"""keaki_hip_kzg_verify_batch / _dev, K.verify_batch, K.vec_verify on the GPU against the discrete-log model (tests/verify_batch_model.py) and
the C oracle. Inputs have KNOWN discrete logs (as tests/test_gpu_structured_srs.py does for the group kernels): secret tau, polynomial p,
C = p(tau) g1, y_i = p(z_i), proof_i = q_i g1 -- so the expected sums L and R are two oracle scalar-mults of big-int sums, whatever n is,
and never come from the library under test. The points themselves come from the oracle's g1_mul_batch (up to 2^16 + 3) or, at 2^20 - 1, from
the library's own vec_commit (wrong proofs would miss R = (sum gamma_i q_i) g1). At n <= 1000 the sums are also derived the other way: the
oracle's MSM over the points."""
import os

import numpy as np
import pytest

import verify_batch_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = os.cpu_count() or 1
R = M.R
BAD_ARG, OOM = -1, -3


@pytest.fixture(scope="module")
def K():
    from keaki_amd import keaki as K
    return K


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def g1_of(oc, dls):
    """dl g1 for every discrete log (the oracle's scalar-mult; 0 -> the identity, all-zero words)"""
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU)


class Arrays:
    """a Case as the arrays of the C ABI"""

    def __init__(self, oc, c, roots=None, proofs=None, coms=None):
        self.c, self.n = c, c.n
        self.tau_g2 = oc.g2_mul_batch(oc.generators()[1], mont(oc, [c.tau]))[0]
        self.coms = g1_of(oc, c.com) if coms is None else coms
        self.proofs = (g1_of(oc, c.q) if c.n else np.zeros((0, 8), np.uint64)) if proofs is None else proofs
        self.z, self.y, self.gamma = mont(oc, c.z), mont(oc, c.y), mont(oc, c.gamma)
        self.omega = mont(oc, [roots]) if roots is not None else None

    def expected(self, oc):
        l, r = self.c.sums()
        e = g1_of(oc, [l, r])
        return self.c.verdict(), e[0], e[1]

    def run(self, hip, mode=0, dev=False):
        pts = self.omega if mode else self.z
        if not dev:
            return hip.kzg_verify_batch(self.coms, self.tau_g2, pts, self.y, self.proofs, self.gamma, point_mode=mode)
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
        d = [t(self.coms), t(self.tau_g2), t(pts), t(self.y), t(self.proofs), t(self.gamma)]
        torch.cuda.synchronize()
        return hip.kzg_verify_batch_dev(d[0], 0 if self.coms.shape[0] == 1 else 1, d[1], d[2], mode, d[3], d[4], d[5], self.n)


def check(oc, hip, a, mode=0, dev=False, what=""):
    ok, L, Rp = a.run(hip, mode, dev)
    eok, eL, eR = a.expected(oc)
    assert np.array_equal(L, eL), "L %s" % what
    assert np.array_equal(Rp, eR), "R %s" % what
    assert ok == eok, "verdict %s" % what
    return ok


def oracle_msm_sums(oc, a):
    """L and R the other way: the oracle's Pippenger over the points themselves"""
    c = a.c
    g1 = oc.generators()[0]
    t = sum(g * y for g, y in zip(c.gamma, c.y)) % R
    s = [g * z % R for g, z in zip(c.gamma, c.z)]
    if a.coms.shape[0] == 1:
        bases = np.concatenate([a.coms, a.proofs, g1[None, :]]); sc = [sum(c.gamma) % R] + s + [-t]
    else:
        bases = np.concatenate([a.coms, a.proofs, g1[None, :]]); sc = list(c.gamma) + s + [-t]
    return oc.msm_g1(bases, mont(oc, sc), threads=NCPU), oc.msm_g1(a.proofs, a.gamma, threads=NCPU)


_CACHE = {}


def arrays_for(oc, py, n, roots):
    """(stride-0 arrays, stride-1 arrays) of n valid openings of a degree-7 polynomial, at random points or at the powers of omega. The n
    polynomials of stride 1 are p + shift_i: different commitments and values, the same quotients -- one set of proof points serves both."""
    key = (n, roots)
    if key not in _CACHE:
        r = rand_fr_ints(3 * n + 16, 9000 + n + (1 if roots else 0))
        w = py.fr_root_of_unity(1 << n.bit_length()) if roots else None
        zs = M.powers(w, n) if roots else r[9:9 + n]
        gam, sh = r[9 + n:9 + 2 * n], r[9 + 2 * n:9 + 3 * n]
        c0 = M.valid_case(r[0], r[1:9], zs, gam)
        c1 = M.valid_case(r[0], r[1:9], zs, gam, sh)
        a0 = Arrays(oc, c0, roots=w)
        a1 = Arrays(oc, c1, roots=w, proofs=a0.proofs)
        _CACHE[key] = (a0, a1)
    return _CACHE[key]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 1000, (1 << 16) + 3])
def test_sums_are_bit_exact(oc, py, hip, n):
    """sums_out_aff == the model's L and R, and ok == its verdict: both com_strides, both point_modes, host and _dev forms"""
    for roots in (False, True):
        a0, a1 = arrays_for(oc, py, n, roots)
        for stride, a in ((0, a0), (1, a1)):
            if n <= 1000:
                eok, eL, eR = a.expected(oc)
                mL, mR = oracle_msm_sums(oc, a)
                assert eok and np.array_equal(mL, eL) and np.array_equal(mR, eR), "the two derivations of the expected sums disagree"
            for mode in ((0, 1) if roots else (0,)):
                for dev in (False, True):
                    assert check(oc, hip, a, mode, dev, "n=%d stride=%d mode=%d dev=%s" % (n, stride, mode, dev))


def test_verdict_matrix_n_1000(oc, py, hip):
    a0, a1 = arrays_for(oc, py, 1000, False)
    assert check(oc, hip, a0)
    k = 0xC0FFEE

    def variant(base, edit, proofs_edit=None, coms_edit=None):
        c = base.c.copy()
        edit(c)
        pr = base.proofs.copy()
        if proofs_edit:
            proofs_edit(pr)
        cm = base.coms.copy()
        if coms_edit:
            coms_edit(cm)
        return Arrays(oc, c, proofs=pr, coms=cm)

    def set_y(c): c.y[17] = (c.y[17] + 1) % R
    def set_z(c): c.z[400] = (c.z[400] + 1) % R
    def set_q(c): c.q[999] = k
    def set_com(c): c.com[0] = (c.com[0] + 1) % R
    def swap_q(c): c.q[3], c.q[700] = c.q[700], c.q[3]
    kg = g1_of(oc, [k])[0]

    def put_k(pr): pr[999] = kg
    def swap_pr(pr): pr[[3, 700]] = pr[[700, 3]]
    def put_com(cm): cm[0] = g1_of(oc, [a0.c.com[0] + 1])[0]
    for name, v in (("value", variant(a0, set_y)), ("point", variant(a0, set_z)), ("proof = k g1", variant(a0, set_q, proofs_edit=put_k)),
                    ("commitment", variant(a0, set_com, coms_edit=put_com)), ("two proofs exchanged", variant(a0, swap_q, proofs_edit=swap_pr))):
        eok, eL, eR = v.expected(oc)
        assert not eok, name
        assert not check(oc, hip, v, what=name)
    # one wrong commitment among n (stride 1)
    def set_com1(c): c.com[5] = (c.com[5] + 1) % R
    def put_com1(cm): cm[5] = g1_of(oc, [a1.c.com[5] + 1])[0]
    assert not check(oc, hip, variant(a1, set_com1, coms_edit=put_com1), what="commitment 5 of n")
    # the cancelling pair: accepted at equal gammas (the contract), rejected otherwise
    def cancel(eq):
        def f(c):
            c.y[0] = (c.y[0] + 99) % R
            c.y[1] = (c.y[1] - 99) % R
            c.gamma[1] = c.gamma[0] if eq else (c.gamma[0] + 1) % R
        return f
    assert check(oc, hip, variant(a0, cancel(True)), what="cancelling pair, equal gammas")
    assert not check(oc, hip, variant(a0, cancel(False)), what="cancelling pair, different gammas")


@pytest.mark.parametrize("good", [True, False])
def test_n_1_agrees_with_single_verify(oc, py, hip, good):
    a = arrays_for(oc, py, 1, False)[0]
    c = a.c.copy()
    if not good:
        c.y[0] = (c.y[0] + 1) % R
    v = Arrays(oc, c, proofs=a.proofs, coms=a.coms)
    assert check(oc, hip, v) == good
    assert hip.kzg_verify(v.coms[0], v.tau_g2, v.z[0], v.y[0], v.proofs[0]) == good


def test_degenerate_operands(oc, py, hip):
    r = rand_fr_ints(400, 31337)
    n = 100
    zs, gam = r[10:10 + n], r[200:200 + n]
    zero8 = np.zeros(8, np.uint64)
    # degree 0: every proof is the identity, L = R = identity, accepted
    a = Arrays(oc, M.valid_case(r[0], [r[1]], zs, gam))
    assert not a.proofs.any()
    ok, L, Rp = a.run(hip)
    assert ok and np.array_equal(L, zero8) and np.array_equal(Rp, zero8)
    assert check(oc, hip, a, dev=True)
    # degree 1: all n proofs are the SAME point (every bucket meets its own point: the doubling branch)
    a = Arrays(oc, M.valid_case(r[0], [r[1], r[2]], zs, gam))
    assert (a.proofs == a.proofs[0]).all() and a.proofs.any()
    assert check(oc, hip, a)
    assert check(oc, hip, Arrays(oc, M.valid_case(r[0], [r[1], r[2]], zs, [7] * n)), what="same point, same gamma")
    # proofs containing P and -P (an arbitrary, invalid set: the sums must still be exact), zero gammas, a zero value vector
    c = M.valid_case(r[0], r[1:9], zs, gam)
    c.q[1] = (-c.q[0]) % R
    c.q[2] = c.q[0]
    c.gamma[3] = c.gamma[50] = 0
    c.gamma[1] = c.gamma[0]
    assert not check(oc, hip, Arrays(oc, c), what="P and -P")
    c = M.valid_case(r[0], r[1:9], zs, [0] * n)
    c.y[4] += 1
    ok, L, Rp = Arrays(oc, c).run(hip)
    assert ok and not L.any() and not Rp.any(), "gamma = 0 accepts anything (the contract)"
    c = M.valid_case(r[0], r[1:9], zs, gam)
    c.y = [0] * n
    assert not check(oc, hip, Arrays(oc, c), what="zero values")
    c = M.valid_case(r[0], [0] + r[2:9], [0] + zs[1:], gam)           # p(0) = 0: a zero value at the zero point
    assert c.y[0] == 0 and check(oc, hip, Arrays(oc, c), what="zero point and value")
    # an identity commitment: the zero polynomial (valid), and p with C replaced by the identity (invalid)
    assert check(oc, hip, Arrays(oc, M.valid_case(r[0], [0], zs, gam)), what="zero polynomial")
    c = M.valid_case(r[0], r[1:9], zs, gam)
    c.com[0] = 0
    assert not check(oc, hip, Arrays(oc, c), what="identity commitment")
    # n = 0
    e = Arrays(oc, M.Case(r[0], [5], [], [], [], []))
    for dev in (False, True):
        ok, L, Rp = e.run(hip, dev=dev)
        assert ok and not L.any() and not Rp.any()


def test_independent_openings_through_the_mirror(K, oc, py):
    """d = 2^9, proofs made as tests/test_gpu_config5.py makes them (the oracle's quotient and MSM over the SRS, no discrete logs)"""
    from bench import random_fr_limbs
    d = 1 << 9
    rng = K.Rng(515)
    s = K.KZGSetup.setup(rng.fr_rand(), d)
    try:
        srs_pts = s.g1_pow()
        n = d - 1
        w = py.fr_root_of_unity(d)
        evals = np.zeros((d, 4), np.uint64)
        evals[:n] = random_fr_limbs(n, 616)
        evals[n] = random_fr_limbs(1, 617)[0]
        m1 = lambda x: mont(oc, [x])[0]
        coeffs = oc.fr_fft(evals, m1(pow(w, -1, R)), m1(pow(d, -1, R)))
        com = oc.msm_g1(srs_pts, coeffs, threads=NCPU)
        zs = mont(oc, M.powers(w, n))
        proofs = np.zeros((n, 8), np.uint64)
        for i in range(n):
            q, v = oc.fr_quotient(coeffs, zs[i])
            assert np.array_equal(v, evals[i])
            proofs[i] = oc.msm_g1(srs_pts[:q.shape[0]], q, threads=NCPU)
        assert K.vec_verify(rng, s, com, evals[:n], proofs)
        assert K.verify_batch(rng, s, com, zs, evals[:n], proofs)
        assert K.verify_batch(rng, s, np.repeat(com[None, :], n, 0), zs, evals[:n], proofs)
        assert K.verify_batch(rng, s, com, zs[1:2], evals[:n], proofs, roots_of_unity=True)
        bad = evals[:n].copy()
        bad[n // 2] = evals[0] if not np.array_equal(evals[0], evals[n // 2]) else evals[1]
        assert not K.vec_verify(rng, s, com, bad, proofs)
        assert not K.verify_batch(rng, s, com, zs, bad, proofs)
        # below the crossover the mirror checks item by item: same answers
        assert K.verify_batch(rng, s, com, zs[:2], evals[:2], proofs[:2]) and not K.verify_batch(rng, s, com, zs[:2], evals[1:3], proofs[:2])
        assert K.verify_batch(rng, s, com, zs[1:2], evals[:3], proofs[:3], roots_of_unity=True)      # ... also over the powers of omega
    finally:
        s.close()


def test_all_openings_of_a_vector_commitment_2p20(K, oc, py, hip):
    """n = 2^20 - 1 (domain 2^20), proofs from K.vec_commit: L, R equal the discrete-log model, verdict 1; one value changed -> 0. p(tau) comes from
    the test's own data (the 2^20 evaluations, the padding value being the next draw of the test's Rng) by the barycentric formula."""
    from bench import random_fr_limbs
    log2d = int(os.environ.get("KEAKI_TEST_VERIFY_BATCH_LOG2D", "20"))
    d = 1 << log2d
    n = d - 1
    rng = K.Rng(777)
    secret = rng.fr_rand()
    s = K.KZGSetup.setup(secret, d)
    try:
        v = random_fr_limbs(n, 888)
        com, proofs = K.vec_commit(rng, s, v)
        replay = K.Rng(777)
        assert np.array_equal(replay.fr_rand(), secret)
        pad = replay.fr_rand()
        tau = oc.limbs_to_ints(oc.fr_from_mont(secret[None, :]))[0]
        evals = oc.limbs_to_ints(oc.fr_from_mont(np.concatenate([v, pad[None, :]])))
        w = py.fr_root_of_unity(d)
        ptau, inv = M.barycentric_at(evals, w, d, tau)
        qs = [(ptau - evals[i]) * inv[i] % R for i in range(n)]
        gam_m = random_fr_limbs(n, 999)
        gam = oc.limbs_to_ints(oc.fr_from_mont(gam_m))
        c = M.Case(tau, [ptau], M.powers(w, n), evals[:n], qs, gam)
        assert c.verdict()
        assert np.array_equal(com, g1_of(oc, [ptau])[0]), "the commitment is not p(tau) g1"
        a = Arrays(oc, c, roots=w, proofs=proofs[:n], coms=com[None, :])
        assert check(oc, hip, a, mode=1, what="2^%d - 1 openings, host" % log2d)
        assert check(oc, hip, a, mode=1, dev=True, what="2^%d - 1 openings, dev" % log2d)
        assert check(oc, hip, a, mode=0, what="explicit points")
        c2 = c.copy()
        c2.y[n // 3] = (c2.y[n // 3] + 1) % R
        assert not check(oc, hip, Arrays(oc, c2, roots=w, proofs=proofs[:n], coms=com[None, :]), mode=1, what="one value changed")
        assert K.vec_verify(rng, s, com, v, proofs)
        v2 = v.copy()
        v2[5] = v[6]
        assert not K.vec_verify(rng, s, com, v2, proofs)
    finally:
        s.close()


def test_no_state_leaks_and_trim(oc, py, hip):
    """an MSM over an SRS with tables, an encap_batch and a kzg_open give the same bytes before and after a verify_batch on the same context"""
    from bench import random_fr_limbs
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        n = 4096
        pts = g1_of(oc, rand_fr_ints(n, 42))
        srs = h.srs_g1_upload(pts)
        h.srs_g1_precompute(srs)
        sc = random_fr_limbs(n, 43)
        a = arrays_for(oc, py, 1000, False)[0]
        four = random_fr_limbs(12, 44)

        def others():
            return (h.msm_g1(srs, sc).copy(), [x.copy() for x in h.encap_batch(a.coms[0], a.tau_g2, four[:4], four[4:8], four[8:12], 32)],
                    [x.copy() for x in h.kzg_open(srs, sc, four[0])])

        def same(x, y):
            return np.array_equal(x[0], y[0]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1])) and all(np.array_equal(p, q) for p, q in zip(x[2], y[2]))
        before = others()
        assert check(oc, h, a)
        assert same(before, others())
        before_mem = h.memory()
        assert before_mem["workspaces"] > 1000 * 32
        h.trim()
        assert h.memory()["workspaces"] == 0
        assert check(oc, h, a) and check(oc, h, a, dev=True)
        assert same(before, others())
        srs.free()
    finally:
        h.close()


def test_error_paths(oc, py, hip):
    import ctypes as C
    from keaki_amd.hip import KeakiHip, KeakiHipError, _ptr
    h = KeakiHip(0)
    try:
        a = arrays_for(oc, py, 64, False)[0]
        ok = C.c_int32(7)

        def raw(com, stride, tau, pts, mode, vals, proofs, gam, n, okp):
            return h.lib.keaki_hip_kzg_verify_batch(h.ctx, com, stride, tau, pts, mode, vals, proofs, gam, n, okp, None)
        full = [_ptr(a.coms), 0, _ptr(a.tau_g2), _ptr(a.z), 0, _ptr(a.y), _ptr(a.proofs), _ptr(a.gamma), a.n, C.byref(ok)]
        for pos, val in ((1, 2), (1, -1), (4, 2), (4, -1), (0, None), (2, None), (3, None), (5, None), (6, None), (7, None), (9, None)):
            args = list(full)
            args[pos] = val
            assert raw(*args) == BAD_ARG, pos
            assert h.lib.keaki_hip_last_error(h.ctx), pos
            assert h.lib.keaki_hip_kzg_verify_batch_dev(h.ctx, None, 0, None, None, 0, None, None, None, 4, C.byref(ok), None) == BAD_ARG
        assert check(oc, h, a), "the context is usable after refused calls"
        # too little memory for the workspace: KEAKI_ERR_OOM, and the next call (limit lifted) succeeds
        h.trim()
        h.debug_set_alloc_limit(64)
        with pytest.raises(KeakiHipError) as e:
            a.run(h)
        assert e.value.status == OOM
        h.debug_set_alloc_limit(0)
        assert check(oc, h, a)
    finally:
        h.close()
