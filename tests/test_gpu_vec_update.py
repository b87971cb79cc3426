"""vec_update through the C ABI (keaki_hip_vec_update*, keaki_hip_srs_g1_precompute_update) and the host mirror: an updated (commitment, proofs)
is byte for byte what keaki_hip_vec_commit returns for the changed vector on the same handle. Shapes around the wave edge, the pass split of
tests/vec_update_model.py, operands that force equal, opposite and identity additions, SRS with a known secret (every result = (its scalar) g1),
the oracle's own openings and the pairing check, and the contract of the call."""
import ctypes as C
import os

import numpy as np
import pytest

import structured_inputs as S
import vec_update_model as M
from conftest_helpers import rand_fr_ints
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(16, os.cpu_count() or 1)
N_SRS = 512
ERR_BAD_ARG, ERR_OOM, ERR_TOO_LARGE = -1, -3, -5


def consts(oc, log2d):
    """(omega_d^-1, 1/d, omega_2d, omega_2d^-1, 1/2d): the five domain constants of vec_commit"""
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    return [mont(oc, [x])[0] for x in (pow(w2 * w2, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]


def uconsts(oc, log2d):
    """(omega_d, omega_d^-1, 1/d): the three of vec_update"""
    d = 1 << log2d
    w = M.omega(d)
    return [mont(oc, [x])[0] for x in (w, pow(w, -1, R), pow(d, -1, R))]


def g1_of(oc, ks):
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, [k % R for k in ks]), threads=TH)


def commit(oc, h, srs, evals, log2d):
    return h.vec_commit(srs, mont(oc, [e % R for e in evals]), None, log2d, *consts(oc, log2d))


def changed(evals, changes):
    new = list(evals)
    for i, dl in changes:
        new[i] = (new[i] + dl) % R
    return new


def update(oc, h, srs, log2d, changes, com, proofs):
    """on copies: the caller's arrays stay what they were"""
    com = None if com is None else com.copy()
    proofs = None if proofs is None else proofs.copy()
    idx = np.array([i for i, _ in changes], np.uint32)
    deltas = mont(oc, [dl % R for _, dl in changes])
    return h.vec_update(srs, log2d, *uconsts(oc, log2d), idx, deltas, com, proofs)


def check(oc, h, srs, log2d, evals, changes, start=None, what=""):
    com0, pr0 = start if start is not None else commit(oc, h, srs, evals, log2d)
    exp_com, exp_pr = commit(oc, h, srs, changed(evals, changes), log2d)
    com, pr = update(oc, h, srs, log2d, changes, com0, pr0)
    assert np.array_equal(pr, exp_pr), ("proofs", what, log2d, [i for i, _ in changes])
    assert np.array_equal(com, exp_com), ("commitment", what, log2d, [i for i, _ in changes])
    return com, pr


@pytest.fixture(scope="module")
def base(oc, hip):
    """512 unrelated points, the same SRS with and without window tables"""
    g1, _ = oc.generators()
    pts = hip.g1_mul_batch(g1, mont(oc, rand_fr_ints(N_SRS, 5151)))
    plain, tabled = hip.srs_g1_upload(pts), hip.srs_g1_upload(pts)
    hip.srs_g1_precompute(tabled)
    yield {"pts": pts, "plain": plain, "tabled": tabled}
    plain.free()
    tabled.free()


@pytest.fixture()
def own_ctx():
    """a context of its own: its options, workspaces and allocation limit are its own"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        yield h
    finally:
        h.debug_set_alloc_limit(0)
        h.close()


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [0, 1, 2, 3, 6, 7, 8])
def test_shapes(oc, hip, base, log2d):
    """one change at index 0, at d - 1, at 63 and at 64 (the wave edge) where the domain has them, and a random set with a duplicate; the plain and
    the tabled handle; the _dev form on resident arrays gives the bytes of the host form"""
    import torch
    d = 1 << log2d
    evals = rand_fr_ints(d, 200 + log2d)
    rnd = rand_fr_ints(16, 300 + log2d)
    singles = sorted({0, d - 1} | {i for i in (63, 64) if i < d})
    rset = [(rnd[8 + t] % d, rnd[t]) for t in range(5)] + [(rnd[8] % d, rnd[7])]
    for name in ("plain", "tabled"):
        start = commit(oc, hip, base[name], evals, log2d)
        for i in singles:
            check(oc, hip, base[name], log2d, evals, [(i, rnd[i % 7])], start, name)
        com, pr = check(oc, hip, base[name], log2d, evals, rset, start, name)
    # resident form (the tabled handle's start and result are the last of the loop)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda:0")
    d_idx = dev(np.array([i for i, _ in rset], np.uint32), np.int32)
    d_dl = dev(mont(oc, [dl for _, dl in rset]), np.int64)
    d_com, d_pr = dev(start[0], np.int64), dev(start[1], np.int64)
    torch.cuda.synchronize()
    hip.vec_update_dev(base["tabled"], log2d, *uconsts(oc, log2d), d_idx.data_ptr(), d_dl.data_ptr(), len(rset), d_com.data_ptr(), d_pr.data_ptr())
    hip.synchronize()
    assert np.array_equal(d_pr.cpu().numpy().view(np.uint64), pr) and np.array_equal(d_com.cpu().numpy().view(np.uint64), com)


# ---- 2. passes ------------------------------------------------------------------------------------------------------------------------------------
def test_passes(oc, base, own_ctx):
    """the list lengths at which the split changes shape (vec_update_model.pass_edge_ks) with three entries per pass, then every position of the
    domain with the built-in pass size"""
    log2d, h, srs = 6, own_ctx, base["plain"]
    d = 1 << log2d
    evals = rand_fr_ints(d, 77)
    rnd = rand_fr_ints(d, 78)
    start = commit(oc, h, srs, evals, log2d)
    h.set_option("vec_update_k_pass", 3)
    ks = M.pass_edge_ks(3)
    assert ks == [1, 2, 3, 4, 7]
    for k in ks:
        assert len(M.passes(k, 3)) == -(-k // 3)
        check(oc, h, srs, log2d, evals, [((11 * t + 60) % d, rnd[t]) for t in range(k)], start, "k_pass 3, k = %d" % k)
    for bad in (-1, M.UPD_K_PASS + 1):
        with pytest.raises(Exception):
            h.set_option("vec_update_k_pass", bad)
    h.set_option("vec_update_k_pass", 0)
    assert len(M.passes(d)) == d // M.UPD_K_PASS
    check(oc, h, srs, log2d, evals, [(i, rnd[i]) for i in range(d)], start, "every position")


# ---- 3. degenerate operands --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [2, 6])
def test_degenerate_operands(oc, hip, base, log2d):
    d = 1 << log2d
    srs = base["plain"]
    v = rand_fr_ints(1, 900 + log2d)[0]
    zero = commit(oc, hip, srs, [0] * d, log2d)
    assert not zero[1].any() and not zero[0][8:].any(), "the all-zero vector: identity proofs (0, 0) and the identity commitment (R, R, 0)"
    for i in (0, d - 1):
        unit = [0] * d
        unit[i] = v
        start = commit(oc, hip, srs, unit, log2d)
        # delta = v: the polynomial doubles, so lane i adds its proof to itself and the commitment meets itself
        com, pr = check(oc, hip, srs, log2d, unit, [(i, v)], start, "delta = v")
        assert pr.any()
        # delta = -v: every sum ends in a point and its negative
        com, pr = check(oc, hip, srs, log2d, unit, [(i, R - v)], start, "delta = -v")
        assert not pr.any() and np.array_equal(com, zero[0])
        # identity inputs
        check(oc, hip, srs, log2d, [0] * d, [(i, v)], zero, "from the all-zero vector")
    evals = rand_fr_ints(d, 910 + log2d)
    start = commit(oc, hip, srs, evals, log2d)
    dl = rand_fr_ints(1, 911)[0]
    com, pr = update(oc, hip, srs, log2d, [(1, dl), (1, R - dl)], *start)
    assert np.array_equal(com, start[0]) and np.array_equal(pr, start[1]), "(i, delta) with (i, -delta): bytes unchanged"
    com, pr = update(oc, hip, srs, log2d, [(d - 1, 0)], *start)
    assert np.array_equal(com, start[0]) and np.array_equal(pr, start[1]), "delta = 0"
    check(oc, hip, srs, log2d, evals, [(d // 2, R - 1)], start, "delta = r - 1")
    check(oc, hip, srs, log2d, evals, [(0, R - 1), (d - 1, 1), (0, 2)], start, "r - 1, 1, 2")


# ---- 4. structured SRS ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [3, 6])
@pytest.mark.parametrize("secret", ["zero", "one", "omega_1", "omega_half"])
def test_structured_srs(oc, hip, secret, log2d):
    """SRS tau^k g1 with tau = 0, 1 and on the domain: most table points a_i are the identity there, the transforms that build the tables run over
    equal points, and every result is a known multiple of g1 (vec_update_model on scalars)"""
    d = 1 << log2d
    w = M.omega(d)
    tau = {"zero": 0, "one": 1, "omega_1": w, "omega_half": pow(w, d // 2, R)}[secret]
    dl = S.powers(tau, d)
    a, u, _, _ = M.tables(dl, d)
    if secret != "zero":
        assert sum(1 for x in a if x) == 1, "tau on the domain: a_i is the identity for every i but one"
    srs = hip.srs_g1_upload(g1_of(oc, dl))
    try:
        evals = rand_fr_ints(d, 40 + log2d)
        rnd = rand_fr_ints(8, 41)
        start = commit(oc, hip, srs, evals, log2d)
        m_com, m_pr = M.commit_and_open(dl, evals)
        assert np.array_equal(start[1], g1_of(oc, m_pr)) and np.array_equal(jac_to_aff(start[0]), g1_of(oc, [m_com])[0])
        for changes in ([(0, rnd[0])], [(d // 2, rnd[1])], [(d - 1, rnd[2])], [(1, rnd[3]), (d // 2, rnd[4]), (1, rnd[5]), (d - 1, rnd[6])],
                        [(i, rnd[i % 8]) for i in range(d)] if log2d == 3 else [(i, rnd[i % 8]) for i in range(0, d, 7)]):
            com, pr = check(oc, hip, srs, log2d, evals, changes, start, secret)
            e_com, e_pr = M.update(dl, d, m_com, m_pr, changes)
            assert (e_com, e_pr) == M.commit_and_open(dl, changed(evals, changes))
            assert np.array_equal(pr, g1_of(oc, e_pr)) and np.array_equal(jac_to_aff(com), g1_of(oc, [e_com])[0]), (secret, changes)
    finally:
        srs.free()


# ---- 5. independent checks ----------------------------------------------------------------------------------------------------------------------------
def test_oracle_openings_and_pairing_check(oc, hip):
    """d = 8 on tau^k g1 with [tau]_2: the updated proofs are the oracle's MSMs of the quotients of the NEW polynomial, the pairing check accepts all
    of them against the updated commitment. With only the commitment updated no old proof survives (the commitment entered every one of them);
    with both updated, the check against the OLD values rejects exactly the changed positions."""
    log2d = 3
    d = 1 << log2d
    tau = S.secrets()["random"]
    g1, g2 = oc.generators()
    pts = g1_of(oc, S.powers(tau, d))
    tau_g2 = hip.g2_mul_batch(g2, mont(oc, [tau]))[0]
    w = mont(oc, [M.omega(d)])
    srs = hip.srs_g1_upload(pts)
    try:
        evals = rand_fr_ints(d, 31)
        changes = [(1, 1111), (6, R - 5), (1, 7)]
        new = changed(evals, changes)
        start = commit(oc, hip, srs, evals, log2d)
        com, pr = check(oc, hip, srs, log2d, evals, changes, start)
        p = M.coeffs_of(new)
        direct = []
        for j in range(d):
            z, acc, quot = pow(M.omega(d), j, R), 0, [0] * (d - 1)
            for t in range(d - 1, 0, -1):
                acc = (acc * z + p[t]) % R
                quot[t - 1] = acc
            direct.append(oc.msm_g1(pts[:d - 1], mont(oc, quot), threads=TH))
        assert np.array_equal(pr, np.stack(direct))
        assert np.array_equal(jac_to_aff(com), oc.msm_g1(pts, mont(oc, p), threads=TH))
        status, n_bad, _ = hip.kzg_verify_each(jac_to_aff(com), tau_g2, w, mont(oc, new), pr, point_mode=1)
        assert n_bad == 0 and not status.any()
        # only the commitment: proofs NULL in the call
        com_only, none = update(oc, hip, srs, log2d, changes, start[0], None)
        assert none is None and np.array_equal(com_only, com)
        status, n_bad, _ = hip.kzg_verify_each(jac_to_aff(com_only), tau_g2, w, mont(oc, new), start[1], point_mode=1)
        m_com, m_pr = M.commit_and_open(S.powers(tau, d), evals)
        m_new_com = M.commit_and_open(S.powers(tau, d), new)[0]
        expect = [int((m_new_com - new[j] - m_pr[j] * (tau - pow(M.omega(d), j, R))) % R != 0) for j in range(d)]
        assert expect == [1] * d and status.tolist() == expect
        status, n_bad, first = hip.kzg_verify_each(jac_to_aff(com), tau_g2, w, mont(oc, evals), pr, point_mode=1)
        assert status.tolist() == [int(j in (1, 6)) for j in range(d)] and n_bad == 2 and first == 1
    finally:
        srs.free()


# ---- 6. contract ------------------------------------------------------------------------------------------------------------------------------------------
def test_single_outputs_and_empty_calls(oc, hip, base):
    log2d, srs = 5, base["plain"]
    d = 1 << log2d
    evals = rand_fr_ints(d, 55)
    changes = [(3, 9), (d - 1, 123456789), (17, R - 2)]
    start = commit(oc, hip, srs, evals, log2d)
    exp = commit(oc, hip, srs, changed(evals, changes), log2d)
    com, none = update(oc, hip, srs, log2d, changes, start[0], None)
    assert none is None and np.array_equal(com, exp[0])
    none, pr = update(oc, hip, srs, log2d, changes, None, start[1])
    assert none is None and np.array_equal(pr, exp[1])
    assert update(oc, hip, srs, log2d, changes, None, None) == (None, None)
    com, pr = start[0].copy(), start[1].copy()
    hip.vec_update(srs, log2d, *uconsts(oc, log2d), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64), com, pr)          # k = 0
    assert np.array_equal(com, start[0]) and np.array_equal(pr, start[1])


def test_errors_write_nothing(oc, hip, base):
    lib, srs = hip.lib, base["plain"]
    log2d = 3
    d = 1 << log2d
    u = uconsts(oc, log2d)
    start = commit(oc, hip, srs, rand_fr_ints(d, 66), log2d)
    com, pr = start[0].copy(), start[1].copy()
    idx, dl = np.array([1, 7], np.uint32), mont(oc, [5, 6])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.keaki_hip_last_error(hip.ctx).decode()

    def call(srs_h=srs.handle, l=log2d, c=u, ix=idx, de=dl, k=2, cm=com, o=pr, fn=lib.keaki_hip_vec_update):
        return fn(hip.ctx, srs_h, l, p(c[0]), p(c[1]), p(c[2]), p(ix), p(de), k, p(cm), p(o))

    for bad in (dict(srs_h=None), dict(c=[None] + u[1:]), dict(c=[u[0], None, u[2]]), dict(c=u[:2] + [None]), dict(ix=None), dict(de=None), dict(l=28),
                dict(k=1 << 31), dict(ix=np.array([1, d], np.uint32)), dict(ix=np.array([0xFFFFFFFF, 0], np.uint32))):
        assert call(**bad) == ERR_BAD_ARG and "vec_update" in err(), bad
    for bad in (dict(srs_h=None), dict(c=[None] + u[1:]), dict(ix=None), dict(de=None), dict(l=28), dict(k=1 << 31)):
        assert call(fn=lib.keaki_hip_vec_update_dev, **bad) == ERR_BAD_ARG and "vec_update_dev" in err(), bad
    assert lib.keaki_hip_srs_g1_precompute_update(hip.ctx, None, log2d, p(u[0]), p(u[1]), p(u[2])) == ERR_BAD_ARG
    assert lib.keaki_hip_srs_g1_precompute_update(hip.ctx, srs.handle, 28, p(u[0]), p(u[1]), p(u[2])) == ERR_BAD_ARG
    u10 = uconsts(oc, 10)
    assert call(l=10, c=u10) == ERR_TOO_LARGE and call(l=10, c=u10, fn=lib.keaki_hip_vec_update_dev) == ERR_TOO_LARGE     # d = 1024 > 512 points
    assert lib.keaki_hip_srs_g1_precompute_update(hip.ctx, srs.handle, 10, p(u10[0]), p(u10[1]), p(u10[2])) == ERR_TOO_LARGE
    assert np.array_equal(com, start[0]) and np.array_equal(pr, start[1]), "a refused call writes nothing"
    assert call() == 0 and not np.array_equal(pr, start[1])                                                                # and the context still works


def test_refused_tables_and_accounting(oc, base, own_ctx):
    """an allocation limit below the table size: KEAKI_ERR_OOM, the arrays untouched, the next call without the limit correct; the tables are
    counted in the context's table bytes and leave with the handle"""
    from keaki_amd.hip import KeakiHipError
    log2d, h = 6, own_ctx
    d = 1 << log2d
    table_bytes = 192 * d
    evals = rand_fr_ints(d, 88)
    changes = [(0, 3), (63, 4)]
    srs = h.srs_g1_upload(base["pts"])
    try:
        start = commit(oc, h, srs, evals, log2d)
        exp = commit(oc, h, srs, changed(evals, changes), log2d)
        before = h.memory()["tables"]
        com, pr = start[0].copy(), start[1].copy()
        idx, dl = np.array([i for i, _ in changes], np.uint32), mont(oc, [x for _, x in changes])
        h.debug_set_alloc_limit(table_bytes - 1)
        with pytest.raises(KeakiHipError) as e:
            h.vec_update(srs, log2d, *uconsts(oc, log2d), idx, dl, com, pr)
        assert e.value.status == ERR_OOM
        with pytest.raises(KeakiHipError) as e:
            h.srs_g1_precompute_update(srs, log2d, *uconsts(oc, log2d))
        assert e.value.status == ERR_OOM
        assert np.array_equal(com, start[0]) and np.array_equal(pr, start[1]) and h.memory()["tables"] == before
        h.debug_set_alloc_limit(0)
        h.vec_update(srs, log2d, *uconsts(oc, log2d), idx, dl, com, pr)
        assert np.array_equal(com, exp[0]) and np.array_equal(pr, exp[1])
        assert h.memory()["tables"] == before + table_bytes
        h.srs_g1_precompute_update(srs, log2d - 1, *uconsts(oc, log2d - 1))          # another d replaces them
        assert h.memory()["tables"] == before + table_bytes // 2
    finally:
        srs.free()
    assert h.memory()["tables"] == before - 2 * d * 96, "the handle took its update tables and its FK23 transform (2d Jacobian points) along"


def test_cache_and_interleaving(oc, hip, base):
    """d, then d', then d again on one handle; vec_commit calls at the same d in between (its FK23 transform and the update tables do not evict
    each other: the table bytes hold both)"""
    la, lb = 5, 3
    srs = hip.srs_g1_upload(base["pts"])
    try:
        ea, eb = rand_fr_ints(1 << la, 1), rand_fr_ints(1 << lb, 2)
        ca, cb = [(0, 5), (31, 6), (7, 7)], [(7, 8), (0, 9)]
        sa, sb = commit(oc, hip, srs, ea, la), commit(oc, hip, srs, eb, lb)
        t0 = hip.memory()["tables"]
        first_a = check(oc, hip, srs, la, ea, ca, sa)
        assert hip.memory()["tables"] == t0 - (2 << lb) * 96 + (2 << la) * 96 + (192 << la)      # check() committed at d: the transform of d and the tables of d
        first_b = check(oc, hip, srs, lb, eb, cb, sb)
        again = check(oc, hip, srs, la, ea, ca, sa)
        assert np.array_equal(again[0], first_a[0]) and np.array_equal(again[1], first_a[1])
        for _ in range(2):
            assert np.array_equal(commit(oc, hip, srs, ea, la)[1], sa[1])
            com, pr = update(oc, hip, srs, la, ca, *sa)
            assert np.array_equal(com, first_a[0]) and np.array_equal(pr, first_a[1])
        assert hip.memory()["tables"] == t0 - (2 << lb) * 96 + (2 << la) * 96 + (192 << la)
        hip.srs_g1_precompute_update(srs, lb, *uconsts(oc, lb))
        com, pr = update(oc, hip, srs, lb, cb, *sb)
        assert np.array_equal(com, first_b[0]) and np.array_equal(pr, first_b[1])
    finally:
        srs.free()


# ---- 7. host API --------------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_vec_update(oc):
    """keaki::vec::vec_update of the C++ mirror: vec_commit, three changes, and the result is vec_commit of the changed vector from the same
    padding scalar (the same rng seed); vec_verify accepts it"""
    import keaki_amd.keaki as K
    dev = K.Device(0)
    st = K.KZGSetup.setup(mont(oc, [S.secrets()["random"]])[0], 32, device=dev)
    try:
        v = rand_fr_ints(20, 1234)
        new = list(v)
        idx = [0, 19, 7]
        for t, i in enumerate(idx):
            new[i] = (new[i] * 3 + t + 1) % R
        K.precompute_vec_update(st, 32)
        com, proofs = K.vec_commit(K.Rng(11), st, mont(oc, v))
        assert proofs.shape[0] == 32
        c2, p2 = K.vec_update(st, com, proofs, idx, mont(oc, [v[i] for i in idx]), mont(oc, [new[i] for i in idx]))
        e_com, e_pr = K.vec_commit(K.Rng(11), st, mont(oc, new))
        assert np.array_equal(c2, e_com) and np.array_equal(p2, e_pr)
        assert K.vec_verify(K.Rng(5), st, c2, mont(oc, new), p2) and not K.vec_verify(K.Rng(5), st, c2, mont(oc, v), p2)
        # the flat form takes the differences and works in place
        c3, p3 = com.copy(), proofs.copy()
        K.vec_update_flat(st, 32, idx, mont(oc, [(new[i] - v[i]) % R for i in idx]), c3, p3)
        assert np.array_equal(c3, e_com) and np.array_equal(p3, e_pr)
        with pytest.raises(K.KeakiHostError):
            K.vec_update(st, com, proofs, [32], mont(oc, [1]), mont(oc, [2]))
    finally:
        st.close()
        dev.close()
