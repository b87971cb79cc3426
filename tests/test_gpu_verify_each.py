"""keaki_hip_kzg_verify_each / _dev, K.verify_each, K.locate_invalid and K.vec_verify_each on the GPU against the discrete-log model
(tests/verify_each_model.py). Inputs have KNOWN discrete logs -- C_i = c_i g1, proof_i = p_i g1, [tau]_2 = s g2 -- so the expected verdicts are
exact integer arithmetic and the expected L_i are oracle scalar-mults; nothing expected comes from the library under test. In every case
status, n_bad and first_bad are compared with the model."""
import ctypes as C
import os

import numpy as np
import pytest

import verify_each_model as M
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
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU)


class Arrays:
    """a Case as the arrays of the C ABI; omega: the generator of point_mode 1 (then c.z must be its powers)"""

    def __init__(self, oc, c, omega=None, proofs=None, coms=None):
        self.c, self.n = c, c.n
        self.tau_g2 = oc.g2_mul_batch(oc.generators()[1], mont(oc, [c.s]))[0]
        self.coms = g1_of(oc, c.com) if coms is None else coms
        self.proofs = g1_of(oc, c.p) if proofs is None else proofs
        self.z, self.y = mont(oc, c.z), mont(oc, c.y)
        self.omega = mont(oc, [omega]) if omega is not None else None

    def run(self, hip, mode=0, want_lhs=False):
        return hip.kzg_verify_each(self.coms, self.tau_g2, self.omega if mode else self.z, self.y, self.proofs, point_mode=mode, want_lhs=want_lhs)


def check(hip, a, mode=0, what=""):
    """status, n_bad, first_bad == the model's; returns the status list"""
    status, n_bad, first = a.run(hip, mode)
    assert status.tolist() == a.c.status(), "status %s" % what
    assert (n_bad, first) == a.c.counters(), "counters %s" % what
    return status.tolist()


def base_case(n, seed, stride=0):
    r = rand_fr_ints(3 * n + 2, seed)
    return M.valid_case(r[0], r[1:2] if stride == 0 else r[2 + 2 * n:2 + 3 * n], r[2:2 + n], r[2 + n:2 + 2 * n])


def with_bad(c, idx):
    b = c.copy()
    for i in idx:
        b.y[i] = (b.y[i] + 1) % R
    return b


_P65 = {}


def proofs65(oc):
    """the 65-item base case and its proof points, shared by the wave-edge cases"""
    if not _P65:
        c = base_case(65, 6500)
        _P65["c"], _P65["proofs"], _P65["coms"] = c, g1_of(oc, c.p), g1_of(oc, c.com)
    return _P65["c"], _P65["proofs"], _P65["coms"]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65])
def test_wave_edges_all_valid(oc, hip, n):
    c, proofs, coms = proofs65(oc)
    assert check(hip, Arrays(oc, c.head(n), proofs=proofs[:n], coms=coms)) == [0] * n


@pytest.mark.parametrize("bad", [[0], [31], [32], [64], list(range(0, 65, 2)), list(range(65))], ids=["0", "31", "32", "64", "every_second", "all"])
def test_wave_edges_invalid_sets_at_65(oc, hip, bad):
    """a wave holds 32 items and tail lanes redo the last one: a bad last item must not leak into the lanes that repeat it, and the reverse"""
    c, proofs, coms = proofs65(oc)
    st = check(hip, Arrays(oc, with_bad(c, bad), proofs=proofs, coms=coms))
    assert [i for i, s in enumerate(st) if s] == bad


def test_kinds_of_corruption_n_64(oc, hip):
    """wrong value, wrong point, wrong proof (stride 0) and wrong commitment (stride 1), each on its own subset"""
    c0, c1 = base_case(64, 6400), base_case(64, 6401, stride=1)
    p0, p1 = g1_of(oc, c0.p), g1_of(oc, c1.p)
    k = c0.copy()
    for i in (1, 5, 63):
        k.y[i] = (k.y[i] + 7) % R
    assert sum(check(hip, Arrays(oc, k, proofs=p0), what="value")) == 3
    k = c0.copy()
    for i in (10, 33):
        k.z[i] = (k.z[i] + 1) % R
    assert sum(check(hip, Arrays(oc, k, proofs=p0), what="point")) == 2
    k = c0.copy()
    k.p[20], k.p[62] = (k.p[20] + 1) % R, 0xC0FFEE
    assert sum(check(hip, Arrays(oc, k), what="proof")) == 2
    k = c1.copy()
    k.com[0], k.com[40] = (k.com[0] + 1) % R, 0
    assert sum(check(hip, Arrays(oc, k, proofs=p1), what="commitment")) == 2
    assert sum(check(hip, Arrays(oc, c1, proofs=p1), what="stride 1, valid")) == 0


def special_case(n=100):
    """n items, stride 1, valid and invalid, with the boundary scalars and every branch of the two additions"""
    r = rand_fr_ints(3 * n + 1, 1009)
    c = M.valid_case(r[0], r[1:1 + n], r[1 + n:1 + 2 * n], r[1 + 2 * n:1 + 3 * n])
    for i in range(40, 60, 3):
        c.y[i] = (c.y[i] + i) % R                                         # ordinary invalid items
    c.z[0] = 0; c.y[1] = 0; c.z[2] = R - 1; c.y[3] = R - 1
    c.com[4] = 0                                                          # C the identity
    c.p[5] = 0                                                            # proof the identity, L is not: invalid
    c.p[6] = 0; c.y[6] = c.com[6]                                         # both identities: valid
    c.y[7] = (c.com[7] - c.z[7] * c.p[7]) % R                             # C - y g1 = z proof: the doubling branch of the last addition
    c.y[8] = (c.com[8] + c.z[8] * c.p[8]) % R                             # C - y g1 = -z proof: L the identity, the proof is not
    c.y[9] = c.com[9]                                                     # y g1 = C: the first addition meets -C, L = z proof
    c.y[10] = (-c.com[10]) % R                                            # y g1 = -C: the first addition doubles
    c.com[11] = 0; c.y[11] = 0; c.z[11] = 0                               # L = 0 + 0 + 0 with a proof: identity from three identities
    return c


def test_lhs_out_is_bit_exact(oc, hip):
    c = special_case()
    a = Arrays(oc, c)
    status, n_bad, first, lhs = a.run(hip, want_lhs=True)
    expect = g1_of(oc, c.lhs())
    # the same points by the oracle's group arithmetic on the POINTS: C + (-y) g1 + z proof
    g1 = oc.generators()[0]
    my = oc.g1_mul_batch(g1, mont(oc, [-y for y in c.y]), threads=NCPU)
    zp = oc.g1_mul_batch(a.proofs, a.z, threads=NCPU)
    for i in range(c.n):
        assert np.array_equal(oc.g1_sum(np.stack([a.coms[i], my[i], zp[i]])), expect[i]), "the two derivations of L_%d disagree" % i
    assert not expect[8].any() and not expect[6].any() and not expect[11].any() and expect[7].any()
    for i in range(c.n):
        assert np.array_equal(lhs[i], expect[i]), "L_%d" % i
    assert status.tolist() == c.status() and (n_bad, first) == c.counters()
    assert c.status()[6] == 0 and c.status()[5] == 1 and c.status()[8] == 1 and c.status()[11] == 1
    # lhs_out_aff does not change the verdicts
    s2, b2, f2 = a.run(hip)
    assert s2.tolist() == c.status() and (b2, f2) == (n_bad, first)


def test_degenerate_operands_share_a_wave_with_ordinary_items(oc, hip):
    r = rand_fr_ints(200, 4242)
    n = 64
    c = M.valid_case(r[0], [r[1]], r[2:2 + n], r[70:70 + n])
    for i in (3, 17, 40):
        c.y[i] = (c.y[i] + 1) % R
    c.p[8] = 0; c.y[8] = c.com[0]                                         # both identities: valid
    c.p[9] = 0; c.y[9] = (c.com[0] + 5) % R                               # the proof alone: invalid
    c.y[10] = (c.com[0] + c.z[10] * c.p[10]) % R                          # L alone: invalid
    c.p[31] = 0; c.y[31] = c.com[0]                                       # ... and on the wave's last lane pair
    c.p[32] = 0; c.y[32] = (c.com[0] + 1) % R
    st = check(hip, Arrays(oc, c))
    assert [i for i, s in enumerate(st) if s] == [3, 9, 10, 17, 32, 40]
    # [tau]_2 = identity: valid_i <=> L_i is the identity
    t = M.valid_case(0, [r[1]], r[2:2 + n], r[70:70 + n])
    assert all(l == 0 for l in t.lhs())
    t.y[5] = (t.y[5] + 1) % R
    t.p[6] = 0; t.y[6] = t.com[0]
    t.p[7] = 0; t.y[7] = (t.com[0] + 1) % R
    a = Arrays(oc, t)
    assert not a.tau_g2.any()
    st = check(hip, a)
    assert [i for i, s in enumerate(st) if s] == [5, 7]


def test_modes(oc, py, hip):
    """com_stride 0 and 1, point_mode 0 and 1 (omega of order 128, n = 70)"""
    n = 70
    w = py.fr_root_of_unity(128)
    r = rand_fr_ints(2 * n + 2, 7070)
    zs = M.powers(w, n)
    for coms in (r[1:2], r[2 + n:2 + 2 * n]):
        c = M.valid_case(r[0], coms, zs, r[2:2 + n])
        for i in (0, 33, 69):
            c.y[i] = (c.y[i] + 1) % R
        a = Arrays(oc, c, omega=w)
        for mode in (0, 1):
            st = check(hip, a, mode, what="coms=%d mode=%d" % (len(coms), mode))
            assert [i for i, s in enumerate(st) if s] == [0, 33, 69]


def test_agreement_with_single_verify_and_verify_batch(oc, hip):
    r = rand_fr_ints(64, 808)
    c = M.valid_case(r[0], r[1:9], r[9:17], r[17:25])
    c.y[1] = (c.y[1] + 1) % R
    c.z[2] = (c.z[2] + 1) % R
    c.p[4] = 0
    c.p[6] = 0; c.y[6] = c.com[6]
    c.com[7] = (c.com[7] + 1) % R
    a = Arrays(oc, c)
    st = check(hip, a)
    assert st == [0, 1, 1, 0, 1, 0, 0, 1]
    for i in range(8):
        assert st[i] == (0 if hip.kzg_verify(a.coms[i], a.tau_g2, a.z[i], a.y[i], a.proofs[i]) else 1), i
    good = Arrays(oc, M.valid_case(r[0], r[1:9], r[9:17], r[17:25]))
    gam = mont(oc, r[30:38])
    assert hip.kzg_verify_batch(good.coms, good.tau_g2, good.z, good.y, good.proofs, gam)[0]
    assert check(hip, good) == [0] * 8
    one = good.c.copy()
    one.y[5] = (one.y[5] + 1) % R
    b = Arrays(oc, one, proofs=good.proofs, coms=good.coms)
    assert not hip.kzg_verify_batch(b.coms, b.tau_g2, b.z, b.y, b.proofs, gam)[0]
    assert check(hip, b) == [0, 0, 0, 0, 0, 1, 0, 0]


def test_locate_invalid_through_the_host_mirror(K, oc, py):
    rng = K.Rng(2025)
    secret = rng.fr_rand()
    s = K.KZGSetup.setup(secret, 4)
    try:
        tau = oc.limbs_to_ints(oc.fr_from_mont(secret[None, :]))[0]
        n = 12
        r = rand_fr_ints(3 * n, 1212)
        c = M.valid_case(tau, r[:n], r[n:2 * n], r[2 * n:3 * n])
        a = Arrays(oc, c)
        assert K.verify_batch(K.Rng(1), s, a.coms, a.z, a.y, a.proofs)
        assert K.verify_each(s, a.coms, a.z, a.y, a.proofs).tolist() == [0] * n
        r1, r2 = K.Rng(77), K.Rng(77)
        assert K.locate_invalid(r1, s, a.coms, a.z, a.y, a.proofs) == []
        assert K.verify_batch(r2, s, a.coms, a.z, a.y, a.proofs)
        assert np.array_equal(r1.fr_rand(), r2.fr_rand()), "locate_invalid must draw what verify_batch draws"
        c.y[7] = (c.y[7] + 1) % R
        b = Arrays(oc, c, proofs=a.proofs, coms=a.coms)
        r1, r2 = K.Rng(78), K.Rng(78)
        assert not K.verify_batch(r2, s, b.coms, b.z, b.y, b.proofs)
        assert K.locate_invalid(r1, s, b.coms, b.z, b.y, b.proofs) == [7]
        assert np.array_equal(r1.fr_rand(), r2.fr_rand())
        assert K.verify_each(s, b.coms, b.z, b.y, b.proofs).tolist() == c.status()
        # vec_verify_each: the powers of the generator of the domain of n + PADDING_LEN evaluations, one shared commitment
        w = py.fr_root_of_unity(16)
        v = M.valid_case(tau, r[:1], M.powers(w, n), r[2 * n:3 * n])
        v.y[3] = (v.y[3] + 1) % R
        av = Arrays(oc, v)
        assert K.vec_verify_each(s, av.coms[0], av.y, av.proofs).tolist() == v.status()
        assert K.verify_each(s, av.coms, mont(oc, [w]), av.y, av.proofs, roots_of_unity=True).tolist() == v.status()
    finally:
        s.close()


def big_case(oc, hip):
    """n = 2^17 + 3 (one launch chunk + 3), com_stride 0, point_mode 1; the proofs come from the GPU's g1_mul_batch"""
    n = (1 << 17) + 3
    r = rand_fr_ints(4, 131)
    w_int = py_root18()
    ps = [(r[2] * (i + 1) * (i + 1) + r[3]) % R for i in range(n)]
    c = M.valid_case(r[0], [r[1]], M.powers(w_int, n), ps)
    for i in (0, (1 << 17) - 1, 1 << 17, n - 1):
        c.y[i] = (c.y[i] + 1) % R
    proofs = hip.g1_mul_batch(oc.generators()[0], mont(oc, ps))
    # a sample of the GPU-made proofs against the oracle
    idx = [0, 1, (1 << 17) - 1, 1 << 17, n - 1]
    assert np.array_equal(proofs[idx], g1_of(oc, [ps[i] for i in idx]))
    return Arrays(oc, c, omega=w_int, proofs=proofs)


def test_launch_chunk_and_halving(oc):
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        a = big_case(oc, h)
        bad = [0, (1 << 17) - 1, 1 << 17, a.n - 1]
        status, n_bad, first = a.run(h, mode=1)
        assert np.flatnonzero(status).tolist() == bad and (n_bad, first) == (4, 0)
        full = h.memory()["workspaces"]
        # the same under an allocation limit that refuses the slots of a full chunk: the chunk halves, the verdicts stay
        h.trim()
        h.debug_set_alloc_limit(64 << 20)
        status, n_bad, first = a.run(h, mode=1)
        assert np.flatnonzero(status).tolist() == bad and (n_bad, first) == (4, 0)
        assert h.memory()["workspaces"] < full // 2
        h.debug_set_alloc_limit(0)
        # not even one wave of items fits: KEAKI_ERR_OOM, and the context stays usable
        from keaki_amd.hip import KeakiHipError
        h.trim()
        h.debug_set_alloc_limit(64)
        with pytest.raises(KeakiHipError) as e:
            a.run(h, mode=1)
        assert e.value.status == OOM
        h.debug_set_alloc_limit(0)
        small = Arrays(oc, a.c.head(40), omega=py_root18(), proofs=a.proofs[:40])
        assert check(h, small, mode=1) == [1] + [0] * 39
    finally:
        h.close()


def py_root18():
    import bn254_py as py
    return py.fr_root_of_unity(1 << 18)


def test_dev_form_queued_behind_its_producer(oc, hip):
    """status in device memory, counters on the host; the proofs are produced by a g1_mul_batch_dev enqueued on the context's stream right before"""
    import torch
    n = 97
    r = rand_fr_ints(3 * n + 2, 9797)
    c = M.valid_case(r[0], r[1:2], r[2:2 + n], r[2 + n:2 + 2 * n])
    for i in (2, 64, 96):
        c.y[i] = (c.y[i] + 1) % R
    a = Arrays(oc, c, proofs=np.zeros((n, 8), np.uint64))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64).copy()).cuda()
    d_g1, d_p, d_com, d_tau, d_z, d_y = t(oc.generators()[0]), t(mont(oc, c.p)), t(a.coms), t(a.tau_g2), t(a.z), t(a.y)
    d_proofs = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    d_status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_lhs = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_p.data_ptr(), n, d_proofs.data_ptr())
    n_bad, first = hip.kzg_verify_each_dev(d_com, 0, d_tau, d_z, 0, d_y, d_proofs, n, d_status, d_lhs)
    assert d_status.cpu().numpy().tolist() == c.status() and (n_bad, first) == c.counters() == (3, 2)
    assert np.array_equal(d_lhs.cpu().numpy().view(np.uint64).reshape(n, 8), g1_of(oc, c.lhs()))
    # without d_lhs, and with the commitment per item
    c1 = M.valid_case(r[0], r[2 + 2 * n:2 + 3 * n], r[2:2 + n], r[2 + n:2 + 2 * n])
    c1.y[50] = (c1.y[50] + 1) % R
    a1 = Arrays(oc, c1, proofs=np.zeros((n, 8), np.uint64))
    d_com1, d_y1 = t(a1.coms), t(a1.y)
    torch.cuda.synchronize()
    assert hip.kzg_verify_each_dev(d_com1, 1, d_tau, d_z, 0, d_y1, d_proofs, n, d_status) == (1, 50)
    assert d_status.cpu().numpy().tolist() == c1.status()


def test_state_tau_rekeys_and_nothing_leaks(oc):
    from bench import random_fr_limbs
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        n = 40
        r = rand_fr_ints(3 * n + 4, 5151)
        ps = g1_of(oc, r[4:4 + n])
        c1 = M.valid_case(r[0], [r[2]], r[4 + n:4 + 2 * n], r[4:4 + n])
        c2 = M.valid_case(r[1], [r[2]], r[4 + n:4 + 2 * n], r[4:4 + n])
        a1, a2 = Arrays(oc, c1, proofs=ps), Arrays(oc, c2, proofs=ps)
        # the items valid under tau_1 presented with tau_2, and the reverse: all invalid (the proofs are not the identity)
        x12 = Arrays(oc, M.Case(c2.s, c1.com, c1.z, c1.y, c1.p), proofs=ps)
        four = random_fr_limbs(12, 44)

        def others():
            ct, gt, key = h.encap_batch(a1.coms[0], a1.tau_g2, four[:4], four[4:8], four[8:12], 32)
            dgt, dkey = h.decap_batch(ps[:4], ct, 32)
            return [x.copy() for x in (ct, gt, key, dgt, dkey)]
        before = others()
        for a in (a1, a2, a1, x12, a1):
            check(h, a)
        assert check(h, x12) == [1] * n and check(h, a2) == [0] * n
        assert all(np.array_equal(p, q) for p, q in zip(before, others()))
        assert h.memory()["workspaces"] > 32 * 3840
        h.trim()
        assert h.memory()["workspaces"] == 0
        assert check(h, a2) == [0] * n and check(h, a1) == [0] * n
        assert all(np.array_equal(p, q) for p, q in zip(before, others()))
    finally:
        h.close()


def test_error_paths_and_n_0(oc, hip):
    from keaki_amd.hip import _ptr
    c, proofs, coms = proofs65(oc)
    a = Arrays(oc, c, proofs=proofs, coms=coms)
    status = np.full(a.n, 9, np.uint8)
    lhs = np.full((a.n, 8), 9, np.uint64)
    bad, first = C.c_uint64(1234), C.c_uint64(5678)
    full = [_ptr(a.coms), 0, _ptr(a.tau_g2), _ptr(a.z), 0, _ptr(a.y), _ptr(a.proofs), a.n, _ptr(status), C.byref(bad), C.byref(first), _ptr(lhs)]
    cases = [(1, 2), (1, -1), (4, 2), (4, -1), (0, None), (2, None), (3, None), (5, None), (6, None), (8, None), (9, None), (7, 1 << 31), (7, (1 << 40) + 5)]
    for fn in (hip.lib.keaki_hip_kzg_verify_each, hip.lib.keaki_hip_kzg_verify_each_dev):
        for pos, val in cases:
            args = list(full)
            args[pos] = val
            assert fn(hip.ctx, *args) == BAD_ARG, pos
            assert hip.lib.keaki_hip_last_error(hip.ctx), pos
            assert (status == 9).all() and (lhs == 9).all() and (bad.value, first.value) == (1234, 5678), "a refused call wrote something (%d)" % pos
    # n = 0: the counters, nothing else; null arrays are fine
    for fn in (hip.lib.keaki_hip_kzg_verify_each, hip.lib.keaki_hip_kzg_verify_each_dev):
        bad.value, first.value = 1234, 5678
        assert fn(hip.ctx, None, 0, None, None, 0, None, None, 0, None, C.byref(bad), C.byref(first), None) == 0
        assert (bad.value, first.value) == (0, (1 << 64) - 1) and (status == 9).all()
        assert fn(hip.ctx, None, 0, None, None, 0, None, None, 0, None, C.byref(bad), None, None) == 0
    # first_bad and lhs_out_aff are optional; the context is usable after the refused calls
    args = list(full)
    args[10] = None
    args[11] = None
    assert hip.lib.keaki_hip_kzg_verify_each(hip.ctx, *args) == 0
    assert bad.value == 0 and not status.any() and (lhs == 9).all()
