"""One verdict per coset on the GPU (keaki_hip_kzg_verify_cosets_each, _dev) against the big-integer model (tests/coset_pairs_model.py): status, n_bad,
first_bad and the bytes of L_k = A_k + c_k proof_k. The SRS comes from a KNOWN tau; expected points are (integer) x generator from the oracle,
expected proofs come from long division by x^l - c (fk_coset_model); nothing expected comes from the library under test.
tests/test_coset_pairs_model.py shows on the CPU that every corruption used here flips exactly the verdicts it is meant to."""
import os

import numpy as np
import pytest

import coset_pairs_model as P
import coset_verify_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu
corrupt = P.corrupt

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, TOO_LARGE = -1, -5
TAU = rand_fr_ints(1, 20261021)[0]
SRS_LEN = 1024
SHAPES = [(4, 1), (6, 2), (6, 6), (8, 3), (10, 4), (11, 10), (5, 0)]
SENT = np.uint64(0xDEADBEEFDEADBEEF)


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def g1_of(oc, dls):
    out = oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU).copy()
    for i, x in enumerate(dls):
        if x % R == 0:
            out[i] = 0
    return out


def g2_of(oc, dl):
    if dl % R == 0:
        return np.zeros(16, np.uint64)
    return oc.g2_mul_batch(oc.generators()[1], mont(oc, [dl]), threads=1)[0]


def dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def env(oc, hip):
    pw = [1]
    for _ in range(SRS_LEN - 1):
        pw.append(pw[-1] * TAU % R)
    g1 = g1_of(oc, pw)
    plain, tabled = hip.srs_g1_upload(g1), hip.srs_g1_upload(g1)
    hip.srs_g1_precompute(tabled)
    e = {"g1": g1, "plain": plain, "tabled": tabled, "cache": {}}
    yield e
    hip.set_option("coset_rows_route", 0)
    hip.debug_set_alloc_limit(0)
    for h in (plain, tabled):
        h.free()


class Inputs:
    def __init__(self, oc, c):
        self.c, self.n, self.l, self.log2l = c, c.n, c.l, c.l.bit_length() - 1
        pts = g1_of(oc, list(c.com) + list(c.q) + [P.lhs_dl(c, k) for k in range(c.n)])
        self.com, self.proofs, self.want_l = pts[:len(c.com)], pts[len(c.com):len(c.com) + c.n], pts[len(c.com) + c.n:]
        self.want = np.array(P.statuses(c), np.uint8)
        self.tau_l = g2_of(oc, c.tau_l)
        self.h = mont(oc, c.h)
        self.values = mont(oc, [v for row in c.y for v in row])
        w = M.omega(c.l)
        self.winv, self.linv = mont(oc, [M.inv(w)])[0], mont(oc, [M.inv(c.l)])[0]

    def call(self, hip, srs, **kw):
        a = dict(com=self.com, points=self.h, values=self.values, strides=(self.l, 1), point_mode=0, proofs=self.proofs, tau_l=self.tau_l, want_lhs=True)
        a.update(kw)
        return hip.kzg_verify_cosets_each(srs, a["com"], a["tau_l"], a["points"], a["values"], a["strides"][0], a["strides"][1], self.log2l, self.winv,
                                          self.linv, a["proofs"], point_mode=a["point_mode"], want_lhs=a["want_lhs"])

    def check(self, got, what=""):
        status, n_bad, first = got[:3]
        assert np.array_equal(status, self.want), (what, np.nonzero(status != self.want)[0][:8])
        bad = np.nonzero(self.want)[0]
        assert n_bad == len(bad) and first == (int(bad[0]) if len(bad) else None), what
        if len(got) > 3:
            wrong = [k for k in range(self.n) if not np.array_equal(got[3][k], self.want_l[k])]
            assert not wrong, (what, wrong[:8])


def both_routes(hip, x, srs, what, **kw):
    try:
        for route in (1, 2):
            hip.set_option("coset_rows_route", route)
            x.check(x.call(hip, srs, **kw), (what, route))
    finally:
        hip.set_option("coset_rows_route", 0)


def rows_case(n, l, degree, seed, shared=True):
    r = rand_fr_ints(2 * n + (degree + 1) * (1 if shared else n), seed)
    hs, gammas, rest = r[:n], r[n:2 * n], r[2 * n:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(TAU, polys, hs, l, gammas)


def vector(oc, env, log2d, log2l):
    key = (log2d, log2l)
    if key not in env["cache"]:
        r = 1 << (log2d - log2l)
        rnd = rand_fr_ints(r + (1 << log2d), 5000 + 32 * log2d + log2l)
        c, evals = M.vector_case(TAU, rnd[r:], log2d, log2l, rnd[:r])
        env["cache"][key] = (c, Inputs(oc, c), mont(oc, evals))
    return env["cache"][key]


# ---- 1. valid vectors -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d,log2l", SHAPES)
def test_valid_vectors_give_all_zeros(oc, hip, env, log2d, log2l):
    c, x, evals = vector(oc, env, log2d, log2l)
    assert not x.want.any()
    omega_d = mont(oc, [M.omega(1 << log2d)])
    both_routes(hip, x, env["tabled"], "rows")
    got = x.call(hip, env["plain"], values=evals, strides=(1, c.n), point_mode=1, points=omega_d)
    x.check(got, "domain order, omega")
    assert got[1] == 0 and got[2] is None
    x.check(x.call(hip, env["plain"], com=np.repeat(x.com, c.n, axis=0), want_lhs=False), "n commitments, no L")


# ---- 2. corrupted items -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["value", "proof", "shift", "swap"])
def test_one_corruption_marks_exactly_its_items(oc, hip, env, kind):
    c, _, _ = vector(oc, env, 6, 2)
    b = corrupt(c, kind, 5, 11)
    x = Inputs(oc, b)
    assert sorted(np.nonzero(x.want)[0]) == ([5, 11] if kind == "swap" else [5])
    both_routes(hip, x, env["tabled"], kind)


def test_bad_items_at_the_edges_of_the_launch_chunks(oc, hip, env):
    """300 items of l = 16 under an allocation limit of 180,000 B (set after a warm-up call has built the context's tables): the rows of 300 items
    (201,600 B) are refused and the halved chunk of 150 fits; the final exponentiation's slots (1.2 MB for 300 items) are refused too and verify_each's
    own chunk halves down to 64 or 32 items. Bad: the first and last item of both row chunks and of the first pairing chunk at either size, and two more"""
    n, l = 300, 16
    c = rows_case(n, l, 24, 909)
    for k in (0, 31, 32, 63, 64, 149, 150, 200, 299):
        c.q[k] = (c.q[k] + 1 + k) % R
    x = Inputs(oc, c)
    assert x.want.sum() == 9
    warm = Inputs(oc, rows_case(2, l, 24, 910))
    warm.check(warm.call(hip, env["plain"]))
    try:
        hip.debug_set_alloc_limit(180000)
        x.check(x.call(hip, env["plain"]), "chunked")
    finally:
        hip.debug_set_alloc_limit(0)
    x.check(x.call(hip, env["plain"]), "whole")


# ---- 3. identities ---------------------------------------------------------------------------------------------------------------------------------------
def test_identities_are_ordinary_inputs(oc, hip, env):
    l = 4
    r = rand_fr_ints(4 * (l + 1) + 2, 29)
    hs, a = r[:4], [r[4 + k * l:4 + (k + 1) * l] for k in range(4)]
    i_tau = [sum(aj * pow(TAU, j, R) for j, aj in enumerate(a[k])) % R for k in range(4)]
    # 0: A and the proof the identity: valid | 1: A the identity, a proof: invalid | 2: a proof of the identity, A not: invalid | 3: C the identity, valid
    q3 = r[-1]
    com = [i_tau[0], i_tau[1], (i_tau[2] + 5) % R, 0]
    q = [0, r[-2], 0, q3]
    c = M.Case(TAU, l, com, hs, [P.values_from_coeffs(hs[k], a[k]) for k in range(4)], q, [1] * 4)
    # item 3: C = 0, so A = -I(tau); choose a_0 of item 3 so that -I(tau) = q3 (tau^l - h^l)
    shift = (i_tau[3] + q3 * (pow(TAU, l, R) - pow(hs[3], l, R))) % R
    a[3][0] = (a[3][0] - shift) % R
    c.y[3] = P.values_from_coeffs(hs[3], a[3])
    x = Inputs(oc, c)
    assert list(x.want) == [0, 1, 1, 0] and not x.want_l[0].any() and not x.proofs[0].any() and not x.com[3].any()
    both_routes(hip, x, env["tabled"], "identities")


def test_tau_l_the_identity(oc, hip, env):
    """[tau^l]_2 = identity: no pairing, valid <=> L_k is the identity"""
    l = 2
    r = rand_fr_ints(3 * 4, 31)
    hs, a, q = r[:3], [r[3 + 2 * k:5 + 2 * k] for k in range(3)], r[9:12]
    i_tau = [sum(aj * pow(TAU, j, R) for j, aj in enumerate(a[k])) % R for k in range(3)]
    com = [(i_tau[0] - pow(hs[0], l, R) * q[0]) % R, (i_tau[1] + 1) % R, (i_tau[2] - pow(hs[2], l, R) * q[2]) % R]      # L_0 = L_2 = identity
    c = M.Case(TAU, l, com, hs, [P.values_from_coeffs(hs[k], a[k]) for k in range(3)], q, [1] * 3, tau_l=0)
    x = Inputs(oc, c)
    assert list(x.want) == [0, 1, 0] and not x.tau_l.any() and not x.want_l[0].any()
    both_routes(hip, x, env["plain"], "tau_l = identity")


# ---- 4. the stated equalities --------------------------------------------------------------------------------------------------------------------------------
def test_l_1_gives_the_bytes_of_verify_each(oc, hip, env):
    c = rows_case(37, 1, 9, 31, shared=False)
    c.q[3] = (c.q[3] + 1) % R
    c.y[20][0] = (c.y[20][0] + 1) % R
    x = Inputs(oc, c)
    assert sorted(np.nonzero(x.want)[0]) == [3, 20]
    got = x.call(hip, env["tabled"])
    x.check(got)
    ve = hip.kzg_verify_each(x.com, g2_of(oc, TAU), x.h, x.values, x.proofs, want_lhs=True)
    assert np.array_equal(ve[0], got[0]) and ve[1:3] == got[1:3] and np.array_equal(ve[3], got[3])


def test_status_is_verify_multi_and_n_bad_zero_is_verify_cosets(oc, hip, env):
    c, x0, _ = vector(oc, env, 4, 2)
    pw = [1]
    for _ in range(c.l):
        pw.append(pw[-1] * TAU % R)
    srs2 = hip.srs_g2_upload(oc.g2_mul_batch(oc.generators()[1], mont(oc, pw), threads=NCPU))
    try:
        for b in (c, corrupt(c, "value", 2), corrupt(c, "proof", 0)):
            x = Inputs(oc, b)
            got = x.call(hip, env["tabled"])
            x.check(got)
            vals = x.values.reshape(b.n, b.l, 4)
            singles = [hip.kzg_verify_multi(env["tabled"], srs2, x.com[0], mont(oc, M.coset_points(b.h[k], b.l)), vals[k], x.proofs[k]) for k in range(b.n)]
            assert [0 if s else 1 for s in singles] == list(got[0])
            ok = hip.kzg_verify_cosets(env["tabled"], x.com, x.tau_l, x.h, x.values, b.l, 1, x.log2l, x.winv, x.linv, x.proofs, mont(oc, b.gamma))[0]
            assert ok == (got[1] == 0) == b.verdict()
    finally:
        srs2.free()


# ---- 5. the resident form, n = 0, refusals ---------------------------------------------------------------------------------------------------------------
def test_dev_form(oc, hip, env):
    c, _, evals = vector(oc, env, 8, 3)
    b = corrupt(c, "proof", 9)
    x = Inputs(oc, b)
    r = b.n
    d = [dev(a) for a in (x.com, x.tau_l, mont(oc, [M.omega(1 << 8)]), evals, x.proofs)]
    d_status, d_lhs = dev(np.full(r, 0xEE, np.uint8)), dev(np.full((r, 8), SENT))
    got = hip.kzg_verify_cosets_each_dev(env["tabled"], d[0], 0, d[1], d[2], 1, d[3], 1, r, 3, x.winv, x.linv, d[4], r, d_status, d_lhs)
    assert got == (1, 9)
    x.check((d_status.cpu().numpy(), got[0], got[1], d_lhs.cpu().numpy().view(np.uint64).reshape(r, 8)))
    got = hip.kzg_verify_cosets_each_dev(env["tabled"], d[0], 0, d[1], d[2], 1, d[3], 1, r, 3, x.winv, x.linv, d[4], r, d_status)
    assert got == (1, 9)


def test_empty_call_and_refusals_write_nothing(oc, hip, env):
    import ctypes as C
    from keaki_amd.hip import _ptr
    c = rows_case(6, 4, 7, 5)
    x = Inputs(oc, c)
    status, lhs = np.full(6, 0xEE, np.uint8), np.full((6, 8), SENT)
    short = hip.srs_g1_upload(env["g1"][:3])

    def raw(srs=env["plain"], com=x.com, com_stride=0, tau=x.tau_l, points=x.h, point_mode=0, values=x.values, strides=(4, 1), log2l=2, winv=x.winv,
            linv=x.linv, proofs=x.proofs, n=6, st=status, want_bad=True, out_l=lhs):
        p = lambda a: None if a is None else _ptr(np.ascontiguousarray(a))
        bad, first = C.c_uint64(77), C.c_uint64(77)
        rc = hip.lib.keaki_hip_kzg_verify_cosets_each(hip.ctx, srs.handle if srs is not None else None, p(com), com_stride, p(tau), p(points), point_mode,
                                                      p(values), strides[0], strides[1], log2l, p(winv), p(linv), p(proofs), n, p(st),
                                                      C.byref(bad) if want_bad else None, C.byref(first), p(out_l))
        return rc, bad.value, first.value

    try:
        bad = [dict(com_stride=2), dict(point_mode=2), dict(srs=None), dict(log2l=11), dict(com=None), dict(tau=None), dict(points=None), dict(values=None),
               dict(winv=None), dict(linv=None), dict(proofs=None), dict(st=None), dict(want_bad=False), dict(strides=(0, 1)), dict(strides=(2, 1)),
               dict(strides=(1 << 47, 1)), dict(n=1 << 31), dict(n=1 << 29)]
        for kw in bad:
            assert raw(**kw) == (BAD_ARG, 77, 77), kw
        assert raw(srs=short) == (TOO_LARGE, 77, 77)
        assert (status == 0xEE).all() and (lhs == SENT).all()
        assert raw(n=0) == (0, 0, 2**64 - 1) and (status == 0xEE).all() and (lhs == SENT).all()
        assert raw() == (0, 0, 2**64 - 1) and not status.any()
        assert np.array_equal(lhs, x.want_l)
    finally:
        short.free()
