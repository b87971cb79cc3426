"""The per-item points of the KZG coset check on the GPU (keaki_hip_kzg_coset_pairs, _dev, keaki_hip_srs_g1_precompute_cosets) against the
big-integer model (tests/coset_pairs_model.py on tests/coset_verify_model.py). The SRS comes from a KNOWN tau, so every expected point is
(integer) x generator from the oracle's scalar multiplication and every expected c_k an integer power; nothing expected comes from the library
under test. tests/test_coset_pairs_model.py shows on the CPU that the structured rows below meet the digit cases and branches they are named for."""
import os

import numpy as np
import pytest

import coset_pairs_model as P
import coset_verify_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, OOM, TOO_LARGE = -1, -3, -5
TAU = rand_fr_ints(1, 20261021)[0]
SRS_LEN = 1024
SHAPES = [(4, 1), (6, 2), (6, 6), (8, 3), (10, 4), (11, 10), (5, 0)]      # (log2d, log2l): r = 1 at (6, 6); l = KEAKI_SET_MAX, n = 2 at (11, 10)
SENT = np.uint64(0xDEADBEEFDEADBEEF)


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def g1_of(oc, dls):
    """(integer) x generator, affine; 0 -> (0, 0) written here, not asked of anyone"""
    out = oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU).copy()
    for i, x in enumerate(dls):
        if x % R == 0:
            out[i] = 0
    return out


def dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def srs_points(oc, zero_at=None):
    pw = [1]
    for _ in range(SRS_LEN - 1):
        pw.append(pw[-1] * TAU % R)
    if zero_at is not None:
        pw[zero_at] = 0
    return g1_of(oc, pw)


@pytest.fixture(scope="module")
def env(oc, hip):
    g1 = srs_points(oc)
    plain, tabled, pre = hip.srs_g1_upload(g1), hip.srs_g1_upload(g1), hip.srs_g1_upload(g1)
    hip.srs_g1_precompute(tabled)
    e = {"g1": g1, "plain": plain, "tabled": tabled, "pre": pre, "cache": {}}
    yield e
    hip.set_option("coset_rows_route", 0)
    hip.set_option("coset_rows_min_lanes", 0)
    hip.set_option("coset_rows_wb", 0)
    hip.debug_set_alloc_limit(0)
    for h in (plain, tabled, pre):
        h.free()


class Inputs:
    """a model case as the arrays the ABI takes (rows layout), with the expected A_k and c_k"""

    def __init__(self, oc, c):
        self.c, self.n, self.l, self.log2l = c, c.n, c.l, c.l.bit_length() - 1
        pairs = [P.pair_dl(c, k) for k in range(c.n)]
        pts = g1_of(oc, list(c.com) + [a for a, _ in pairs])
        self.com, self.want_a = pts[:len(c.com)], pts[len(c.com):]
        self.want_c = mont(oc, [ck for _, ck in pairs])
        self.h = mont(oc, c.h)
        self.values = mont(oc, [v for row in c.y for v in row])
        w = M.omega(c.l)
        self.winv, self.linv = mont(oc, [M.inv(w)])[0], mont(oc, [M.inv(c.l)])[0]

    def call(self, hip, srs, **kw):
        a = dict(com=self.com, points=self.h, values=self.values, strides=(self.l, 1), point_mode=0)
        a.update(kw)
        return hip.kzg_coset_pairs(srs, a["com"], a["points"], a["values"], a["strides"][0], a["strides"][1], self.log2l, self.winv, self.linv, self.n,
                                   point_mode=a["point_mode"])

    def check(self, got, what=""):
        A, cs = got
        assert np.array_equal(cs, self.want_c), what
        bad = [k for k in range(self.n) if not np.array_equal(A[k], self.want_a[k])]
        assert not bad, (what, bad[:8])


def routes(hip, x, srs, what, **kw):
    """route 1 == route 2 == model"""
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


# ---- 1. all cosets of a vector: layouts, point modes, commitment strides, handles, routes ----------------------------------------------------------
@pytest.mark.parametrize("log2d,log2l", SHAPES)
def test_all_cosets_of_a_vector(oc, hip, env, log2d, log2l):
    c, x, evals = vector(oc, env, log2d, log2l)
    r = c.n
    omega_d = mont(oc, [M.omega(1 << log2d)])
    hip.srs_g1_precompute_cosets(env["pre"], log2l)
    for name in ("plain", "tabled", "pre"):
        srs = env[name]
        routes(hip, x, srs, (name, "rows"))
        routes(hip, x, srs, (name, "rows, omega"), point_mode=1, points=omega_d)
        routes(hip, x, srs, (name, "domain order"), values=evals, strides=(1, r))
        routes(hip, x, srs, (name, "domain order, omega"), values=evals, strides=(1, r), point_mode=1, points=omega_d)
        routes(hip, x, srs, (name, "n commitments"), com=np.repeat(x.com, r, axis=0))


def test_pairs_are_the_pair_points_of_verify_multi(oc, hip, env):
    """lhs_out_aff[k] followed by [tau^l]_2 - c_k g2 is pair_out_aff of keaki_hip_kzg_verify_multi on the l points of coset k"""
    c, x, _ = vector(oc, env, 6, 2)
    pw = [1]
    for _ in range(c.l):
        pw.append(pw[-1] * TAU % R)
    srs2 = hip.srs_g2_upload(oc.g2_mul_batch(oc.generators()[1], mont(oc, pw), threads=NCPU))
    try:
        A, cs = x.call(hip, env["tabled"])
        x.check((A, cs))
        proofs = g1_of(oc, c.q)
        vals = x.values.reshape(c.n, c.l, 4)
        for k in (0, 7, c.n - 1):
            ok, a_multi, z_multi = hip.kzg_verify_multi(env["tabled"], srs2, x.com[0], mont(oc, M.coset_points(c.h[k], c.l)), vals[k], proofs[k], want_pair=True)
            assert ok and np.array_equal(a_multi, A[k])
            z_want = oc.g2_mul_batch(oc.generators()[1], mont(oc, [pow(TAU, c.l, R) - pow(c.h[k], c.l, R)]), threads=1)[0]
            assert np.array_equal(z_multi, z_want)
            assert np.array_equal(cs[k], mont(oc, [pow(c.h[k], c.l, R)])[0])
    finally:
        srs2.free()


# ---- 2. item counts at the edges of the transform tile, of the batched inversions and of the launch chunk --------------------------------------------
@pytest.mark.parametrize("n,l", [(1, 16), (M.tile_items(16) + 1, 16), (17, 2), (9, 1), (7, 8)])
def test_item_counts(oc, hip, env, n, l):
    """n = 1; one LDS tile of the transform + 1 (65 items at l = 16); 17 = one Fermat chunk + 1 and two lanes + 1 of the affine kernel's 8 items per
    inversion; 9 and 7 = one such lane + 1 and - 1. Separate commitments, so that a wrong item index shows."""
    c = rows_case(n, l, l + 3, 300 + n, shared=False)
    x = Inputs(oc, c)
    routes(hip, x, env["pre"], (n, l))
    try:
        for lanes in (1, 1 << 20):                                         # one slice per item | as many slices as l and the wave allow
            hip.set_option("coset_rows_min_lanes", lanes)
            x.check(x.call(hip, env["plain"]), (n, l, lanes))
    finally:
        hip.set_option("coset_rows_min_lanes", 0)


def test_ragged_last_launch_chunk(oc, hip, env):
    """a small chunk forced through the allocation limit, not by a big n: 37 items of l = 16 in the resident form (which reserves nothing but the
    kernels' workspace: 32 B per item for 1 / h and 640 B per item of a chunk) under a limit of 20,000 B. 37 items (24,960 B) are refused, the halved chunk of
    19 (13,440 B) fits: launches of 19 and 18 items. The table is built before the limit is set."""
    n, l = 37, 16
    c = rows_case(n, l, 20, 808, shared=False)
    x = Inputs(oc, c)
    hip.srs_g1_precompute_cosets(env["pre"], 4)
    d = [dev(a) for a in (x.com, x.h, x.values)]
    d_a, d_c = dev(np.full((n, 8), SENT)), dev(np.full((n, 4), SENT))
    hip.synchronize()
    hip.trim()
    try:
        hip.debug_set_alloc_limit(20000)
        hip.kzg_coset_pairs_dev(env["pre"], d[0], 1, d[1], 0, d[2], l, 1, 4, x.winv, x.linv, n, d_a, d_c)
        hip.synchronize()
        work = hip.memory()["workspaces"]
        assert 13440 <= work <= 20000, work
    finally:
        hip.debug_set_alloc_limit(0)
    x.check((d_a.cpu().numpy().view(np.uint64), d_c.cpu().numpy().view(np.uint64)), "chunks of 19 and 18")
    x.check(x.call(hip, env["pre"]), "one chunk again")


# ---- 3. digit families and branch families from chosen coefficients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("log2l", [1, 7, 10])                              # 13-, 10- and 8-bit tables
@pytest.mark.parametrize("family", ["zero", "half", "half_plus_1", "carry_to_top", "r_minus_1", "one_base"])
def test_digit_families(oc, hip, env, log2l, family):
    l, wb = 1 << log2l, P.cr_wb(log2l)
    h, com, seed_v = rand_fr_ints(3, 60 + log2l)
    rows = P.digit_family(family, wb, l, seed_v)
    c = P.case_from_rows(TAU, com, h, rows)
    x = Inputs(oc, c)
    if family == "zero":
        assert np.array_equal(x.want_a[0], x.com[0])                        # A = C
    routes(hip, x, env["pre"], (family, l))
    try:
        hip.set_option("coset_rows_min_lanes", 1)                           # the whole row in one lane
        x.check(x.call(hip, env["plain"]), (family, l, "one slice"))
    finally:
        hip.set_option("coset_rows_min_lanes", 0)


@pytest.mark.parametrize("family,min_lanes", [("double_mid_walk", 1), ("identity_mid_walk", 1), ("slices_equal", 4), ("slices_opposite", 4)])
def test_branch_families(oc, hip, env, family, min_lanes):
    """l = 2, one item: with coset_rows_min_lanes = 1 the lane walks both bases (S = 1), with 4 each base has its lane (S = 2)"""
    wb = P.cr_wb(1)
    h, com = rand_fr_ints(2, 91)
    rows = P.branch_family(family, TAU, wb)
    assert P.cr_slices(1, 1, min_lanes) == (1 if min_lanes == 1 else 2)
    c = P.case_from_rows(TAU, com, h, rows)
    x = Inputs(oc, c)
    if family == "slices_opposite":
        assert np.array_equal(x.want_a[0], x.com[0])                        # the rows sum to the identity
    try:
        hip.set_option("coset_rows_min_lanes", min_lanes)
        routes(hip, x, env["pre"], family)
    finally:
        hip.set_option("coset_rows_min_lanes", 0)


@pytest.mark.parametrize("wb", [8, 10, 13])
def test_every_table_width_at_one_l(oc, hip, env, wb):
    """"coset_rows_wb" runs any of the three widths at any l (the switch of the width sweep): l = 4, every digit family in one call"""
    l = 4
    r = rand_fr_ints(2 + 6, 70 + wb)
    names = ["zero", "half", "half_plus_1", "carry_to_top", "r_minus_1", "one_base"]
    rows = [P.digit_family(f, wb, l, r[-1]) for f in names]
    c = M.Case(TAU, l, [r[0]], r[1:7], [P.values_from_coeffs(r[1 + k], P.neg_rows_to_coeffs(rows[k])) for k in range(6)], [0] * 6, [1] * 6)
    x = Inputs(oc, c)
    try:
        hip.set_option("coset_rows_wb", wb)
        for lanes in (1, 0):
            hip.set_option("coset_rows_min_lanes", lanes)
            x.check(x.call(hip, env["plain"]), (wb, lanes))
        from keaki_amd.hip import KeakiHipError
        with pytest.raises(KeakiHipError):
            hip.set_option("coset_rows_wb", 9)
    finally:
        hip.set_option("coset_rows_wb", 0)
        hip.set_option("coset_rows_min_lanes", 0)


# ---- 4. degenerate points --------------------------------------------------------------------------------------------------------------------------------
def test_identity_results_and_identity_commitments(oc, hip, env):
    l = 4
    r = rand_fr_ints(3 * (l + 1), 17)
    items = []
    for k in range(3):
        h, a = r[k * (l + 1)], r[k * (l + 1) + 1:(k + 1) * (l + 1)]
        i_tau = sum(aj * pow(TAU, j, R) for j, aj in enumerate(a)) % R
        items.append((h, a, i_tau))
    # item 0: C = [I(tau)]_1, so A is the identity; item 1: C the identity, A = -[I(tau)]_1; item 2: ordinary
    com = [items[0][2], 0, 777]
    c = M.Case(TAU, l, com, [h for h, _, _ in items], [P.values_from_coeffs(h, a) for h, a, _ in items], [0, 0, 0], [1, 1, 1])
    x = Inputs(oc, c)
    assert not x.want_a[0].any() and not x.com[1].any() and x.want_a[1].any()
    routes(hip, x, env["pre"], "identities")
    try:
        hip.set_option("coset_rows_min_lanes", 1)
        routes(hip, x, env["plain"], "identities, one slice")
    finally:
        hip.set_option("coset_rows_min_lanes", 0)


def test_srs_with_an_identity_point(oc, hip, env):
    """a handle whose point 1 is (0,0): its table entries are identities and are skipped, the term a_1 [tau]_1 drops out of I(tau)"""
    g1 = env["g1"].copy()
    g1[1] = 0
    srs = hip.srs_g1_upload(g1)
    try:
        c = rows_case(5, 4, 9, 23, shared=False)
        x = Inputs(oc, c)
        dls = [(P.com_of(c, k) - sum(aj * pow(TAU, j, R) for j, aj in enumerate(c.a(k)) if j != 1)) % R for k in range(c.n)]
        x.want_a = g1_of(oc, dls)
        routes(hip, x, srs, "identity SRS point")
    finally:
        srs.free()


# ---- 5. refusals: nothing written --------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(oc, hip, env):
    import ctypes as C
    from keaki_amd.hip import KeakiHipError, _ptr
    c = rows_case(6, 4, 7, 5)
    x = Inputs(oc, c)
    lhs, cs = np.full((6, 8), SENT), np.full((6, 4), SENT)
    short = hip.srs_g1_upload(env["g1"][:3])

    def raw(srs=env["plain"], com=x.com, com_stride=0, points=x.h, point_mode=0, values=x.values, strides=(4, 1), log2l=2, winv=x.winv, linv=x.linv, n=6,
            out_a=lhs, out_c=cs):
        p = lambda a: None if a is None else _ptr(np.ascontiguousarray(a))
        return hip.lib.keaki_hip_kzg_coset_pairs(hip.ctx, srs.handle if srs is not None else None, p(com), com_stride, p(points), point_mode, p(values),
                                                 strides[0], strides[1], log2l, p(winv), p(linv), n, p(out_a), p(out_c))

    try:
        bad = [dict(com_stride=2), dict(point_mode=2), dict(point_mode=-1), dict(srs=None), dict(log2l=11), dict(log2l=32), dict(com=None), dict(points=None),
               dict(values=None), dict(winv=None), dict(linv=None), dict(out_a=None), dict(out_c=None), dict(strides=(0, 1)), dict(strides=(4, 0)),
               dict(strides=(2, 1)), dict(strides=(1, 3)), dict(strides=(1 << 47, 1)), dict(strides=(4, 1 << 47)), dict(n=1 << 31), dict(n=1 << 29)]
        for kw in bad:
            assert raw(**kw) == BAD_ARG, kw
        assert raw(srs=short) == TOO_LARGE
        assert (lhs == SENT).all() and (cs == SENT).all()
        assert raw(n=0) == 0 and (lhs == SENT).all() and (cs == SENT).all()
        assert raw() == 0
        x.check((lhs, cs))
        for name, v in (("coset_rows_route", 3), ("coset_rows_route", -1), ("coset_rows_min_lanes", -1), ("coset_rows_min_lanes", (1 << 31) + 1)):
            with pytest.raises(KeakiHipError):
                hip.set_option(name, v)
        with pytest.raises(KeakiHipError):
            hip.srs_g1_precompute_cosets(short, 2)
        with pytest.raises(KeakiHipError):
            hip.srs_g1_precompute_cosets(env["plain"], 11)
    finally:
        short.free()


# ---- 6. the table is optional memory ------------------------------------------------------------------------------------------------------------------------
def test_refused_table_falls_back_to_the_msm_route(oc, hip, env):
    """with the allocation limit below the table's size the call runs route 2 and gives the same bytes; the handle's FK23 cache and the byte counts
    of the context are what they were"""
    log2l = 3
    c = rows_case(11, 1 << log2l, 12, 41, shared=False)
    x = Inputs(oc, c)
    srs = hip.srs_g1_upload(env["g1"])
    try:
        hip.srs_g1_precompute_fk(srs, 4, mont(oc, [M.omega(32)])[0])
        before = hip.memory()["tables"]
        hip.debug_set_alloc_limit(P.cr_table_bytes(log2l, P.cr_wb(log2l)) - 1)
        x.check(x.call(hip, srs), "table refused")
        assert hip.memory()["tables"] == before
        hip.debug_set_alloc_limit(0)
        x.check(x.call(hip, srs), "table built")
        assert hip.memory()["tables"] == before + P.cr_table_bytes(log2l, P.cr_wb(log2l))
        hip.srs_g1_precompute_cosets(srs, log2l)                             # there already: nothing changes
        assert hip.memory()["tables"] == before + P.cr_table_bytes(log2l, P.cr_wb(log2l))
        hip.srs_g1_precompute_cosets(srs, 1)                                 # another l replaces it and evicts no other cache
        assert hip.memory()["tables"] == before + P.cr_table_bytes(1, P.cr_wb(1))
    finally:
        hip.debug_set_alloc_limit(0)
        srs.free()
    assert hip.memory()["tables"] == before - ((2 << 4) * 96)                # the handle's FK23 transform and coset table are gone with it


# ---- 7. the resident form, queued behind a producer ------------------------------------------------------------------------------------------------------
def test_dev_form_runs_behind_a_producer_on_the_context_stream(oc, hip, env):
    """a context on a caller-created stream: the values are produced on that stream (a device copy from a staging tensor) right before the call and
    the outputs copied away right behind it, with ONE synchronisation at the end: the call orders itself by the stream alone"""
    import torch
    from keaki_amd.hip import KeakiHip
    c, x, evals = vector(oc, env, 8, 3)
    r = c.n
    hip.srs_g1_precompute_cosets(env["pre"], 3)
    hip.synchronize()                                                        # the table is complete before another context's stream reads it
    stream = torch.cuda.Stream()
    h = KeakiHip(0, stream=stream.cuda_stream)
    try:
        staging, d_vals = dev(evals), dev(np.zeros_like(evals))
        d_com, d_omega = dev(x.com), dev(mont(oc, [M.omega(1 << 8)]))
        d_a, d_c = dev(np.full((r, 8), SENT)), dev(np.full((r, 4), SENT))
        with torch.cuda.stream(stream):
            d_vals.copy_(staging)                                            # the producer
            h.kzg_coset_pairs_dev(env["pre"], d_com, 0, d_omega, 1, d_vals, 1, r, 3, x.winv, x.linv, r, d_a, d_c)
            d_vals.zero_()                                                   # the input overwritten right behind the call
            out_a, out_c = d_a.clone(), d_c.clone()
        stream.synchronize()
        x.check((out_a.cpu().numpy().view(np.uint64), out_c.cpu().numpy().view(np.uint64)))
    finally:
        h.close()
