"""FK23 coset openings on the GPU (keaki_hip_open_fk_cosets, _poly, _poly_dev, keaki_hip_srs_g1_precompute_fk_cosets) against the big-integer model
(tests/fk_coset_model.py). The SRS comes from a KNOWN tau, so every proof has a known discrete log: expected points are (integer) x generator from
the oracle's scalar multiplication, expected quotients come from the model's division by x^l - c_i (never from the Toeplitz route, which is what
the kernels compute), and nothing expected comes from the library under test."""
import ctypes as C
import os

import numpy as np
import pytest

import fk_coset_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, OOM, TOO_LARGE = -1, -3, -5
TAU = rand_fr_ints(1, 20261021)[0]
D_MAX = 1024
# l below, equal to and above the group of 4 terms, r = 1 and r = 2, positions unsplit (S = 1) and split over 2 .. 16 lanes
SHAPES = [(0, 0), (3, 0), (3, 3), (4, 1), (6, 2), (6, 5), (8, 3), (10, 4), (10, 10), (10, 6)]
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


def jac_to_aff(j):
    j = np.asarray(j, np.uint64)
    return np.zeros(8, np.uint64) if not j[8:].any() else j[:8].copy()


def roots(oc, log2d, log2l):
    """(omega_2r, 1 / omega_2r, 1 / 2r) in Montgomery limbs"""
    n2 = 2 << (log2d - log2l)
    w = M.omega(n2)
    return tuple(mont(oc, [x])[0] for x in (w, M.inv(w), M.inv(n2)))


def dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_fill(words):
    import torch
    t = torch.from_numpy(np.full(words, SENT).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def env(oc, hip):
    """the powers of tau, uploaded once: a G1 handle with window tables and one without; expectations are computed once per shape"""
    pw = [1]
    for _ in range(D_MAX - 1):
        pw.append(pw[-1] * TAU % R)
    g1 = g1_of(oc, pw)
    plain, tabled = hip.srs_g1_upload(g1), hip.srs_g1_upload(g1)
    hip.srs_g1_precompute(tabled)
    e = {"pw": pw, "g1": g1, "plain": plain, "tabled": tabled, "cache": {}}
    yield e
    for h in (plain, tabled):
        h.free()


def expected(oc, env, log2d, log2l):
    """(coefficients, their Montgomery limbs, the r expected affine proofs) of this shape: long division, then (integer) x G"""
    key = (log2d, log2l)
    if key not in env["cache"]:
        p = rand_fr_ints(1 << log2d, 7000 + 32 * log2d + log2l)
        env["cache"][key] = (p, mont(oc, p), g1_of(oc, M.proofs_direct(p, log2d, log2l, TAU)))
    return env["cache"][key]


# ---- 1. _poly on host and _dev, against long division ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d,log2l", SHAPES)
def test_poly_against_long_division(oc, hip, env, log2d, log2l):
    p, pm, want = expected(oc, env, log2d, log2l)
    r = 1 << (log2d - log2l)
    rt = roots(oc, log2d, log2l)
    if r == 1:
        assert not want.any(), "one coset: the identity"
    seen = []
    for srs in (env["plain"], env["tabled"]):
        got = hip.open_fk_cosets_poly(srs, log2d, log2l, pm, *rt)
        assert np.array_equal(got, want), (log2d, log2l)
        d_c, d_o = dev(pm), dev_fill(8 * r)
        hip.open_fk_cosets_poly_dev(srs, log2d, log2l, d_c.data_ptr(), *rt, d_o.data_ptr())
        hip.synchronize()
        assert np.array_equal(host(d_o).reshape(-1, 8), got), (log2d, log2l)
        seen.append(got)
    assert np.array_equal(seen[0], seen[1]), "with and without window tables: the same bytes"


@pytest.mark.parametrize("log2d,log2l", [(8, 3), (10, 4), (6, 5)])
def test_every_split_and_group_size_gives_the_same_bytes(oc, hip, env, log2d, log2l):
    """both sides of the split threshold and every group size, through the context's options: (fk_coset_group, fk_coset_min_lanes)"""
    p, pm, want = expected(oc, env, log2d, log2l)
    rt = roots(oc, log2d, log2l)
    n2, l = 2 << (log2d - log2l), 1 << log2l
    plans = set()
    try:
        for g, min_lanes in [(0, 0), (0, 1), (0, 2 * n2), (1, 0), (1, 1), (2, 1), (2, 1 << 20), (4, n2)]:
            hip.set_option("fk_coset_group", g)
            hip.set_option("fk_coset_min_lanes", min_lanes)
            plans.add(M.split_plan(n2, l, g, min_lanes))
            assert np.array_equal(hip.open_fk_cosets_poly(env["plain"], log2d, log2l, pm, *rt), want), (g, min_lanes)
    finally:
        hip.set_option("fk_coset_group", 0)
        hip.set_option("fk_coset_min_lanes", 0)
    assert {s for _, s, _ in plans} >= {1, 2} and {g for g, _, _ in plans} == {1, 2, 4}
    from keaki_amd.hip import KeakiHipError
    for name, bad in (("fk_coset_group", 3), ("fk_coset_group", 8), ("fk_coset_group", -1), ("fk_coset_min_lanes", -1), ("fk_coset_min_lanes", (1 << 31) + 1)):
        with pytest.raises(KeakiHipError):
            hip.set_option(name, bad)


# ---- 2. the same bytes as the routes that were there before ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d,log2l", [(8, 3), (6, 2)])
def test_same_bytes_as_open_multi_and_aggregate(oc, hip, env, log2d, log2l):
    p, pm, want = expected(oc, env, log2d, log2l)
    d, l = 1 << log2d, 1 << log2l
    r = d // l
    got = hip.open_fk_cosets_poly(env["tabled"], log2d, log2l, pm, *roots(oc, log2d, log2l))
    wd = M.omega(d)
    singles = hip.open_fk_poly(env["tabled"], log2d, pm, *roots(oc, log2d, 0))
    for i in range(r):
        idx = M.coset_indices(d, l, i)
        zm = mont(oc, [pow(wd, k, R) for k in idx])
        proof, _ = hip.kzg_open_multi(env["tabled"], pm, zm)
        assert np.array_equal(jac_to_aff(proof), got[i]), i
        assert np.array_equal(jac_to_aff(hip.kzg_aggregate(zm, singles[idx])), got[i]), i
    # l = 1: open_fk_poly itself
    assert np.array_equal(hip.open_fk_cosets_poly(env["tabled"], log2d, 0, pm, *roots(oc, log2d, 0)), singles)


# ---- 3. the raw hat_a entry with host-chosen scalars: the branches of the pointwise kernel -----------------------------------------------------------
def _patterns(l, n2):
    """rows of scalars: term j of EVERY position takes pattern[j] (lists of l) -- or a full l x 2r matrix"""
    z = [0] * l
    out = {
        "equal points": [1, 1] + z[2:],
        "cancellation": [1, R - 1] + z[2:],
        "1 + 1 - 2": [1, 1, R - 2] + z[3:],
        "all zero": z,
        "last group only": z[:-1] + [0x1234567890ABCDEF],
        "r - 1 everywhere": [R - 1] * l,
    }
    out = {k: [[v] * n2 for v in pat] for k, pat in out.items()}
    rnd = rand_fr_ints(l * n2, 31 * l + n2)
    out["random"] = [rnd[j * n2:(j + 1) * n2] for j in range(l)]
    return out


@pytest.mark.parametrize("log2d,log2l", [(5, 3), (6, 4)])
def test_raw_entry_with_tau_one(oc, hip, log2d, log2l):
    """tau = 1: the l bases of a lane coincide (every row's transform is the same) and the even positions q != 0 hold the identity"""
    d, l = 1 << log2d, 1 << log2l
    n2 = 2 * d // l
    srs_dl = [1] * d
    hs = M.hat_s_rows(srs_dl, log2d, log2l)
    L2 = n2.bit_length() - 1
    assert all(hs[j] == hs[0] for j in range(l)) and all(hs[0][q] == 0 for q in range(n2) if M.bitrev(q, L2) % 2 == 0 and q) and hs[0][0]
    srs = hip.srs_g1_upload(g1_of(oc, srs_dl))
    w = M.omega(n2)
    rt = (mont(oc, [w])[0], mont(oc, [M.inv(w)])[0])
    try:
        for min_lanes in (0, 1):                            # split over lanes | one lane per position, two or four groups in a row
            hip.set_option("fk_coset_min_lanes", min_lanes)
            for name, ha in _patterns(l, n2).items():
                want = g1_of(oc, M.proofs_from_hat(hs, ha, log2d, log2l))
                got = hip.open_fk_cosets(srs, log2d, log2l, mont(oc, [x for row in ha for x in row]), *rt)
                assert np.array_equal(got, want), (name, min_lanes)
                if name in ("cancellation", "1 + 1 - 2", "all zero"):
                    assert not got.any(), name
    finally:
        hip.set_option("fk_coset_min_lanes", 0)
        srs.free()


@pytest.mark.parametrize("log2d,log2l", [(5, 3), (6, 4)])
def test_raw_entry_with_random_tau(oc, hip, env, log2d, log2l):
    d, l = 1 << log2d, 1 << log2l
    n2 = 2 * d // l
    hs = M.hat_s_rows(env["pw"][:d], log2d, log2l)
    w = M.omega(n2)
    rt = (mont(oc, [w])[0], mont(oc, [M.inv(w)])[0])
    for name, ha in _patterns(l, n2).items():
        want = g1_of(oc, M.proofs_from_hat(hs, ha, log2d, log2l))
        got = hip.open_fk_cosets(env["plain"], log2d, log2l, mont(oc, [x for row in ha for x in row]), *rt)
        assert np.array_equal(got, want), name
    # the hat_a of a polynomial gives the polynomial's proofs
    p, pm, want = expected(oc, env, log2d, log2l)
    ha = M.hat_a_rows(p, log2d, log2l)
    assert np.array_equal(hip.open_fk_cosets(env["plain"], log2d, log2l, mont(oc, [x for row in ha for x in row]), *rt), want)


# ---- 4. whole rows of zero scalars, and an SRS whose transforms are mostly the identity ---------------------------------------------------------------
def test_sparse_polynomial_and_tau_a_root_of_unity(oc, hip, env):
    log2d, log2l = 6, 2
    d, l = 64, 4
    rt = roots(oc, log2d, log2l)
    p = rand_fr_ints(d, 515)
    for m in range(d):
        if m % l in (1, 3) or m >= 40:                      # residues 1 and 3 have no coefficient at all, the top of the others is zero
            p[m] = 0
    want = g1_of(oc, M.proofs_direct(p, log2d, log2l, TAU))
    assert np.array_equal(hip.open_fk_cosets_poly(env["plain"], log2d, log2l, mont(oc, p), *rt), want)
    zero = hip.open_fk_cosets_poly(env["plain"], log2d, log2l, mont(oc, [0] * d), *rt)
    assert not zero.any(), "the zero polynomial: r identities"
    tau = M.omega(2 * d // l)                               # tau^(2r) = 1
    pw = [pow(tau, k, R) for k in range(d)]
    hs = M.hat_s_rows(pw, log2d, log2l)
    assert sum(1 for row in hs for x in row if x == 0) > len(hs) * len(hs[0]) // 4, "many transformed points are the identity"
    srs = hip.srs_g1_upload(g1_of(oc, pw))
    try:
        q = rand_fr_ints(d, 516)
        assert np.array_equal(hip.open_fk_cosets_poly(srs, log2d, log2l, mont(oc, q), *rt), g1_of(oc, M.proofs_direct(q, log2d, log2l, tau)))
    finally:
        srs.free()


# ---- 5. the cache of the handle ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def ctx_tables():
    """an own context (its accounting starts at a known value, its allocation limit is its own) and `tables()` relative to that start"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    base = h.memory()["tables"]
    try:
        yield h, (lambda: h.memory()["tables"] - base)
    finally:
        h.debug_set_alloc_limit(0)
        h.close()


def cache_bytes(log2d):
    return 192 << log2d                                     # 2d Jacobian points of 96 B


def open_shape(oc, h, srs, env, log2d, log2l):
    return h.open_fk_cosets_poly(srs, log2d, log2l, expected(oc, env, log2d, log2l)[1], *roots(oc, log2d, log2l))


def test_cache_rebuilds_precompute_and_the_other_caches(oc, env, ctx_tables):
    h, tables = ctx_tables
    srs, fresh = h.srs_g1_upload(env["g1"]), h.srs_g1_upload(env["g1"])
    log2d, d = 6, 64
    try:
        # the FK23 transform and the vec_update tables first: they must survive everything below
        pm = expected(oc, env, log2d, 2)[1]
        fk = h.open_fk_poly(srs, log2d, pm, *roots(oc, log2d, 0))
        wd = M.omega(d)
        upd_args = (log2d, mont(oc, [wd])[0], mont(oc, [M.inv(wd)])[0], mont(oc, [M.inv(d)])[0], [3, 17], mont(oc, [5, R - 9]))
        _, upd = h.vec_update(srs, *upd_args, None, fk.copy())
        others = tables()
        assert others == 2 * cache_bytes(log2d)             # 2d Jacobian points | 192 B x d of update tables
        a = open_shape(oc, h, srs, env, 6, 2)
        assert np.array_equal(a, expected(oc, env, 6, 2)[2]) and tables() == others + cache_bytes(6)
        assert np.array_equal(open_shape(oc, h, srs, env, 6, 2), a) and tables() == others + cache_bytes(6)
        b = open_shape(oc, h, srs, env, 6, 5)               # another l at the same d: rebuilt, not added
        assert np.array_equal(b, expected(oc, env, 6, 5)[2]) and tables() == others + cache_bytes(6)
        c = open_shape(oc, h, srs, env, 8, 3)               # another d
        assert np.array_equal(c, expected(oc, env, 8, 3)[2]) and tables() == others + cache_bytes(8)
        assert not open_shape(oc, h, srs, env, 3, 3).any() and tables() == others + cache_bytes(8), "r = 1 needs no transform and drops none"
        assert np.array_equal(open_shape(oc, h, srs, env, 6, 2), a) and tables() == others + cache_bytes(6)
        # precompute, then open: the same bytes as open alone
        h.srs_g1_precompute_fk_cosets(fresh, 6, 2, roots(oc, 6, 2)[0])
        assert tables() == others + 2 * cache_bytes(6)
        assert np.array_equal(open_shape(oc, h, fresh, env, 6, 2), a) and tables() == others + 2 * cache_bytes(6)
        h.srs_g1_precompute_fk_cosets(fresh, 6, 2, roots(oc, 6, 2)[0])
        assert tables() == others + 2 * cache_bytes(6)
        # the other two caches are where they were and give their bytes
        assert np.array_equal(h.open_fk_poly(srs, log2d, pm, *roots(oc, log2d, 0)), fk)
        assert np.array_equal(h.vec_update(srs, *upd_args, None, fk.copy())[1], upd)
        assert tables() == others + 2 * cache_bytes(6)
    finally:
        srs.free(); fresh.free()
    assert tables() == 0


def test_refused_cache_build(oc, env, ctx_tables):
    from keaki_amd.hip import _ptr
    h, tables = ctx_tables
    sa, sb = h.srs_g1_upload(env["g1"]), h.srs_g1_upload(env["g1"])
    try:
        a = open_shape(oc, h, sa, env, 6, 2)               # warms every workspace of the call: the rows of handle B are the only allocation left
        assert tables() == cache_bytes(6)
        h.debug_set_alloc_limit(1024)
        out = np.full((16, 8), SENT)
        pm, rt = expected(oc, env, 6, 2)[1], roots(oc, 6, 2)
        st = h.lib.keaki_hip_open_fk_cosets_poly(h.ctx, sb.handle, 6, 2, _ptr(pm), _ptr(rt[0]), _ptr(rt[1]), _ptr(rt[2]), _ptr(out))
        assert st == OOM and b"keaki_hip_debug_set_alloc_limit" in h.lib.keaki_hip_last_error(h.ctx)
        assert (out == SENT).all() and tables() == cache_bytes(6)
        st = h.lib.keaki_hip_srs_g1_precompute_fk_cosets(h.ctx, sb.handle, 6, 2, _ptr(rt[0]))
        assert st == OOM and tables() == cache_bytes(6)
        assert np.array_equal(open_shape(oc, h, sa, env, 6, 2), a), "handle A is untouched"
        h.debug_set_alloc_limit(0)
        assert np.array_equal(open_shape(oc, h, sb, env, 6, 2), a) and tables() == 2 * cache_bytes(6)
    finally:
        sa.free(); sb.free()
    assert tables() == 0


def test_workspace_is_counted_and_trimmed(oc, env, ctx_tables):
    h, _ = ctx_tables
    before = h.memory()["workspaces"]
    a = open_shape(oc, h, env["plain"], env, 8, 3)
    n2, (G, S, _) = 64, M.split_plan(64, 8)
    assert h.memory()["workspaces"] - before >= S * n2 * G * 1024, "G KB of window tables per lane"
    h.trim()
    assert h.memory()["workspaces"] == 0
    assert np.array_equal(open_shape(oc, h, env["plain"], env, 8, 3), a)


# ---- 6. errors: nothing is written and the context stays usable -----------------------------------------------------------------------------------------
def test_errors_write_nothing(oc, hip, env):
    from keaki_amd.hip import _ptr
    lib, ctx = hip.lib, hip.ctx
    p, pm, want = expected(oc, env, 6, 2)
    rt = roots(oc, 6, 2)
    w, wi, s = (_ptr(x) for x in rt)
    ha = mont(oc, [x for row in M.hat_a_rows(p, 6, 2) for x in row])
    big = np.zeros((1 << 12, 4), np.uint64)
    out = np.full((D_MAX, 8), SENT)
    d_c, d_o = dev(pm), dev_fill(8 * 16)
    srs, o = env["plain"].handle, _ptr(out)
    short = hip.srs_g1_upload(env["g1"][:50])
    calls = [
        ("poly null srs", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, None, 6, 2, _ptr(pm), w, wi, s, o)),
        ("poly null coeffs", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 2, None, w, wi, s, o)),
        ("poly null omega", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 2, _ptr(pm), None, wi, s, o)),
        ("poly null omega_inv", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 2, _ptr(pm), w, None, s, o)),
        ("poly null inv_2r", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 2, _ptr(pm), w, wi, None, o)),
        ("poly null out", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 2, _ptr(pm), w, wi, s, None)),
        ("poly log2l > log2d", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 6, 7, _ptr(pm), w, wi, s, o)),
        ("poly log2d > 27", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 28, 2, _ptr(pm), w, wi, s, o)),
        ("poly l > KEAKI_SET_MAX", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 12, 11, _ptr(big), w, wi, s, o)),
        ("poly short SRS", TOO_LARGE, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, short.handle, 6, 2, _ptr(pm), w, wi, s, o)),
        ("poly d > len(srs)", TOO_LARGE, lambda: lib.keaki_hip_open_fk_cosets_poly(ctx, srs, 12, 10, _ptr(big), w, wi, s, o)),
        ("raw null hat_a", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets(ctx, srs, 6, 2, None, w, wi, o)),
        ("raw null omega", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets(ctx, srs, 6, 2, _ptr(ha), None, wi, o)),
        ("raw null out", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets(ctx, srs, 6, 2, _ptr(ha), w, wi, None)),
        ("raw log2l > log2d", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets(ctx, srs, 2, 3, _ptr(ha), w, wi, o)),
        ("raw short SRS", TOO_LARGE, lambda: lib.keaki_hip_open_fk_cosets(ctx, short.handle, 6, 2, _ptr(ha), w, wi, o)),
        ("dev null coeffs", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly_dev(ctx, srs, 6, 2, None, w, wi, s, C.c_void_p(d_o.data_ptr()))),
        ("dev null out", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly_dev(ctx, srs, 6, 2, C.c_void_p(d_c.data_ptr()), w, wi, s, None)),
        ("dev unaligned out", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly_dev(ctx, srs, 6, 2, C.c_void_p(d_c.data_ptr()), w, wi, s, C.c_void_p(d_o.data_ptr() + 8))),
        ("dev l > KEAKI_SET_MAX", BAD_ARG, lambda: lib.keaki_hip_open_fk_cosets_poly_dev(ctx, srs, 11, 11, C.c_void_p(d_c.data_ptr()), w, wi, s, C.c_void_p(d_o.data_ptr()))),
        ("dev short SRS", TOO_LARGE, lambda: lib.keaki_hip_open_fk_cosets_poly_dev(ctx, short.handle, 6, 2, C.c_void_p(d_c.data_ptr()), w, wi, s, C.c_void_p(d_o.data_ptr()))),
        ("precompute null omega", BAD_ARG, lambda: lib.keaki_hip_srs_g1_precompute_fk_cosets(ctx, srs, 6, 2, None)),
        ("precompute log2l > log2d", BAD_ARG, lambda: lib.keaki_hip_srs_g1_precompute_fk_cosets(ctx, srs, 6, 7, w)),
        ("precompute short SRS", TOO_LARGE, lambda: lib.keaki_hip_srs_g1_precompute_fk_cosets(ctx, short.handle, 6, 2, w)),
    ]
    try:
        for what, code, call in calls:
            assert call() == code, what
            assert lib.keaki_hip_last_error(ctx), what
        hip.synchronize()
        assert (out == SENT).all() and (host(d_o) == SENT).all()
    finally:
        short.free()
    assert np.array_equal(hip.open_fk_cosets_poly(env["plain"], 6, 2, pm, *rt), want), "the context is still usable"


# ---- 7. a coset proof is an ordinary set proof --------------------------------------------------------------------------------------------------------
def test_every_coset_proof_verifies_as_a_set_proof(oc, hip, env):
    log2d, log2l = 8, 3
    d, l = 256, 8
    r = d // l
    p, pm, _ = expected(oc, env, log2d, log2l)
    proofs = hip.open_fk_cosets_poly(env["tabled"], log2d, log2l, pm, *roots(oc, log2d, log2l))
    srs2 = hip.srs_g2_upload(oc.g2_mul_batch(oc.generators()[1], mont(oc, env["pw"][:l + 1]), threads=NCPU))
    com = g1_of(oc, [M.poly_eval(p, TAU)])[0]
    wd = M.omega(d)
    try:
        sets = []
        for i in range(r):
            zs = [pow(wd, k, R) for k in M.coset_indices(d, l, i)]
            sets.append((mont(oc, zs), mont(oc, [M.poly_eval(p, z) for z in zs])))
        for i in range(r):
            assert hip.kzg_verify_multi(env["tabled"], srs2, com, sets[i][0], sets[i][1], proofs[i]), i
        for i in (0, 7, r - 1):
            nb = (i + 1) % r
            assert not hip.kzg_verify_multi(env["tabled"], srs2, com, sets[i][0], sets[nb][1], proofs[i]), "the neighbouring coset's values"
            assert not hip.kzg_verify_multi(env["tabled"], srs2, com, sets[nb][0], sets[nb][1], proofs[i]), "the neighbouring coset's proof"
    finally:
        srs2.free()
