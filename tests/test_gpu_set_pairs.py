"""The per-item points of the KZG set check over arbitrary point sets on the GPU (keaki_hip_kzg_set_pairs, _dev, keaki_hip_srs_g2_precompute_sets) against
the big-integer model (tests/set_pairs_model.py). The SRS comes from a KNOWN tau, so A_i = C_i - [I_i(tau)]_1 and Z2_i = [Z_i(tau)]_2 have known discrete
logs: expected points are (integer) x generator from the oracle's scalar multiplication, and nothing expected comes from the library under test -- except
where a test says that two of its routes must agree to the byte, and where the pair is held against keaki_hip_kzg_verify_multi's pair_out_aff.
Every test forces set_rows_wb = coset_rows_wb = 8 (tables of a few MB at most) except the width cases at k <= 3 and one default-plan case."""
import os

import numpy as np
import pytest

import set_pairs_model as P
import verify_sets_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = P.R
BAD_ARG, OOM, TOO_LARGE = -1, -3, -5
TAU = rand_fr_ints(1, 20261022)[0]
SRS_LEN = 66
SENT = np.uint64(0xDEADBEEFDEADBEEF)
TWO_ADICITY_ROOT = pow(5, (R - 1) >> 28, R)  # ark-bn254's 2^28-th root of unity
KS = [1, 2, 3, 5, 8, 9, 17, 64]


def omega(d):
    return pow(TWO_ADICITY_ROOT, (1 << 28) // d, R)


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def g1_of(oc, dls):
    """(integer) x generator, affine; 0 -> (0, 0) written here, not asked of anyone"""
    out = oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU).copy()
    for i, x in enumerate(dls):
        if x % R == 0:
            out[i] = 0
    return out


def g2_of(oc, dls):
    out = oc.g2_mul_batch(oc.generators()[1], mont(oc, dls), threads=NCPU).copy()
    for i, x in enumerate(dls):
        if x % R == 0:
            out[i] = 0
    return out


def dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    t = torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return t


def handles(oc, hip, tau, n):
    pw = [pow(tau, t, R) for t in range(n)]
    return hip.srs_g1_upload(g1_of(oc, pw)), hip.srs_g2_upload(g2_of(oc, pw))


@pytest.fixture(scope="module")
def env(oc, hip):
    s1, s2 = handles(oc, hip, TAU, SRS_LEN)
    e = {"srs1": s1, "srs2": s2}
    yield e
    s1.free()
    s2.free()


@pytest.fixture(autouse=True)
def small_tables(hip):
    hip.set_option("set_rows_wb", 8)
    hip.set_option("coset_rows_wb", 8)
    yield
    for name in ("set_rows_wb", "coset_rows_wb", "coset_rows_route", "coset_rows_min_lanes", "set_rows_min_lanes", "set_each_route"):
        hip.set_option(name, 0)
    hip.debug_set_alloc_limit(0)


def make_case(n, k, seed, shared=False, tau=TAU):
    degree = k + 2
    r = rand_fr_ints(n + n * k + (degree + 1) * (1 if shared else n), seed)
    gammas, zs, rest = r[:n], [r[n + i * k:n + (i + 1) * k] for i in range(n)], r[n + n * k:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(tau, polys, zs, gammas)


class Inputs:
    """a model case as the arrays the ABI takes (rows of k, item_stride = k), with the expected pairs as points"""

    def __init__(self, oc, c):
        self.c, self.n, self.k = c, c.n, c.k
        dl = [P.pair_dl(c, i) for i in range(c.n)]
        pts = g1_of(oc, list(c.com) + list(c.q) + [a for a, _ in dl])
        self.com, self.proofs, self.want_a = pts[:len(c.com)], pts[len(c.com):len(c.com) + c.n], pts[len(c.com) + c.n:]
        self.want_z2 = g2_of(oc, [z for _, z in dl])
        self.points = mont(oc, [v for row in c.z for v in row])
        self.values = mont(oc, [v for row in c.y for v in row])

    def call(self, hip, env, **kw):
        a = dict(com=self.com, points=self.points, values=self.values, item_stride=None, omega=None)
        a.update(env or {})
        a.update(kw)
        return hip.kzg_set_pairs(a["srs1"], a["srs2"], a["com"], a["points"], a["values"], self.k, self.n, item_stride=a["item_stride"], omega=a["omega"])

    def check(self, got, what=""):
        a, z2 = got
        assert a.shape == (self.n, 8) and z2.shape == (self.n, 16), what
        assert np.array_equal(a, self.want_a), what
        assert np.array_equal(z2, self.want_z2), what


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. against the oracle, and against verify_multi ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 9])
@pytest.mark.parametrize("k", KS)
def test_pairs_against_the_oracle(oc, hip, env, k, n):
    x = Inputs(oc, make_case(n, k, 2000 * k + n))
    x.check(x.call(hip, env), "k = %d, n = %d" % (k, n))


@pytest.mark.parametrize("k", [1, 3, 8])
def test_pairs_are_verify_multis_pair_byte_for_byte(oc, hip, env, k):
    n = 8 if k < 8 else 3
    x = Inputs(oc, make_case(n, k, 3100 + k))
    a, z2 = x.call(hip, env)
    for i in range(n):
        ok, pa, pz = hip.kzg_verify_multi(env["srs1"], env["srs2"], x.com[i], x.points[i * k:(i + 1) * k], x.values[i * k:(i + 1) * k], x.proofs[i], want_pair=True)
        assert ok
        assert a[i].tobytes() + z2[i].tobytes() == pa.tobytes() + pz.tobytes(), i
    if k == 1:      # A_i = C_i - y_i g1, Z2_i = [tau]_2 - z_i g2
        c = x.c
        assert np.array_equal(a, g1_of(oc, [(c.com[i] - c.y[i][0]) % R for i in range(n)]))
        assert np.array_equal(z2, g2_of(oc, [(TAU - c.z[i][0]) % R for i in range(n)]))


@pytest.mark.parametrize("k,n", [(3, 63), (3, 64), (3, 65), (64, 3), (64, 4), (64, 5)])
def test_tile_edges_of_the_polynomial_kernel(oc, hip, env, k, n):
    assert n in (256 // M.kp_of(k) - 1, 256 // M.kp_of(k), 256 // M.kp_of(k) + 1)
    x = Inputs(oc, make_case(n, k, 4000 + 10 * k + n, shared=True))
    assert len(x.com) == 1                                            # com_stride 0
    x.check(x.call(hip, env))


# ---- 2. routes, widths and forms agree to the byte -------------------------------------------------------------------------------------------------
def test_both_g1_routes_every_g2_width_and_the_resident_form_agree(oc, hip, env):
    import torch
    k, n = 3, 9
    x = Inputs(oc, make_case(n, k, 5001))
    s1, s2 = handles(oc, hip, TAU, 4)
    own = {"srs1": s1, "srs2": s2}
    try:
        base = x.call(hip, own)
        x.check(base)
        hip.set_option("coset_rows_route", 2)
        assert same(x.call(hip, own), base)
        hip.set_option("coset_rows_route", 0)
        before = hip.memory()["tables"]
        for wb in (10, 13, 8):
            hip.set_option("set_rows_wb", wb)
            assert same(x.call(hip, own), base), wb
        # one table per handle: the last width replaced the others
        assert hip.memory()["tables"] == before
        d_a, d_z = torch.zeros(n * 8, dtype=torch.int64).cuda(), torch.zeros(n * 16, dtype=torch.int64).cuda()
        d = [dev(x.com), dev(x.points), dev(x.values)]
        hip.kzg_set_pairs_dev(s1, s2, d[0], 1, d[1], 0, None, d[2], k, k, n, d_a, d_z)
        hip.synchronize()
        got = (d_a.cpu().numpy().view(np.uint64).reshape(n, 8), d_z.cpu().numpy().view(np.uint64).reshape(n, 16))
        assert same(got, base)
    finally:
        s1.free()
        s2.free()
    for bad in ("set_rows_wb", 9), ("set_rows_wb", 16), ("set_rows_min_lanes", -1), ("set_each_route", 3):
        with pytest.raises(Exception) as e:
            hip.set_option(*bad)
        assert e.value.status == BAD_ARG


def test_the_default_plan_at_small_k_and_a_table_that_grows(oc, hip, env):
    s1, s2 = handles(oc, hip, TAU, 6)
    try:
        hip.set_option("set_rows_wb", 0)
        hip.set_option("coset_rows_wb", 0)
        t0 = hip.memory()["tables"]
        x = Inputs(oc, make_case(5, 2, 5101))
        x.check(x.call(hip, env, srs1=s1, srs2=s2))
        g1_table = P.sr_table_bytes(2, 13) // 2                          # the coset table over kp = 2 points: 64-byte entries
        assert P.sr_wb(2) == 13 and hip.memory()["tables"] - t0 == P.sr_table_bytes(2, 13) + g1_table
        hip.set_option("set_rows_wb", 8)
        hip.set_option("coset_rows_wb", 8)
        hip.srs_g2_precompute_sets(s2, 5)
        t1 = hip.memory()["tables"]
        y = Inputs(oc, make_case(4, 3, 5102))
        y.check(y.call(hip, env, srs1=s1, srs2=s2))                   # k = 3 <= 5: the table serves it
        assert hip.memory()["tables"] - t1 == P.sr_table_bytes(4, 8) // 2 - g1_table      # only the G1 side rebuilt (kp = 4 at 8 bits)
        with pytest.raises(Exception) as e:
            hip.srs_g2_precompute_sets(s2, 6)                            # 7 points needed
        assert e.value.status == TOO_LARGE
    finally:
        s1.free()
        s2.free()


def test_point_modes_one_commitment_and_a_stride_with_a_gap(oc, hip, env):
    k, n, d, stride = 5, 9, 64, 8
    w = omega(d)
    idx = [[(7 * i + 11 * j * j + j) % d for j in range(k)] for i in range(n)]
    assert all(len(set(r)) == k for r in idx)
    r = rand_fr_ints(k + 3, 5201)
    poly = r
    zs = [[pow(w, e, R) for e in row] for row in idx]
    c = M.valid_case(TAU, [poly], zs, [1] * n)
    x = Inputs(oc, c)
    base = x.call(hip, env)
    x.check(base)
    # the same items through domain indices, with a gap of stride - k elements that is never read
    flat_idx = np.full(n * stride, 0x7FFFFFFF, np.uint32)
    vals = np.full((n * stride, 4), SENT, np.uint64)
    pts = np.full((n * stride, 4), SENT, np.uint64)
    for i in range(n):
        flat_idx[i * stride:i * stride + k] = idx[i]
        vals[i * stride:i * stride + k] = x.values[i * k:(i + 1) * k]
        pts[i * stride:i * stride + k] = x.points[i * k:(i + 1) * k]
    assert same(x.call(hip, env, points=flat_idx, values=vals, item_stride=stride, omega=mont(oc, [w])), base)
    assert same(x.call(hip, env, points=pts, values=vals, item_stride=stride), base)


@pytest.mark.parametrize("k,n", [(8, 9), (64, 3), (9, 5)])
def test_slices_forced_to_one_two_and_kp(oc, hip, env, k, n):
    x = Inputs(oc, make_case(n, k, 5300 + k))
    kp = M.kp_of(k)
    for lanes, S in ((1, 1), (2 * n, 2), (1 << 31, min(kp, 64))):
        assert P.sr_slices(n, P.sr_log2kp(k), lanes) == S
        hip.set_option("set_rows_min_lanes", lanes)
        x.check(x.call(hip, env), "S = %d" % S)


def test_a_launch_chunk_edge_by_a_small_allocation_limit(oc, hip, env):
    k, n = 3, 65
    x = Inputs(oc, make_case(n, k, 5400, shared=True))
    base = x.call(hip, env)                                             # tables and small buffers are resident now
    x.check(base)
    hip.trim()
    per_item = P.sr_item_bytes(k, 2, 0, False)
    hip.debug_set_alloc_limit(30000)
    assert n * per_item > 30000 > 33 * per_item * 9 // 8 + 256          # 65 items are refused, 33 fit: chunks of 33 + 32
    assert same(x.call(hip, env), base)
    hip.debug_set_alloc_limit(0)


# ---- 3. the digit edges of the G2 walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wb", [8, 10, 13])
def test_digit_edges_where_the_scalar_is_the_tests(oc, hip, env, wb):
    hip.set_option("set_rows_wb", wb)
    vs = P.edge_scalars(wb)
    n = len(vs)
    # k = 1: Z_0 = -z
    c = M.valid_case(TAU, [rand_fr_ints(4, 5500 + wb)], [[P.point_for_coeff(v)] for v in vs], [1] * n)
    assert [c.Z(i)[0] for i in range(n)] == vs
    x = Inputs(oc, c)
    assert np.array_equal(x.want_z2, g2_of(oc, [(v + TAU) % R for v in vs]))
    x.check(x.call(hip, env), "k = 1")
    # k = 2 with z_1 = 0: Z_1 = -z_0 and Z_0 = 0, the all-zero row (v = 0 would repeat the point 0)
    vs2 = [v for v in vs if v]
    c = M.valid_case(TAU, [rand_fr_ints(5, 5600 + wb)], [[P.point_for_coeff(v), 0] for v in vs2], [1] * len(vs2))
    assert [c.Z(i)[:2] for i in range(len(vs2))] == [[0, v] for v in vs2]
    x = Inputs(oc, c)
    for lanes in (1, 1 << 31):
        hip.set_option("set_rows_min_lanes", lanes)
        x.check(x.call(hip, env), "k = 2")


# ---- 4. the group law's branches, with SRS of known tau ------------------------------------------------------------------------------------------------
def test_tau_one_meets_equal_and_opposite_operands(oc, hip):
    s1, s2 = handles(oc, hip, 1, 4)
    try:
        for wb in (8, 13):
            hip.set_option("set_rows_wb", wb)
            d, pts = P.opposite_pair(wb)
            zs = [pts, [R - 1, 0], [5, 7]]
            c = M.valid_case(1, [rand_fr_ints(5, 5700 + wb)], zs, [1] * 3)
            ev0, _ = P.walk(c.Z(0)[:2], [1, 1, 1], wb)
            ev1, _ = P.walk(c.Z(1)[:2], [1, 1, 1], wb)
            assert P.event_kinds(ev0)["opposite"] == 1 and P.event_kinds(ev1)["equal"] == 1
            x = Inputs(oc, c)
            assert np.array_equal(x.want_z2, g2_of(oc, [(1 << wb) + 1, 2, 24]))      # (1 - z_0)(1 - z_1) each
            for lanes in (1, 1 << 31):
                hip.set_option("set_rows_min_lanes", lanes)
                x.check(x.call(hip, {"srs1": s1, "srs2": s2}), "wb = %d" % wb)
            # k = 1, z = -1: Z_0 = 1, the accumulator g2 meets [tau]_2 = g2 at the top: a doubling
            c = M.valid_case(1, [rand_fr_ints(3, 5800)], [[R - 1], [R - 2]], [1] * 2)
            x = Inputs(oc, c)
            assert np.array_equal(x.want_z2, g2_of(oc, [2, 3]))
            x.check(x.call(hip, {"srs1": s1, "srs2": s2}))
    finally:
        s1.free()
        s2.free()


def test_tau_zero_has_identity_entries_and_tau_in_the_set_gives_identities(oc, hip, env):
    s1, s2 = handles(oc, hip, 0, 5)
    try:
        c = make_case(5, 3, 5900, tau=0)
        x = Inputs(oc, c)
        assert np.array_equal(x.want_z2, g2_of(oc, [c.Z(i)[0] for i in range(5)]))          # every base but g2 is the identity
        x.check(x.call(hip, {"srs1": s1, "srs2": s2}))
    finally:
        s1.free()
        s2.free()
    # tau inside the point set: Z2_i is the identity; with a constant polynomial A_i is too
    r = rand_fr_ints(8, 5901)
    zs = [[TAU, r[0], r[1]], [r[2], TAU, r[3]], [r[4], r[5], r[6]]]
    c = M.valid_case(TAU, [[r[7]]], zs, [1] * 3)
    x = Inputs(oc, c)
    assert not x.want_z2[0].any() and not x.want_z2[1].any() and x.want_z2[2].any() and not x.want_a.any()
    x.check(x.call(hip, env))
    # an identity commitment and zero values are ordinary inputs
    c = M.Case(TAU, 3, [0], zs[2:], [[0, 0, 0]], [0], [1])
    x = Inputs(oc, c)
    assert not x.com.any() and not x.want_a.any()
    x.check(x.call(hip, env))


# ---- 5. empty calls and refusals ----------------------------------------------------------------------------------------------------------------------
def raw_call(hip, env, x, n=None, k=None, com_stride=1, point_mode=0, om=None, stride=None, com=True, pts=True, vals=True, lhs=True, z2=True, srs1=None, srs2=None,
             s1=True, s2=True):
    """the C entry point itself, on sentinel-filled outputs -> (status, outputs untouched)"""
    n = x.n if n is None else n
    k = x.k if k is None else k
    a = np.full((max(x.n, 1), 8), SENT, np.uint64)
    z = np.full((max(x.n, 1), 16), SENT, np.uint64)
    p = lambda arr, on: arr.ctypes.data if on else None
    st = hip.lib.keaki_hip_kzg_set_pairs(hip.ctx, (srs1 or env["srs1"]).handle if s1 else None, (srs2 or env["srs2"]).handle if s2 else None, p(x.com, com),
                                         com_stride, p(x.points, pts), point_mode, om, p(x.values, vals), k if stride is None else stride, k, n, p(a, lhs), p(z, z2))
    return st, bool((a == SENT).all() and (z == SENT).all())


def test_empty_calls_and_every_refusal_write_nothing(oc, hip, env):
    x = Inputs(oc, make_case(4, 3, 6000))
    assert raw_call(hip, env, x, n=0) == (0, True)
    for kw in (dict(com=False), dict(pts=False), dict(vals=False), dict(lhs=False), dict(z2=False), dict(s1=False), dict(s2=False), dict(k=0), dict(k=65),
               dict(stride=2), dict(com_stride=2), dict(point_mode=2), dict(point_mode=1), dict(n=1 << 31), dict(n=1 << 30, k=3), dict(n=3, stride=1 << 47)):
        assert raw_call(hip, env, x, **kw) == (BAD_ARG, True), kw
    s1, s2 = handles(oc, hip, TAU, 3)
    try:
        assert raw_call(hip, env, x, srs2=s2) == (TOO_LARGE, True)          # k + 1 = 4 points of the G2 SRS
        x2 = Inputs(oc, make_case(4, 3, 6000))
        assert raw_call(hip, env, x2, srs1=s1) == (0, False)                  # kp = 4 > len(srs_g1) = 3 >= k: the MSM route
        y = Inputs(oc, make_case(2, 5, 6001))
        assert raw_call(hip, env, y, srs1=s1) == (TOO_LARGE, True)
    finally:
        s1.free()
        s2.free()
    x.check(x.call(hip, env))                                                # the context is still usable


def test_the_short_g1_srs_takes_the_msm_route(oc, hip, env):
    s1, s2 = handles(oc, hip, TAU, 4)
    s1.free()
    s1 = hip.srs_g1_upload(g1_of(oc, [pow(TAU, t, R) for t in range(3)]))
    try:
        x = Inputs(oc, make_case(9, 3, 6100))
        x.check(x.call(hip, env, srs1=s1, srs2=s2))
    finally:
        s1.free()
        s2.free()


def test_a_refused_table_falls_to_the_narrower_width_and_then_to_oom(oc, hip, env):
    s1, s2 = handles(oc, hip, TAU, 3)
    try:
        x = Inputs(oc, make_case(3, 1, 6200))
        base = x.call(hip, env)
        x.check(base)
        x.call(hip, env, srs1=s1, srs2=s2)                                   # the G1 table and the workspaces exist now
        hip.set_option("set_rows_wb", 10)
        t0 = hip.memory()["tables"]
        hip.debug_set_alloc_limit(P.sr_table_bytes(1, 8) + 4096)
        assert P.sr_table_bytes(1, 10) > P.sr_table_bytes(1, 8) + 4096
        assert same(x.call(hip, env, srs1=s1, srs2=s2), base)                # 10 bits refused, 8 bits built: the same points
        assert hip.memory()["tables"] == t0                                  # an 8-bit table replaced an 8-bit table
        hip.set_option("set_rows_wb", 13)
        hip.debug_set_alloc_limit(100000)
        st, untouched = raw_call(hip, env, x, srs1=s1, srs2=s2)
        assert (st, untouched) == (OOM, True)
        assert hip.memory()["tables"] == t0 - P.sr_table_bytes(1, 8)         # the refused rebuild dropped the old table and booked nothing
        hip.debug_set_alloc_limit(0)
        assert same(x.call(hip, env, srs1=s1, srs2=s2), base)                # ... and the context and the handle stay usable
    finally:
        hip.debug_set_alloc_limit(0)
        s1.free()
        s2.free()
