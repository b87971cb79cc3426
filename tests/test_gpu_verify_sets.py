"""KZG set batch verification on the GPU (keaki_hip_kzg_verify_sets, _dev) against the big-integer model (tests/verify_sets_model.py). The SRS
comes from a KNOWN tau, so every commitment, proof and sum has a known discrete log: expected points are (integer) x generator from the oracle's
scalar multiplication or the oracle's MSM of the model's scalar rows, expected proofs come from long division by Z (kzg_set_model), and nothing
expected comes from the library under test. tests/test_verify_sets_model.py shows on the CPU that every corruption used here breaks the equation."""
import ctypes as C
import os

import numpy as np
import pytest

import kzg_set_model as KM
import verify_sets_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, OOM, TOO_LARGE = -1, -3, -5
TAU = rand_fr_ints(1, 20261021)[0]
SRS_LEN = 80                                 # more than KEAKI_VERIFY_SETS_K_MAX points on both sides
N_BATCH_MAX = 16384                          # csrc/internal.h: rows of the batched MSM
SENT = np.uint64(0xDEADBEEFDEADBEEF)
TWO_ADICITY_ROOT = pow(5, (R - 1) >> 28, R)  # ark-bn254's 2^28-th root of unity


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


def dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    t = torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def env(oc, hip):
    pw = [1]
    for _ in range(SRS_LEN - 1):
        pw.append(pw[-1] * TAU % R)
    g1 = g1_of(oc, pw)
    g2 = oc.g2_mul_batch(oc.generators()[1], mont(oc, pw), threads=NCPU)
    plain, tabled, srs2 = hip.srs_g1_upload(g1), hip.srs_g1_upload(g1), hip.srs_g2_upload(g2)
    hip.srs_g1_precompute(tabled)
    e = {"g1": g1, "g2": g2, "plain": plain, "tabled": tabled, "srs2": srs2}
    yield e
    for h in (plain, tabled, srs2):
        h.free()


class Inputs:
    """a model case as the arrays the ABI takes (rows of k, item_stride = k), with the expected sums as points"""

    def __init__(self, oc, c, want=True):
        self.c, self.n, self.k = c, c.n, c.k
        pts = g1_of(oc, list(c.com) + list(c.q) + (list(c.sums()) if want else []))
        self.com, self.proofs = pts[:len(c.com)], pts[len(c.com):len(c.com) + c.n]
        self.want = pts[len(c.com) + c.n:] if want else None
        self.gamma = mont(oc, c.gamma)
        self.points = mont(oc, [v for row in c.z for v in row])
        self.values = mont(oc, [v for row in c.y for v in row])

    def call(self, hip, env, srs="tabled", **kw):
        a = dict(com=self.com, points=self.points, values=self.values, proofs=self.proofs, gammas=self.gamma, item_stride=None, omega=None)
        a.update(kw)
        return hip.kzg_verify_sets(env[srs], env["srs2"], a["com"], a["points"], a["values"], self.k, a["proofs"], a["gammas"], item_stride=a["item_stride"],
                                   omega=a["omega"])

    def check(self, got, what=""):
        ok, sums = got
        assert ok == self.c.verdict(), what
        assert sums.shape == (self.k + 1, 8) and np.array_equal(sums, self.want), what


def make_case(n, k, seed, shared=False, degree=None):
    degree = k + 2 if degree is None else degree
    r = rand_fr_ints(n + n * k + (degree + 1) * (1 if shared else n), seed)
    gammas, zs, rest = r[:n], [r[n + i * k:n + (i + 1) * k] for i in range(n)], r[n + n * k:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(TAU, polys, zs, gammas)


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 17, 64])
def test_sums_and_verdict_against_the_oracle(oc, hip, env, k, n):
    c = make_case(n, k, 1000 * k + n)
    x = Inputs(oc, c)
    assert c.verdict()
    got = x.call(hip, env)
    x.check(got, "valid")
    assert got[0]
    # R_t is the oracle's MSM of the model's scalar row t over the proofs; L adds the commitment and the interpolant terms
    rows = c.rows()
    if all(c.q):
        for t in range(1, k + 1):
            assert np.array_equal(got[1][t], oc.msm_g1(x.proofs, mont(oc, rows[t]), threads=NCPU)), t
    assert same(x.call(hip, env, srs="plain"), got)
    rnd = rand_fr_ints(3, 77 * k + n)
    for what in ("value", "point", "proof"):
        b = c.copy()
        i, j = rnd[0] % n, rnd[1] % k
        if what == "value":
            b.y[i][j] = (b.y[i][j] + 1) % R
        elif what == "point":
            b.z[i][j] = (b.z[i][j] + 1) % R
        else:
            b.q[i] = (b.q[i] + 1) % R
        xb = Inputs(oc, b)
        bad = xb.call(hip, env)
        assert not b.verdict() and not bad[0], what
        xb.check(bad, what)


# ---- 2. the verdict is the AND of verify_multi -----------------------------------------------------------------------------------------------------
def test_verdict_is_the_and_of_verify_multi_per_item(oc, hip, env):
    c = make_case(4, 3, 4242)
    for corrupt in (None, 2):
        b = c.copy()
        if corrupt is not None:
            b.y[corrupt][1] = (b.y[corrupt][1] + 1) % R
        x = Inputs(oc, b)
        singles = [hip.kzg_verify_multi(env["tabled"], env["srs2"], x.com[i], x.points[3 * i:3 * i + 3], x.values[3 * i:3 * i + 3], x.proofs[i]) for i in range(4)]
        assert singles == [b.single(i) for i in range(4)]
        ok, _ = x.call(hip, env)
        assert ok == all(singles) == b.verdict()


# ---- 3. k = 1 is verify_batch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_k_1_gives_the_bytes_of_verify_batch(oc, hip, env, shared):
    n, d = 37, 64
    w = omega(d)
    r = rand_fr_ints(n + 10 * n, 31 + shared)
    polys = [r[n + 10 * i:n + 10 * i + 10] for i in range(1 if shared else n)]
    tau_g2 = env["g2"][1]
    for point_mode in (0, 1):
        zs = [[pow(w, i, R)] for i in range(n)] if point_mode else [[v] for v in rand_fr_ints(n, 33)]
        c = M.valid_case(TAU, polys, zs, r[:n])
        c.y[4][0] = (c.y[4][0] + 1) % R if point_mode else c.y[4][0]              # an invalid batch too: the equality is one of sums
        x = Inputs(oc, c)
        if point_mode:
            om = mont(oc, [w])
            got = x.call(hip, env, points=np.arange(n, dtype=np.uint32), omega=om[0])
            vb = hip.kzg_verify_batch(x.com, tau_g2, om, x.values, x.proofs, x.gamma, point_mode=1)
        else:
            got = x.call(hip, env)
            vb = hip.kzg_verify_batch(x.com, tau_g2, x.points, x.values, x.proofs, x.gamma)
        x.check(got, point_mode)
        assert vb[0] == got[0] == (not point_mode)
        assert np.array_equal(vb[1], got[1][0]) and np.array_equal(vb[2], got[1][1])


# ---- 4. the tile edges of the polynomial kernel and the chunk edges of the batched inversion ----------------------------------------------------------
@pytest.mark.parametrize("k", [3, 64])
def test_tile_edges_and_workgroup_counts(oc, hip, env, k):
    """k = 3: kp = 4, T = 64 items a tile; k = 64: T = 4. n = 2 T + 1 is three tiles: with "verify_sets_blocks" = 1 one workgroup runs them all and keeps
    its sums in registers between them, with 2 the workgroups run two and one. Every grid must give the same bytes: Fr sums are exact."""
    T = M.tile_items(k)
    assert T == (64 if k == 3 else 4)
    for n in (T - 1, T, T + 1, 2 * T + 1):
        c = make_case(n, k, 500 + n + k, shared=True)
        x = Inputs(oc, c)
        assert c.verdict()
        try:
            for blocks in (1, 2, 0):
                hip.set_option("verify_sets_blocks", blocks)
                x.check(x.call(hip, env, srs="plain" if blocks == 1 else "tabled"), (n, blocks))
        finally:
            hip.set_option("verify_sets_blocks", 0)
    from keaki_amd.hip import KeakiHipError
    for bad in (-1, 1025):
        with pytest.raises(KeakiHipError):
            hip.set_option("verify_sets_blocks", bad)


@pytest.mark.parametrize("n,k", [(M.VS_INV - 1, 1), (M.VS_INV, 1), (M.VS_INV + 1, 1), (5, 3), (11, 3), (3, 17), (700, 2)])
def test_inversion_chunks(oc, hip, env, n, k):
    """a lane inverts 16 (item, j) pairs with one inversion: n k around the chunk edge, chunks that straddle items (k = 3: 15 and 33 pairs; k = 17: 51),
    and 1,400 pairs = 88 chunks"""
    c = make_case(n, k, 9 * n + k, shared=True)
    x = Inputs(oc, c)
    assert c.verdict()
    x.check(x.call(hip, env), (n, k))


# ---- 5. point_mode 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_point_mode_1_gives_the_bytes_of_mode_0_on_the_same_powers(oc, hip, env):
    log2d, n, k = 10, 9, 5
    d = 1 << log2d
    w = omega(d)
    r = rand_fr_ints(n + 12 + n * k, 55)
    idx = [[0, d - 1, 1, 2, 3]] + [sorted({v % d for v in r[n + 12 + i * k:n + 12 + (i + 1) * k]}) for i in range(1, n)]
    for i in range(1, n):
        while len(idx[i]) < k:
            idx[i].append((max(idx[i]) + 1) % d)
        assert len(set(idx[i])) == k
    c = M.valid_case(TAU, [r[n:n + 12]], [[pow(w, e, R) for e in row] for row in idx], r[:n])
    x = Inputs(oc, c)
    host = x.call(hip, env)
    x.check(host, "mode 0")
    om = mont(oc, [w])[0]
    flat = np.array([e for row in idx for e in row], np.uint32)
    assert same(x.call(hip, env, points=flat, omega=om), host)
    wide = np.full(n * 8, 0xFFFFFFFF, np.uint32)                      # item_stride 8: the gaps hold indices nobody may read
    wide.reshape(n, 8)[:, :k] = flat.reshape(n, k)
    vals = np.full((n * 8, 4), SENT)
    vals.reshape(n, 8, 4)[:, :k] = x.values.reshape(n, k, 4)
    assert same(x.call(hip, env, points=wide, values=vals, omega=om, item_stride=8), host)
    # one index changed: the point moves, the verdict with it
    b = c.copy()
    b.z[3][2] = b.z[3][2] * w % R
    if b.z[3][2] not in c.z[3]:
        bad = flat.copy()
        bad[3 * k + 2] = (bad[3 * k + 2] + 1) % d
        got = x.call(hip, env, points=bad, omega=om)
        assert not got[0] and not b.verdict() and np.array_equal(got[1], g1_of(oc, b.sums()))


# ---- 6. item_stride ----------------------------------------------------------------------------------------------------------------------------------
def test_item_stride_with_poisoned_gaps(oc, hip, env):
    n, k, stride = 7, 3, 5
    c = make_case(n, k, 66)
    x = Inputs(oc, c)
    tight = x.call(hip, env)
    x.check(tight)
    pts, vals = np.full((n * stride, 4), SENT), np.full((n * stride, 4), SENT)
    pts.reshape(n, stride, 4)[:, :k] = x.points.reshape(n, k, 4)
    vals.reshape(n, stride, 4)[:, :k] = x.values.reshape(n, k, 4)
    assert same(x.call(hip, env, points=pts, values=vals, item_stride=stride), tight)
    # the last row may end right behind its k-th element
    end = (n - 1) * stride + k
    assert same(x.call(hip, env, points=pts[:end].copy(), values=vals[:end].copy(), item_stride=stride), tight)


# ---- 7. ordinary inputs --------------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(oc, hip, env):
    c = make_case(5, 4, 71)
    # all gammas zero: accepts anything, every sum is the identity
    b = c.copy()
    b.gamma = [0] * b.n
    b.y[1][0] = (b.y[1][0] + 1) % R
    x = Inputs(oc, b)
    got = x.call(hip, env)
    x.check(got, "gamma = 0")
    assert got[0] and not got[1].any()
    # a polynomial of degree < k: p = I, the proof is the identity
    s = make_case(4, 6, 72, degree=3)
    assert not any(s.q) and s.verdict()
    x = Inputs(oc, s)
    got = x.call(hip, env)
    x.check(got, "identity proofs")
    assert got[0] and not got[1][1:].any()
    # an identity commitment with zero values: the zero polynomial
    z = M.valid_case(TAU, [[0, 0, 0]], c.z, c.gamma)
    assert z.com == [0] and not any(z.q) and not any(v for row in z.y for v in row) and z.verdict()
    x = Inputs(oc, z)
    got = x.call(hip, env, srs="plain")
    x.check(got, "zero polynomial")
    assert got[0] and not got[1].any()
    # ... and a non-trivial one: p(tau) = 0 by the choice of the constant coefficient
    r = rand_fr_ints(10, 73)
    p = r[:8]
    p[0] = (p[0] - KM.poly_eval(p, TAU)) % R
    y = M.valid_case(TAU, [p], c.z, c.gamma)
    assert y.com == [0] and y.verdict()
    x = Inputs(oc, y)
    x.check(x.call(hip, env), "identity commitment")
    # the same item four times with four gammas
    d = c.copy()
    d.z, d.y, d.q, d.com, d.gamma, d.n = [c.z[0]] * 4, [c.y[0]] * 4, [c.q[0]] * 4, [c.com[0]] * 4, c.gamma[:4], 4
    assert d.verdict()
    x = Inputs(oc, d)
    got = x.call(hip, env)
    x.check(got, "one item repeated")
    assert got[0]
    # n = 0
    e4, e8 = np.zeros((0, 4), np.uint64), np.zeros((0, 8), np.uint64)
    ok, sums = hip.kzg_verify_sets(env["plain"], env["srs2"], x.com[:1], e4, e4, 4, e8, e4)
    assert ok and sums.shape == (5, 8) and not sums.any()


def test_cancelling_pair_is_accepted_at_equal_gammas_only(oc, hip, env):
    """the documented trap: the call evaluates the combined equation for the gammas it is given"""
    r = rand_fr_ints(40, 4243)
    zs = [r[0:3], r[0:3], r[3:6]]
    c = M.valid_case(TAU, [r[6:14], r[14:22], r[22:30]], zs, [1, 1, 1])
    c.y[0][2] = (c.y[0][2] + 987654321) % R
    c.y[1][2] = (c.y[1][2] - 987654321) % R
    assert c.verdict() and not c.single(0) and not c.single(1)
    x = Inputs(oc, c)
    got = x.call(hip, env)
    x.check(got)
    assert got[0]
    c.gamma = r[30:33]
    x = Inputs(oc, c)
    got = x.call(hip, env)
    x.check(got)
    assert not got[0]


# ---- 8. beyond the row limit of the batched MSM ---------------------------------------------------------------------------------------------------------
def test_one_item_more_than_the_batched_msm_takes(oc, hip, env):
    """n = N_BATCH_MAX + 1, k = 2: the k + 1 rows over the proofs run one MSM each. Eight distinct valid items repeated with distinct gammas; the
    expected sums come from the eight items' polynomials, combined here with the gammas."""
    n, k, m = N_BATCH_MAX + 1, 2, 8
    base = make_case(m, k, 88)
    gam = rand_fr_ints(n, 89)
    x8 = Inputs(oc, base, want=False)
    rep = np.arange(n) % m
    com, proofs = x8.com[rep], x8.proofs[rep]
    points, values = x8.points.reshape(m, k, 4)[rep].reshape(-1, 4), x8.values.reshape(m, k, 4)[rep].reshape(-1, 4).copy()
    gammas = mont(oc, gam)
    zc, ic = [base.Z(i) for i in range(m)], [base.I(i) for i in range(m)]

    def sums(ic_last):
        dl = [0] * (k + 1)
        for i in range(n):
            e, g = i % m, gam[i]
            icur = ic_last if i == n - 1 else ic[e]
            dl[0] += g * (base.com[e] - KM.poly_eval(icur, TAU) - zc[e][0] * base.q[e])
            for t in range(1, k + 1):
                dl[t] += g * zc[e][t] * base.q[e]
        return g1_of(oc, [v % R for v in dl])

    ok, got = hip.kzg_verify_sets(env["tabled"], env["srs2"], com, points, values, k, proofs, gammas)
    assert ok and np.array_equal(got, sums(ic[(n - 1) % m]))
    e = (n - 1) % m
    ybad = [(base.y[e][0] + 1) % R, base.y[e][1]]
    values[(n - 1) * k] = mont(oc, [ybad[0]])[0]
    ok, got = hip.kzg_verify_sets(env["tabled"], env["srs2"], com, points, values, k, proofs, gammas)
    assert not ok and np.array_equal(got, sums(KM.interpolant(base.z[e], ybad)))


# ---- 9. _dev: the same bytes as the host form, in stream order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["private", "torch"])
def test_dev_calls_in_stream_order(oc, env, form):
    """Three _dev calls of changing n and k on one stream (the second grows the workspace behind the first). In front of each call the caller's stream
    WRITES the inputs (copies from staging tensors into buffers that held zeros), right behind it the stream overwrites them with zeros: a call must
    have read what the buffers held at its place in the stream. A private stream is unordered against the caller's by contract, so there the caller
    synchronises torch in front of the call (the call itself ends synchronised: its results are host values)."""
    import torch
    from keaki_amd.hip import KeakiHip
    if form == "torch":
        stream = torch.cuda.Stream()
        h = KeakiHip(0, stream=stream.cuda_stream)
    else:
        stream = torch.cuda.default_stream()
        h = KeakiHip(0)
    front = torch.cuda.synchronize if form == "private" else (lambda: None)
    try:
        cases = [make_case(9, 2, 201), make_case(150, 9, 202, shared=True), make_case(3, 64, 203)]
        xs = [Inputs(oc, c) for c in cases]
        staged = [[dev(a) for a in (x.com, x.points, x.values, x.proofs, x.gamma)] for x in xs]
        work = [[torch.zeros_like(t) for t in st] for st in staged]
        torch.cuda.synchronize()
        got = []
        with torch.cuda.stream(stream):
            for x, st, b in zip(xs, staged, work):
                for dst, src in zip(b, st):
                    dst.copy_(src, non_blocking=True)                     # the producer, on the caller's stream
                front()
                got.append(h.kzg_verify_sets_dev(env["tabled"], env["srs2"], b[0], 0 if len(x.com) == 1 else 1, b[1], 0, None, b[2], x.k, x.k, b[3], b[4], x.n))
                for dst in b:
                    dst.zero_()                                           # the inputs overwritten right behind the call
        for x, g in zip(xs, got):
            x.check(g)
            assert g[0]
            assert same(x.call(h, env), g)                                # the host form: same verdict, same bytes
        # point_mode 1 with resident indices
        d, n, k = 16, 4, 3
        w = omega(d)
        idx = np.array([[0, 15, 7], [1, 2, 3], [4, 9, 14], [15, 0, 8]], np.uint32)
        r = rand_fr_ints(n + 9, 204)
        c = M.valid_case(TAU, [r[n:]], [[pow(w, int(e), R) for e in row] for row in idx], r[:n])
        x = Inputs(oc, c)
        om = mont(oc, [w])[0]
        g = h.kzg_verify_sets_dev(env["plain"], env["srs2"], dev(x.com), 0, dev(idx.reshape(-1)), 1, om, dev(x.values), k, k, dev(x.proofs), dev(x.gamma), n)
        x.check(g)
        assert g[0]
    finally:
        h.close()


# ---- 10. errors: refused on the host, nothing written, the context stays usable ------------------------------------------------------------------------
def test_errors_write_nothing_and_leave_the_context_usable(oc, hip, env):
    c = make_case(6, 4, 71)
    x = Inputs(oc, c)
    lib, ptr = hip.lib, lambda a: a.ctypes.data_as(C.c_void_p)
    ok = C.c_int32(77)
    sums = np.full(8 * 70, SENT)
    om = mont(oc, [omega(16)])[0]

    def raw(srs=env["tabled"], srs2=env["srs2"], com=x.com, com_stride=0 if len(x.com) == 1 else 1, points=x.points, point_mode=0, omega_=None, values=x.values,
            item_stride=4, k=4, proofs=x.proofs, gammas=x.gamma, n=c.n, okp=C.byref(ok), fn=lib.keaki_hip_kzg_verify_sets):
        p = lambda a: None if a is None else ptr(a)
        return fn(hip.ctx, srs.handle if srs else None, srs2.handle if srs2 else None, p(com), com_stride, p(points), point_mode, p(omega_), p(values),
                  item_stride, k, p(proofs), p(gammas), n, okp, ptr(sums))

    held_before = hip.memory()
    for fn in (lib.keaki_hip_kzg_verify_sets, lib.keaki_hip_kzg_verify_sets_dev):
        for name, kw, want in [
            ("null srs_g1", dict(srs=None), BAD_ARG), ("null srs_g2", dict(srs2=None), BAD_ARG), ("null com", dict(com=None), BAD_ARG),
            ("null points", dict(points=None), BAD_ARG), ("null values", dict(values=None), BAD_ARG), ("null proofs", dict(proofs=None), BAD_ARG),
            ("null gammas", dict(gammas=None), BAD_ARG), ("null ok_out", dict(okp=None), BAD_ARG), ("com_stride 2", dict(com_stride=2), BAD_ARG),
            ("point_mode 2", dict(point_mode=2, omega_=om), BAD_ARG), ("point_mode -1", dict(point_mode=-1), BAD_ARG),
            ("point_mode 1 without omega", dict(point_mode=1), BAD_ARG), ("k = 0", dict(k=0, item_stride=0), BAD_ARG), ("k = 65", dict(k=65, item_stride=65), BAD_ARG),
            ("item_stride < k", dict(item_stride=3), BAD_ARG), ("n k = 2^31", dict(n=1 << 29), BAD_ARG), ("n = 2^31", dict(n=1 << 31, k=1, item_stride=1), BAD_ARG),
            ("extent 2^47", dict(item_stride=((1 << 47) + 4) // 5), BAD_ARG), ("extent wraps 64 bits", dict(n=1 << 20, item_stride=1 << 59), BAD_ARG),
        ]:
            assert raw(fn=fn, **kw) == want, name
            assert ok.value == 77 and (sums == SENT).all(), name
    assert hip.memory() == held_before, "a refused call reserves nothing"
    short1, short2 = hip.srs_g1_upload(env["g1"][:3]), hip.srs_g2_upload(env["g2"][:4])
    try:
        for kw in (dict(srs=short1), dict(srs2=short2)):                  # k = 4: I needs 4 points of G1, Z 5 of G2
            assert raw(**kw) == TOO_LARGE and ok.value == 77 and (sums == SENT).all()
        assert hip.memory() == held_before
    finally:
        short1.free(); short2.free()
    x.check(x.call(hip, env), "the next valid call")


def test_workspace_is_counted_trimmed_and_refusable(oc, env):
    from keaki_amd.hip import KeakiHip, KeakiHipError
    c = make_case(70, 9, 91, shared=True)
    x = Inputs(oc, c)
    h = KeakiHip(0)
    try:
        base = h.memory()["workspaces"]
        x.check(x.call(h, env, srs="plain"))
        grown = h.memory()["workspaces"]
        tiles = -(-c.n // M.tile_items(c.k))
        assert grown >= base + 32 * ((c.k + 1) * c.n + c.n * c.k + M.K_MAX + 1 + tiles * (c.k + 1))
        h.trim()
        assert h.memory()["workspaces"] == 0
        ok = C.c_int32(77)
        sums = np.full((c.k + 1, 8), SENT)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        h.debug_set_alloc_limit(1024)                # the io block and everything larger is refused
        st = h.lib.keaki_hip_kzg_verify_sets(h.ctx, env["plain"].handle, env["srs2"].handle, ptr(x.com), 0, ptr(x.points), 0, None, ptr(x.values), c.k, c.k,
                                             ptr(x.proofs), ptr(x.gamma), c.n, C.byref(ok), ptr(sums))
        assert st == OOM and ok.value == 77 and (sums == SENT).all()
        with pytest.raises(KeakiHipError) as e:
            x.call(h, env, srs="plain")
        assert e.value.status == OOM
        h.debug_set_alloc_limit(0)
        x.check(x.call(h, env, srs="plain"), "after the refusal")
    finally:
        h.close()
