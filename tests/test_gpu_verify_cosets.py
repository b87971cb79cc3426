"""KZG coset batch verification on the GPU (keaki_hip_kzg_verify_cosets, _dev) against the big-integer model (tests/coset_verify_model.py). The
SRS comes from a KNOWN tau, so every commitment, proof and sum has a known discrete log: expected points are (integer) x generator from the
oracle's scalar multiplication, expected proofs come from long division by x^l - c (fk_coset_model), and nothing expected comes from the library
under test. tests/test_coset_verify_model.py shows on the CPU that every corruption used here breaks the equation itself."""
import ctypes as C
import os

import numpy as np
import pytest

import coset_verify_model as M
import fk_coset_model as FM
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, OOM, TOO_LARGE = -1, -3, -5
TAU = rand_fr_ints(1, 20261020)[0]
SRS_LEN = 1024                               # KEAKI_SET_MAX points: l = 1,024 reads them all
SHAPES = [(4, 1), (6, 2), (6, 6), (8, 3), (10, 4), (11, 10), (5, 0)]      # (log2d, log2l): r = 1 at (6, 6); l = KEAKI_SET_MAX, n = 2 at (11, 10)
L_TILE = 16
TILE = M.tile_items(L_TILE)                  # 64 items of l = 16 fill one LDS tile of the transform kernel (VC_TILE_ELEMS = 1,024 values)
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


def g2_of(oc, dl):
    return oc.g2_mul_batch(oc.generators()[1], mont(oc, [dl]), threads=1)[0]


def dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64).copy()).cuda()
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
    for h in (plain, tabled):
        h.free()


class Inputs:
    """a model case as the arrays the ABI takes (rows layout), with the expected sums as points"""

    def __init__(self, oc, c):
        self.c, self.n, self.l, self.log2l = c, c.n, c.l, c.l.bit_length() - 1
        pts = g1_of(oc, list(c.com) + list(c.q) + list(c.sums()))
        self.com, self.proofs, self.want = pts[:len(c.com)], pts[len(c.com):len(c.com) + c.n], pts[-2:]
        self.tau_l = g2_of(oc, c.tau_l)
        self.h, self.gamma = mont(oc, c.h), mont(oc, c.gamma)
        self.values = mont(oc, [v for row in c.y for v in row])
        w = M.omega(c.l)
        self.winv, self.linv = mont(oc, [M.inv(w)])[0], mont(oc, [M.inv(c.l)])[0]

    def call(self, hip, srs, **kw):
        a = dict(com=self.com, points=self.h, values=self.values, strides=(self.l, 1), point_mode=0, gammas=self.gamma, proofs=self.proofs, tau_l=self.tau_l)
        a.update(kw)
        return hip.kzg_verify_cosets(srs, a["com"], a["tau_l"], a["points"], a["values"], a["strides"][0], a["strides"][1], self.log2l, self.winv, self.linv,
                                     a["proofs"], a["gammas"], point_mode=a["point_mode"])

    def check(self, got, what=""):
        ok, L, Rp = got
        assert ok == self.c.verdict(), what
        assert np.array_equal(L, self.want[0]) and np.array_equal(Rp, self.want[1]), what


def rows_case(n, l, degree, seed, shared=True):
    r = rand_fr_ints(2 * n + (degree + 1) * (1 if shared else n), seed)
    hs, gammas, rest = r[:n], r[n:2 * n], r[2 * n:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(TAU, polys, hs, l, gammas)


def vector(oc, env, log2d, log2l):
    """(model case, Inputs, the d evaluations in domain order, the coefficients) of all r cosets of one vector, computed once per shape"""
    key = (log2d, log2l)
    if key not in env["cache"]:
        r = 1 << (log2d - log2l)
        rnd = rand_fr_ints(r + (1 << log2d), 5000 + 32 * log2d + log2l)
        c, evals = M.vector_case(TAU, rnd[r:], log2d, log2l, rnd[:r])
        env["cache"][key] = (c, Inputs(oc, c), mont(oc, evals), mont(oc, rnd[r:]))
    return env["cache"][key]


# ---- 1. valid inputs: all cosets of a vector, both layouts, both point modes, both handles ---------------------------------------------------------
@pytest.mark.parametrize("log2d,log2l", SHAPES)
def test_all_cosets_of_a_vector(oc, hip, env, log2d, log2l):
    c, x, evals, _ = vector(oc, env, log2d, log2l)
    r = c.n
    assert c.verdict()
    omega_d = mont(oc, [M.omega(1 << log2d)])
    seen = []
    for srs in (env["plain"], env["tabled"]):
        seen.append(x.call(hip, srs))                                                              # rows, the shifts given
        x.check(seen[-1], "rows")
        seen.append(x.call(hip, srs, point_mode=1, points=omega_d))                                # h_k = omega_d^k derived on the device
        seen.append(x.call(hip, srs, values=evals, strides=(1, r)))                                # the vector in domain order
        seen.append(x.call(hip, srs, values=evals, strides=(1, r), point_mode=1, points=omega_d))
    for s in seen[1:]:
        assert s[0] == seen[0][0] and np.array_equal(s[1], seen[0][1]) and np.array_equal(s[2], seen[0][2])


def test_proofs_of_open_fk_cosets_poly_dev_verify(oc, hip, env):
    """the prover's call feeds the verifier's, everything resident: the proofs never leave the device"""
    log2d, log2l = 6, 2
    c, x, evals, coeffs = vector(oc, env, log2d, log2l)
    r, n2 = c.n, 2 * c.n
    w2 = FM.omega(n2)
    rt = tuple(mont(oc, [v])[0] for v in (w2, FM.inv(w2), FM.inv(n2)))
    d_c, d_proofs = dev(coeffs), dev(np.full((r, 8), SENT))
    hip.open_fk_cosets_poly_dev(env["tabled"], log2d, log2l, d_c.data_ptr(), *rt, d_proofs.data_ptr())
    hip.synchronize()
    assert np.array_equal(d_proofs.cpu().numpy().view(np.uint64), x.proofs)
    d = [dev(a) for a in (x.com, x.tau_l, mont(oc, [M.omega(1 << log2d)]), evals, x.gamma)]
    got = hip.kzg_verify_cosets_dev(env["tabled"], d[0], 0, d[1], d[2], 1, d[3], 1, r, log2l, x.winv, x.linv, d_proofs, d[4], r)
    x.check(got)
    assert got[0]
    # one changed evaluation in place on the device
    bad = evals.copy()
    bad[5] = mont(oc, [c.y[5][0] + 1])[0]
    got = hip.kzg_verify_cosets_dev(env["tabled"], d[0], 0, d[1], d[2], 1, dev(bad), 1, r, log2l, x.winv, x.linv, d_proofs, d[4], r)
    b = c.copy()
    b.y[5][0] += 1
    assert not got[0] and not b.verdict()
    assert np.array_equal(np.concatenate(got[1:]), g1_of(oc, list(b.sums())).reshape(-1))


# ---- 2. the tile edges of the transform kernel and the chunk edges of the batched inversion --------------------------------------------------------
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_tile_edges_separate_commitments(oc, hip, env, n):
    """l = 16: TILE = 64 items fill a tile; 3 TILE + 5 items are four workgroups, whose rows k_vc_finish folds in one pass (its waves run over ALL rows,
    however many: there is no second pass to overflow). With "verify_cosets_blocks" = 2 each workgroup runs two tiles and keeps its sums in registers between them."""
    c = rows_case(n, L_TILE, 2 * L_TILE + 3, 100 + n, shared=False)
    x = Inputs(oc, c)
    assert c.verdict()
    x.check(x.call(hip, env["tabled"]), n)
    if n > 2 * TILE:
        try:
            for blocks in (1, 2, 3):
                hip.set_option("verify_cosets_blocks", blocks)
                x.check(x.call(hip, env["plain"]), (n, blocks))
        finally:
            hip.set_option("verify_cosets_blocks", 0)
        from keaki_amd.hip import KeakiHipError
        for bad in (-1, 1025):
            with pytest.raises(KeakiHipError):
                hip.set_option("verify_cosets_blocks", bad)


@pytest.mark.parametrize("n,l", [(M.VC_INV - 1, 2), (M.VC_INV, 2), (M.VC_INV + 1, 2), (16 * M.VC_INV + 3, 4), (1025, 1), (5, 32), (3, 512)])
def test_inversion_chunks_and_small_tiles(oc, hip, env, n, l):
    """a lane inverts 16 shifts with one inversion: n around the chunk edge; l = 1, 2 put several items into one lane's four values;
    l = 1 with 1,025 items is a tile and one value"""
    c = rows_case(n, l, l + 2, 7 * n + l)
    x = Inputs(oc, c)
    x.check(x.call(hip, env["tabled"]), (n, l))
    assert c.verdict()


def test_many_workgroups_of_every_kernel(oc, hip, env):
    """n = 4,500 items of l = 4 with the grid left automatic, the shapes of the kernels' loops at production sizes: 282 inversion chunks = two workgroups
    of k_vc_prepare (the second starts its powers at omega^4096 and k_vc_finish folds two entries of part_g), 18 tiles of 256 items = 18 workgroups of
    k_vc_transform with k_base > 0, 18 rows for the four waves of k_vc_finish (five turns of its row loop, the last one partial). In domain order with
    point_mode 1 -- the addressing of vec_verify_cosets: value (k, t) at k + t n -- and in row order with the shifts given: the model's bytes both times.
    With 7 workgroups a workgroup runs 2 or 3 tiles. One shared polynomial keeps the model cheap."""
    n, l = 4500, 4
    w = M.omega(8192)
    rnd = rand_fr_ints(n + 12, 4500)
    hs, acc = [], 1
    for _ in range(n):
        hs.append(acc)
        acc = acc * w % R
    c = M.valid_case(TAU, [rnd[n:]], hs, l, rnd[:n])
    x = Inputs(oc, c)
    assert c.verdict()
    by_t = np.ascontiguousarray(x.values.reshape(n, l, 4).transpose(1, 0, 2)).reshape(-1, 4)
    omega = mont(oc, [w])
    x.check(x.call(hip, env["tabled"], values=by_t, strides=(1, n), point_mode=1, points=omega), "domain order, point_mode 1")
    x.check(x.call(hip, env["plain"]), "rows, point_mode 0")
    x.check(x.call(hip, env["plain"], values=by_t, strides=(1, n)), "domain order, point_mode 0")
    try:
        hip.set_option("verify_cosets_blocks", 7)
        x.check(x.call(hip, env["tabled"], values=by_t, strides=(1, n), point_mode=1, points=omega), "7 workgroups")
    finally:
        hip.set_option("verify_cosets_blocks", 0)
    # one wrong value in the last tile, seen through the last row and the second workgroup's shifts
    b = c.copy()
    b.y[n - 3][l - 1] = (b.y[n - 3][l - 1] + 1) % R
    bad = by_t.copy()
    bad[(n - 3) + (l - 1) * n] = mont(oc, [b.y[n - 3][l - 1]])[0]
    ok, L, Rp = x.call(hip, env["tabled"], values=bad, strides=(1, n), point_mode=1, points=omega)
    want = g1_of(oc, list(b.sums()))
    assert not ok and not b.verdict() and np.array_equal(L, want[0]) and np.array_equal(Rp, want[1]), "a wrong value in the last tile"


# ---- 3. l = 1 is verify_batch --------------------------------------------------------------------------------------------------------------------------
def test_l_1_gives_the_bytes_of_verify_batch(oc, hip, env):
    c = rows_case(37, 1, 9, 31, shared=False)
    x = Inputs(oc, c)
    got = x.call(hip, env["tabled"])
    x.check(got)
    vb = hip.kzg_verify_batch(x.com, g2_of(oc, TAU), x.h, x.values, x.proofs, x.gamma)
    assert vb[0] == got[0] and np.array_equal(vb[1], got[1]) and np.array_equal(vb[2], got[2])
    bad = x.values.copy()
    bad[4] = mont(oc, [1])[0]
    got, vb = x.call(hip, env["plain"], values=bad), hip.kzg_verify_batch(x.com, g2_of(oc, TAU), x.h, bad, x.proofs, x.gamma)
    assert not got[0] and not vb[0] and np.array_equal(vb[1], got[1]) and np.array_equal(vb[2], got[2])


# ---- 4. com_stride --------------------------------------------------------------------------------------------------------------------------------------
def test_one_commitment_or_the_same_one_repeated(oc, hip, env):
    c = rows_case(21, 8, 30, 55)
    x = Inputs(oc, c)
    one = x.call(hip, env["tabled"])
    x.check(one)
    many = x.call(hip, env["tabled"], com=np.repeat(x.com, c.n, axis=0))
    assert many[0] == one[0] and np.array_equal(many[1], one[1]) and np.array_equal(many[2], one[2])


# ---- 5. the verdict is the AND of verify_multi ----------------------------------------------------------------------------------------------------------
def test_verdict_is_the_and_of_four_verify_multi_calls(oc, hip, env):
    log2d, log2l = 4, 2
    c, x, _, _ = vector(oc, env, log2d, log2l)
    assert c.n == 4
    pw = [1]
    for _ in range(c.l):
        pw.append(pw[-1] * TAU % R)
    srs2 = hip.srs_g2_upload(oc.g2_mul_batch(oc.generators()[1], mont(oc, pw), threads=NCPU))
    try:
        for corrupt in (None, 2):
            vals = x.values.reshape(c.n, c.l, 4).copy()
            b = c.copy()
            if corrupt is not None:
                b.y[corrupt][1] = (b.y[corrupt][1] + 1) % R
                vals[corrupt, 1] = mont(oc, [b.y[corrupt][1]])[0]
            singles = [hip.kzg_verify_multi(env["tabled"], srs2, x.com[0], mont(oc, M.coset_points(c.h[k], c.l)), vals[k], x.proofs[k]) for k in range(c.n)]
            assert singles == [b.single(k) for k in range(c.n)]
            ok, _, _ = x.call(hip, env["tabled"], values=vals.reshape(-1, 4))
            assert ok == all(singles) == b.verdict()
    finally:
        srs2.free()


# ---- 6. rejections: verdict AND sums are the model's ---------------------------------------------------------------------------------------------------
def test_rejections_match_the_model(oc, hip, env):
    c = rows_case(6, 8, 21, 808, shared=False)
    cases = {}
    for name, t in (("value at t = 0", 0), ("value at t = l - 1", c.l - 1)):
        b = c.copy()
        b.y[1][t] = (b.y[1][t] + 1) % R
        cases[name] = b
    b = c.copy(); b.q[0], b.q[2] = b.q[2], b.q[0]; cases["two proofs swapped"] = b
    b = c.copy(); b.y[0], b.y[2] = b.y[2], b.y[0]; cases["two value rows swapped"] = b
    b = c.copy(); b.h[1] = (b.h[1] + 1) % R; cases["a wrong shift"] = b
    assert c.verdict()
    for name, b in cases.items():
        x = Inputs(oc, b)
        assert not b.verdict(), name
        x.check(x.call(hip, env["tabled"]), name)
    # [tau]_2 in place of [tau^2]_2: the sums are those of the valid call, the verdict is not
    c2 = rows_case(5, 2, 7, 809)
    b = c2.copy()
    b.tau_l = TAU
    x = Inputs(oc, b)
    assert c2.verdict() and not b.verdict() and b.sums() == c2.sums()
    x.check(x.call(hip, env["tabled"]), "[tau]_2 at l = 2")


def test_cancelling_pair_is_accepted_at_equal_gammas_only(oc, hip, env):
    """the documented trap: the call evaluates the combined equation for the gammas it is given"""
    rnd = rand_fr_ints(64, 4242)
    h = rnd[0]
    c = M.valid_case(TAU, [rnd[4:16], rnd[16:28], rnd[28:40], rnd[40:52]], [h, h, rnd[1], rnd[2]], 4, [1] * 4)
    d = 987654321
    c.y[0][2] = (c.y[0][2] + d) % R
    c.y[1][2] = (c.y[1][2] - d) % R
    assert c.verdict() and not c.single(0) and not c.single(1)
    x = Inputs(oc, c)
    got = x.call(hip, env["tabled"])
    x.check(got)
    assert got[0]
    c.gamma = rnd[52:56]
    x = Inputs(oc, c)
    got = x.call(hip, env["tabled"])
    x.check(got)
    assert not got[0]


# ---- 7. ordinary inputs ------------------------------------------------------------------------------------------------------------------------------------
def test_identities_zeros_and_the_empty_call(oc, hip, env):
    # deg p < l: every proof is the identity, R = identity, L = identity
    c = rows_case(5, 8, 5, 61)
    assert not any(c.q) and c.sums() == (0, 0) and c.verdict()
    x = Inputs(oc, c)
    got = x.call(hip, env["tabled"])
    x.check(got)
    assert got[0] and not got[1].any() and not got[2].any()
    # an identity commitment: p(tau) = 0 by the choice of the constant coefficient
    rnd = rand_fr_ints(30, 62)
    p = rnd[:20]
    p[0] = (p[0] - FM.poly_eval(p, TAU)) % R
    c = M.valid_case(TAU, [p], rnd[20:24], 4, rnd[24:28])
    assert c.com == [0] and c.verdict()
    x = Inputs(oc, c)
    x.check(x.call(hip, env["plain"]), "identity commitment")
    # gamma = 0 accepts anything; zero values are values
    b = c.copy()
    b.gamma = [0] * b.n
    b.y[1][0] += 1
    x = Inputs(oc, b)
    got = x.call(hip, env["plain"])
    x.check(got, "gamma = 0")
    assert got[0] and b.sums() == (0, 0)
    z = c.copy()
    z.y = [[0] * z.l for _ in range(z.n)]
    x = Inputs(oc, z)
    x.check(x.call(hip, env["plain"]), "zero values")
    # n = 0
    e = np.zeros((0, 4), np.uint64)
    ok, L, Rp = hip.kzg_verify_cosets(env["plain"], x.com, x.tau_l, e, e, 4, 1, 2, x.winv, x.linv, np.zeros((0, 8), np.uint64), e)
    assert ok and not L.any() and not Rp.any()


# ---- 8. errors: refused on the host, nothing written, the context stays usable -------------------------------------------------------------------------
def test_errors_write_nothing_and_leave_the_context_usable(oc, hip, env):
    c = rows_case(6, 4, 11, 71)
    x = Inputs(oc, c)
    lib, ptr = hip.lib, lambda a: a.ctypes.data_as(C.c_void_p)
    ok = C.c_int32(77)
    sums = np.full(16, SENT)

    def raw(srs=env["tabled"], com=x.com, com_stride=0, tau=x.tau_l, points=x.h, point_mode=0, values=x.values, item_stride=4, t_stride=1, log2l=2,
            winv=x.winv, linv=x.linv, proofs=x.proofs, gammas=x.gamma, n=c.n, okp=C.byref(ok)):
        p = lambda a: None if a is None else ptr(a)
        return lib.keaki_hip_kzg_verify_cosets(hip.ctx, srs.handle if srs else None, p(com), com_stride, p(tau), p(points), point_mode, p(values), item_stride,
                                               t_stride, log2l, p(winv), p(linv), p(proofs), p(gammas), n, okp, ptr(sums))

    held_before = hip.memory()
    for name, kw, want in [
        ("null srs", dict(srs=None), BAD_ARG), ("null com", dict(com=None), BAD_ARG), ("null tau", dict(tau=None), BAD_ARG),
        ("null points", dict(points=None), BAD_ARG), ("null values", dict(values=None), BAD_ARG), ("null proofs", dict(proofs=None), BAD_ARG),
        ("null gammas", dict(gammas=None), BAD_ARG), ("null omega_l_inv", dict(winv=None), BAD_ARG), ("null inv_l", dict(linv=None), BAD_ARG),
        ("null ok_out", dict(okp=None), BAD_ARG), ("com_stride 2", dict(com_stride=2), BAD_ARG), ("point_mode -1", dict(point_mode=-1), BAD_ARG),
        ("l > KEAKI_SET_MAX", dict(log2l=11), BAD_ARG), ("log2l 40", dict(log2l=40), BAD_ARG), ("n l = 2^31", dict(n=1 << 29), BAD_ARG),
        ("rows overlap", dict(item_stride=3), BAD_ARG), ("zero t_stride", dict(t_stride=0), BAD_ARG), ("zero item_stride", dict(item_stride=0), BAD_ARG),
        ("transposed too short", dict(item_stride=1, t_stride=5), BAD_ARG), ("crossing", dict(item_stride=2, t_stride=3), BAD_ARG),
        ("extent wraps 64 bits", dict(n=1 << 20, item_stride=1 << 59), BAD_ARG), ("extent 2^47 by items", dict(item_stride=((1 << 47) + 4) // 5), BAD_ARG),
        ("extent 2^47 by t", dict(item_stride=1, t_stride=((1 << 47) + 2) // 3), BAD_ARG), ("stride 2^63", dict(t_stride=1 << 63), BAD_ARG),
    ]:
        assert raw(**kw) == want, name
        assert ok.value == 77 and (sums == SENT).all(), name
    assert hip.memory() == held_before, "a refused call reserves nothing"
    short = hip.srs_g1_upload(env["g1"][:2])
    try:
        assert raw(srs=short) == TOO_LARGE and ok.value == 77 and (sums == SENT).all()
    finally:
        short.free()
    x.check(x.call(hip, env["tabled"]), "the next valid call")
    # strides that name distinct addresses without nesting are accepted: 5 k = 7 t has no solution with 0 < k < 6, 0 < t < 4
    wide = np.zeros((5 * 5 + 7 * 3 + 1, 4), np.uint64)
    for k in range(c.n):
        for t in range(c.l):
            wide[5 * k + 7 * t] = x.values[k * c.l + t]
    x.check(x.call(hip, env["tabled"], values=wide, strides=(5, 7)), "strides (5, 7)")


def test_workspace_is_counted_trimmed_and_refusable(oc, env):
    from keaki_amd.hip import KeakiHip, KeakiHipError
    c = rows_case(70, 16, 40, 91)
    x = Inputs(oc, c)
    h = KeakiHip(0)
    try:
        base = h.memory()["workspaces"]
        x.check(x.call(h, env["plain"]))
        grown = h.memory()["workspaces"]
        assert grown >= base + M_work_bytes(c.n, c.l)
        h.trim()
        assert h.memory()["workspaces"] == 0
        h.debug_set_alloc_limit(1024)                # the 1,792-byte io block and everything larger is refused
        with pytest.raises(KeakiHipError) as e:
            x.call(h, env["plain"])
        assert e.value.status == OOM
        h.debug_set_alloc_limit(0)
        x.check(x.call(h, env["plain"]), "after the refusal")
    finally:
        h.close()


def M_work_bytes(n, l):
    """csrc/kzg_cosets.hip: verify_cosets_work_bytes for a call of fewer than 1,024 tiles"""
    tiles = -(-n // M.tile_items(l))
    return 32 * (2 * n + l + 1 + 1024 + tiles * l)


# ---- 9. _dev on a stream of the caller's, and as queued work ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["private", "legacy", "torch"])
def test_dev_calls_in_stream_order(oc, env, form):
    """Three _dev calls of changing size and l on one stream (the second grows the workspace behind the first). In front of each call the caller's
    stream WRITES the inputs (copies from staging tensors into buffers that held zeros), right behind it the stream overwrites them with zeros, and
    the host never synchronises in between: a call must have read what the buffers held at its place in the stream. A caller-created stream and the
    legacy default stream order the calls with torch's copies by themselves; a private stream is unordered against the caller's by contract, so there
    the caller synchronises torch in front of the call (the call itself ends synchronised: its results are host values)."""
    import torch
    from keaki_amd.hip import KeakiHip, KEAKI_HIP_STREAM_LEGACY
    if form == "torch":
        stream = torch.cuda.Stream()
        h = KeakiHip(0, stream=stream.cuda_stream)
    elif form == "legacy":
        stream = torch.cuda.default_stream()
        assert stream.cuda_stream == 0
        h = KeakiHip(0, stream=KEAKI_HIP_STREAM_LEGACY)
    else:
        stream = torch.cuda.default_stream()
        h = KeakiHip(0)
    front = torch.cuda.synchronize if form == "private" else (lambda: None)
    try:
        cases = [rows_case(9, 4, 13, 201, shared=False), rows_case(150, 16, 35, 202), rows_case(3, 64, 70, 203)]
        xs = [Inputs(oc, c) for c in cases]
        staged = [[dev(a) for a in (x.com, x.tau_l, x.h, x.values, x.proofs, x.gamma)] for x in xs]
        work = [[torch.zeros_like(t) for t in st] for st in staged]
        torch.cuda.synchronize()
        got = []
        with torch.cuda.stream(stream):
            for x, st, b in zip(xs, staged, work):
                for dst, src in zip(b, st):
                    dst.copy_(src, non_blocking=True)                     # the producer, on the caller's stream
                front()
                got.append(h.kzg_verify_cosets_dev(env["tabled"], b[0], 0 if len(x.com) == 1 else 1, b[1], b[2], 0, b[3], x.l, 1, x.log2l, x.winv, x.linv, b[4],
                                                   b[5], x.n))
                for dst in b:
                    dst.zero_()                                           # the inputs overwritten right behind the call
        for x, g in zip(xs, got):
            x.check(g)
            assert g[0]
    finally:
        h.close()
