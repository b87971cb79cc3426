"""Batched FK23 openings and vec_commit through the C ABI (keaki_hip_open_fk_poly_batch*, keaki_hip_vec_commit_batch*): every row byte for byte
the single call's, one case against the oracle's per-point openings, adversarial rows side by side in one wave on SRS with a known secret
(proof = (its scalar) G), and every route tests/fk_batch_model.py lists: one pass, passes split by the cap, passes halved under an allocation
limit, the row-by-row fallback."""
import ctypes as C
import os

import numpy as np
import pytest

import fk_batch_model as M
import structured_inputs as S
from conftest_helpers import rand_fr_ints
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(16, os.cpu_count() or 1)
N_SRS = 512
ERR_BAD_ARG, ERR_TOO_LARGE = -1, -5
GAP = 0xFFFFFFFFFFFFFFFF                  # what the gap behind a row holds: all bits set, not even a field element


def consts(oc, log2d):
    """(omega_d^-1, 1/d, omega_2d, omega_2d^-1, 1/2d) in Montgomery limbs: the five domain constants of vec_commit, the last three of open_fk_poly"""
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    return [mont(oc, [x])[0] for x in (pow(w2 * w2, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]


def rows_of(oc, ints, m, n, stride=None):
    stride = n if stride is None else stride
    rows = np.full((m, stride, 4), GAP, np.uint64)
    if n:
        rows[:, :n] = mont(oc, ints).reshape(m, n, 4)
    return rows


def g1_of(oc, ks):
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, [k % R for k in ks]), threads=TH)


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
    """a context of its own: its workspaces start empty and its allocation limit is its own"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        yield h
    finally:
        h.debug_set_alloc_limit(0)
        h.close()


SHAPES = [(l, m) for l in (1, 2, 3) for m in (1, 2, 65)] + [(6, 63), (6, 64), (6, 65), (8, 1), (8, 130), (9, 3)]


@pytest.mark.parametrize("log2d,m", SHAPES)
def test_open_batch_equals_single_calls(oc, hip, base, log2d, m):
    d = 1 << log2d
    k = consts(oc, log2d)
    rows = rows_of(oc, rand_fr_ints(m * d, 40 * log2d + m), m, d, stride=d + (m % 2))
    ref = np.stack([hip.open_fk_poly(base["plain"], log2d, np.ascontiguousarray(rows[j, :d]), *k[2:]) for j in range(m)])
    for name in ("plain", "tabled"):
        got = hip.open_fk_poly_batch(base[name], log2d, rows, *k[2:])
        assert got.shape == (m, d, 8) and np.array_equal(got, ref), name


@pytest.mark.parametrize("log2d,m", SHAPES)
def test_vec_commit_batch_equals_single_calls(oc, hip, base, log2d, m):
    """row j = its first n evaluations: n = d, a length in between, 1 and 0 (the all-zero rows: identity commitment, identity proofs)"""
    d = 1 << log2d
    k = consts(oc, log2d)
    for n in sorted({d, d // 2 + 1, 1, 0}):
        rows = rows_of(oc, rand_fr_ints(m * n, 50 * log2d + m + n), m, n, stride=n + 1)
        # a commitment is an MSM: on the handle with tables the single call takes another MSM route, so each handle has its own reference
        for name in (("plain", "tabled") if m <= 3 or (n == d and m <= 65) else ("plain",)):
            ref = [hip.vec_commit(base[name], np.ascontiguousarray(rows[j, :n]), None, log2d, *k) for j in range(m)]
            com, proofs = hip.vec_commit_batch(base[name], rows, log2d, *k, n=n)
            assert np.array_equal(com, np.stack([r[0] for r in ref])), (name, n)
            assert np.array_equal(proofs, np.stack([r[1] for r in ref])), (name, n)
        if n == 0:
            assert not proofs.any() and not com[:, 8:].any(), "all-zero rows: identity proofs (0, 0) and the identity commitment (R, R, 0)"
            assert np.array_equal(com[0], hip.msm_g1(base["plain"], np.zeros((0, 4), np.uint64)))


def test_against_the_oracle_directly(oc, hip, base):
    """log2d = 6, m = 3: every proof is the oracle's MSM of the quotient (p - p(w^i)) / (x - w^i), every commitment its MSM of the coefficients"""
    log2d, m = 6, 3
    d = 1 << log2d
    k = consts(oc, log2d)
    wd = S.root_of_unity(d)
    evals = [rand_fr_ints(d, 600 + j) for j in range(m)]
    evals[1][d - 5:] = [0] * 5
    coeffs = [[c * pow(d, -1, R) % R for c in S.ntt(e, pow(wd, -1, R))] for e in evals]
    pts = base["pts"]

    def direct(p):
        out = []
        for i in range(d):
            z, acc, quot = pow(wd, i, R), 0, [0] * (d - 1)
            for t in range(d - 1, 0, -1):
                acc = (acc * z + p[t]) % R
                quot[t - 1] = acc
            out.append(oc.msm_g1(pts[:d - 1], mont(oc, quot), threads=TH))
        return np.stack(out)

    exp = np.stack([direct(p) for p in coeffs])
    assert np.array_equal(hip.open_fk_poly_batch(base["plain"], log2d, rows_of(oc, sum(coeffs, []), m, d), *k[2:]), exp)
    com, proofs = hip.vec_commit_batch(base["tabled"], rows_of(oc, sum(evals, []), m, d), log2d, *k)
    assert np.array_equal(proofs, exp)
    for j in range(m):
        assert np.array_equal(jac_to_aff(com[j]), oc.msm_g1(pts[:d], mont(oc, coeffs[j]), threads=TH))


def adversarial_polys(d, seed):
    rnd = rand_fr_ints(2 * d, seed)
    a, b = rnd[:d], rnd[d:]
    return [("zero", [0] * d), ("const", [7] + [0] * (d - 1)), ("twin", a), ("twin again", a), ("b", b), ("minus b", [(R - x) % R for x in b]),
            ("single", [0] * 5 + [3] + [0] * (d - 6)), ("ones", [1] * d), ("alternating", [1, R - 1] * (d // 2))]


@pytest.mark.parametrize("secret", ["one", "minus_one", "omega_d", "random"])
def test_adversarial_rows_side_by_side(oc, hip, secret):
    """nine rows in ONE wave of every butterfly, on SRS tau^i G: the structured rows meet equal and opposite operands and identities in the
    butterflies (structured_inputs.fk_model counts them: the generic additions behind j29_addsub are taken), their neighbours must not notice"""
    log2d = 6
    d = 1 << log2d
    tau = S.secrets(8, log2d)[secret]
    polys = adversarial_polys(d, 6100)
    if secret != "random":
        ev = [S.fk_model(tau, p, log2d, radix4=False)[1] for _, p in polys]
        assert sum(e["inv_addsub_special"] + e["fwd_addsub_special"] for e in ev) > 0
    k = consts(oc, log2d)
    wd = S.root_of_unity(d)
    srs = hip.srs_g1_upload(g1_of(oc, S.powers(tau, d)))
    try:
        got = hip.open_fk_poly_batch(srs, log2d, rows_of(oc, sum([p for _, p in polys], []), len(polys), d), *k[2:])
        for j, (name, p) in enumerate(polys):
            assert np.array_equal(got[j], g1_of(oc, S.fk_dlogs(tau, p, S.ntt(p, wd)))), (secret, name)
        assert not got[0].any() and not got[1].any(), "the zero and the constant polynomial: every proof is the identity"
        assert np.array_equal(got[2], got[3])
        # the same rows as evaluations: vec_commit_batch interpolates them first; commitment = p(tau) G
        evals = [S.ntt(p, wd) for _, p in polys]
        com, proofs = hip.vec_commit_batch(srs, rows_of(oc, sum(evals, []), len(polys), d), log2d, *k)
        assert np.array_equal(proofs, got)
        exp_com = g1_of(oc, [S.poly_eval(p, tau) for _, p in polys])
        for j in range(len(polys)):
            assert np.array_equal(jac_to_aff(com[j]), exp_com[j]), (secret, polys[j][0])
    finally:
        srs.free()


def test_gap_bytes_are_not_read(oc, hip, base):
    log2d, m = 3, 65
    d = 1 << log2d
    k = consts(oc, log2d)
    ints = rand_fr_ints(m * d, 77)
    tight = rows_of(oc, ints, m, d)
    ref = hip.open_fk_poly_batch(base["plain"], log2d, tight, *k[2:])
    ref_com, ref_pr = hip.vec_commit_batch(base["plain"], tight, log2d, *k)
    for fill in (GAP, 0x0123456789ABCDEF):
        wide = rows_of(oc, ints, m, d, stride=d + 3)
        wide[:, d:] = fill
        assert np.array_equal(hip.open_fk_poly_batch(base["plain"], log2d, wide, *k[2:]), ref)
        com, pr = hip.vec_commit_batch(base["plain"], wide, log2d, *k, n=d)
        assert np.array_equal(com, ref_com) and np.array_equal(pr, ref_pr)


def _case_rows(oc, k):
    """the rows of a route case: 130 distinct rows, repeated when the case has more (the reference is then 130 single calls)"""
    _, log2d, m, stride, _ = k
    d = 1 << log2d
    distinct = min(m, 130)
    rows = rows_of(oc, rand_fr_ints(distinct * d, 900 + log2d), distinct, d, stride=stride)
    reps = -(-m // distinct)
    return distinct, np.ascontiguousarray(np.tile(rows, (reps, 1, 1))[:m])


@pytest.mark.parametrize("name", [k[0] for k in M.GPU_CASES])
def test_routes(oc, base, own_ctx, name):
    """every route of the model's table gives the bytes of the single calls: the context starts without workspaces, one single call grows what
    the row-by-row route needs, then the limit of the case is set for the batch calls alone"""
    k = M.case(name)
    _, log2d, m, stride, _ = k
    d = 1 << log2d
    c = consts(oc, log2d)
    h, srs = own_ctx, base["plain"]
    distinct, rows = _case_rows(oc, k)
    ref_open = np.stack([h.open_fk_poly(srs, log2d, np.ascontiguousarray(rows[j, :d]), *c[2:]) for j in range(distinct)])
    ref_vec = [h.vec_commit(srs, np.ascontiguousarray(rows[j, :d]), None, log2d, *c) for j in range(distinct)]
    assert h.memory()["workspaces"] > 0
    reach = M.reach(k)
    tile = lambda a: np.tile(a, (-(-m // distinct),) + (1,) * (a.ndim - 1))[:m]
    h.debug_set_alloc_limit(M.case_limit(k))
    try:
        got_open = h.open_fk_poly_batch(srs, log2d, rows, *c[2:])
        com, proofs = h.vec_commit_batch(srs, rows, log2d, *c, n=d)
    finally:
        h.debug_set_alloc_limit(0)
    assert np.array_equal(got_open, tile(ref_open)), reach
    assert np.array_equal(proofs, tile(np.stack([r[1] for r in ref_vec]))) and np.array_equal(com, tile(np.stack([r[0] for r in ref_vec]))), reach
    if name == "halved":
        # the context holds the workspaces of a pass of 33 rows: without the limit the same call grows them to one pass; then from nothing
        assert np.array_equal(h.open_fk_poly_batch(srs, log2d, rows, *c[2:]), got_open)
        h.trim()
        assert np.array_equal(h.open_fk_poly_batch(srs, log2d, rows, *c[2:]), got_open)


def test_workspace_accounting(oc, base, own_ctx):
    log2d, m = 6, 65
    d = 1 << log2d
    c = consts(oc, log2d)
    h = own_ctx
    assert h.memory()["workspaces"] == 0
    rows = rows_of(oc, rand_fr_ints(m * d, 31), m, d)
    first = h.open_fk_poly_batch(base["plain"], log2d, rows, *c[2:])
    held = M.plan(log2d, m)["held"]
    assert held == (M.request(M.pts_bytes(log2d, m)), M.request(M.fr_bytes(log2d, m)))
    assert h.memory()["workspaces"] >= sum(held) + rows.nbytes + first.nbytes
    h.trim()
    assert h.memory()["workspaces"] == 0
    assert np.array_equal(h.open_fk_poly_batch(base["plain"], log2d, rows, *c[2:]), first)


def test_state_between_calls(oc, hip, base):
    """batch at d, single at d, batch at d' (replaces the handle's cached transform), batch at d again -- then the same from a second context
    on the same handle: all equal to the first"""
    from keaki_amd.hip import KeakiHip
    la, lb, m = 5, 3, 66
    ca, cb = consts(oc, la), consts(oc, lb)
    ra, rb = rows_of(oc, rand_fr_ints(m << la, 41), m, 1 << la), rows_of(oc, rand_fr_ints(m << lb, 42), m, 1 << lb)
    srs = hip.srs_g1_upload(base["pts"])
    other = KeakiHip(0)
    try:
        first_a = hip.open_fk_poly_batch(srs, la, ra, *ca[2:])
        assert np.array_equal(hip.open_fk_poly(srs, la, np.ascontiguousarray(ra[7]), *ca[2:]), first_a[7])
        first_b = hip.vec_commit_batch(srs, rb, lb, *cb)
        assert np.array_equal(hip.vec_commit(srs, np.ascontiguousarray(rb[65]), None, lb, *cb)[1], first_b[1][65])
        assert np.array_equal(hip.open_fk_poly_batch(srs, la, ra, *ca[2:]), first_a)
        for h in (other, hip, other):
            assert np.array_equal(h.open_fk_poly_batch(srs, la, ra, *ca[2:]), first_a)
            assert np.array_equal(h.open_fk_poly(srs, la, np.ascontiguousarray(ra[0]), *ca[2:]), first_a[0])
            com, pr = h.vec_commit_batch(srs, rb, lb, *cb)
            assert np.array_equal(com, first_b[0]) and np.array_equal(pr, first_b[1])
    finally:
        other.close()
        srs.free()


def test_errors_and_empty_calls(oc, hip, base):
    lib, srs = hip.lib, base["plain"]
    log2d = 3
    rows = rows_of(oc, rand_fr_ints(16, 3), 2, 8)
    k = consts(oc, log2d)
    out, com = np.full((2, 8, 8), 7, np.uint64), np.full((2, 12), 7, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.keaki_hip_last_error(hip.ctx).decode()

    def open_(srs_h=srs.handle, l=log2d, r=rows, m=2, stride=8, w=k[2], wi=k[3], inv=k[4], o=out, fn=lib.keaki_hip_open_fk_poly_batch):
        return fn(hip.ctx, srs_h, l, p(r), m, stride, p(w), p(wi), p(inv), p(o))

    def vec_(srs_h=srs.handle, r=rows, n=8, m=2, stride=8, l=log2d, c=k, cm=com, o=out, fn=lib.keaki_hip_vec_commit_batch):
        return fn(hip.ctx, srs_h, p(r), n, m, stride, l, p(c[0]), p(c[1]), p(c[2]), p(c[3]), p(c[4]), p(cm), p(o))

    for dev in (False, True):
        fo = lib.keaki_hip_open_fk_poly_batch_dev if dev else lib.keaki_hip_open_fk_poly_batch
        fv = lib.keaki_hip_vec_commit_batch_dev if dev else lib.keaki_hip_vec_commit_batch
        for bad in (dict(srs_h=None), dict(r=None), dict(w=None), dict(wi=None), dict(inv=None), dict(o=None), dict(stride=7), dict(l=28),
                    dict(l=4, m=1 << 27, stride=16)):
            assert open_(fn=fo, **bad) == ERR_BAD_ARG and "open_fk_poly_batch" in err(), bad
        for bad in (dict(srs_h=None), dict(r=None), dict(c=[None] + k[1:]), dict(c=k[:1] + [None] + k[2:]), dict(c=k[:4] + [None]), dict(cm=None),
                    dict(o=None), dict(stride=7), dict(n=9, stride=9), dict(l=28), dict(l=4, m=1 << 27)):
            assert vec_(fn=fv, **bad) == ERR_BAD_ARG and "vec_commit_batch" in err(), bad
        # d > len(srs): what the single call answers
        assert open_(fn=fo, l=10, stride=1024) == ERR_TOO_LARGE and vec_(fn=fv, l=10) == ERR_TOO_LARGE
        assert lib.keaki_hip_open_fk_poly(hip.ctx, srs.handle, 10, p(rows), p(k[2]), p(k[3]), p(k[4]), p(out)) == ERR_TOO_LARGE
        # m = 0 writes nothing
        assert open_(fn=fo, m=0, r=None, o=None) == 0 and vec_(fn=fv, m=0, r=None, cm=None, o=None) == 0
    assert (out == 7).all() and (com == 7).all(), "a refused call writes nothing"
    # n = 0 needs no rows
    assert vec_(r=None, n=0, stride=0) == 0 and not out.any() and not com[:, 8:].any()


@pytest.mark.parametrize("form", ["private", "torch"])
def test_dev_forms_are_queued_work(oc, base, form):
    """three _dev calls of changing size on the stream without a synchronisation between them (the second grows both workspaces behind the
    first), one at the end; device buffers are torch tensors on the context's stream (private stream: the caller synchronises around the queue)"""
    import torch
    from keaki_amd.hip import KeakiHip
    stream = torch.cuda.Stream() if form == "torch" else None
    h = KeakiHip(0, stream=stream.cuda_stream) if stream else KeakiHip(0)
    srs = base["plain"]
    calls = [(3, 5, 9), (6, 65, 64), (2, 2, 4)]                  # (log2d, m, stride)
    try:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
        host = lambda t: t.cpu().numpy().view(np.uint64)
        rows = [rows_of(oc, rand_fr_ints(m << l, 70 + l), m, 1 << l, stride=s) for l, m, s in calls]
        with torch.cuda.stream(stream) if stream else torch.cuda.stream(torch.cuda.current_stream()):
            d_rows = [dev(r) for r in rows]
            d_open = [torch.full((m << l, 8), -1, dtype=torch.int64, device="cuda:0") for l, m, _ in calls]
            d_pr = [torch.full((m << l, 8), -1, dtype=torch.int64, device="cuda:0") for l, m, _ in calls]
            d_com = [torch.full((m, 12), -1, dtype=torch.int64, device="cuda:0") for _, m, _ in calls]
            if not stream:
                torch.cuda.synchronize()
            for j, (l, m, s) in enumerate(calls):
                c = consts(oc, l)
                h.open_fk_poly_batch_dev(srs, l, d_rows[j].data_ptr(), m, s, *c[2:], d_open[j].data_ptr())
                h.vec_commit_batch_dev(srs, d_rows[j].data_ptr(), 1 << l, m, s, l, *c, d_com[j].data_ptr(), d_pr[j].data_ptr())
            h.synchronize()
        for j, (l, m, s) in enumerate(calls):
            c = consts(oc, l)
            assert np.array_equal(host(d_open[j]).reshape(m, 1 << l, 8), h.open_fk_poly_batch(srs, l, rows[j], *c[2:])), calls[j]
            com, pr = h.vec_commit_batch(srs, rows[j], l, *c, n=1 << l)
            assert np.array_equal(host(d_pr[j]).reshape(m, 1 << l, 8), pr) and np.array_equal(host(d_com[j]), com), calls[j]
    finally:
        h.close()


def test_host_mirror_vec_commit_batch(oc):
    """keaki::vec::vec_commit_batch of the C++ mirror: one padding scalar per vector in index order, so the same rng seed gives what a loop of
    vec_commit gives when every vector's own domain is the batch's"""
    import keaki_amd.keaki as K
    dev = K.Device(0)
    st = K.KZGSetup.setup(mont(oc, [S.secrets()["random"]])[0], 32, device=dev)
    try:
        vecs = [mont(oc, rand_fr_ints(n, 800 + n)) for n in (31, 17, 20, 16)]           # 17 .. 32 evaluations with the padding: the domain of 32
        com, proofs = K.vec_commit_batch(K.Rng(11), st, vecs)
        rng = K.Rng(11)
        for j, v in enumerate(vecs):
            c1, p1 = K.vec_commit(rng, st, v)
            assert np.array_equal(com[j], c1) and np.array_equal(proofs[j], p1), j
    finally:
        st.close()
        dev.close()
