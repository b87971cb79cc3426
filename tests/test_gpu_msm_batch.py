"""Batched commit / open through the C ABI (keaki_hip_msm_g1_batch*, keaki_hip_kzg_open_batch*): every row bit-exact against the oracle's MSM,
against (sum s_i tau^i) G on structured SRS, and against the single calls keaki_hip_msm_g1 / keaki_hip_kzg_open row by row. The adversarial
rows and the route (batch kernels or row-by-row fallback) come from tests/msm_batch_model.py."""
import ctypes as C
import os

import numpy as np
import pytest

import msm_batch_model as M
import structured_inputs as S
from conftest_helpers import rand_fr_ints
from test_gpu_fk_shard import DevMem
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = M.R
TH = min(16, os.cpu_count() or 1)
NB = M.N_BATCH_MAX
N_MAX = 1000
ERR_BAD_ARG, ERR_OOM, ERR_TOO_LARGE = -1, -3, -5


def _aff_rows(jac):
    return np.stack([jac_to_aff(row) for row in jac])


@pytest.fixture(scope="module")
def base(oc, hip):
    """1,000 unrelated points, the same SRS with and without window tables"""
    g1, _ = oc.generators()
    pts = hip.g1_mul_batch(g1, mont(oc, rand_fr_ints(N_MAX, 4242)))
    plain, tabled = hip.srs_g1_upload(pts), hip.srs_g1_upload(pts)
    hip.srs_g1_precompute(tabled)
    yield {"pts": pts, "plain": plain, "tabled": tabled}
    plain.free()
    tabled.free()


@pytest.fixture(scope="module")
def structured(oc, hip):
    """SRS tau^i G of N_BATCH_MAX + 1 points for tau = 1, -1 and a random secret (points made on the device)"""
    g1, _ = oc.generators()
    out = {}
    for name in ("one", "minus_one", "random"):
        tau = S.secrets()[name]
        dl = S.powers(tau, NB + 1)
        out[name] = (dl, hip.srs_g1_upload(hip.g1_mul_batch(g1, mont(oc, dl))))
    yield out
    for _, srs in out.values():
        srs.free()


def _rows(oc, m, n, seed, stride=None):
    """(m, stride, 4) Montgomery rows; the gap behind the n scalars of a row is garbage (all bits set: not even a field element)"""
    stride = n if stride is None else stride
    ints = rand_fr_ints(m * n, seed)
    if m * n >= 3:
        ints[0], ints[1], ints[-1] = 0, R - 1, 1
    rows = np.full((m, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    rows[:, :n] = mont(oc, ints).reshape(m, n, 4)
    return rows


def _point_of(oc, k):
    """k * G as the affine words of the ABI ((0, 0) for the identity)"""
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, [k % R]), threads=1)[0]


SHAPES = [(m, n) for m in (1, 2, 3, 65, 257) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000) if m * n <= 70000]


@pytest.mark.parametrize("m,n", SHAPES)
def test_batch_equals_oracle(oc, hip, base, m, n):
    assert M.route(n, m) == "batch"
    rows = _rows(oc, m, n, 100 * m + n)
    got = _aff_rows(hip.msm_g1_batch(base["plain"], rows))
    for j in range(m):
        assert np.array_equal(got[j], oc.msm_g1(base["pts"][:n], rows[j], threads=TH)), "row %d of (m, n) = (%d, %d)" % (j, m, n)


@pytest.mark.parametrize("n", [1, 65, 257, 1000])
def test_rows_are_independent_and_tables_do_not_matter(oc, hip, base, n):
    """every out[j] is keaki_hip_msm_g1 of row j alone, byte for byte (normalised Jacobian), with window tables and without; the garbage in the
    gap of stride > n is not read"""
    m = 5
    rows = _rows(oc, m, n, 900 + n, stride=n + 3)
    for srs in (base["plain"], base["tabled"]):
        got = hip.msm_g1_batch(srs, rows, n=n)
        for j in range(m):
            assert np.array_equal(got[j], hip.msm_g1(srs, np.ascontiguousarray(rows[j, :n])))


def test_boundary_pair_straddles_the_fallback(oc, hip, structured):
    """n = N_BATCH_MAX runs the batch kernels, N_BATCH_MAX + 1 the single-MSM pipeline row by row: both are (sum s_i tau^i) G"""
    dl, srs = structured["random"]
    for n in (NB, NB + 1):
        assert M.route(n, 2) == ("batch" if n == NB else "fallback")
        ints = rand_fr_ints(2 * n, 31 + n)
        got = _aff_rows(hip.msm_g1_batch(srs, mont(oc, ints).reshape(2, n, 4)))
        for j in range(2):
            assert np.array_equal(got[j], _point_of(oc, S.msm_dlog(dl, ints[j * n:(j + 1) * n]))), "n = %d row %d" % (n, j)


@pytest.mark.parametrize("secret", ["one", "minus_one"])
@pytest.mark.parametrize("n", [65, 257, 2500])
def test_adversarial_rows_side_by_side(oc, hip, structured, secret, n):
    """zero row, n equal scalars, r - 1 everywhere and a random row in ONE batch, on SRS where every point is G (the doubling branch) and
    +-G (cancellation to the identity inside a bucket and in the reduction): msm_batch_model counts those events for exactly these rows"""
    dl, srs = structured[secret]
    rows = M.adversarial_rows(n, rand_fr_ints(n, 5 + n))
    if n == 65:
        ev = M.Events()
        for row in rows:
            M.msm_row(dl[:n], row, ev)
        assert ev.get("bucket_equal" if secret == "one" else "bucket_opposite", 0) > 0
    got = hip.msm_g1_batch(srs, mont(oc, [v for row in rows for v in row]).reshape(4, n, 4))
    aff = _aff_rows(got)
    for j, row in enumerate(rows):
        assert np.array_equal(aff[j], _point_of(oc, S.msm_dlog(dl[:n], row))), "row %d" % j
    one = np.array(mont(oc, [1])[0])
    assert not aff[0].any() and not got[0, 8:].any(), "the all-zero row is the identity (R, R, 0)"
    # the ABI's identity: x = y = R (Montgomery one of Fq), z = 0
    assert np.array_equal(got[0, :4], got[0, 4:8]) and got[0, :4].any() and one.any()


def test_state_between_calls(oc, hip, base):
    """m = 65 then m = 3 on the same context (the second call runs in workspaces larger than it needs), a batch after keaki_hip_ctx_trim, and a batch
    under an allocation limit too small for the batch workspace: the route model says fallback and the result does not change"""
    n = 257
    big, small = _rows(oc, 65, n, 1), _rows(oc, 3, n, 2)
    ref_big = hip.msm_g1_batch(base["plain"], big)
    ref_small = hip.msm_g1_batch(base["plain"], small)
    for j in range(3):
        assert np.array_equal(ref_small[j], hip.msm_g1(base["plain"], small[j]))
    hip.trim()
    assert hip.memory()["workspaces"] == 0
    assert np.array_equal(hip.msm_g1_batch(base["plain"], big), ref_big)
    assert hip.memory()["workspaces"] >= 65 * n * 32
    hip.trim()
    # The limit refuses the batch workspace only: the rows are resident (no staging buffer of the host form), and one single MSM of the same length
    # has grown the single-MSM workspaces beforehand, so the fallback's rows run in memory the context already holds.
    hip.msm_g1(base["plain"], big[0])
    mem = DevMem()
    d_rows, d_out = mem.alloc(big.nbytes), mem.alloc(65 * 96)
    mem.put(d_rows, big)
    limit = M.workspace_requests(n, 65)[0] - 1
    assert M.route(n, 65, alloc_limit=limit) == "fallback" and M.route(n, 65) == "batch"
    before = hip.memory()["workspaces"]
    hip.debug_set_alloc_limit(limit)
    try:
        hip.msm_g1_batch_dev(base["plain"], d_rows, n, 65, n, d_out)
        hip.synchronize()
    finally:
        hip.debug_set_alloc_limit(0)
    assert np.array_equal(mem.get(d_out, 65 * 96).view(np.uint64).reshape(65, 12), ref_big)
    assert hip.memory()["workspaces"] == before, "the fallback allocated nothing: the batch workspace was refused, the rows ran in held memory"
    mem.free()
    hip.trim()


def test_errors_and_empty_calls(oc, hip, base):
    lib, srs = hip.lib, base["plain"]
    rows = _rows(oc, 2, 8, 3)
    out = np.full((2, 12), 7, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda fn, *a: fn(hip.ctx, *a)
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, p(rows), N_MAX + 1, 1, N_MAX + 1, p(out)) == ERR_TOO_LARGE
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, p(rows), 8, 2, 7, p(out)) == ERR_BAD_ARG            # stride < n
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, None, 8, 2, 8, p(out)) == ERR_BAD_ARG
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, p(rows), 8, 2, 8, None) == ERR_BAD_ARG
    assert call(lib.keaki_hip_msm_g1_batch, None, p(rows), 8, 2, 8, p(out)) == ERR_BAD_ARG
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, p(rows), 1 << 16, 1 << 15, 1 << 16, p(out)) == ERR_BAD_ARG     # m * n = 2^31
    assert call(lib.keaki_hip_msm_g1_batch_dev, srs.handle, None, 8, 2, 8, None) == ERR_BAD_ARG
    assert call(lib.keaki_hip_kzg_open_batch, srs.handle, p(rows), N_MAX + 2, 1, N_MAX + 2, p(rows), p(out), None) == ERR_TOO_LARGE
    assert call(lib.keaki_hip_kzg_open_batch, srs.handle, p(rows), 8, 2, 7, p(rows), p(out), None) == ERR_BAD_ARG
    assert call(lib.keaki_hip_kzg_open_batch, srs.handle, p(rows), 8, 2, 8, None, p(out), None) == ERR_BAD_ARG
    assert call(lib.keaki_hip_kzg_open_batch_dev, srs.handle, None, 8, 2, 8, None, None, None) == ERR_BAD_ARG
    assert (out == 7).all(), "a refused call writes nothing"
    # m = 0 writes nothing; n = 0 writes m identities
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, None, 8, 0, 8, None) == 0
    assert call(lib.keaki_hip_kzg_open_batch, srs.handle, None, 8, 0, 8, None, None, None) == 0
    assert (out == 7).all()
    assert call(lib.keaki_hip_msm_g1_batch, srs.handle, None, 0, 2, 0, p(out)) == 0
    ident = hip.msm_g1(srs, np.zeros((0, 4), np.uint64))
    assert np.array_equal(out[0], ident) and np.array_equal(out[1], ident)
    vals = np.full((2, 4), 7, np.uint64)
    out[:] = 7
    assert call(lib.keaki_hip_kzg_open_batch, srs.handle, None, 0, 2, 0, p(rows), p(out), p(vals)) == 0
    assert np.array_equal(out[0], ident) and np.array_equal(out[1], ident) and not vals.any()


def test_dev_form_is_queued_work(oc, hip, base):
    """two batch calls and a single keaki_hip_msm_g1_dev on the ctx stream without a synchronisation between them, one at the end"""
    srs, mem = base["plain"], DevMem()
    a, b, s = _rows(oc, 65, 257, 11), _rows(oc, 3, 1000, 12, stride=1001), _rows(oc, 1, 1000, 13)
    d = {k: mem.alloc(v.nbytes) for k, v in (("a", a), ("b", b), ("s", s))}
    for k, v in (("a", a), ("b", b), ("s", s)):
        mem.put(d[k], v)
    o = {"a": mem.alloc(65 * 96), "b": mem.alloc(3 * 96), "s": mem.alloc(96)}
    hip.synchronize()
    hip.msm_g1_batch_dev(srs, d["a"], 257, 65, 257, o["a"])
    hip.msm_g1_dev(srs, d["s"], 1000, o["s"])
    hip.msm_g1_batch_dev(srs, d["b"], 1000, 3, 1001, o["b"])
    hip.synchronize()
    got = {k: mem.get(o[k], sz).view(np.uint64).reshape(-1, 12) for k, sz in (("a", 65 * 96), ("b", 3 * 96), ("s", 96))}
    assert np.array_equal(got["a"], hip.msm_g1_batch(srs, a))
    assert np.array_equal(got["b"], hip.msm_g1_batch(srs, b, n=1000))
    assert np.array_equal(got["s"][0], hip.msm_g1(srs, s[0]))
    for j in (0, 64):
        assert np.array_equal(jac_to_aff(got["a"][j]), oc.msm_g1(base["pts"][:257], a[j], threads=TH))
    mem.free()


OPEN_SHAPES = [(m, n) for m in (1, 3, 65) for n in (1, 2, 33, 257, 1000)]


@pytest.mark.parametrize("m,n", OPEN_SHAPES)
def test_open_batch_equals_open_row_by_row(oc, hip, base, m, n):
    """values and proofs of keaki_hip_kzg_open for every row; row 0 is opened at a root of the polynomial (value 0), the last row is constant
    (proof = identity)"""
    ints = rand_fr_ints(m * n, 77 * m + n)
    zs = rand_fr_ints(m, 78 * m + n)
    if n >= 2:                                              # row 0 := (x - z_0) * (rest): p(z_0) = 0
        rest = ints[:n - 1]
        row0 = [0] * n
        for i, c in enumerate(rest):
            row0[i] = (row0[i] - zs[0] * c) % R
            row0[i + 1] = (row0[i + 1] + c) % R
        ints[:n] = row0
    if m > 1:
        ints[(m - 1) * n + 1:m * n] = [0] * (n - 1)              # last row: constant (with m = 1 the one row is constant only at n = 1)
    rows = mont(oc, ints).reshape(m, n, 4)
    z = mont(oc, zs)
    for srs in (base["plain"], base["tabled"]):
        proofs, values = hip.kzg_open_batch(srs, rows, z)
        for j in range(m):
            pr, val = hip.kzg_open(srs, np.ascontiguousarray(rows[j]), z[j])
            assert np.array_equal(proofs[j], pr) and np.array_equal(values[j], val), "row %d" % j
    if n >= 2:
        assert not values[0].any(), "opened at a root"
    if m > 1 or n == 1:
        assert not proofs[m - 1, 8:].any(), "constant row: the proof is the identity"
        assert np.array_equal(values[m - 1], rows[m - 1, 0])


def test_commit_open_verify_end_to_end(oc, hip, base):
    """commit_batch -> open_batch -> keaki_hip_kzg_verify_batch(com_stride = 1) on an SRS with a known secret accepts; one altered value rejects"""
    g1, g2 = oc.generators()
    tau, m, n = S.secrets()["random"], 9, 33
    pts = hip.g1_mul_batch(g1, mont(oc, S.powers(tau, n)))
    tau_g2 = hip.g2_mul_batch(g2, mont(oc, [tau]))[0]
    srs = hip.srs_g1_upload(pts)
    try:
        rows = _rows(oc, m, n, 500)
        z, gammas = mont(oc, rand_fr_ints(m, 501)), mont(oc, rand_fr_ints(m, 502))
        coms = _aff_rows(hip.msm_g1_batch(srs, rows))
        proofs, values = hip.kzg_open_batch(srs, rows, z)
        ok, _, _ = hip.kzg_verify_batch(coms, tau_g2, z, values, _aff_rows(proofs), gammas)
        assert ok
        bad = values.copy()
        bad[4] = mont(oc, [12345])[0]
        ok, _, _ = hip.kzg_verify_batch(coms, tau_g2, z, bad, _aff_rows(proofs), gammas)
        assert not ok
    finally:
        srs.free()
