"""The batched commit / open on every window plan, pass split and route (keaki_amd/csrc/msm_batch.hip, open_batch_core in api.hip). The shapes
are the case table GPU_CASES of tests/msm_batch_model.py; tests/test_msm_batch_model.py proves on the CPU that the table covers every window
width and both sides of every width boundary, both inner pass splits, the halving outer loop of open, both routes, and -- for the adversarial
rows of every width -- the exceptional additions of the bucket loop, the tree and the close.

Every base has a known discrete log, so every expected point is (a scalar computed in Python or by the oracle's dot product) * G, made by ONE
oracle g1_mul_batch per test; everything is bit for bit."""
import os

import numpy as np
import pytest

import msm_batch_model as M
import structured_inputs as S
from conftest_helpers import rand_fr_ints
from test_gpu_fk_shard import DevMem
from test_gpu_msm_batch import _rows, structured      # noqa: F401 (structured is a fixture)
from test_gpu_parity import mont

pytestmark = pytest.mark.gpu
R = M.R
TH = min(16, os.cpu_count() or 1)
NB = M.N_BATCH_MAX
N_KNOWN = 2500
GARBAGE = 0xFFFFFFFFFFFFFFFF


def _ids(cases):
    return [k[0] for k in cases]


def _points(oc, dlogs):
    """dlogs[j] * G as affine words, (0, 0) for the identity: one oracle call"""
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, [k % R for k in dlogs]), threads=TH)


def _aff(jac):
    """(m, 12) normalised Jacobian -> (m, 8) affine words, zeros for the identity"""
    jac = np.asarray(jac).reshape(-1, 12)
    return jac[:, :8] * jac[:, 8:].any(axis=1).astype(np.uint64)[:, None]


def _strided(oc, rows, stride):
    """rows: m lists of n integers -> (m, stride, 4) Montgomery, all bits set behind the n scalars of a row (not even a field element)"""
    m, n = len(rows), len(rows[0])
    out = np.full((m, stride, 4), GARBAGE, np.uint64)
    out[:, :n] = mont(oc, [v % R for row in rows for v in row]).reshape(m, n, 4)
    return out


@pytest.fixture(scope="module")
def known(oc, hip):
    """2,500 unrelated points k_i G with the k_i on record (made on the device, spot-checked against the oracle)"""
    g1, _ = oc.generators()
    dl = rand_fr_ints(N_KNOWN, 4243)
    pts = hip.g1_mul_batch(g1, mont(oc, dl))
    idx = list(range(0, N_KNOWN, 97))
    assert np.array_equal(pts[idx], _points(oc, [dl[i] for i in idx]))
    srs = hip.srs_g1_upload(pts)
    yield {"dl": dl, "pts": pts, "srs": srs}
    srs.free()


@pytest.fixture(scope="module")
def ident(hip, known):
    """the ABI's identity as keaki_hip_msm_g1 writes it: x = y = Montgomery one of Fq, z = 0"""
    out = hip.msm_g1(known["srs"], np.zeros((0, 4), np.uint64))
    assert np.array_equal(out[:4], out[4:8]) and out[:4].any() and not out[8:].any()
    return out


# ---- every plan, both sides of every width boundary --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.cases_of("plan"), ids=_ids(M.cases_of("plan")))
def test_every_plan_and_boundary(oc, hip, known, case):
    """m = 3 rows of stride n + 3 over unrelated points: the edge scalars of the width at the front of row 0 and at the end of row 1, row 2
    random. Every row is (sum s_i k_i) G; row 2 is also the oracle's MSM over the points and row 0 the bytes of keaki_hip_msm_g1."""
    _, _, n, m, stride, _, _, _ = case
    assert stride == n + 3 and M.route(n, m) == "batch"
    edge = M.edge_scalars(n)
    ints = [rand_fr_ints(n, 3000 + 7 * n + j) for j in range(m)]
    ints[0][:len(edge)] = edge
    ints[1][-len(edge):] = edge
    rows = _strided(oc, ints, stride)
    got = hip.msm_g1_batch(known["srs"], rows, n=n)
    exp = _points(oc, [S.msm_dlog(known["dl"][:n], row) for row in ints])
    assert np.array_equal(_aff(got), exp), "rows %s" % [j for j in range(m) if not np.array_equal(_aff(got[j])[0], exp[j])]
    assert np.array_equal(exp[2], oc.msm_g1(known["pts"][:n], np.ascontiguousarray(rows[2, :n]), threads=TH))
    assert np.array_equal(got[0], hip.msm_g1(known["srs"], np.ascontiguousarray(rows[0, :n])))


# ---- exceptional additions at every width ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.cases_of("branches"), ids=_ids(M.cases_of("branches")))
def test_branch_rows_at_every_width(oc, hip, structured, ident, case):
    """msm_batch_model.branch_rows on the SRS of equal points (tau = 1) and of alternating +-G (tau = -1): the CPU test proves that these rows
    meet equal operands, opposite operands and an identity accumulator in the bucket loop, and equal and opposite operands at the first and
    at the last level of the tree, at this width"""
    _, _, n, m, _, secret, _, _ = case
    dl, srs = structured[secret]
    rows = M.branch_rows(n, rand_fr_ints(n, 5 + n))
    assert len(rows) == m
    got = hip.msm_g1_batch(srs, _strided(oc, rows, n))
    exp = _points(oc, [S.msm_dlog(dl[:n], row) for row in rows])
    for j in range(m):
        assert np.array_equal(_aff(got[j])[0], exp[j]), "row %d" % j
    assert np.array_equal(got[0], ident), "the all-zero row is the ABI's identity"


# ---- identity points in the SRS -------------------------------------------------------------------------------------------------------------
def _holes(n, mixed, kind):
    """indices of the identity points: the first, the last, a run, and every index whose digit of the mixed row lands in bucket 2 of window 1
    (that lane has entries and stays empty); the SRS of tau = 0 is G followed by identities"""
    if kind == "zero":
        return list(range(1, n))
    ct = M.window_bits(n)
    lane = [i for i in range(n) if abs(M.digits(mixed[i], ct)[1]) == 3]
    assert len(lane) >= 2
    return sorted({0, n - 1, 10, 11, 12, 13} | set(lane))


@pytest.mark.parametrize("case", M.cases_of("identity_points"), ids=_ids(M.cases_of("identity_points")))
def test_identity_points_in_the_srs(oc, hip, ident, case):
    """rows over an SRS that holds the identity: a row whose only non-zero scalars sit on identity points (result: the identity), a mixed
    row, the all-ones row and r - 1 on two identity points. Every row is its discrete-log point and the bytes of keaki_hip_msm_g1."""
    _, _, n, m, _, kind, _, _ = case
    mixed = rand_fr_ints(n, 8100 + n)
    holes = _holes(n, mixed, kind)
    dl = [1] + [0] * (n - 1) if kind == "zero" else rand_fr_ints(n, 8200 + n)
    for i in holes:
        dl[i] = 0
    pts = _points(oc, dl)
    assert not pts[holes].any() and pts[[i for i in range(n) if i not in set(holes)]].any(axis=1).all()
    only = [0] * n
    for i, v in zip(holes, rand_fr_ints(len(holes), 8300 + n)):
        only[i] = v or 1
    two = [0] * n
    two[holes[0]] = two[holes[-1]] = R - 1
    rows = [only, mixed, [1] * n, two]
    assert len(rows) == m
    srs = hip.srs_g1_upload(pts)
    try:
        mrows = _strided(oc, rows, n)
        got = hip.msm_g1_batch(srs, mrows)
        exp = _points(oc, [S.msm_dlog(dl, row) for row in rows])
        for j in range(m):
            assert np.array_equal(_aff(got[j])[0], exp[j]), "row %d" % j
            assert np.array_equal(got[j], hip.msm_g1(srs, mrows[j])), "row %d against the single call" % j
        assert np.array_equal(got[0], ident) and np.array_equal(got[3], ident) and exp[1].any()
    finally:
        srs.free()


# ---- inner pass split -----------------------------------------------------------------------------------------------------------------------
_ROWS_MAX_REF = {}


def _rows_max_ref(oc, dl, n, m):
    """the rows of the ROWS_MAX cases and their expected points, made once per n"""
    if n not in _ROWS_MAX_REF:
        ints = rand_fr_ints(m * n, 9100 + n)
        ints[0], ints[-1] = 0, R - 1
        rows = [ints[j * n:(j + 1) * n] for j in range(m)]
        _ROWS_MAX_REF[n] = (rows, _points(oc, [S.msm_dlog(dl[:n], row) for row in rows]))
    return _ROWS_MAX_REF[n]


@pytest.mark.parametrize("case", M.cases_of("rows_max"), ids=_ids(M.cases_of("rows_max")))
def test_second_pass_by_rows_max(oc, hip, structured, case):
    """m = ROWS_MAX + 1 rows: the second pass of msm_g1_batch_run holds the last row (scalars at r0 * stride, results at out + 3 * r0). The host
    form at stride = n, the device form at stride = n + 1 with garbage in the gap; every row is checked."""
    _, _, n, m, stride, _, _, _ = case
    assert M.inner_passes(n, m) == [M.ROWS_MAX, 1]
    dl, srs = structured["random"]
    ints, exp = _rows_max_ref(oc, dl, n, m)
    rows = _strided(oc, ints, stride)
    if stride == n:
        got = hip.msm_g1_batch(srs, rows)
    else:
        mem = DevMem()
        try:
            d_rows, d_out = mem.alloc(rows.nbytes), mem.alloc(m * 96)
            mem.put(d_rows, rows)
            hip.msm_g1_batch_dev(srs, d_rows, n, m, stride, d_out)
            hip.synchronize()
            got = mem.get(d_out, m * 96).view(np.uint64).reshape(m, 12)
        finally:
            mem.free()
    bad = np.flatnonzero((_aff(got) != exp).any(axis=1))
    assert bad.size == 0, "%d rows differ, the first at %d" % (bad.size, bad[0])
    for j in (0, M.ROWS_MAX - 1, M.ROWS_MAX):
        assert np.array_equal(got[j], hip.msm_g1(srs, np.ascontiguousarray(rows[j, :n]))), "row %d against the single call" % j
    hip.trim()


def test_second_pass_by_canon_bytes(oc, hip, structured):
    """513 rows of N_BATCH_MAX scalars are 2^28 + 2^19 bytes of canonical scalars: 512 rows, then one. MSM_BATCH_CANON_BYTES fixes the size,
    no smaller shape takes this pass. Row j must be <s_j, tau^i> G with the dot product from the oracle."""
    _, _, n, m, _, _, _, _ = M.case("canon_bytes")
    assert M.inner_passes(n, m) == [m - 1, 1] and (m - 1) * n * 32 == M.CANON_BYTES
    dl, srs = structured["random"]
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 2**63, size=(m, n, 4), dtype=np.int64).astype(np.uint64)
    rows[:, :, 3] &= np.uint64((1 << 60) - 1)                    # < 2^252 < r: valid Montgomery residues
    k = mont(oc, dl[:n])
    g1, _ = oc.generators()
    exp = oc.g1_mul_batch(g1, np.stack([oc.fr_dot(rows[j], k).reshape(4) for j in range(m)]), threads=TH)
    try:
        got = hip.msm_g1_batch(srs, rows)
    finally:
        hip.trim()
    bad = np.flatnonzero((_aff(got) != exp).any(axis=1))
    assert bad.size == 0, "%d rows differ, the first at %d" % (bad.size, bad[0])


# ---- open: the outer loop under an allocation limit -------------------------------------------------------------------------------------------
def _open_inputs(oc, m, n, stride, seed):
    rows = _rows(oc, m, n, seed, stride=stride)
    return rows, mont(oc, rand_fr_ints(m, seed + 1))


class _OpenDev:
    """device buffers of one keaki_hip_kzg_open_batch_dev call; the result buffers are preset to 7s"""

    def __init__(self, mem, rows, z):
        self.mem, self.m = mem, rows.shape[0]
        self.rows, self.z = mem.alloc(rows.nbytes), mem.alloc(z.nbytes)
        self.proofs, self.values = mem.alloc(self.m * 96 + 96), mem.alloc(self.m * 32)
        mem.put(self.rows, rows)
        mem.put(self.z, z)
        mem.put(self.proofs, np.full(self.m * 12 + 12, 7, np.uint64))
        mem.put(self.values, np.full(self.m * 4, 7, np.uint64))

    def get(self):
        p = self.mem.get(self.proofs, self.m * 96 + 96).view(np.uint64)
        assert (p[self.m * 12:] == 7).all(), "nothing is written behind proof m - 1"
        return p[:self.m * 12].reshape(self.m, 12), self.mem.get(self.values, self.m * 32).view(np.uint64).reshape(self.m, 4)


@pytest.mark.parametrize("cid", ["open_halving", "open_fallback"])
def test_open_outer_loop_under_an_allocation_limit(oc, hip, known, cid):
    """open_halving: the limit admits 17 quotient rows, not 33 -- the rows halve 65 -> 33 -> 17 and four outer passes (17, 17, 17, 14) run the
    batch kernels. open_fallback: the limit admits the quotient and canonical rows of 65 short polynomials but not their window sums -- one
    outer pass whose MSMs run row by row in the workspaces a single MSM has grown beforehand. Both give the bytes of the unlimited call and
    of keaki_hip_kzg_open row by row, and leave exactly the workspaces the model predicts."""
    case = M.case(cid)
    _, _, n, m, stride, _, _, limit = case
    reach = M.reach(case)
    srs = known["srs"]
    rows, z = _open_inputs(oc, m, n, stride, 600 + n)
    ref_p, ref_v = hip.kzg_open_batch(srs, rows, z)
    for j in range(m):
        pr, val = hip.kzg_open(srs, np.ascontiguousarray(rows[j, :n]), z[j])
        assert np.array_equal(ref_p[j], pr) and np.array_equal(ref_v[j], val), "row %d" % j
    hip.trim()
    if "fallback" in reach["routes"]:
        hip.msm_g1(srs, np.ascontiguousarray(rows[0, :n - 1]))        # the fallback's rows run in memory the context already holds
    before = hip.memory()["workspaces"]
    mem = DevMem()
    try:
        dev = _OpenDev(mem, rows, z)
        hip.debug_set_alloc_limit(limit)
        try:
            hip.kzg_open_batch_dev(srs, dev.rows, n, m, stride, dev.z, dev.proofs, dev.values)
            hip.synchronize()
        finally:
            hip.debug_set_alloc_limit(0)
        got_p, got_v = dev.get()
        after = hip.memory()["workspaces"]
    finally:
        mem.free()
        hip.trim()
    assert np.array_equal(got_p, ref_p) and np.array_equal(got_v, ref_v)
    assert after - before == sum(reach["held"]), "the workspaces of the route the model predicts: %s" % (reach,)
    assert after - before != sum(M.open_rows(n - 1, m)["held"]), "and not those of the unlimited call"


# ---- open: the device form ---------------------------------------------------------------------------------------------------------------------
def test_open_dev_surface(oc, hip, known):
    """keaki_hip_kzg_open_batch_dev doing work: stride = n + 5 with garbage in the gap, d_values = NULL (the proofs do not change, the inputs
    are not written), and two open-batch calls with one MSM of an open's size queued without a synchronisation between them"""
    _, _, n, m, stride, _, _, _ = M.case("open_dev[stride]")
    assert stride == n + 5
    srs = known["srs"]
    rows, z = _open_inputs(oc, m, n, stride, 700)
    rows2, z2 = _open_inputs(oc, 2, 200, 200, 710)
    sc = np.ascontiguousarray(_rows(oc, 1, n - 1, 720)[0])
    ref_p, ref_v = hip.kzg_open_batch(srs, np.ascontiguousarray(rows[:, :n]), z)
    for j in range(m):
        pr, val = hip.kzg_open(srs, np.ascontiguousarray(rows[j, :n]), z[j])
        assert np.array_equal(ref_p[j], pr) and np.array_equal(ref_v[j], val), "row %d" % j
    ref2_p, ref2_v = hip.kzg_open_batch(srs, rows2, z2)
    ref_s = hip.msm_g1(srs, sc)
    mem = DevMem()
    try:
        a, a_null, b = _OpenDev(mem, rows, z), _OpenDev(mem, rows, z), _OpenDev(mem, rows2, z2)
        d_sc, d_s = mem.alloc(sc.nbytes), mem.alloc(96)
        mem.put(d_sc, sc)
        hip.synchronize()
        hip.kzg_open_batch_dev(srs, a.rows, n, m, stride, a.z, a.proofs, a.values)
        hip.msm_g1_dev(srs, d_sc, n - 1, d_s)
        hip.kzg_open_batch_dev(srs, b.rows, 200, 2, 200, b.z, b.proofs, b.values)
        hip.kzg_open_batch_dev(srs, a_null.rows, n, m, stride, a_null.z, a_null.proofs, 0)
        hip.synchronize()
        for dev, p, v in ((a, ref_p, ref_v), (b, ref2_p, ref2_v)):
            got_p, got_v = dev.get()
            assert np.array_equal(got_p, p) and np.array_equal(got_v, v)
        got_p, got_v = a_null.get()
        assert np.array_equal(got_p, ref_p) and (got_v == 7).all(), "d_values = NULL: the proofs alone"
        assert np.array_equal(mem.get(d_s, 96).view(np.uint64), ref_s)
        assert np.array_equal(mem.get(a_null.rows, rows.nbytes).view(np.uint64), rows.reshape(-1)), "the coefficients are read only"
        assert np.array_equal(mem.get(a_null.z, z.nbytes).view(np.uint64), z.reshape(-1))
    finally:
        mem.free()


# ---- open across N_BATCH_MAX -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.cases_of("open_route"), ids=_ids(M.cases_of("open_route")))
def test_open_straddles_the_fallback(oc, hip, structured, case):
    """quotients of N_BATCH_MAX coefficients run the batch kernels, of N_BATCH_MAX + 1 the single-MSM pipeline row by row: both proofs are
    q(tau) G and both values p(z)"""
    _, _, n, m, _, _, _, _ = case
    assert M.reach(case)["routes"] == ["batch" if n - 1 <= NB else "fallback"]
    tau = S.secrets()["random"]
    dl, srs = structured["random"]
    assert len(dl) >= n - 1
    ints, zs = rand_fr_ints(m * n, 41 + n), rand_fr_ints(m, 42 + n)
    polys = [ints[j * n:(j + 1) * n] for j in range(m)]
    proofs, values = hip.kzg_open_batch(srs, mont(oc, ints).reshape(m, n, 4), mont(oc, zs))
    assert np.array_equal(_aff(proofs), _points(oc, [S.open_dlog(tau, p, z) for p, z in zip(polys, zs)]))
    assert np.array_equal(values, mont(oc, [S.poly_eval(p, z) for p, z in zip(polys, zs)]))
    hip.trim()


# ---- the quotient's segments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.cases_of("quotient"), ids=_ids(M.cases_of("quotient")))
def test_quotient_segment_edges(oc, hip, structured, case):
    """k_fr_quotient_batch cuts a row into 256 segments of L = ceil(n / 256): n = 255 / 256 (L = 1, the last lane idle / busy), 512 / 513 (the
    step to L = 3 with a ragged tail and idle lanes). Row 0 is opened at z = 0 (z^L = 0: every carry vanishes), row 1 at z = 1, row 2 at a
    random point; proofs are q(tau) G, values p(z), both also the bytes of keaki_hip_kzg_open."""
    _, _, n, m, _, _, _, _ = case
    tau = S.secrets()["random"]
    dl, srs = structured["random"]
    ints = rand_fr_ints(m * n, 51 + n)
    zs = [0, 1] + rand_fr_ints(m - 2, 52 + n)
    polys = [ints[j * n:(j + 1) * n] for j in range(m)]
    rows, z = mont(oc, ints).reshape(m, n, 4), mont(oc, zs)
    proofs, values = hip.kzg_open_batch(srs, rows, z)
    assert np.array_equal(_aff(proofs), _points(oc, [S.open_dlog(tau, p, x) for p, x in zip(polys, zs)]))
    assert np.array_equal(values, mont(oc, [S.poly_eval(p, x) for p, x in zip(polys, zs)]))
    assert np.array_equal(values[0], rows[0, 0]), "p(0) is the constant coefficient"
    for j in range(m):
        pr, val = hip.kzg_open(srs, np.ascontiguousarray(rows[j]), z[j])
        assert np.array_equal(proofs[j], pr) and np.array_equal(values[j], val), "row %d" % j
