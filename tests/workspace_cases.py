"""The call table of tests/test_gpu_workspace_poison.py: one row per public entry-point family that reserves a workspace of its context.

Every entry point of the library runs in the grow-only workspaces of keaki_hip_ctx (csrc/internal.h: for_each_scratch). A call must return the same
bytes whatever those buffers held before it; keaki_hip_debug_poison_workspaces makes that testable. A row names the family and the functions of
include/keaki_hip.h it covers, lists one to three shapes (each with the strictly larger shape of the residue step), builds the inputs of a shape,
makes the call, and says where the independent expected value comes from: `expect` compares the baseline with the oracle or a Python model
directly; a row without it names in `reference` the existing test that ties the shape to its reference.

Plain test infrastructure in the style of variant_cases.py and heavy_cases.py: importing it needs no GPU. tests/test_workspace_cases_model.py checks
the table against the header on a CPU: every keaki_hip_* function is in a row or in EXEMPT with its reason."""
import os

import numpy as np

from conftest import rand_fr_ints

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TH = min(16, os.cpu_count() or 1)
POISON_BYTES = (0x00, 0xFF, 0x5A)      # "no entry" and the affine identity | DIGIT_NONE and an all-ones count | a non-canonical field element, a non-zero segment word
ARENA_FILL = 0xC3                      # what surrounds every slice of a _dev call


class Env:
    """the oracle and what the rows share: points made once by the oracle (inputs, never results)"""

    def __init__(self, oc, py):
        self.oc, self.py, self.cache = oc, py, {}

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def mont(self, ints):
        return self.oc.fr_to_mont(self.oc.ints_to_limbs([int(x) % R for x in ints]))

    def unmont(self, a):
        return self.oc.limbs_to_ints(self.oc.fr_from_mont(np.ascontiguousarray(a, np.uint64).reshape(-1, 4)))

    def g1_of(self, dls):
        out = self.oc.g1_mul_batch(self.oc.generators()[0], self.mont(dls), threads=TH).copy()
        for i, x in enumerate(dls):
            if x % R == 0:
                out[i] = 0
        return out

    def g2_of(self, dls):
        out = self.oc.g2_mul_batch(self.oc.generators()[1], self.mont(dls), threads=TH).copy()
        for i, x in enumerate(dls):
            if x % R == 0:
                out[i] = 0
        return out

    def g1_pts(self, n):
        """unrelated G1 points with an identity and a repeated base among them"""
        def make():
            p = self.g1_of(rand_fr_ints(8192, 0x5EED1))
            p[3] = 0; p[300] = 0; p[9] = p[8]
            return p
        return self.once("g1_pts", make)[:n]

    def g2_pts(self, n):
        def make():
            p = self.g2_of(rand_fr_ints(7001, 0x5EED2))
            p[3] = 0; p[9] = p[8]
            return p
        return self.once("g2_pts", make)[:n]

    def tau_srs(self, tau, n1, n2=0):
        """([tau^i]_1 i < n1, [tau^i]_2 i < n2) of a known tau"""
        def make():
            pw = [pow(tau, t, R) for t in range(max(n1, n2))]
            return self.g1_of(pw[:n1]), (self.g2_of(pw[:n2]) if n2 else None)
        return self.once(("tau_srs", tau, n1, n2), make)

    def scalars(self, n, seed):
        """n Fr with a zero and r - 1 mixed in"""
        s = rand_fr_ints(n, seed)
        if n > 2:
            s[1], s[n // 2] = 0, R - 1
        return self.mont(s)


class Case:
    """one prepared call. setup(h) -> state (SRS handles live in state["free"]); run(h, st) -> tuple of arrays / scalars; expect(out): asserts the
    baseline against the independent reference (None: the row's `reference` names the test that does); run_dev(h, st, A) -> the same tuple through
    the _dev form with every input and output a slice of the arena A (None: the family has no _dev form); options: set on every context"""

    def __init__(self, run, setup=None, expect=None, run_dev=None, options=None):
        self.run, self.setup, self.expect, self.run_dev, self.options = run, setup or (lambda h: {"free": []}), expect, run_dev, dict(options or {})


class Row:
    def __init__(self, family, functions, shapes, build, reference):
        """shapes: [(id, params of the call, params of the strictly larger call of the residue step)]"""
        self.family, self.functions, self.shapes, self.build, self.reference = family, tuple("keaki_hip_" + f for f in functions), shapes, build, reference


def jac_to_aff(j):
    """normalised Jacobian -> affine, (0, 0) for the identity; both forms are unique"""
    j = np.asarray(j, np.uint64)
    w = j.shape[-1] // 3
    return np.zeros(2 * w, np.uint64) if not j[2 * w:].any() else j[:2 * w].copy()


def synthetic_division(coeffs, z):
    """(quotient of (p - p(z)) / (x - z), p(z)) by Horner's recurrence Q_i = c_i + z Q_(i+1) in plain integers"""
    q, acc = [0] * max(len(coeffs) - 1, 0), 0
    for i in range(len(coeffs) - 1, -1, -1):
        acc = (acc * z + coeffs[i]) % R
        if i:
            q[i - 1] = acc
    return q, acc


# ---- generic and table MSM -------------------------------------------------------------------------------------------------------------------------
def _msm_build(group):
    g2 = group == "g2"
    words = 24 if g2 else 12

    def build(E, p):
        oc = E.oc
        if p.get("heavy"):
            return _heavy_build(E, p)
        n, tables, host_only = p["n"], p.get("tables", False), p.get("chunks", 0) >= 2
        srs_len = p.get("srs_len", n)
        pts = (E.g2_pts if g2 else E.g1_pts)(srs_len)
        sc = E.scalars(n, 0xA000 + 7 * n + p.get("seed", 0))
        opts = dict(p.get("opts", {}))
        if host_only:
            opts.update(msm_pipe_chunks=p["chunks"], msm_pipe_min=1, msm_pipe_growth=100)

        def setup(h):
            srs = (h.srs_g2_upload if g2 else h.srs_g1_upload)(pts)
            if tables:
                assert (h.srs_g2_precompute if g2 else h.srs_g1_precompute)(srs) > 0
            return {"srs": srs, "free": [srs]}

        def run(h, st):
            return ((h.msm_g2 if g2 else h.msm_g1)(st["srs"], sc),)

        def expect(out):
            assert np.array_equal(jac_to_aff(out[0]), (oc.msm_g2 if g2 else oc.msm_g1)(pts[:n], sc, threads=TH)), "MSM against the oracle"

        def run_dev(h, st, A):
            d_s, d_o = A.put(sc), A.out(8 * words)
            A.ready()
            (h.msm_g2_dev if g2 else h.msm_g1_dev)(st["srs"], d_s, n, d_o)
            h.synchronize()
            return (A.read(d_o, np.uint64, (words,)),)

        return Case(run, setup, expect, None if host_only else run_dev, opts)
    return build


def _heavy_build(E, p):
    """the smallest counts_case of tests/heavy_cases.py (designed buckets around HEAVY_MIN and HEAVY_SLICE among fillers); the larger call of the
    residue step is an ordinary MSM over the same bases and 1,000 more"""
    import heavy_cases as H
    oc = E.oc
    case = min(H.count_cases(), key=lambda c: len(c["scalars"]))
    g2 = case["group"] == "g2"
    extra = 1000 if p.get("larger") else 0

    def make():
        return (E.g2_of if g2 else E.g1_of)(list(case["dlogs"]) + rand_fr_ints(1000, 0x4EA7))
    pts_all = E.once("heavy_pts", make)
    n = len(case["scalars"])
    pts = pts_all[:n + extra]
    sc = E.mont(case["scalars"]) if not extra else E.scalars(n + extra, 0x4EA8)
    opts = {"msm_c_shared" if case["tables"] else "msm_c": case["c"], "acc_u29": case["acc_u29"]}

    def setup(h):
        srs = (h.srs_g2_upload if g2 else h.srs_g1_upload)(pts)
        if case["tables"]:
            (h.srs_g2_precompute if g2 else h.srs_g1_precompute)(srs)
        return {"srs": srs, "free": [srs]}

    def run(h, st):
        return ((h.msm_g2 if g2 else h.msm_g1)(st["srs"], sc),)

    def expect(out):
        k = H.expected_dlog(case)
        assert np.array_equal(jac_to_aff(out[0]), (E.g2_of if g2 else E.g1_of)([k])[0]), case["name"]

    return Case(run, setup, None if extra else expect, None, opts)


def _msm_shapes(group):
    import variant_cases as V
    nxt = {1: 33, 33: 257, 257: 5000, 5000: 7001}
    shapes = []
    for tables in (False, True):
        for n in (1, 33, 257, 5000):
            shapes.append(("n%d-%s" % (n, "tables" if tables else "generic"), {"n": n, "tables": tables}, {"n": nxt[n], "tables": tables, "seed": 1}))
    if group == "g1":
        big = {"n": 7001, "seed": 1}
        shapes.append(("n5000-chunks3", {"n": 5000, "chunks": 3}, dict(big, chunks=3)))           # parked Acc29 state, the heavy list between passes
        shapes.append(("n5000-c16", {"n": 5000, "opts": {"msm_c": 16}}, dict(big, opts={"msm_c": 16})))      # a static tile sort
        shapes.append(("n5000-c12", {"n": 5000, "opts": {"msm_c": 12}}, dict(big, opts={"msm_c": 12})))      # the run-time digit walk
        lbs = V.switch_lbs(5000)                                       # the part_shift values the sort keeps at this size: the two ends
        for lb in sorted({lbs[0], lbs[-1]}):
            shapes.append(("n5000-part_shift%d" % lb, {"n": 5000, "opts": {"part_shift": lb}}, dict(big, opts={"part_shift": lb})))
        shapes.append(("heavy-counts", {"heavy": True}, {"heavy": True, "larger": True}))
    return shapes


def _g1_sum_build(E, p):
    k = p["k"]
    jac = np.zeros((k, 12), np.uint64)
    pts = E.g1_pts(k + 16)[p.get("off", 0):p.get("off", 0) + k]
    fq_one = E.oc.fq_to_mont(E.oc.ints_to_limbs([1]))[0]
    for i in range(k):
        if pts[i].any():
            jac[i, :8], jac[i, 8:] = pts[i], fq_one
        else:
            jac[i, :4], jac[i, 4:8] = fq_one, fq_one

    def run(h, st):
        return (h.g1_sum(jac),)

    def expect(out):
        assert np.array_equal(jac_to_aff(out[0]), E.oc.g1_sum(pts)), "g1_sum against the oracle"

    def run_dev(h, st, A):
        d_p, d_o = A.put(jac), A.out(96)
        A.ready()
        h.g1_sum_dev(d_p, k, d_o)
        h.synchronize()
        return (A.read(d_o, np.uint64, (12,)),)

    return Case(run, None, expect, run_dev)


# ---- kzg_open, kzg_quotient, the batched MSM and open ---------------------------------------------------------------------------------------------
def _open_build(E, p):
    oc, n = E.oc, p["n"]
    pts = E.g1_pts(max(n - 1, 1))
    coeffs = rand_fr_ints(n, 0xB000 + n + p.get("seed", 0))
    z = rand_fr_ints(1, 0xB001 + n)[0]
    cm, zm = E.mont(coeffs), E.mont([z])[0]
    opts = {"msm_pipe_chunks": p["chunks"], "msm_pipe_min": 1, "msm_pipe_growth": 100} if p.get("chunks") else {}

    def setup(h):
        srs = h.srs_g1_upload(pts)
        return {"srs": srs, "free": [srs]}

    def run(h, st):
        return h.kzg_open(st["srs"], cm, zm)

    def expect(out):
        q, val = synthetic_division(coeffs, z)
        assert E.unmont(out[1]) == [val], "p(z)"
        want = oc.msm_g1(pts[:n - 1], E.mont(q), threads=TH) if n > 1 else np.zeros(8, np.uint64)
        assert np.array_equal(jac_to_aff(out[0]), want), "proof = the oracle's MSM of the quotient"

    return Case(run, setup, expect, None, opts)


def _quotient_build(E, p):
    n = p["n"]
    coeffs = rand_fr_ints(n, 0xB100 + n + p.get("seed", 0))
    z = rand_fr_ints(1, 0xB101 + n)[0]
    cm, zm = E.mont(coeffs), E.mont([z])[0]

    def run(h, st):
        return h.kzg_quotient(cm, zm)

    def expect(out):
        q, val = synthetic_division(coeffs, z)
        assert E.unmont(out[0]) == q, "every quotient coefficient"
        assert E.unmont(out[1]) == [val], "p(z)"

    return Case(run, None, expect)


def _batch_build(what):
    def build(E, p):
        oc, m, n = E.oc, p["m"], p["n"]
        stride = n + 1
        pts = E.g1_pts(n)
        ints = [rand_fr_ints(n, 0xB200 + 131 * j + n + p.get("seed", 0)) for j in range(m)]
        rows = np.full((m, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)        # the gap behind a row is never read
        rows[:, :n] = E.mont(sum(ints, [])).reshape(m, n, 4)
        zs = rand_fr_ints(m, 0xB201 + m)
        zm = E.mont(zs)

        def setup(h):
            srs = h.srs_g1_upload(pts)
            return {"srs": srs, "free": [srs]}

        if what == "msm":
            def run(h, st):
                return (h.msm_g1_batch(st["srs"], rows, n=n),)

            def expect(out):
                for j in range(m):
                    assert np.array_equal(jac_to_aff(out[0][j]), oc.msm_g1(pts, rows[j, :n], threads=TH)), ("row", j)

            def run_dev(h, st, A):
                d_r, d_o = A.put(rows), A.out(96 * m)
                A.ready()
                h.msm_g1_batch_dev(st["srs"], d_r, n, m, stride, d_o)
                h.synchronize()
                return (A.read(d_o, np.uint64, (m, 12)),)
        else:
            def run(h, st):
                return h.kzg_open_batch(st["srs"], rows, zm, n=n)

            def expect(out):
                for j in range(m):
                    q, val = synthetic_division(ints[j], zs[j])
                    assert E.unmont(out[1][j]) == [val], ("value", j)
                    assert np.array_equal(jac_to_aff(out[0][j]), oc.msm_g1(pts[:n - 1], E.mont(q), threads=TH)), ("proof", j)

            def run_dev(h, st, A):
                d_r, d_z, d_o, d_v = A.put(rows), A.put(zm), A.out(96 * m), A.out(32 * m)
                A.ready()
                h.kzg_open_batch_dev(st["srs"], d_r, n, m, stride, d_z, d_o, d_v)
                h.synchronize()
                return A.read(d_o, np.uint64, (m, 12)), A.read(d_v, np.uint64, (m, 4))

        return Case(run, setup, expect, run_dev)
    return build


# ---- FK23 --------------------------------------------------------------------------------------------------------------------------------------
def _fk_consts(E, log2d):
    """(omega_d^-1, 1 / d, omega_2d, omega_2d^-1, 1 / 2d): the five domain constants of vec_commit, the last three of open_fk_poly"""
    import structured_inputs as S
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    return [E.mont([x])[0] for x in (pow(w2 * w2, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]


def _fk_srs_setup(pts):
    def setup(h):
        srs = h.srs_g1_upload(pts)
        return {"srs": srs, "free": [srs]}
    return setup


def _fk_poly_build(E, p):
    log2d = p["log2d"]
    d = 1 << log2d
    k = _fk_consts(E, log2d)
    pts = E.g1_pts(max(d, 2))
    coeffs = rand_fr_ints(d, 0xC000 + log2d + p.get("seed", 0))
    cm = E.mont(coeffs)

    def run(h, st):
        return (h.open_fk_poly(st["srs"], log2d, cm, *k[2:]),)

    def expect(out):
        if d > 8:
            return                        # log2d = 9: tests/test_gpu_variants.py::test_open_fk_ladder_variants ties it to the oracle
        wd = pow(E.unmont(k[2])[0], 2, R)
        for i in range(d):
            q, _ = synthetic_division(coeffs, pow(wd, i, R))
            assert np.array_equal(out[0][i], E.oc.msm_g1(pts[:d - 1], E.mont(q), threads=TH)), ("proof", i)

    return Case(run, _fk_srs_setup(pts), expect, None, {"fk_gtab": p.get("gtab", 1)})


def _fk_raw_build(E, p):
    """keaki_hip_open_fk: hat_a and the twiddle tables from the host (the oracle's DFT)"""
    log2d = p["log2d"]
    d = 1 << log2d
    k = _fk_consts(E, log2d)
    w2, w2i = E.unmont(k[2])[0], E.unmont(k[3])[0]
    pts = E.g1_pts(max(d, 2))
    coeffs = rand_fr_ints(d, 0xC100 + log2d + p.get("seed", 0))
    hat_a = E.oc.fr_fft(E.mont([0] * d + coeffs), k[2], k[4])
    tw, twi = E.mont([pow(w2, j, R) for j in range(d)]), E.mont([pow(w2i, j, R) for j in range(d)])
    twd = E.mont([pow(w2, 2 * j, R) for j in range(d // 2)] or [1])

    def run(h, st):
        return (h.open_fk(st["srs"], log2d, hat_a, tw, twi, twd),)

    def expect(out):
        wd = pow(w2, 2, R)
        for i in range(d if d <= 8 else 0):
            q, _ = synthetic_division(coeffs, pow(wd, i, R))
            assert np.array_equal(out[0][i], E.oc.msm_g1(pts[:d - 1], E.mont(q), threads=TH)), ("proof", i)

    return Case(run, _fk_srs_setup(pts), expect)


def _vec_commit_build(E, p):
    log2d, n = p["log2d"], p["n"]
    d = 1 << log2d
    k = _fk_consts(E, log2d)
    pts = E.g1_pts(d)
    vals, pad = E.mont(rand_fr_ints(n, 0xC200 + log2d + p.get("seed", 0))), E.mont(rand_fr_ints(1, 0xC201 + log2d))[0]

    def run(h, st):
        return h.vec_commit(st["srs"], vals, pad, log2d, *k)

    return Case(run, _fk_srs_setup(pts))


def _fk_batch_build(what):
    def build(E, p):
        log2d, m = p["log2d"], p["m"]
        d = 1 << log2d
        k = _fk_consts(E, log2d)
        pts = E.g1_pts(max(d, 2))
        stride = d + 1
        rows = np.full((m, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
        rows[:, :d] = E.mont(rand_fr_ints(m * d, 0xC300 + 40 * log2d + m + p.get("seed", 0))).reshape(m, d, 4)

        if what == "open":
            def run(h, st):
                return (h.open_fk_poly_batch(st["srs"], log2d, rows, *k[2:]),)

            def run_dev(h, st, A):
                d_r, d_o = A.put(rows), A.out(64 * m * d)
                A.ready()
                h.open_fk_poly_batch_dev(st["srs"], log2d, d_r, m, stride, *k[2:], d_o)
                h.synchronize()
                return (A.read(d_o, np.uint64, (m, d, 8)),)
        else:
            def run(h, st):
                return h.vec_commit_batch(st["srs"], rows, log2d, *k, n=d)

            def run_dev(h, st, A):
                d_r, d_c, d_o = A.put(rows), A.out(96 * m), A.out(64 * m * d)
                A.ready()
                h.vec_commit_batch_dev(st["srs"], d_r, d, m, stride, log2d, *k, d_c, d_o)
                h.synchronize()
                return A.read(d_c, np.uint64, (m, 12)), A.read(d_o, np.uint64, (m, d, 8))

        return Case(run, _fk_srs_setup(pts), None, run_dev)
    return build


def _fk_coset_build(raw):
    def build(E, p):
        import fk_coset_model as FM
        log2d, log2l = p["log2d"], p["log2l"]
        d, l, r = 1 << log2d, 1 << log2l, 1 << (log2d - log2l)
        w2 = FM.omega(2 * r)
        rt = [E.mont([v])[0] for v in (w2, FM.inv(w2), FM.inv(2 * r))]
        pts = E.g1_pts(d)
        coeffs = rand_fr_ints(d, 0xC400 + 32 * log2d + log2l + p.get("seed", 0))
        cm = E.mont(coeffs)

        if raw:
            # row j = DFT_2r(r zeros, then f_(u l + j), u < r) with the (2r)^-1 folded in, natural order
            hat_a = np.concatenate([E.oc.fr_fft(E.mont([0] * r + [coeffs[u * l + j] for u in range(r)]), rt[0], rt[2]) for j in range(l)])

            def run(h, st):
                return (h.open_fk_cosets(st["srs"], log2d, log2l, hat_a, rt[0], rt[1]),)
            return Case(run, _fk_srs_setup(pts))

        def run(h, st):
            return (h.open_fk_cosets_poly(st["srs"], log2d, log2l, cm, *rt),)

        def run_dev(h, st, A):
            d_c, d_o = A.put(cm), A.out(64 * r)
            A.ready()
            h.open_fk_cosets_poly_dev(st["srs"], log2d, log2l, d_c, *rt, d_o)
            h.synchronize()
            return (A.read(d_o, np.uint64, (r, 8)),)

        return Case(run, _fk_srs_setup(pts), None, run_dev)
    return build


def _vec_update_build(E, p):
    import vec_update_model as UM
    log2d, kk = p["log2d"], p["k"]
    d = 1 << log2d
    k5 = _fk_consts(E, log2d)
    w = UM.omega(d)
    u3 = [E.mont([x])[0] for x in (w, pow(w, -1, R), pow(d, -1, R))]
    pts = E.g1_pts(d)
    rnd = rand_fr_ints(2 * kk + d, 0xC500 + log2d + kk + p.get("seed", 0))
    idx = np.array([v % d for v in rnd[:kk]], np.uint32)
    if kk > 1:
        idx[1] = idx[0]                                  # a duplicate: the entries add
    deltas, evals = E.mont(rnd[kk:2 * kk]), E.mont(rnd[2 * kk:])

    def setup(h):
        srs = h.srs_g1_upload(pts)
        com, proofs = h.vec_commit(srs, evals, None, log2d, *k5)       # the state the update starts from (its own call: it is not what is compared)
        return {"srs": srs, "free": [srs], "com": com, "proofs": proofs}

    def run(h, st):
        return h.vec_update(st["srs"], log2d, *u3, idx, deltas, st["com"].copy(), st["proofs"].copy())

    def run_dev(h, st, A):
        d_i, d_d, d_c, d_p = A.put(idx), A.put(deltas), A.put(st["com"], out=True), A.put(st["proofs"], out=True)
        A.ready()
        h.vec_update_dev(st["srs"], log2d, *u3, d_i, d_d, kk, d_c, d_p)
        h.synchronize()
        return A.read(d_c, np.uint64, (12,)), A.read(d_p, np.uint64, (d, 8))

    return Case(run, setup, None, run_dev, {"vec_update_k_pass": p.get("k_pass", 0)})


def _fr_fft_build(E, p):
    log2n = p["log2n"]
    n = 1 << log2n
    w = E.py.fr_root_of_unity(n)
    a = rand_fr_ints(n, 0xC600 + log2n)
    a[1], a[2] = 0, R - 1
    am, wm, sm = E.mont(a), E.mont([w])[0], E.mont([pow(n, -1, R)])[0]

    def run(h, st):
        return h.fr_fft(am, log2n, wm), h.fr_fft(am, log2n, wm, sm)

    def expect(out):
        assert np.array_equal(out[0], E.oc.fr_fft(am, wm)) and np.array_equal(out[1], E.oc.fr_fft(am, wm, sm)), "the oracle's DFT"
        if n <= 32:
            assert E.unmont(out[0]) == [sum(a[i] * pow(w, i * j, R) for i in range(n)) % R for j in range(n)], "the O(n^2) definition"

    return Case(run, None, expect)


# ---- scalar multiplication, pairing, KEM --------------------------------------------------------------------------------------------------------
def _mul_build(group):
    g2 = group == "g2"
    w = 16 if g2 else 8

    def build(E, p):
        oc, n = E.oc, p["n"]
        pts = (E.g2_pts if g2 else E.g1_pts)(n + 16)[p.get("seed", 0):p.get("seed", 0) + n]
        ks = rand_fr_ints(n, 0xD000 + n + (1 if g2 else 0))
        if n > 2:
            ks[0], ks[1], ks[2] = 0, R - 1, 1
        km = E.mont(ks)

        def run(h, st):
            return ((h.g2_mul_batch if g2 else h.g1_mul_batch)(pts, km),)           # n = 1: one point for every scalar, the same call

        def expect(out):
            assert np.array_equal(out[0], (oc.g2_mul_batch if g2 else oc.g1_mul_batch)(pts, km, threads=TH)), "the oracle's multiples"

        def run_dev(h, st, A):
            d_p, d_k, d_o = A.put(pts), A.put(km), A.out(8 * w * n)
            A.ready()
            (h.g2_mul_batch_dev if g2 else h.g1_mul_batch_dev)(d_p, 1 if n > 1 else 0, d_k, n, d_o)
            h.synchronize()
            return (A.read(d_o, np.uint64, (n, w)),)

        return Case(run, None, expect, run_dev)
    return build


def _pair_points(E, n, off=0):
    def make():
        P, Q = E.g1_of(rand_fr_ints(320, 0xD100)), E.g2_of(rand_fr_ints(320, 0xD101))
        P[2] = 0; P[70] = 0; Q[4] = 0; Q[133] = 0
        return P, Q
    P, Q = E.once("pair_points", make)
    return P[off:off + n], Q[off:off + n]


def _pairing_build(E, p):
    oc, n = E.oc, p["n"]
    P, Q = _pair_points(E, n, p.get("off", 0))

    def run(h, st):
        return (h.pairing_batch(P, Q),)

    def expect(out):
        assert np.array_equal(out[0], oc.pairing_batch(P, Q, threads=TH)), "the oracle's pairings"

    def run_dev(h, st, A):
        d_p, d_q, d_o = A.put(P), A.put(Q), A.out(384 * n)
        A.ready()
        h.pairing_batch_dev(d_p, d_q, 1, n, d_o)
        h.synchronize()
        return (A.read(d_o, np.uint8, (n, 384)),)

    return Case(run, None, expect, run_dev, {"pair_wide_max": p["wide"]})


def _pairing_product_build(E, p):
    oc, n = E.oc, p["n"]

    def make():
        a, b = rand_fr_ints(320, 0xD200), rand_fr_ints(320, 0xD201)
        return a, b, E.g1_of(a), E.g2_of(b)
    a, b, P, Q = E.once("product_pairs", make)
    off = p.get("off", 0)
    a, b, P, Q = a[off:off + n], b[off:off + n], P[off:off + n], Q[off:off + n]

    def run(h, st):
        return (h.pairing_product(P, Q),)

    def expect(out):
        s = sum(x * y for x, y in zip(a, b)) % R
        g1, g2 = oc.generators()
        assert np.array_equal(out[0], oc.pairing_batch(oc.g1_mul_batch(g1, E.mont([s]), threads=1), g2, threads=1)[0]), "one pairing of the summed exponent"

    def run_dev(h, st, A):
        d_p, d_q, d_o = A.put(P), A.put(Q), A.out(384)
        A.ready()
        h.pairing_product_dev(d_p, d_q, n, d_o)
        h.synchronize()
        return (A.read(d_o, np.uint8, (384,)),)

    return Case(run, None, expect, run_dev)


def _pairing_stages_build(E, p):
    """the test hooks of the pairing's two halves and the line table: miller_loop_batch, final_exp_batch, g2_prepare"""
    oc, n = E.oc, p["n"]
    P, Q = _pair_points(E, n, p.get("off", 5))

    def run(h, st):
        f = h.miller_loop_batch(P, Q)
        return f, h.final_exp_batch(f), h.g2_prepare(Q[0])

    def expect(out):
        assert np.array_equal(out[1], oc.pairing_batch(P, Q, threads=TH)), "final_exp(miller_loop) = the oracle's pairing"

    return Case(run, None, expect)


def _kem_inputs(E, n, seed, which=1):
    """n items to the commitment c g1 under [tau]_2 with the proofs that decapsulate them (tests/test_gpu_dev_queue.py: _kem_inputs)"""
    import test_gpu_dev_queue as Q
    oc = E.oc

    def make():
        tau, c1, c2 = rand_fr_ints(3, 0xE0)
        return tau, {1: c1, 2: c2}, E.g2_of([tau])[0], {1: E.g1_of([c1])[0], 2: E.g1_of([c2])[0]}
    tau, dlog, tau_g2, coms = E.once("kem_setup", make)
    A, V, Rr, proofs = Q._kem_inputs(oc, rand_fr_ints, seed, n, dlog[which], tau, zero_r=(n // 2,) if n > 2 else ())
    return {"tau_g2": tau_g2, "com": coms[which], "A": A, "V": V, "R": Rr, "proofs": proofs}


def _encap_build(encrypt):
    def build(E, p):
        oc, n, ml = E.oc, p["n"], 33
        x = _kem_inputs(E, n, 0xE100 + n, p.get("which", 1))
        msgs = np.random.default_rng(0xE1 + n).integers(0, 256, (n, ml), dtype=np.uint8)

        def oracle():
            return E.once(("encap_oracle", n, p.get("which", 1)), lambda: oc.encap_batch(x["com"], x["tau_g2"], x["A"], x["V"], x["R"], ml, threads=TH))

        if not encrypt:
            def run(h, st):
                return h.encap_batch(x["com"], x["tau_g2"], x["A"], x["V"], x["R"], ml)

            def expect(out):
                for got, want, name in zip(out, oracle(), ("ct", "gt", "key")):
                    assert np.array_equal(got, want), name

            def run_dev(h, st, A):
                d = [A.put(x[k]) for k in ("com", "tau_g2", "A", "V", "R")]
                d_ct, d_gt, d_key = A.out(128 * n), A.out(384 * n), A.out(ml * n)
                A.ready()
                h.encap_batch_dev(*d, n, d_ct, d_gt, d_key, ml)
                h.synchronize()
                return A.read(d_ct, np.uint64, (n, 16)), A.read(d_gt, np.uint8, (n, 384)), A.read(d_key, np.uint8, (n, ml))
        else:
            def run(h, st):
                return h.encrypt_batch(x["com"], x["tau_g2"], x["A"], x["V"], x["R"], msgs)

            def expect(out):
                ct, _, key = oracle()
                assert np.array_equal(out[0], ct) and np.array_equal(out[1], key ^ msgs), "ciphertext, body = key XOR message"

            def run_dev(h, st, A):
                d = [A.put(x[k]) for k in ("com", "tau_g2", "A", "V", "R")]
                d_ct, d_body = A.out(128 * n), A.put(msgs, out=True)
                A.ready()
                h.encrypt_batch_dev(*d, n, d_ct, d_body, ml)
                h.synchronize()
                return A.read(d_ct, np.uint64, (n, 16)), A.read(d_body, np.uint8, (n, ml))

        return Case(run, None, expect, run_dev)
    return build


def _decap_build(decrypt):
    def build(E, p):
        oc, n, ml = E.oc, p["n"], 33
        x = _kem_inputs(E, n, 0xE100 + n, p.get("which", 1))
        ct, gt, key = E.once(("encap_oracle", n, p.get("which", 1)), lambda: oc.encap_batch(x["com"], x["tau_g2"], x["A"], x["V"], x["R"], ml, threads=TH))
        msgs = np.random.default_rng(0xE2 + n).integers(0, 256, (n, ml), dtype=np.uint8)
        bodies = key ^ msgs

        if not decrypt:
            def run(h, st):
                return h.decap_batch(x["proofs"], ct, ml)

            def expect(out):
                assert np.array_equal(out[0], gt) and np.array_equal(out[1], key), "the GT values and keys of the oracle's encapsulation"
                og, ok = oc.decap_batch(x["proofs"], ct, ml, threads=TH)
                assert np.array_equal(out[0], og) and np.array_equal(out[1], ok), "the oracle's decapsulation"

            def run_dev(h, st, A):
                d_p, d_c, d_gt, d_key = A.put(x["proofs"]), A.put(ct), A.out(384 * n), A.out(ml * n)
                A.ready()
                h.decap_batch_dev(d_p, d_c, n, d_gt, d_key, ml)
                h.synchronize()
                return A.read(d_gt, np.uint8, (n, 384)), A.read(d_key, np.uint8, (n, ml))
        else:
            def run(h, st):
                return (h.decrypt_batch(x["proofs"], ct, bodies),)

            def expect(out):
                assert np.array_equal(out[0], msgs), "every message comes back"

            def run_dev(h, st, A):
                d_p, d_c, d_b = A.put(x["proofs"]), A.put(ct), A.put(bodies, out=True)
                A.ready()
                h.decrypt_batch_dev(d_p, d_c, n, d_b, ml)
                h.synchronize()
                return (A.read(d_b, np.uint8, (n, ml)),)

        return Case(run, None, expect, run_dev)
    return build


def _encap_multi_build(encrypt):
    def build(E, p):
        import test_gpu_encap_multi as EM
        oc, sizes, ml = E.oc, p["sizes"], 32
        n, m = sum(sizes), len(sizes)
        x = _kem_inputs(E, n, 0xE300 + n)
        coms = E.once("multi_coms", lambda: E.g1_of(rand_fr_ints(8, 0xE301)))[:m]
        off = EM.offsets_of(sizes)
        msgs = np.random.default_rng(0xE3 + n).integers(0, 256, (n, ml), dtype=np.uint8)

        def oracle():
            return E.once(("multi_oracle", tuple(sizes)), lambda: EM.oracle_groups(oc, coms, sizes, x["tau_g2"], x["A"], x["V"], x["R"], ml))

        if not encrypt:
            def run(h, st):
                return h.encap_multi(coms, off, x["tau_g2"], x["A"], x["V"], x["R"], ml)

            def expect(out):
                for got, want, name in zip(out, oracle(), ("ct", "gt", "key")):
                    assert np.array_equal(got, want), name

            def run_dev(h, st, A):
                d = [A.put(a) for a in (x["tau_g2"], x["A"], x["V"], x["R"])]
                d_c, d_ct, d_gt, d_key = A.put(coms), A.out(128 * n), A.out(384 * n), A.out(ml * n)
                A.ready()
                h.encap_multi_dev(d_c, off, *d, n, d_ct, d_gt, d_key, ml)
                h.synchronize()
                return A.read(d_ct, np.uint64, (n, 16)), A.read(d_gt, np.uint8, (n, 384)), A.read(d_key, np.uint8, (n, ml))
        else:
            def run(h, st):
                return h.encrypt_multi(coms, off, x["tau_g2"], x["A"], x["V"], x["R"], msgs)

            def expect(out):
                ct, _, key = oracle()
                assert np.array_equal(out[0], ct) and np.array_equal(out[1], key ^ msgs), "ciphertext, body = key XOR message"

            def run_dev(h, st, A):
                d = [A.put(a) for a in (x["tau_g2"], x["A"], x["V"], x["R"])]
                d_c, d_ct, d_body = A.put(coms), A.out(128 * n), A.put(msgs, out=True)
                A.ready()
                h.encrypt_multi_dev(d_c, off, *d, n, d_ct, d_body, ml)
                h.synchronize()
                return A.read(d_ct, np.uint64, (n, 16)), A.read(d_body, np.uint8, (n, ml))

        return Case(run, None, expect, run_dev)
    return build


# ---- KZG verification and sets ---------------------------------------------------------------------------------------------------------------------
def _verify_build(E, p):
    """keaki_hip_kzg_verify: a valid opening and the same with a changed value (the larger call of the residue step: verify_batch over 64 items)"""
    import test_gpu_verify_batch as TB
    if p.get("larger"):
        return _verify_batch_build(E, {"n": 64})
    a = TB.arrays_for(E.oc, E.py, 1, False)[0]
    bad_y = E.mont([a.c.y[0] + 1])[0]

    def run(h, st):
        return h.kzg_verify(a.coms[0], a.tau_g2, a.z[0], a.y[0], a.proofs[0]), h.kzg_verify(a.coms[0], a.tau_g2, a.z[0], bad_y, a.proofs[0])

    def expect(out):
        assert a.c.verdict() and out == (True, False), "the model's verdicts"

    return Case(run, None, expect)


def _verify_batch_build(E, p):
    import test_gpu_verify_batch as TB
    n = p["n"]
    a0, a1 = TB.arrays_for(E.oc, E.py, n, False)

    def run(h, st):
        return a0.run(h) + a1.run(h)

    def expect(out):
        for a, got in ((a0, out[:3]), (a1, out[3:])):
            ok, L, Rp = a.expected(E.oc)
            assert got[0] == ok and np.array_equal(got[1], L) and np.array_equal(got[2], Rp), "the model's verdict and sums"

    def run_dev(h, st, A):
        d = [A.put(x) for x in (a1.coms, a1.tau_g2, a1.z, a1.y, a1.proofs, a1.gamma)]
        A.ready()
        return (None, None, None) + tuple(h.kzg_verify_batch_dev(d[0], 1, d[1], d[2], 0, d[3], d[4], d[5], n))

    return Case(run, None, expect, run_dev)


def _verify_each_build(E, p):
    import test_gpu_verify_each as TE
    n = p["n"]
    c = TE.with_bad(TE.base_case(n, 0xF100 + n, stride=1), sorted({0, n - 1}) if n > 2 else [0])
    a = TE.Arrays(E.oc, c)

    def run(h, st):
        return a.run(h, want_lhs=True)

    def expect(out):
        assert out[0].tolist() == c.status() and (out[1], out[2]) == c.counters(), "the model's status bytes and counters"

    def run_dev(h, st, A):
        d = [A.put(x) for x in (a.coms, a.tau_g2, a.z, a.y, a.proofs)]
        d_st, d_lhs = A.out(n), A.out(64 * n)                 # n status bytes: nothing behind them may change
        A.ready()
        bad, first = h.kzg_verify_each_dev(d[0], 1, d[1], d[2], 0, d[3], d[4], n, d_st, d_lhs)
        return A.read(d_st, np.uint8, (n,)), bad, first, A.read(d_lhs, np.uint64, (n, 8))

    return Case(run, None, expect, run_dev)


def _coset_env(E, mod):
    g1, _ = E.tau_srs(mod.TAU, mod.SRS_LEN)
    return g1


def _coset_family_build(kind):
    """verify_cosets | verify_cosets_each | coset_pairs on rows of n items over cosets of size l (tests/test_gpu_verify_cosets.py and its neighbours)"""
    def build(E, p):
        import importlib
        T = importlib.import_module({"verify": "test_gpu_verify_cosets", "each": "test_gpu_verify_cosets_each", "pairs": "test_gpu_coset_pairs"}[kind])
        n, l = p["n"], p["l"]
        c = T.rows_case(n, l, l + 3, 0xF200 + 17 * n + l, shared=False)
        if kind == "each" and n > 2:
            import coset_pairs_model as CP
            c = CP.corrupt(c, "value", n - 1)
        x = T.Inputs(E.oc, c)
        g1 = _coset_env(E, T)

        def setup(h):
            srs = h.srs_g1_upload(g1)
            return {"srs": srs, "free": [srs]}

        def run(h, st):
            return x.call(h, st["srs"])

        def expect(out):
            x.check(out, kind)

        log2l = l.bit_length() - 1

        def run_dev(h, st, A):
            d_com, d_h, d_v = A.put(x.com), A.put(x.h), A.put(x.values)
            if kind == "verify":
                d_t, d_p, d_g = A.put(x.tau_l), A.put(x.proofs), A.put(x.gamma)
                A.ready()
                return h.kzg_verify_cosets_dev(st["srs"], d_com, 1, d_t, d_h, 0, d_v, l, 1, log2l, x.winv, x.linv, d_p, d_g, n)
            if kind == "each":
                d_t, d_p, d_st, d_l = A.put(x.tau_l), A.put(x.proofs), A.out(n), A.out(64 * n)
                A.ready()
                bad, first = h.kzg_verify_cosets_each_dev(st["srs"], d_com, 1, d_t, d_h, 0, d_v, l, 1, log2l, x.winv, x.linv, d_p, n, d_st, d_l)
                return A.read(d_st, np.uint8, (n,)), bad, first, A.read(d_l, np.uint64, (n, 8))
            d_a, d_c = A.out(64 * n), A.out(32 * n)
            A.ready()
            h.kzg_coset_pairs_dev(st["srs"], d_com, 1, d_h, 0, d_v, l, 1, log2l, x.winv, x.linv, n, d_a, d_c)
            h.synchronize()
            return A.read(d_a, np.uint64, (n, 8)), A.read(d_c, np.uint64, (n, 4))

        return Case(run, setup, expect, run_dev)
    return build


def _set_family_build(kind):
    """verify_sets | verify_sets_each | set_pairs on n items of k arbitrary points (tests/test_gpu_verify_sets.py, test_gpu_set_pairs.py)"""
    def build(E, p):
        import test_gpu_set_pairs as TP
        import test_gpu_verify_sets as TS
        T = TS if kind == "verify" else TP
        n, k = p["n"], p["k"]
        c = T.make_case(n, k, 0xF300 + 100 * k + n)
        if kind == "each" and n > 1:
            import set_pairs_model as SP
            c = SP.corrupt(c, "value", n - 1, k - 1, delta=2)
        x = T.Inputs(E.oc, c)
        g1, g2 = E.tau_srs(T.TAU, 80, 80)

        def setup(h):
            s1, s2 = h.srs_g1_upload(g1), h.srs_g2_upload(g2)
            return {"srs1": s1, "srs2": s2, "plain": s1, "free": [s1, s2]}

        if kind == "verify":
            def run(h, st):
                return x.call(h, st, srs="plain")

            def expect(out):
                x.check(out, "verify_sets")

            def run_dev(h, st, A):
                d = [A.put(a) for a in (x.com, x.points, x.values, x.proofs, x.gamma)]
                A.ready()
                return h.kzg_verify_sets_dev(st["srs1"], st["srs2"], d[0], 0 if len(x.com) == 1 else 1, d[1], 0, None, d[2], k, k, d[3], d[4], n)
        elif kind == "pairs":
            def run(h, st):
                return x.call(h, st)

            def expect(out):
                x.check(out, "set_pairs")

            def run_dev(h, st, A):
                d = [A.put(a) for a in (x.com, x.points, x.values)]
                d_a, d_z = A.out(64 * n), A.out(128 * n)
                A.ready()
                h.kzg_set_pairs_dev(st["srs1"], st["srs2"], d[0], 1, d[1], 0, None, d[2], k, k, n, d_a, d_z)
                h.synchronize()
                return A.read(d_a, np.uint64, (n, 8)), A.read(d_z, np.uint64, (n, 16))
        else:
            def run(h, st):
                return h.kzg_verify_sets_each(st["srs1"], st["srs2"], x.com, x.points, x.values, k, x.proofs, want_pairs=True)

            def expect(out):
                import set_pairs_model as SP
                want = SP.statuses(c)
                assert out[0].tolist() == want and out[1] == sum(want) and out[2] == (want.index(1) if 1 in want else None), "the model's status bytes and counters"
                x.check(out[3:], "pairs")

            def run_dev(h, st, A):
                d = [A.put(a) for a in (x.com, x.points, x.values, x.proofs)]
                d_st, d_a, d_z = A.out(n), A.out(64 * n), A.out(128 * n)
                A.ready()
                bad, first = h.kzg_verify_sets_each_dev(st["srs1"], st["srs2"], d[0], 1, d[1], 0, None, d[2], k, k, d[3], n, d_st, d_a, d_z)
                return A.read(d_st, np.uint8, (n,)), bad, first, A.read(d_a, np.uint64, (n, 8)), A.read(d_z, np.uint64, (n, 16))

        return Case(run, setup, expect, run_dev, {"set_rows_wb": 8, "coset_rows_wb": 8})
    return build


def _kzg_set_build(kind):
    """set_polys | open_multi | aggregate | verify_multi (tests/test_gpu_kzg_set.py, tests/kzg_set_model.py)"""
    def build(E, p):
        import kzg_set_model as KM
        import test_gpu_kzg_set as TK
        oc, k, n = E.oc, p["k"], p.get("n", 200)
        zs = TK.points_for(k, 1000 * k + n % 997)
        zm = E.mont(zs)
        g1, g2 = E.tau_srs(TK.TAU, 1100, 70)
        coeffs = E.once("set_coeffs", lambda: rand_fr_ints(1100, 4242))[:n]
        cm = E.mont(coeffs)

        def setup(h):
            s1, s2 = h.srs_g1_upload(g1), h.srs_g2_upload(g2)
            return {"srs": s1, "srs2": s2, "free": [s1, s2]}

        def model():
            return E.once(("set_model", n, k), lambda: KM.quotient_long_division(coeffs, zs))

        if kind == "polys":
            ys = rand_fr_ints(k, 17 * k + 1)
            ym = E.mont(ys)

            def run(h, st):
                return h.kzg_set_polys(zm, ym)

            def expect(out):
                assert E.unmont(out[0]) == KM.vanishing(zs) and E.unmont(out[1]) == KM.weights(zs) and E.unmont(out[2]) == KM.interpolant(zs, ys), "Z, weights, I"

            def run_dev(h, st, A):
                d_z, d_y, o_z, o_w, o_i = A.put(zm), A.put(ym), A.out(32 * (k + 1)), A.out(32 * k), A.out(32 * k)
                A.ready()
                h.kzg_set_polys_dev(d_z, d_y, k, o_z, o_w, o_i)
                h.synchronize()
                return A.read(o_z, np.uint64, (k + 1, 4)), A.read(o_w, np.uint64, (k, 4)), A.read(o_i, np.uint64, (k, 4))
            return Case(run, None, expect, run_dev)

        if kind == "open":
            def run(h, st):
                return h.kzg_open_multi(st["srs"], cm, zm)

            def expect(out):
                q, ys = model()
                assert E.unmont(out[1]) == ys and np.array_equal(jac_to_aff(out[0]), E.g1_of([KM.poly_eval(q, TK.TAU)])[0]), "values and the proof's discrete log"

            def run_dev(h, st, A):
                d_c, d_z, d_p, d_v = A.put(cm), A.put(zm), A.out(96), A.out(32 * k)
                A.ready()
                h.kzg_open_multi_dev(st["srs"], d_c, n, d_z, k, d_p, d_v)
                h.synchronize()
                return A.read(d_p, np.uint64, (12,)), A.read(d_v, np.uint64, (k, 4))
            return Case(run, setup, expect, run_dev)

        # the k single proofs as points of known discrete log: q_j(tau) for q_j = (p - p(z_j)) / (x - z_j)
        singles = E.once(("set_singles", n, k), lambda: E.g1_of([KM.poly_eval(synthetic_division(coeffs, z)[0], TK.TAU) for z in zs]))
        if kind == "aggregate":
            def run(h, st):
                return (h.kzg_aggregate(zm, singles),)

            def expect(out):
                q, _ = model()
                assert np.array_equal(jac_to_aff(out[0]), E.g1_of([KM.poly_eval(q, TK.TAU)])[0]), "the set proof's discrete log"

            def run_dev(h, st, A):
                d_z, d_s, d_o = A.put(zm), A.put(singles), A.out(96)
                A.ready()
                h.kzg_aggregate_dev(d_z, d_s, k, d_o)
                h.synchronize()
                return (A.read(d_o, np.uint64, (12,)),)
            return Case(run, None, expect, run_dev)

        q, ys = model()
        com, proof = E.g1_of([KM.poly_eval(coeffs, TK.TAU)])[0], E.g1_of([KM.poly_eval(q, TK.TAU)])[0]
        ym, bad = E.mont(ys), E.mont([ys[0] + 1] + ys[1:])

        def run(h, st):
            return h.kzg_verify_multi(st["srs"], st["srs2"], com, zm, ym, proof, want_pair=True) + (h.kzg_verify_multi(st["srs"], st["srs2"], com, zm, bad, proof),)

        def expect(out):
            assert out[0] is True and out[3] is False, "an honest opening and one changed value"

        return Case(run, setup, expect)
    return build


# ---- point codec -------------------------------------------------------------------------------------------------------------------------------
def _codec_build(what):
    g2 = what.startswith("g2")

    def build(E, p):
        import test_gpu_point_codec as PC
        n = p["n"]
        pts = PC.points(E.oc, n, g2)
        wire, w = (64, 16) if g2 else (32, 8)

        def model():
            return E.once(("codec_model", n, g2), lambda: (PC.model_g2_bytes if g2 else PC.model_g1_bytes)(pts))

        if what.endswith("_compress"):
            def run(h, st):
                return ((h.g2_compress if g2 else h.g1_compress)(pts),)

            def expect(out):
                assert np.array_equal(out[0], model()), "the model's bytes"

            def run_dev(h, st, A):
                d_p, d_o = A.put(pts), A.out(wire * n)
                A.ready()
                h.point_codec_dev(what, d_p, n, d_o)
                h.synchronize()
                return (A.read(d_o, np.uint8, (n, wire)),)
        elif what.endswith("_decompress"):
            data = model().copy()
            if n > 2:
                data[n - 1, 0] ^= 1                     # one item that no longer decodes to a curve point (or decodes to another one): a status and the counters

            def run(h, st):
                return (h.g2_decompress(data, 1) if g2 else h.g1_decompress(data))

            def expect(out):
                good = n - 1 if n > 2 else n
                assert np.array_equal(out[0][:good], pts[:good]) and not out[1][:good].any(), "the points come back"
                assert out[2] == int(np.count_nonzero(out[1])) and out[3] == (int(np.flatnonzero(out[1])[0]) if out[2] else None), "counters = the status bytes"

            def run_dev(h, st, A):
                d_i, d_o, d_s = A.put(data), A.out(8 * w * n), A.out(n)           # n status bytes followed by arena bytes
                A.ready()
                bad, first = h.point_codec_dev(what, d_i, n, d_o, d_s, 1)
                return A.read(d_o, np.uint64, (n, w)), A.read(d_s, np.uint8, (n,)), bad, first
        else:
            def run(h, st):
                return h.g2_subgroup_check(pts)

            def expect(out):
                assert out == (0, None), "multiples of the generator lie in the subgroup"

            def run_dev(h, st, A):
                d_p = A.put(pts)
                A.ready()
                return h.point_codec_dev(what, d_p, n)

        return Case(run, None, expect, run_dev)
    return build


def _curve_check_build(E, p):
    n = p["n"]
    g1, g2 = E.g1_pts(n).copy(), E.g2_pts(n).copy()
    if n > 2:
        g1[n - 1, 4] ^= np.uint64(1)                     # off the curve
        g2[1, 8] ^= np.uint64(1)

    def setup(h):
        srs = h.srs_g1_upload(g1)
        return {"srs": srs, "free": [srs]}

    def run(h, st):
        return h.srs_g1_check(st["srs"]) + h.g2_check(g2)

    def expect(out):
        assert out == ((1, n - 1, 1, 1) if n > 2 else (0, None, 0, None)), "the one changed point of each array"

    return Case(run, setup, expect)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _n_shapes(ns, big, key="n", **more):
    ns = list(ns)
    return [("%s%d" % (key, n), dict({key: n}, **more), dict({key: (ns[i + 1] if i + 1 < len(ns) else big), "seed": 1, "off": 3}, **more)) for i, n in enumerate(ns)]


def rows():
    pair_shapes = [("n%d-%s" % (n, "wide" if wide else "k_pairing"), {"n": n, "wide": wide}, {"n": big, "wide": wide, "off": 3})
                   for wide in (0, 1 << 20) for n, big in ((1, 3), (3, 65), (65, 130))]
    kem = [("n1", {"n": 1}, {"n": 65, "which": 2}), ("n65", {"n": 65}, {"n": 300, "which": 2}), ("n300", {"n": 300}, {"n": 520, "which": 2})]
    multi = [("groups-0-1-62-65", {"sizes": [0, 1, 62, 65]}, {"sizes": [3, 70, 0, 100, 2]})]
    coset = [("n3-l4", {"n": 3, "l": 4}, {"n": 9, "l": 8}), ("n65-l16", {"n": 65, "l": 16}, {"n": 130, "l": 16})]       # below and above the 64-item tile of l = 16
    sets = [("k3-n65", {"k": 3, "n": 65}, {"k": 3, "n": 130}), ("k17-n2", {"k": 17, "n": 2}, {"k": 17, "n": 5})]
    ks = [("k3", {"k": 3}, {"k": 9}), ("k9", {"k": 9}, {"k": 17})]                                              # below and above the 8-point pass
    codec = _n_shapes((1, 65, 300), 520)
    fk_batch = [("log2d3-m65", {"log2d": 3, "m": 65}, {"log2d": 4, "m": 70, "seed": 1})]
    return [
        Row("msm_g1", ("msm_g1", "msm_g1_dev"), _msm_shapes("g1"), _msm_build("g1"), "oracle: msm_g1; heavy-counts: the discrete log of tests/heavy_cases.py"),
        Row("msm_g2", ("msm_g2", "msm_g2_dev"), _msm_shapes("g2"), _msm_build("g2"), "oracle: msm_g2"),
        Row("g1_sum", ("g1_sum", "g1_sum_dev"), [("k1", {"k": 1}, {"k": 65, "off": 5}), ("k65", {"k": 65}, {"k": 300, "off": 5})], _g1_sum_build, "oracle: g1_sum"),
        Row("kzg_open", ("kzg_open",),
            [("n%d-%s" % (n, "chunks3" if ch else "resident"), {"n": n, "chunks": ch}, {"n": big, "chunks": ch, "seed": 1})
             for ch in (0, 3) for n, big in ((1, 2), (2, 33), (33, 1025), (1025, 2100))], _open_build, "Python synthetic division, then oracle: msm_g1"),
        Row("kzg_quotient", ("kzg_quotient",), _n_shapes((1, 2, 33, 1025), 2100), _quotient_build, "Python synthetic division, every coefficient"),
        Row("msm_g1_batch", ("msm_g1_batch", "msm_g1_batch_dev"), [("m3-n33", {"m": 3, "n": 33}, {"m": 65, "n": 64, "seed": 1}), ("m65-n64", {"m": 65, "n": 64}, {"m": 70, "n": 130, "seed": 1})],
            _batch_build("msm"), "oracle: msm_g1 per row"),
        Row("kzg_open_batch", ("kzg_open_batch", "kzg_open_batch_dev"), [("m3-n33", {"m": 3, "n": 33}, {"m": 65, "n": 64, "seed": 1}), ("m65-n64", {"m": 65, "n": 64}, {"m": 70, "n": 130, "seed": 1})],
            _batch_build("open"), "Python synthetic division, then oracle: msm_g1 per row"),
        Row("open_fk_poly", ("open_fk_poly",),
            [("log2d%d-gtab%d" % (l, g), {"log2d": l, "gtab": g}, {"log2d": l + 1, "gtab": g, "seed": 1}) for l in (3, 9) for g in (1, 0)], _fk_poly_build,
            "log2d 3: oracle MSM of every quotient; log2d 9: tests/test_gpu_variants.py::test_open_fk_ladder_variants"),
        Row("open_fk", ("open_fk",), [("log2d3", {"log2d": 3}, {"log2d": 5, "seed": 1})], _fk_raw_build, "oracle MSM of every quotient"),
        Row("vec_commit", ("vec_commit",), [("log2d3-n5", {"log2d": 3, "n": 5}, {"log2d": 6, "n": 40, "seed": 1})], _vec_commit_build,
            "tests/test_gpu_keaki_api.py::test_vec_commit_device_fft_branch, tests/test_gpu_fk_batch.py::test_against_the_oracle_directly"),
        Row("open_fk_poly_batch", ("open_fk_poly_batch", "open_fk_poly_batch_dev"), fk_batch, _fk_batch_build("open"),
            "tests/test_gpu_fk_batch.py::test_open_batch_equals_single_calls[3-65]"),
        Row("vec_commit_batch", ("vec_commit_batch", "vec_commit_batch_dev"), fk_batch, _fk_batch_build("vec"),
            "tests/test_gpu_fk_batch.py::test_vec_commit_batch_equals_single_calls[3-65]"),
        Row("open_fk_cosets_poly", ("open_fk_cosets_poly", "open_fk_cosets_poly_dev"), [("log2d6-log2l2", {"log2d": 6, "log2l": 2}, {"log2d": 7, "log2l": 2, "seed": 1})],
            _fk_coset_build(False), "tests/test_gpu_fk_coset.py::test_poly_against_long_division[6-2]"),
        Row("open_fk_cosets", ("open_fk_cosets",), [("log2d6-log2l2", {"log2d": 6, "log2l": 2}, {"log2d": 7, "log2l": 2, "seed": 1})], _fk_coset_build(True),
            "tests/test_gpu_fk_coset.py::test_raw_entry_with_random_tau[6-2]"),
        Row("vec_update", ("vec_update", "vec_update_dev"),
            [("log2d6-one-pass", {"log2d": 6, "k": 3}, {"log2d": 7, "k": 20, "seed": 1}), ("log2d6-two-passes", {"log2d": 6, "k": 9}, {"log2d": 7, "k": 20, "seed": 1})],
            _vec_update_build, "tests/test_gpu_vec_update.py::test_shapes[6], ::test_passes"),
        Row("fr_fft", ("fr_fft",), [("log2n5", {"log2n": 5}, {"log2n": 8})], _fr_fft_build, "oracle: fr_fft, and the O(n^2) definition"),
        Row("g1_mul_batch", ("g1_mul_batch", "g1_mul_batch_dev"), _n_shapes((1, 65), 300), _mul_build("g1"), "oracle: g1_mul_batch"),
        Row("g2_mul_batch", ("g2_mul_batch", "g2_mul_batch_dev"), _n_shapes((1, 65), 300), _mul_build("g2"), "oracle: g2_mul_batch"),
        Row("pairing_batch", ("pairing_batch", "pairing_batch_dev"), pair_shapes, _pairing_build, "oracle: pairing_batch"),
        Row("pairing_product", ("pairing_product", "pairing_product_dev"), [("n1", {"n": 1}, {"n": 129, "off": 3}), ("n129", {"n": 129}, {"n": 300, "off": 3})],
            _pairing_product_build, "oracle: one pairing of the summed exponent"),
        Row("pairing_stages", ("miller_loop_batch", "final_exp_batch", "g2_prepare"), [("n3", {"n": 3}, {"n": 65, "off": 9})], _pairing_stages_build,
            "oracle: pairing_batch; the line table: tests/test_gpu_parity.py::test_g2_line_table_vs_oracle"),
        Row("encap_batch", ("encap_batch", "encap_batch_dev"), kem, _encap_build(False), "oracle: encap_batch"),
        Row("decap_batch", ("decap_batch", "decap_batch_dev"), kem, _decap_build(False), "oracle: encap_batch and decap_batch"),
        Row("encrypt_batch", ("encrypt_batch", "encrypt_batch_dev"), kem, _encap_build(True), "oracle: encap_batch, body = key XOR message"),
        Row("decrypt_batch", ("decrypt_batch", "decrypt_batch_dev"), kem, _decap_build(True), "oracle: encap_batch, the messages come back"),
        Row("encap_multi", ("encap_multi", "encap_multi_dev"), multi, _encap_multi_build(False), "oracle: encap_batch per group"),
        Row("encrypt_multi", ("encrypt_multi", "encrypt_multi_dev"), multi, _encap_multi_build(True), "oracle: encap_batch per group"),
        Row("kzg_verify", ("kzg_verify",), [("valid-and-invalid", {}, {"larger": True})], _verify_build, "tests/verify_batch_model.py: the verdicts"),
        Row("kzg_verify_batch", ("kzg_verify_batch", "kzg_verify_batch_dev"), [("n3", {"n": 3}, {"n": 65}), ("n65", {"n": 65}, {"n": 200})], _verify_batch_build,
            "tests/verify_batch_model.py: verdict, L and R"),
        Row("kzg_verify_each", ("kzg_verify_each", "kzg_verify_each_dev"), [("n3", {"n": 3}, {"n": 65}), ("n65", {"n": 65}, {"n": 200})], _verify_each_build,
            "tests/verify_each_model.py: status bytes and counters; L_i: tests/test_gpu_verify_each.py::test_lhs_out_is_bit_exact"),
        Row("kzg_verify_cosets", ("kzg_verify_cosets", "kzg_verify_cosets_dev"), coset, _coset_family_build("verify"), "tests/coset_verify_model.py: verdict, L and R"),
        Row("kzg_verify_cosets_each", ("kzg_verify_cosets_each", "kzg_verify_cosets_each_dev"), coset, _coset_family_build("each"),
            "tests/coset_pairs_model.py: status bytes, counters and L_k"),
        Row("kzg_coset_pairs", ("kzg_coset_pairs", "kzg_coset_pairs_dev"), coset, _coset_family_build("pairs"), "tests/coset_pairs_model.py: A_k and c_k"),
        Row("kzg_verify_sets", ("kzg_verify_sets", "kzg_verify_sets_dev"), sets, _set_family_build("verify"), "tests/verify_sets_model.py: verdict and the k + 1 sums"),
        Row("kzg_verify_sets_each", ("kzg_verify_sets_each", "kzg_verify_sets_each_dev"), sets, _set_family_build("each"),
            "tests/set_pairs_model.py: status bytes, counters and the pairs"),
        Row("kzg_set_pairs", ("kzg_set_pairs", "kzg_set_pairs_dev"), sets, _set_family_build("pairs"), "tests/set_pairs_model.py: A_i and Z2_i"),
        Row("kzg_set_polys", ("kzg_set_polys", "kzg_set_polys_dev"), ks, _kzg_set_build("polys"), "tests/kzg_set_model.py: Z, weights and I"),
        Row("kzg_open_multi", ("kzg_open_multi", "kzg_open_multi_dev"), [("n33-k3", {"n": 33, "k": 3}, {"n": 200, "k": 9}), ("n1025-k9", {"n": 1025, "k": 9}, {"n": 1100, "k": 17})],
            _kzg_set_build("open"), "tests/kzg_set_model.py: long division by Z"),
        Row("kzg_aggregate", ("kzg_aggregate", "kzg_aggregate_dev"), ks, _kzg_set_build("aggregate"), "tests/kzg_set_model.py: the set proof's discrete log"),
        Row("kzg_verify_multi", ("kzg_verify_multi",), ks, _kzg_set_build("verify_multi"),
            "the verdicts; the pair: tests/test_gpu_kzg_set.py::test_verify_multi_accepts_and_rejects"),
        Row("g1_compress", ("g1_compress", "g1_compress_dev"), codec, _codec_build("g1_compress"), "tests/point_codec_model.py"),
        Row("g2_compress", ("g2_compress", "g2_compress_dev"), codec, _codec_build("g2_compress"), "tests/point_codec_model.py"),
        Row("g1_decompress", ("g1_decompress", "g1_decompress_dev"), codec, _codec_build("g1_decompress"), "the points that were compressed"),
        Row("g2_decompress", ("g2_decompress", "g2_decompress_dev"), codec, _codec_build("g2_decompress"), "the points that were compressed"),
        Row("g2_subgroup_check", ("g2_subgroup_check", "g2_subgroup_check_dev"), codec, _codec_build("g2_subgroup_check"), "multiples of the generator"),
        Row("curve_check", ("srs_g1_check", "g2_check"), [("n65", {"n": 65}, {"n": 300})], _curve_check_build, "one changed point per array"),
    ]


# every other function of include/keaki_hip.h, with the reason it has no row
EXEMPT = {
    "ctx_create": "creates the context: no workspace exists yet", "ctx_destroy": "frees the context",
    "last_error": "reads a host string", "synchronize": "waits for the stream", "ctx_stream": "returns a handle", "ctx_device": "returns an ordinal",
    "version": "returns a constant string", "ctx_set_option": "option setter (host state)", "debug_set_alloc_limit": "option setter (host state)",
    "debug_poison_workspaces": "the hook itself", "ctx_memory": "adds up capacities", "ctx_trim": "frees the workspaces",
    "set_timing": "option setter (host state)", "last_msm_bucket_ms": "reads a host figure", "last_msm_total_ms": "reads a host figure",
    "last_msm_window_bits": "reads a host figure", "last_fk_ms": "reads host figures",
    "srs_g1_upload": "allocates the handle's own points", "srs_g1_wrap_dev": "wraps caller memory", "srs_g1_slice": "a view of a handle",
    "srs_g1_len": "reads the handle", "srs_g1_free": "frees the handle", "srs_g2_upload": "allocates the handle's own points",
    "srs_g2_wrap_dev": "wraps caller memory", "srs_g2_free": "frees the handle",
    "srs_g1_precompute": "builds a table the handle owns; runs inside the msm_g1 rows with tables, on poisoned memory",
    "srs_g2_precompute": "builds a table the handle owns; runs inside the msm_g2 rows with tables, on poisoned memory",
    "srs_g1_precompute_fk": "the handle's FK23 transform: open_fk_poly builds it on first use, inside its row",
    "srs_g1_precompute_fk_cosets": "the handle's coset transforms: open_fk_cosets_poly builds them on first use, inside its row",
    "srs_g1_precompute_update": "the handle's vec_update tables: vec_update builds them on first use, inside its row",
    "srs_g1_precompute_cosets": "the handle's window table: kzg_coset_pairs builds it on first use, inside its row",
    "srs_g2_precompute_sets": "the G2 handle's window table: kzg_set_pairs builds it on first use, inside its row",
    "encap_prepare": "builds the cached tables of KemState only, which the hook leaves alone",
    "fk_shard_create": "sharded FK23: its buffers belong to the shard handle; needs one context per rank",
    "fk_shard_free": "frees the shard handle", "fk_shard_sizes": "reads the shard handle",
    "fk_shard_setup": "sharded FK23: its buffers belong to the shard handle", "fk_shard_open": "sharded FK23: its buffers belong to the shard handle",
    "selftest_field": "a probe with its own operands: owns no workspace row", "selftest_field_ops": "a probe on the caller's records",
    "selftest_tower_ops": "a probe on the caller's records", "selftest_point_ops": "a probe on the caller's records",
}
for _f in ("create", "destroy", "size", "ctx", "last_error", "peer_note", "srs_g1_upload", "srs_g1_len", "srs_g1_has_tables", "srs_g1_free", "msm_g1", "kzg_open",
           "encap_batch", "decap_batch", "encrypt_batch", "decrypt_batch", "fk_create", "fk_open", "fk_free"):
    EXEMPT["group_" + _f] = "device groups: several contexts, each runs the single-context calls of the rows above"
EXEMPT = {"keaki_hip_" + k: v for k, v in EXEMPT.items()}


def covered():
    """{function: family} over the table"""
    out = {}
    for r in rows():
        for f in r.functions:
            out[f] = r.family
    return out


def header_functions(path=None):
    """every keaki_hip_* function include/keaki_hip.h declares"""
    import re
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "keaki_hip.h")
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(keaki_hip_[a-z0-9_]+)\s*\(", hdr)))


def check_against_header(path=None, table=None, exempt=None):
    """-> the list of complaints (empty: the table and the exemptions partition the header's functions)"""
    fns = header_functions(path)
    cov = covered() if table is None else table
    ex = EXEMPT if exempt is None else exempt
    bad = ["%s: neither in a row of the table nor exempt" % f for f in fns if f not in cov and f not in ex]
    bad += ["%s: in a row and exempt" % f for f in fns if f in cov and f in ex]
    bad += ["%s: not a function of the header" % f for f in list(cov) + list(ex) if f not in fns]
    bad += ["%s: exempt without a reason" % f for f, why in ex.items() if not (isinstance(why, str) and why.strip())]
    return bad


def case_ids():
    return [(r, s) for r in rows() for s in r.shapes]
