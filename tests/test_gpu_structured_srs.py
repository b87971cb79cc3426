"""The group kernels on bases with known discrete logs (tests/structured_inputs.py): structured SRS secrets, related bases and identity
results, where additions meet equal points, opposite points and identities produced mid-computation. Every case is compared with the
scalar reference (the expected point is (its scalar) * G, from the oracle's scalar multiplication), and with the oracle where cheap."""
import os

import numpy as np
import pytest

import structured_inputs as S
from test_gpu_fk_shard import DevMem, sharded_open_all_ranks
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(32, os.cpu_count() or 1)
RESET = (("msm_c", 0), ("msm_c_shared", 0), ("msm_short_tables", -1), ("msm_pipe_chunks", -1), ("msm_pipe_growth", 160), ("msm_pipe_min", 1 << 20),
         ("fk_addsub29", 1), ("fk_radix4", 1), ("encap_gt", -1), ("pair_wide_max", -1))


@pytest.fixture()
def opts(hip):
    """the session context with the options under the test's control; automatic again afterwards"""
    yield hip
    for k, v in RESET:
        hip.set_option(k, v)


def g1_of(oc, ks):
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, [k % R for k in ks]), threads=TH)


def g2_of(oc, ks):
    _, g2 = oc.generators()
    return oc.g2_mul_batch(g2, mont(oc, [k % R for k in ks]), threads=TH)


def scalar_sets(rand_fr, dl, c, tables, n, seed):
    out = [("random", rand_fr(n, seed))]
    sc = S.collision_scalars(dl, c, tables)
    if sc is not None:
        out.append(("collide", sc))
    return out


# ---- MSM G1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c", [(64, 8), (1000, 10), (1 << 14, 13), ((1 << 16) + 5, 16)])
def test_msm_g1_structured_srs(oc, opts, rand_fr, n, c):
    """no tables, then window tables (shared buckets) of width c, a short polynomial on the tables with msm_short_tables 0 / 1, and the
    chunked entry forced at this size"""
    hip = opts
    hip.set_option("msm_c", c)
    hip.set_option("msm_c_shared", c)
    names = list(S.secrets(c, 6)) if n < (1 << 16) else ["one", "minus_one", "two_pow_c", "random"]
    for name in names:
        tau = S.secrets(c, 6)[name]
        dl = S.powers(tau, n)
        pts = g1_of(oc, dl) if n < (1 << 16) else hip.g1_mul_batch(oc.generators()[0], mont(oc, dl))
        if n >= (1 << 16):
            idx = list(range(0, n, 4099))
            assert np.array_equal(pts[idx], g1_of(oc, [dl[i] for i in idx]))
        srs = hip.srs_g1_upload(pts)
        try:
            cases = scalar_sets(rand_fr, dl, c, False, n, 7000 + n)
            for label, sc in cases:
                exp = g1_of(oc, [S.msm_dlog(dl, sc)])[0]
                assert np.array_equal(jac_to_aff(hip.msm_g1(srs, mont(oc, sc))), exp), (name, label, "generic")
            hip.set_option("msm_pipe_min", 1)
            for chunks in (3, 2):
                hip.set_option("msm_pipe_chunks", chunks)
                hip.set_option("msm_pipe_growth", 100)
                label, sc = cases[-1]
                assert np.array_equal(jac_to_aff(hip.msm_g1(srs, mont(oc, sc))), g1_of(oc, [S.msm_dlog(dl, sc)])[0]), (name, label, chunks)
            hip.set_option("msm_pipe_chunks", 0)
            hip.srs_g1_precompute(srs)
            for label, sc in scalar_sets(rand_fr, dl, c, True, n, 7100 + n):
                exp = g1_of(oc, [S.msm_dlog(dl, sc)])[0]
                assert np.array_equal(jac_to_aff(hip.msm_g1(srs, mont(oc, sc))), exp), (name, label, "tables")
                for chunks in (3,):
                    hip.set_option("msm_pipe_chunks", chunks)
                    assert np.array_equal(jac_to_aff(hip.msm_g1(srs, mont(oc, sc))), exp), (name, label, "tables", chunks)
                    hip.set_option("msm_pipe_chunks", 0)
                m = max(1, n // 3)                                    # a short polynomial: the table path and the generic path
                short = sc[:m]
                exp_s = g1_of(oc, [S.msm_dlog(dl, short)])[0]
                for st in (1, 0):
                    hip.set_option("msm_short_tables", st)
                    assert np.array_equal(jac_to_aff(hip.msm_g1(srs, mont(oc, short))), exp_s), (name, label, "short", st)
                hip.set_option("msm_short_tables", -1)
            if n <= 1000:
                sc = cases[-1][1]
                assert np.array_equal(g1_of(oc, [S.msm_dlog(dl, sc)])[0], oc.msm_g1(pts, mont(oc, sc), threads=TH))
        finally:
            srs.free()
            hip.set_option("msm_pipe_min", 1 << 20)
            hip.set_option("msm_pipe_chunks", -1)


def test_commit_through_the_setup_of_each_secret(oc, rand_fr):
    """kzg::commit on KZGSetup::setup(tau, n): the setup's context has its shared window width pinned to the width the collision scalars
    are built for (the setup builds its window tables with it)"""
    import keaki_amd.keaki as K
    n, c = 1000, 10
    dev = K.Device(0)
    dev.hip().set_option("msm_c_shared", c)
    for name, tau in S.secrets(c, 6).items():
        dl = S.powers(tau, n)
        st = K.KZGSetup.setup(mont(oc, [tau])[0], n, device=dev)
        try:
            assert np.array_equal(st.g1_pow()[:64], g1_of(oc, dl[:64])), name
            assert np.array_equal(st.tau_g2(), g2_of(oc, [tau])[0]), name
            assert st.has_window_tables(), name
            for label, sc in scalar_sets(rand_fr, dl, c, True, n, 7300):
                got = K.commit(st, mont(oc, sc))
                assert np.array_equal(got, g1_of(oc, [S.msm_dlog(dl, sc)])[0]), (name, label)
        finally:
            st.close()
    dev.close()


# ---- MSM G2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c", [(64, 8), (1000, 10)])
def test_msm_g2_structured_bases(oc, opts, rand_fr, n, c):
    hip = opts
    hip.set_option("msm_c", c)
    hip.set_option("msm_c_shared", c)
    for name in ("zero", "one", "minus_one", "two_pow_c", "lambda", "half", "random"):
        tau = S.secrets(c, 6)[name]
        dl = S.powers(tau, n)
        pts = g2_of(oc, dl)
        srs = hip.srs_g2_upload(pts)
        try:
            for tables in (False, True):
                if tables:
                    hip.srs_g2_precompute(srs)
                for label, sc in scalar_sets(rand_fr, dl, c, tables, n, 7400 + n):
                    exp = g2_of(oc, [S.msm_dlog(dl, sc)])[0]
                    assert np.array_equal(jac_to_aff(hip.msm_g2(srs, mont(oc, sc))), exp), (name, label, tables)
                    if n <= 64:
                        assert np.array_equal(oc.msm_g2(pts, mont(oc, sc)), exp)
        finally:
            srs.free()


# ---- open / verify ---------------------------------------------------------------------------------------------------------------------
def test_open_and_verify_structured(oc, rand_fr):
    import keaki_amd.keaki as K
    n = 64
    for name, tau in S.secrets(8, 6).items():
        st = K.KZGSetup.setup(mont(oc, [tau])[0], n)
        try:
            for p in (rand_fr(n, 7500), [9], [0, 1], [1] * n):
                com = K.commit(st, mont(oc, p))
                assert np.array_equal(com, g1_of(oc, [S.poly_eval(p, tau)])[0]), (name, p[:2])
                for z in {tau, (tau + 3) % R, (R - tau) % R}:
                    proof = K.open(st, mont(oc, p), mont(oc, [z])[0])
                    assert np.array_equal(proof, g1_of(oc, [S.open_dlog(tau, p, z)])[0]), (name, z)
                    v = S.poly_eval(p, z)
                    assert K.verify(st, com, mont(oc, [z])[0], mont(oc, [v])[0], proof), (name, z)
                    assert not K.verify(st, com, mont(oc, [z])[0], mont(oc, [(v + 1) % R])[0], proof), (name, z)
        finally:
            st.close()


# ---- FK23 ------------------------------------------------------------------------------------------------------------------------------
def fk_poly(kind, d):
    from conftest import rand_fr_ints
    return rand_fr_ints(d, 7600 + d) if kind == "rand" else [1] * d if kind == "ones" else [7] + [0] * (d - 1)


@pytest.mark.parametrize("log2d", [2, 3, 6, 9, 12])
def test_open_fk_structured_srs(oc, opts, log2d):
    hip = opts
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    roots = [mont(oc, [x])[0] for x in (w2, pow(w2, -1, R), pow(2 * d, -1, R))]
    import keaki_amd.keaki as K
    dev = K.Device(0)
    for name, tau in S.secrets(8, log2d).items():
        dl = S.powers(tau, d)
        pts = g1_of(oc, dl)
        exps = {}
        for kind in ("rand", "ones", "const"):
            p = fk_poly(kind, d)
            exps[kind] = (p, g1_of(oc, S.fk_dlogs(tau, p, S.ntt(p, S.root_of_unity(d)))))
        for addsub in (1, 0):
            for radix4 in (1, 0):
                hip.set_option("fk_addsub29", addsub)
                hip.set_option("fk_radix4", radix4)
                srs = hip.srs_g1_upload(pts)                # a new handle: hat_s is computed under these options
                try:
                    for kind, (p, exp) in exps.items():
                        got = hip.open_fk_poly(srs, log2d, mont(oc, p), *roots)
                        assert np.array_equal(got, exp), (name, kind, addsub, radix4)
                finally:
                    srs.free()
        # kzg::open_fk through KZGSetup::setup(tau, d) on a context of its own, options automatic
        st = K.KZGSetup.setup(mont(oc, [tau])[0], d, device=dev)
        try:
            for kind, (p, exp) in exps.items():
                assert np.array_equal(K.open_fk(st, mont(oc, p), d), exp), (name, kind, "open_fk")
        finally:
            st.close()
    dev.close()


@pytest.mark.parametrize("log2d,R_", [(6, 2), (8, 4)])
def test_sharded_fk_structured_srs(oc, hip, log2d, R_):
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    roots = [mont(oc, [x])[0] for x in (w2, pow(w2, -1, R), pow(2 * d, -1, R))]
    tau = S.secrets(8, log2d)["omega_d"]
    dl = S.powers(tau, d)
    srs = hip.srs_g1_upload(g1_of(oc, dl))
    mem = DevMem()
    try:
        ps = [fk_poly("ones", d), fk_poly("const", d)]
        got = sharded_open_all_ranks(hip, mem, srs, log2d, R_, [mont(oc, p) for p in ps], roots, n_polys=2)
        for p, g in zip(ps, got):
            assert np.array_equal(g, g1_of(oc, S.fk_dlogs(tau, p, S.ntt(p, S.root_of_unity(d)))))
    finally:
        mem.free()
        srs.free()


# ---- encapsulation / decapsulation -----------------------------------------------------------------------------------------------------
# (tau, c, z, v, r) per item: related bases, z = tau (ct = O), v = c (GT one), and the constructed items of the encap model
# (tests/test_structured_inputs_model.py: ENCAP_CASES). The small batches take secrets that no 256-item batch uses: a context that holds the
# 16-bit table of a [tau]_2 uses it for small batches too, and the small batches are there for the 8-bit tables.
KEM_SMALL = [(3, 5, R - 3, 3, 5), (768, 2, R - 768, 2, 5), (11, 11, 11, 3, 9), (11, 1, 2, 1, 9), (11, 2, 11, 2, 9)]
KEM_LARGE = [(1, 5, R - 1, 3, 5), (256, 2, R - 256, 2, 5), (7, 11, 7, 3, 9), (2, 0, R - 2, 0, 3), (7, 1, 2, 1, 9), (R - 1, R - 1, 1, 2, 4),
             (7, 2, 7, 2, 9)]


def kem_items(n, small):
    from conftest import rand_fr_ints
    base, tau = (KEM_SMALL, 11) if small else (KEM_LARGE, 7)
    extra = rand_fr_ints(max(0, n - len(base)), 7700)
    return base + [(tau, 2, (e * tau) % R, e, e) for e in extra][: n - len(base)]


@pytest.mark.parametrize("path", ["wide8", "wide16", "lane16"])
@pytest.mark.parametrize("gt_path", [True, False])
def test_encap_decap_related_bases(oc, opts, path, gt_path):
    """wide8: < 256 items (8-bit tables, sixteen lanes per item); wide16: 256 items (16-bit tables, sixteen lanes); lane16: 256 items,
    one lane per item (pair_wide_max = 0). gt_path: the GT fixed-base exponentiation, else the per-item pairing (encap_gt = 2^40)"""
    hip = opts
    n = 16 if path == "wide8" else 256
    if path == "lane16":
        hip.set_option("pair_wide_max", 0)
    if not gt_path:
        hip.set_option("encap_gt", 1 << 40)
    items = kem_items(n, path == "wide8")
    by_setup = {}
    for it in items:
        by_setup.setdefault((it[0], it[1]), []).append(it)
    for (tau, c), its in by_setup.items():
        if len(its) < n and path != "wide8":
            its = (its * (n // len(its) + 1))[:n]            # one batch of n items per (setup, commitment)
        com = g1_of(oc, [c])[0]
        tg2 = g2_of(oc, [tau])[0]
        zs = mont(oc, [it[2] for it in its]); vs = mont(oc, [it[3] for it in its]); rs = mont(oc, [it[4] for it in its])
        ct, gt, key = hip.encap_batch(com, tg2, zs, vs, rs, 32)
        assert np.array_equal(ct, g2_of(oc, [it[4] * (tau - it[2]) for it in its])), (tau, c)
        egt = oc.pairing_batch(g1_of(oc, [it[4] * (c - it[3]) for it in its]), oc.generators()[1], threads=TH)
        assert np.array_equal(gt, egt), (tau, c)
        assert all(key[i].tobytes() == oc.blake3_xof(gt[i].tobytes(), 32) for i in range(0, len(its), 37))
        ect, egt2, ekey = oc.encap_batch(com, tg2, zs[:8], vs[:8], rs[:8], 32, threads=TH)
        assert np.array_equal(ct[:8], ect) and np.array_equal(gt[:8], egt2) and np.array_equal(key[:8], ekey)
        # decapsulation with the opening proofs (the identity where the quotient is zero or tau = z)
        proofs = g1_of(oc, [0 if tau == it[2] else (c - it[3]) * pow(tau - it[2], -1, R) for it in its])
        dgt, dkey = hip.decap_batch(proofs, ct, 32)
        odgt, odkey = oc.decap_batch(proofs, ct, 32, threads=TH)
        assert np.array_equal(dgt, odgt) and np.array_equal(dkey, odkey)
        for i, it in enumerate(its):
            if tau != it[2]:
                assert np.array_equal(dkey[i], key[i]), (tau, c, i)
