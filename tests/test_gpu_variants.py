"""Every kernel variant a tuning switch or a window width selects, pinned to the scalar reference (tests/variant_cases.py lists the cases
and the instantiation each one reaches; tests/test_variant_cases_model.py checks that list against the launches in the sources).

Bases have known discrete logs, so the expected MSM is (sum s_i k_i) G from one oracle scalar multiplication at any n; affine results are
compared bit for bit. The module runs on a private context: the session context's switches are never touched."""
import os

import numpy as np
import pytest

import structured_inputs as S
import variant_cases as V
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(32, os.cpu_count() or 1)
DEFAULTS = {"msm_c": 0, "msm_c_shared": 0, "msm_short_tables": -1, "reduce_l": 0, "part_shift": -1, "acc_u29": 1, "acc_nt": 0,
            "acc_prefetch": 1, "acc_idxq": 1, "cs_masked": 1, "msm_pipe_chunks": 0, "msm_pipe_min": 1 << 20, "msm_pipe_growth": 160,
            "fk_uniform": 1, "fk_gtab": 1, "fk_addsub29": 1, "fk_radix4": 1, "fb_occ1": 0}


@pytest.fixture(scope="module")
def vh():
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    yield h
    h.close()


def apply(h, opts=None):
    for k, v in DEFAULTS.items():
        h.set_option(k, (opts or {}).get(k, v))


def g1_of(oc, ks):
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, [k % R for k in ks]), threads=TH)


def g2_of(oc, ks):
    return oc.g2_mul_batch(oc.generators()[1], mont(oc, [k % R for k in ks]), threads=TH)


def dlogs(n, seed):
    """random dlogs with equal (first eight pairs) and opposite (next eight) neighbours, so collision_scalars finds both kinds"""
    from conftest import rand_fr_ints
    dl = rand_fr_ints(n, seed)
    for j in range(16):
        dl[2 * j + 1] = dl[2 * j] if j < 8 else (R - dl[2 * j]) % R
    return dl


@pytest.fixture(scope="module")
def g1_bases(oc, vh):
    dl = dlogs(V.N_LARGE, 8100)
    pts = vh.g1_mul_batch(oc.generators()[0], mont(oc, dl))
    idx = list(range(0, V.N_LARGE, 257)) + [1, 3, 17, 19]
    assert np.array_equal(pts[idx], g1_of(oc, [dl[i] for i in idx]))
    return dl, pts


def scalar_set(name, dl, c, tables, seed):
    from conftest import rand_fr_ints
    n = len(dl)
    if name == "random":
        return rand_fr_ints(n, seed)
    if name == "edge":
        e = V.digit_edge_scalars(c)
        return (e * (n // len(e) + 1))[:n]
    if name == "collide":
        sc = S.collision_scalars(dl, c, tables)
        assert sc is not None
        return sc
    if name == "heavy":       # three points in four take the scalar 1: > HEAVY_MIN pairs in one bucket at 2^14 points
        rnd = rand_fr_ints(1, seed)[0]
        return [1 if i % 4 else rnd for i in range(n)]
    raise ValueError(name)


def check_msm(oc, h, srs, dl, sc, what, g2=False, c=None):
    got = jac_to_aff(h.msm_g2(srs, mont(oc, sc)) if g2 else h.msm_g1(srs, mont(oc, sc)))
    exp = (g2_of if g2 else g1_of)(oc, [S.msm_dlog(dl, sc)])[0]
    assert np.array_equal(got, exp), what
    if c is not None:
        assert h.last_msm_stats()["window_bits"] == c, (what, h.last_msm_stats()["window_bits"], c)


def expect_refused(h, name, c):
    from keaki_amd.hip import KeakiHipError
    with pytest.raises(KeakiHipError) as e:
        h.set_option(name, c)
    assert e.value.status == -1 and name in e.value.message and str(c) in e.value.message, e.value.message


# ---- window plans, G1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [V.N_SMALL, V.N_LARGE])
def test_g1_every_forced_window_width(oc, vh, g1_bases, n):
    """msm_c 3..24 on the generic path: the plan's width and the reference result, or (widths the bucket sort cannot address) a refusal
    at set_option that leaves the context on its automatic width"""
    dl_all, pts = g1_bases
    dl = dl_all[:n]
    srs = vh.srs_g1_upload(pts[:n])
    try:
        for c in V.G1_WINDOW_C:
            apply(vh)
            if V.width_refused(c, False):
                expect_refused(vh, "msm_c", c)
                check_msm(oc, vh, srs, dl, scalar_set("random", dl, c, False, 8200 + c), ("refused", c), c=V.msm(n)["c"])
                continue
            vh.set_option("msm_c", c)
            model = V.msm(n, {"msm_c": c})
            assert not model["refused"]
            for name in ("random", "edge", "collide"):
                check_msm(oc, vh, srs, dl, scalar_set(name, dl, c, False, 8300 + c), (c, name), c=model["c"])
        for c in (0, 2, 25, -1):                      # outside 3..24: automatic
            apply(vh, {"msm_c": c})
            check_msm(oc, vh, srs, dl, scalar_set("random", dl, 0, False, 8400), ("auto", c), c=V.msm(n)["c"])
    finally:
        apply(vh)
        srs.free()


@pytest.mark.parametrize("c", V.G1_SHARED_C)
def test_g1_every_forced_shared_width(oc, vh, g1_bases, c):
    """msm_c_shared 3..24: window tables of that target over 2^14 points; the whole SRS and a 500-point polynomial on the tables
    (msm_short_tables 1)"""
    dl, pts = g1_bases
    srs = vh.srs_g1_upload(pts)
    try:
        apply(vh)
        if V.width_refused(c, True):
            expect_refused(vh, "msm_c_shared", c)
            c_auto = V.choose_window_shared(V.N_LARGE)
            vh.srs_g1_precompute(srs)
            check_msm(oc, vh, srs, dl, scalar_set("random", dl, c_auto, True, 8500), ("refused", c), c=V.plan(c_auto)["c"])
            return
        vh.set_option("msm_c_shared", c)
        vh.srs_g1_precompute(srs)
        ct = V.choose_window_shared(V.N_LARGE, c)
        for n, opts in ((V.N_LARGE, {}), (V.N_SMALL, {"msm_short_tables": 1})):
            apply(vh, dict(opts, msm_c_shared=c))
            model = V.msm(n, opts, srs_len=V.N_LARGE, table_c=ct)
            assert model["shared"] and not model["refused"]
            for name in ("random", "edge", "collide"):
                check_msm(oc, vh, srs, dl[:n], scalar_set(name, dl[:n], ct, True, 8600 + c), (c, n, name), c=model["c"])
    finally:
        apply(vh)
        srs.free()


# ---- window plans, G2 ------------------------------------------------------------------------------------------------------------------
def test_g2_window_widths(oc, vh):
    """every c whose plan has 11..16 windows, and 3, 8, 17, 19: generic and over window tables"""
    n = V.G2_N
    dl = dlogs(n, 8700)
    pts = g2_of(oc, dl)
    try:
        for c in V.G2_WINDOW_C:
            apply(vh)
            if V.width_refused(c, False):
                expect_refused(vh, "msm_c", c)
            else:
                vh.set_option("msm_c", c)
                srs = vh.srs_g2_upload(pts)
                try:
                    for name in ("random", "edge"):
                        check_msm(oc, vh, srs, dl, scalar_set(name, dl, c, False, 8800 + c), ("g2", c, name), g2=True,
                                  c=V.msm(n, {"msm_c": c}, g2=True)["c"])
                finally:
                    srs.free()
            apply(vh)
            if V.width_refused(c, True):
                expect_refused(vh, "msm_c_shared", c)
                continue
            vh.set_option("msm_c_shared", c)
            srs = vh.srs_g2_upload(pts)
            try:
                vh.srs_g2_precompute(srs)
                for name in ("random", "edge"):
                    check_msm(oc, vh, srs, dl, scalar_set(name, dl, c, True, 8900 + c), ("g2 tables", c, name), g2=True,
                              c=V.msm(n, {}, table_c=c, g2=True)["c"])
            finally:
                srs.free()
    finally:
        apply(vh)


# ---- switch matrix, G1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", V.SWITCHES, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()) or "defaults")
def test_g1_switch_matrix(oc, vh, g1_bases, switch):
    """one switch away from the defaults, crossed with every scalar set: one MSM per bin count of the bucket sort that the plan keeps
    (all four chunk-sort geometries), reduce_l cycling through lengths that leave ragged last chunks and lengths above max_b, then the
    chunked host entry (first / middle / last passes)"""
    dl, pts = g1_bases
    n = V.N_LARGE
    c = V.choose_window(n)
    srs = vh.srs_g1_upload(pts)
    sets = {name: scalar_set(name, dl, c, False, 9000 + i) for i, name in enumerate(V.SCALAR_SETS)}
    exps = {name: g1_of(oc, [S.msm_dlog(dl, sc)])[0] for name, sc in sets.items()}
    mont_sets = {name: mont(oc, sc) for name, sc in sets.items()}
    geoms = set()
    try:
        for opts, name, chunks in V.switch_runs(n):
            if {k: v for k, v in opts.items() if k not in ("part_shift", "reduce_l")} != switch:
                continue
            run = dict(opts)
            if chunks:
                run.update(msm_pipe_chunks=chunks, msm_pipe_min=1, msm_pipe_growth=100)
            apply(vh, run)
            model = V.msm(n, opts, chunk_sizes=V.pipe_chunk_sizes(n, chunks) if chunks else None)
            geoms.update(s["geom"] for s in model["shapes"])
            got = jac_to_aff(vh.msm_g1(srs, mont_sets[name]))
            assert np.array_equal(got, exps[name]), (opts, name, chunks, model["shapes"][0], model["L"])
            assert vh.last_msm_stats()["window_bits"] == model["c"]
        assert geoms == {0, 1, 2, 3}
    finally:
        apply(vh)
        srs.free()


# ---- the one automatic shape no other test reaches ----------------------------------------------------------------------------------------
def test_g1_automatic_shape_2p25_with_tables(oc, vh):
    """2^25 points over window tables in one pass (msm_pipe_chunks 0): c = 22 and 2048 bins, geometry 0 (tests/variant_cases.py:
    AUTO_LARGE). The bases tile 2^16 points with known dlogs: MSM = (sum_j k_j sum_(i = j mod 2^16) s_i) G"""
    from bench import random_fr_limbs
    n, m = 1 << 25, 1 << 16
    assert V.auto_shape(n, True) == (True, 22, 11, 0)
    k = random_fr_limbs(m, 9300)
    s = random_fr_limbs(n, 9301)
    pts = vh.g1_mul_batch(oc.generators()[0], k)
    idx = list(range(0, m, 4099))
    assert np.array_equal(pts[idx], oc.g1_mul_batch(oc.generators()[0], k[idx], threads=TH))
    exp = oc.g1_mul_batch(oc.generators()[0], oc.fr_dot(s, np.tile(k, (n // m, 1))).reshape(1, 4))[0]
    srs = vh.srs_g1_upload(np.tile(pts, (n // m, 1)))
    try:
        apply(vh)
        vh.srs_g1_precompute(srs)
        assert np.array_equal(jac_to_aff(vh.msm_g1(srs, s)), exp)
        assert vh.last_msm_stats()["window_bits"] == 22
    finally:
        srs.free()
        vh.trim()


# ---- FK23 ------------------------------------------------------------------------------------------------------------------------------
def fk_poly(kind, d):
    from conftest import rand_fr_ints
    return rand_fr_ints(d, 7600 + d) if kind == "rand" else [1] * d if kind == "ones" else [7] + [0] * (d - 1)


@pytest.mark.parametrize("log2d", V.FK_LOG2D)
def test_open_fk_ladder_variants(oc, vh, log2d):
    """the structured FK23 cases over fk_uniform x fk_gtab (the per-lane ladders, their window tables in the workspace or in private
    memory), each with and without fk_addsub29; every option set on a fresh SRS handle, so hat_s is computed under it too"""
    d = 1 << log2d
    w2 = S.root_of_unity(2 * d)
    roots = [mont(oc, [x])[0] for x in (w2, pow(w2, -1, R), pow(2 * d, -1, R))]
    try:
        for name, tau in S.secrets(8, log2d).items():
            dl = S.powers(tau, d)
            pts = g1_of(oc, dl)
            exps = []
            for kind in ("rand", "ones", "const"):
                p = fk_poly(kind, d)
                exps.append((kind, mont(oc, p), g1_of(oc, S.fk_dlogs(tau, p, S.ntt(p, S.root_of_unity(d))))))
            for o in V.FK_OPTS:
                apply(vh, o)
                srs = vh.srs_g1_upload(pts)
                try:
                    for kind, pm, exp in exps:
                        assert np.array_equal(vh.open_fk_poly(srs, log2d, pm, *roots), exp), (name, kind, o)
                finally:
                    srs.free()
    finally:
        apply(vh)


# ---- G2 fixed-base kernel of encapsulate -----------------------------------------------------------------------------------------------
def test_encap_g2_fixed_base_occupancy_variants(oc, vh):
    """batches of 100,000 items (one launch: above 2^16, below the chunking threshold): first to a new commitment (its table job runs
    beside the ciphertext kernel), then to the same commitment again, with fb_occ1 0 and 1. Byte-equal ciphertexts across the four runs,
    and a sample equal to r ([tau]_2 - z g2)."""
    from conftest import rand_fr_ints
    n = V.ENCAP_N
    tau = rand_fr_ints(1, 9100)[0]
    zs, vs, rs = (rand_fr_ints(n, 9101 + i) for i in range(3))
    zm, vm, rm = mont(oc, zs), mont(oc, vs), mont(oc, rs)
    tg2 = g2_of(oc, [tau])[0]
    coms = {occ: g1_of(oc, [9200 + occ])[0] for occ in (0, 1)}
    cts = []
    try:
        for occ, new in V.ENCAP_RUNS:
            apply(vh, {"fb_occ1": occ})
            ct, key = vh.encap_batch(coms[occ], tg2, zm, vm, rm, 32, want_gt=False)
            cts.append(ct)
        for ct in cts[1:]:
            assert np.array_equal(ct, cts[0])
        idx = list(range(0, n, n // 63))[:63] + [n - 1]
        assert np.array_equal(cts[0][idx], g2_of(oc, [rs[i] * (tau - zs[i]) for i in idx]))
    finally:
        apply(vh)


# ---- the environment: initial values of the options (TUNE_OPTIONS, api.hip), read once when a context is created -------------------
def test_environment_goes_through_the_option_table(oc, vh, monkeypatch):
    """KEAKI_MSM_C=12 makes a new context run a 2^16-point MSM on 12-bit windows; KEAKI_MSM_C=20, a width the bucket sort cannot address
    and set_option refuses, leaves it on the automatic width, as no variable does. Every option of the shipped table is accepted by
    set_option at its default."""
    from conftest import rand_fr_ints
    from keaki_amd.hip import KeakiHip
    n = 1 << 16
    dl = dlogs(n, 9300)
    sc = rand_fr_ints(n, 9301)
    exp = g1_of(oc, [S.msm_dlog(dl, sc)])[0]
    srs = vh.srs_g1_upload(vh.g1_mul_batch(oc.generators()[0], mont(oc, dl)))      # a handle serves every context of its device
    for k in [k for k in os.environ if k.startswith("KEAKI_")]:
        monkeypatch.delenv(k)
    widths = {}
    try:
        for env in (None, "12", "20"):
            if env is not None:
                monkeypatch.setenv("KEAKI_MSM_C", env)
            h = KeakiHip(0)
            try:
                assert np.array_equal(jac_to_aff(h.msm_g1(srs, mont(oc, sc))), exp), env
                widths[env] = h.last_msm_stats()["window_bits"]
                if env is None:
                    expect_refused(h, "msm_c", 20)
                    for name, default in V.shipped_options().items():
                        h.set_option(name, default)
            finally:
                h.close()
    finally:
        srs.free()
    assert widths["12"] == 12
    assert widths["20"] == widths[None] == V.msm(n)["c"] != 12, widths
