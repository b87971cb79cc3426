"""The cached FK23 transform of a G1 SRS handle (keaki_amd/csrc/api_host.h: SrsCache, srs_cache_ensure) and the handle code that G1 and G2 share
(srs_upload / srs_wrap / srs_precompute / srs_free): one handle whose d changes, the four entries that share one transform, a rebuild
that keaki_hip_debug_set_alloc_limit refuses, and both groups through upload, wrap, precompute, MSM and free. `tables` below is
keaki_hip_ctx_memory's first word minus its value before the handles were made: a transform for d counts 2d Jacobian points of 96 B."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SRS = 16


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs(ints)) if len(ints) else np.zeros((0, 4), np.uint64)


def aff(j):
    from keaki_amd.hip import jac_to_affine_words
    return jac_to_affine_words(j)


@pytest.fixture(scope="module")
def srs_pts(oc, rand_fr):
    """any 16 points serve as an "SRS" for the linear-algebra identity of FK23 (made by the oracle: nothing here depends on a GPU)"""
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, rand_fr(N_SRS, 2300)))


@pytest.fixture(scope="module")
def fk_case(oc, py, rand_fr, srs_pts):
    """log2d -> (coefficients, (omega_2d, 1 / omega_2d, 1 / 2d) in Montgomery limbs, the oracle's literal FK23 proofs as integers for d <= 8)"""
    cache = {}

    def make(log2d):
        if log2d not in cache:
            d = 1 << log2d
            p = rand_fr(d, 2310 + log2d)
            w2 = py.fr_root_of_unity(2 * d)
            roots = tuple(mont(oc, [x])[0] for x in (w2, pow(w2, -1, py.R), pow(2 * d, -1, py.R)))
            exp = py.kzg_open_fk(oc.g1_to_ints(srs_pts)[:d], p) if d <= 8 else None
            cache[log2d] = (p, roots, exp)
        return cache[log2d]
    return make


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


def open_poly(oc, h, srs, fk_case, log2d):
    p, roots, _ = fk_case(log2d)
    return h.open_fk_poly(srs, log2d, mont(oc, p), *roots)


def hat_bytes(log2d):
    return 2 * (1 << log2d) * 96


def test_one_handle_changing_d(oc, fk_case, srs_pts, ctx_tables):
    """a handle asked for another d releases its transform and builds the new one: the count follows, the proofs do not change"""
    h, tables = ctx_tables
    srs = h.srs_g1_upload(srs_pts)
    try:
        first = open_poly(oc, h, srs, fk_case, 3)
        assert tables() == hat_bytes(3)
        assert oc.g1_to_ints(first) == fk_case(3)[2]
        assert np.array_equal(open_poly(oc, h, srs, fk_case, 3), first) and tables() == hat_bytes(3)
        small = open_poly(oc, h, srs, fk_case, 2)
        assert tables() == hat_bytes(2)                    # the old transform is released, not added
        assert oc.g1_to_ints(small) == fk_case(2)[2]
        assert np.array_equal(open_poly(oc, h, srs, fk_case, 3), first) and tables() == hat_bytes(3)
    finally:
        srs.free()
    assert tables() == 0


def test_four_entries_share_the_cache(oc, py, fk_case, srs_pts, ctx_tables):
    """srs_g1_precompute_fk builds the transform; open_fk (explicit twiddles), open_fk_poly and vec_commit at that d find it"""
    h, tables = ctx_tables
    log2d, d = 3, 8
    p, roots, exp = fk_case(log2d)
    w2 = py.fr_root_of_unity(2 * d)
    w2i, inv, wd = pow(w2, -1, py.R), pow(2 * d, -1, py.R), py.fr_root_of_unity(d)
    a = [0] * d + p
    hat_a = [sum(a[i] * pow(w2, i * j, py.R) for i in range(2 * d)) * inv % py.R for j in range(2 * d)]
    tw, twi = [pow(w2, k, py.R) for k in range(d)], [pow(w2i, k, py.R) for k in range(d)]
    evals = [sum(p[i] * pow(wd, i * j, py.R) for i in range(d)) % py.R for j in range(d)]        # vec_commit's iFFT gives p back
    srs = h.srs_g1_upload(srs_pts)
    try:
        h.srs_g1_precompute_fk(srs, log2d, roots[0])
        assert tables() == hat_bytes(log2d)
        explicit = h.open_fk(srs, log2d, mont(oc, hat_a), mont(oc, tw), mont(oc, twi), mont(oc, tw[::2]))
        assert tables() == hat_bytes(log2d)
        poly = h.open_fk_poly(srs, log2d, mont(oc, p), *roots)
        assert tables() == hat_bytes(log2d)
        com, vec = h.vec_commit(srs, mont(oc, evals), None, log2d, mont(oc, [pow(wd, -1, py.R)])[0], mont(oc, [pow(d, -1, py.R)])[0], *roots)
        assert tables() == hat_bytes(log2d)
        assert np.array_equal(explicit, poly) and np.array_equal(vec, poly) and oc.g1_to_ints(poly) == exp
        assert np.array_equal(aff(com), aff(h.msm_g1(srs, mont(oc, p))))
        assert np.array_equal(aff(com), oc.msm_g1(srs_pts[:d], mont(oc, p)))
    finally:
        srs.free()
    assert tables() == 0


def test_refused_rebuild(oc, fk_case, srs_pts, ctx_tables):
    """the transform's allocation passes the library's allocation gate: a refused rebuild fails with KEAKI_ERR_OOM, leaves the handle without a
    transform and the count without its bytes, touches no other handle, and the next call builds it"""
    from keaki_amd.hip import KeakiHipError
    h, tables = ctx_tables
    sa, sb = h.srs_g1_upload(srs_pts), h.srs_g1_upload(srs_pts)
    try:
        b3 = open_poly(oc, h, sb, fk_case, 3)              # warms every workspace of a call at d = 8 ...
        assert tables() == hat_bytes(3)
        a4 = open_poly(oc, h, sa, fk_case, 4)              # ... and of the larger one: the transform is the only allocation left
        assert tables() == hat_bytes(3) + hat_bytes(4)
        h.debug_set_alloc_limit(1024)
        with pytest.raises(KeakiHipError) as e:
            open_poly(oc, h, sa, fk_case, 3)
        assert e.value.status == -3 and "keaki_hip_debug_set_alloc_limit" in e.value.message
        assert tables() == hat_bytes(3)                    # A counts nothing, B's transform is unchanged
        assert np.array_equal(open_poly(oc, h, sb, fk_case, 3), b3) and tables() == hat_bytes(3)
        h.debug_set_alloc_limit(0)
        a3 = open_poly(oc, h, sa, fk_case, 3)
        assert oc.g1_to_ints(a3) == fk_case(3)[2] and np.array_equal(a3, b3)
        assert tables() == 2 * hat_bytes(3)
        assert np.array_equal(open_poly(oc, h, sa, fk_case, 4), a4) and tables() == hat_bytes(3) + hat_bytes(4)
        fresh = h.srs_g1_upload(srs_pts)                   # d = 16 is beyond the literal oracle: the same call on a fresh handle
        try:
            assert np.array_equal(open_poly(oc, h, fresh, fk_case, 4), a4)
        finally:
            fresh.free()
    finally:
        sa.free(); sb.free()
    assert tables() == 0


def test_g1_and_g2_handles_through_the_shared_code(oc, rand_fr, ctx_tables):
    """upload (n = 0 and n = 3), wrap_dev, precompute twice, an MSM on every handle, free -- by the context that built the tables and by
    another context of the device -- for both groups"""
    import torch
    from keaki_amd.hip import KeakiHip
    h, tables = ctx_tables
    other = KeakiHip(0)
    n = 48
    g1, g2 = oc.generators()
    ks, sc = mont(oc, rand_fr(n, 2400)), mont(oc, rand_fr(n, 2401))
    try:
        for name, gen, mul, msm_ref in (("g1", g1, oc.g1_mul_batch, oc.msm_g1), ("g2", g2, oc.g2_mul_batch, oc.msm_g2)):
            upload, wrap = getattr(h, "srs_%s_upload" % name), getattr(h, "srs_%s_wrap_dev" % name)
            precompute, msm = getattr(h, "srs_%s_precompute" % name), getattr(h, "msm_%s" % name)
            pts = mul(gen, ks)
            ref = {m: msm_ref(pts[:m], sc[:m]) for m in (3, n)}          # once per group, shared by both rounds
            d_pts = torch.from_numpy(pts.view(np.int64)).to(torch.device("cuda", 0))
            for free_with in (h, other):
                handles = [(upload(pts[:0]), 0), (upload(pts[:3]), 3), (wrap(d_pts.data_ptr(), n), n)]
                try:
                    assert tables() == 0
                    for srs, m in handles:
                        before = tables()
                        nbytes = precompute(srs)
                        assert (nbytes > 0) == (m > 0) and tables() == before + nbytes, (name, m)
                        assert precompute(srs) == nbytes and tables() == before + nbytes, (name, m)
                        got = aff(msm(srs, sc[:m]))
                        if m:
                            assert np.array_equal(got, ref[m]), (name, m)
                        else:
                            assert not np.any(got), name
                finally:
                    for srs, _ in handles:
                        srs.owner = free_with          # whichever context frees the handle, the bytes leave the one that built the tables
                        srs.free()
                assert tables() == 0, (name, free_with is other)
    finally:
        other.close()
