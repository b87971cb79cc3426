"""The bucket reduction of the shared-bucket MSM by row and column sums (k_msm_rowcol* in keaki_amd/csrc/msm.hip.h) against the chunked
running sums (reduce_l = 8), both against the scalar reference: bases have known discrete logs, so the expected point is (sum s_i k_i) G
from one oracle scalar multiplication, compared bit for bit.

A window of B = 2^cr buckets is read as 2^(cr - k) rows of 2^k columns, k = ceil(cr / 2): bucket b = h 2^k + l. Automatic selection
(reduce_l = 0) takes the row / column tail from B0 buckets on. Every case runs at four forced table widths: just below B0 (the chain
under both settings), at B0, and at an odd and an even power of two at or above B0 (rows != columns, rows = columns). Scalars with one
small digit land in window 0 only, whose table row is the base itself: the scalar b + 1 puts P_i into bucket b."""
import numpy as np
import pytest

import structured_inputs as S
from test_gpu_parity import jac_to_aff, mont
from test_gpu_variants import apply, g1_of, g2_of

pytestmark = pytest.mark.gpu
R = S.R
B0_LOG2 = 12                       # ROWCOL_MIN_B of keaki_amd/csrc/msm_host.hip.h
N = 64                             # points per SRS: mostly empty buckets at every width (B >= 2^11)
WIDTHS = (B0_LOG2, B0_LOG2 + 1, B0_LOG2 + 2, B0_LOG2 + 3)          # msm_c_shared: B = 2^(c - 1) -> below B0, B0, and one odd, one even power
REDUCE_L = (0, 8)


@pytest.fixture(scope="module")
def vh():
    """a private context: the session context's switches are never touched"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    yield h
    h.close()


def shared_buckets(c):
    _, W, _, _, widths = S.msm_plan(c)
    return max([1 << (wd - 1) for wd in widths[:-1]] + [1 << widths[-1]])


def rows_cols(c):
    cr = shared_buckets(c).bit_length() - 1
    k = (cr + 1) // 2
    return 1 << (cr - k), 1 << k, k


def test_widths_cover_the_selection():
    bs = [shared_buckets(c) for c in WIDTHS]
    assert bs == [1 << (B0_LOG2 - 1), 1 << B0_LOG2, 1 << (B0_LOG2 + 1), 1 << (B0_LOG2 + 2)]
    shapes = [rows_cols(c)[:2] for c in WIDTHS[1:]]
    assert any(r == q for r, q in shapes) and any(r != q for r, q in shapes)


def cases(c, dl):
    """name -> scalars (len(dl) of them; dl[1] = -dl[0], dl[2] = dl[0]), each checked against the bucket model"""
    NR, NC, k = rows_cols(c)
    B = NR * NC
    n = len(dl)
    out = {}

    def only(pairs):
        s = [0] * n
        for i, v in pairs:
            s[i] = v % R
        return s

    for b in sorted({0, 1, NC - 1, NC, NC + 1, B - 1}):
        sc = only([(0, b + 1)])
        assert {x: len(v) for x, v in S.msm_buckets(dl, sc, c, True).items()} == {b: 1}
        out["single bucket %d" % b] = sc
    h, l1, l2, h2 = NR // 2 + 1, 3, NC - 2, NR - 1
    for name, b1, b2 in (("cancel in a row", h * NC + l1, h * NC + l2), ("cancel in a column", h * NC + l1, h2 * NC + l1)):
        sc = only([(0, b1 + 1), (1, b2 + 1)])
        bk = S.msm_buckets(dl, sc, c, True)
        assert sorted(bk) == sorted((b1, b2)) and (bk[b1][0] + bk[b2][0]) % R == 0
        out[name] = sc
    # S and -S in one row and T = S in the same columns of another row: the sum of row h and the sum of column l2 are both the identity
    sc = only([(0, h * NC + l1 + 1), (1, h * NC + l2 + 1), (2, h2 * NC + l2 + 1)])
    out["cancel in a row and a column"] = sc
    # the result is the identity: s P + s (-P)
    sc = only([(0, 12345 * NC + 7), (1, 12345 * NC + 7)])
    assert S.msm_dlog(dl, sc) == 0
    out["identity result"] = sc
    out["no digits"] = [0] * n
    from conftest import rand_fr_ints
    out["random, mostly empty"] = rand_fr_ints(n, 9700 + c)
    return out


def bases():
    from conftest import rand_fr_ints
    dl = rand_fr_ints(N, 9600)
    dl[1] = (R - dl[0]) % R
    dl[2] = dl[0]
    return dl


def run_cases(oc, h, srs, g2, c, named):
    of = g2_of if g2 else g1_of
    names = list(named)
    exps = of(oc, [S.msm_dlog(dl_sc[0], dl_sc[1]) for dl_sc in named.values()])
    ms = [mont(oc, named[nm][1]) for nm in names]
    for L in REDUCE_L:
        apply(h, {"msm_c_shared": c, "reduce_l": L})
        for i, nm in enumerate(names):
            got = jac_to_aff(h.msm_g2(srs, ms[i]) if g2 else h.msm_g1(srs, ms[i]))
            assert np.array_equal(got, exps[i]), (c, L, nm, "g2" if g2 else "g1")
            assert h.last_msm_stats()["window_bits"] == S.msm_plan(c)[0]          # the shared-bucket path at the forced width


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_tail_structured_buckets(oc, vh, c, g2):
    """single populated buckets at the corners of the row / column grid, cancelling pairs in a row and in a column, an identity result,
    no digit at all, and 64 random scalars against B >= 2^11 buckets"""
    dl = bases()
    pts = (g2_of if g2 else g1_of)(oc, dl)
    try:
        apply(vh, {"msm_c_shared": c})
        srs = vh.srs_g2_upload(pts) if g2 else vh.srs_g1_upload(pts)
        try:
            (vh.srs_g2_precompute if g2 else vh.srs_g1_precompute)(srs)
            run_cases(oc, vh, srs, g2, c, {nm: (dl, sc) for nm, sc in cases(c, dl).items()})
        finally:
            srs.free()
    finally:
        apply(vh)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS[:2])
def test_tail_every_bucket_holds_the_same_point(oc, vh, c, g2):
    """all bases equal, scalars 1 .. B: every bucket of the window holds P, so every addition of every strip and tree meets two equal
    points (the doubling branch). n = B <= 4096: the widths below and at B0."""
    B = shared_buckets(c)
    assert B <= 4096
    dl = [bases()[0]] * B
    sc = list(range(1, B + 1))
    assert {b: len(v) for b, v in S.msm_buckets(dl, sc, c, True).items()} == {b: 1 for b in range(B)}
    pts = np.repeat((g2_of if g2 else g1_of)(oc, dl[:1]), B, axis=0)
    try:
        apply(vh, {"msm_c_shared": c})
        srs = vh.srs_g2_upload(pts) if g2 else vh.srs_g1_upload(pts)
        try:
            (vh.srs_g2_precompute if g2 else vh.srs_g1_precompute)(srs)
            run_cases(oc, vh, srs, g2, c, {"all equal": (dl, sc)})
        finally:
            srs.free()
    finally:
        apply(vh)
