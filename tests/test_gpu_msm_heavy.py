"""The heavy-bucket path of the MSM (csrc/msm.hip.h: k_cnt_hist, k_msm_heavy, k_msm_heavy_combine) at its count, slice and pass edges.
tests/heavy_cases.py builds the inputs and says what every designed bucket holds in every pass; tests/test_heavy_cases_model.py checks
those claims on the CPU. Here every case runs on the GPU: bases are k_i G with known k_i, so the expected point is (sum s_i k_i) G from
one oracle scalar multiplication; affine results are compared word for word and the window width with the one the model planned for.
The module runs on contexts of its own: the session context's switches are never touched."""
import os
import random
import time

import numpy as np
import pytest

import heavy_cases as H
import variant_cases as V
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
TH = min(16, os.cpu_count() or 1)
DEFAULTS = {"msm_c": 0, "msm_c_shared": 0, "acc_u29": 1, "acc_u29_g2": 1, "msm_pipe_chunks": 0, "msm_pipe_min": 1 << 20, "msm_pipe_growth": 160}


@pytest.fixture(scope="module")
def hh():
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    yield h
    h.close()


def configure(h, case=None):
    """the options of a case (forced width, bucket kernel, chunking through the host-pointer entry); case None: this module's defaults"""
    opts = dict(DEFAULTS)
    if case is not None:
        opts["msm_c_shared" if case["tables"] else "msm_c"] = case["c"]
        opts["acc_u29"] = case["acc_u29"]
        if case["passes"] > 1:
            opts.update(msm_pipe_chunks=case["passes"], msm_pipe_min=1, msm_pipe_growth=100)
    for k, v in opts.items():
        h.set_option(k, v)


def point_of(oc, g2, k):
    mul = oc.g2_mul_batch if g2 else oc.g1_mul_batch
    return mul(oc.generators()[1 if g2 else 0], mont(oc, [k % H.R]))[0]


def bases(oc, h, g2, dlogs):
    """k_i G on the device, spot-checked against the oracle; a zero dlog is the identity (an all-zero affine row)"""
    gen = oc.generators()[1 if g2 else 0]
    pts = (h.g2_mul_batch if g2 else h.g1_mul_batch)(gen, mont(oc, dlogs))
    n = len(dlogs)
    idx = [i for i in sorted(set(list(range(0, n, max(1, n // 24))) + [1, n - 1])) if dlogs[i]]
    exp = (oc.g2_mul_batch if g2 else oc.g1_mul_batch)(gen, mont(oc, [dlogs[i] for i in idx]), threads=TH)
    assert np.array_equal(pts[idx], exp)
    zero = [i for i, k in enumerate(dlogs) if k == 0]
    if zero:
        pts[zero] = 0
    return pts


def upload(h, case, pts):
    g2 = case["group"] == "g2"
    srs = (h.srs_g2_upload if g2 else h.srs_g1_upload)(pts)
    if case["tables"]:
        (h.srs_g2_precompute if g2 else h.srs_g1_precompute)(srs)
    return srs


def msm(h, case, srs, sc):
    got = jac_to_aff((h.msm_g2 if case["group"] == "g2" else h.msm_g1)(srs, sc))
    assert h.last_msm_stats()["window_bits"] == H.window_bits(case), (case["name"], h.last_msm_stats())
    return got


def check(oc, h, case, oracle_msm=False):
    g2 = case["group"] == "g2"
    configure(h, case)
    pts, sc = bases(oc, h, g2, case["dlogs"]), mont(oc, case["scalars"])
    k = H.expected_dlog(case)
    exp = point_of(oc, g2, k)
    assert exp.any() == (k != 0)
    srs = upload(h, case, pts)
    try:
        got = msm(h, case, srs, sc)
        assert np.array_equal(got, exp), case["name"]
        if oracle_msm:                                   # the oracle's own MSM on the same arrays: a witness beside the dlog bookkeeping
            assert np.array_equal(got, (oc.msm_g2 if g2 else oc.msm_g1)(pts, sc, threads=TH)), case["name"]
    finally:
        srs.free()
        configure(h)


# ---- family 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4), ids=["g1-static", "g1-walk", "g1-tables", "g2"])
def test_designed_counts_around_the_threshold_and_the_slice_length(oc, hh, i):
    """buckets of exactly 1022 .. 1024, HEAVY_MIN - 1 .. + 1, HEAVY_SLICE - 1 .. + 1, 2 HEAVY_SLICE, C2_CAP + 1 and 3 HEAVY_SLICE + 1
    pairs (G2: the reduced list) among random fillers; then a call whose every pair sits in a bucket of exactly HEAVY_MIN pairs"""
    check(oc, hh, H.count_cases()[i])
    check(oc, hh, H.all_exact_cases()[i], oracle_msm=(i == 3))


# ---- family 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(2), ids=["g1", "g2"])
def test_slices_that_begin_and_end_inside_segments(oc, hh, i):
    """a heavy bucket alone in a bin of two chunks, and one whose bin of five chunks it shares 2 : 3 with light companions: every chunk
    end of that bin lies inside a slice whatever the arrival order (tests/test_heavy_cases_model.py proves the bounds)"""
    check(oc, hh, H.straddle_cases()[i])


# ---- family 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3), ids=["g1-lazy", "g1-saturated", "g2"])
def test_exceptional_additions_inside_heavy_buckets(oc, hh, i):
    """copies of one base (doublings in every lane, at every tree level and in the combine kernel), P and -P in equal numbers, with one
    extra P, identity bases; then a call in which every heavy bucket cancels and the MSM is the identity"""
    check(oc, hh, H.exceptional_cases()[i], oracle_msm=(i == 0))
    case = H.exceptional_cases()[3 + i]
    assert H.expected_dlog(case) == 0
    check(oc, hh, case)


# ---- family 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2, 4], ids=["g1-lazy", "g1-lazy-tables", "g1-saturated", "g2"])
def test_pass_matrix_of_a_chunked_call(oc, hh, i):
    """every sequence of empty / light / heavy over the passes of a chunked call, and a stored point that equals (is opposite to) the
    heavy sum added to it"""
    case = H.matrix_cases()[i]
    modes = {row[1] for row in H.reach(case)}
    assert modes == ({"HV_SET29", "HV_ADD29", "HV_ADD"} if i < 2 else {"HV_SET", "HV_ADD"})
    check(oc, hh, case)


def test_pass_matrix_without_room_for_the_parked_state(oc):
    """the lazy kernel's parked-state workspace refused (144 B per bucket; the canonical buckets' 128 B fit): the passes go on from the
    canonical bucket, HV_SET / HV_ADD, through the saturated kernel"""
    from keaki_amd.hip import KeakiHip
    case = H.matrix_cases()[3]
    assert case["refuse_state"] and not case["tables"]
    nb = V.plan(case["c"])["nb"]
    h = KeakiHip(0)                                        # a context of its own: its workspaces start empty
    try:
        pts, sc = bases(oc, h, False, case["dlogs"]), mont(oc, case["scalars"])
        exp = point_of(oc, False, H.expected_dlog(case))
        configure(h, case)
        srs = upload(h, case, pts)
        try:
            h.set_option("msm_pipe_chunks", 0)
            assert np.array_equal(msm(h, case, srs, sc), exp)              # one pass: every other workspace at its largest
            held = h.memory()["workspaces"]
            h.set_option("msm_pipe_chunks", case["passes"])
            h.debug_set_alloc_limit(nb * 136)
            assert np.array_equal(msm(h, case, srs, sc), exp), "fallback to the canonical-state passes"
            assert h.memory()["workspaces"] - held < nb * 144
            h.debug_set_alloc_limit(0)
            assert np.array_equal(msm(h, case, srs, sc), exp)
            assert h.memory()["workspaces"] - held >= nb * 144, "with room, the parked-register workspace is taken"
        finally:
            srs.free()
    finally:
        h.close()


# ---- family 5 -------------------------------------------------------------------------------------------------------------------------
def test_more_than_256_chunks_in_one_bin(oc, hh):
    """257 C2_CAP + 1 scalars equal to 1: one bucket, alone in a bin of 258 chunks -- the second trip of k_msm_heavy's segment search.
    The bases repeat a block of 2^16 points with known dlogs, tiled on the device."""
    import torch
    m = H.many_chunks_model()
    n, blk = m["n"], H.MANY_BLOCK
    dev = torch.device("cuda", 0)
    dl = H.rand_dlogs(blk, random.Random(1500))
    pts = bases(oc, hh, False, dl)
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev).repeat(-(-n // blk), 1)[:n]
    assert d_pts.is_contiguous() and d_pts.shape == (n, 8)
    torch.cuda.synchronize(dev)
    sc = np.ascontiguousarray(np.tile(mont(oc, [1]), (n, 1)))
    exp = point_of(oc, False, H.many_chunks_dlog(dl))
    configure(hh)
    srs = hh.srs_g1_wrap_dev(d_pts.data_ptr(), n)
    try:
        t0 = time.perf_counter()
        got = jac_to_aff(hh.msm_g1(srs, sc))
        print("msm of %d ones: %.1f ms wall" % (n, 1e3 * (time.perf_counter() - t0)))
        assert np.array_equal(got, exp)
        assert hh.last_msm_stats()["window_bits"] == m["window_bits"]
    finally:
        srs.free()
        del d_pts
        hh.trim()
        torch.cuda.empty_cache()


# ---- family 6 -------------------------------------------------------------------------------------------------------------------------
def test_heavy_list_and_slice_sums_do_not_leak_into_the_next_call(oc, hh):
    """a heavy call, then uniformly random scalars of the same shape and window on the same context (the result of a fresh context),
    then the heavy call again"""
    from conftest import rand_fr_ints
    from keaki_amd.hip import KeakiHip
    case = H.exceptional_cases()[0]
    rnd = dict(case, name="random after heavy", scalars=rand_fr_ints(len(case["scalars"]), 1600))
    configure(hh, case)
    pts = bases(oc, hh, False, case["dlogs"])
    sc_heavy, sc_rnd = mont(oc, case["scalars"]), mont(oc, rnd["scalars"])
    exp_heavy, exp_rnd = point_of(oc, False, H.expected_dlog(case)), point_of(oc, False, H.expected_dlog(rnd))
    srs = upload(hh, case, pts)
    fresh = KeakiHip(0)
    try:
        configure(fresh, case)
        fsrs = upload(fresh, case, pts)
        ref = msm(fresh, rnd, fsrs, sc_rnd)
        fsrs.free()
        assert np.array_equal(ref, exp_rnd)
        assert np.array_equal(msm(hh, case, srs, sc_heavy), exp_heavy)
        assert np.array_equal(msm(hh, rnd, srs, sc_rnd), ref)
        assert np.array_equal(msm(hh, case, srs, sc_heavy), exp_heavy)
    finally:
        fresh.close()
        srs.free()
        configure(hh)
