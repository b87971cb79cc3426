"""CPU tests of the batched-FK23 model (tests/fk_batch_model.py): its constants against the sources, the position-major pipeline with padded
rows, pass split and final bit reversal against a direct per-point opening, the route of a call, and the case table of
tests/test_gpu_fk_batch.py against the kernels fk_batch.hip can launch and the routes api.hip has."""
import random

import pytest

import fk_batch_model as M

Q = M.Q


def test_model_constants_are_the_sources():
    src = M.parse_sources()
    assert (src["LOG2D_MAX"], src["PASS_BYTES"], src["ROW_BYTES"], src["ROWS_MAX"]) == (M.LOG2D_MAX, M.PASS_BYTES, M.ROW_BYTES, M.ROWS_MAX)
    assert src["LOG2D_MAX"] >= 12, "log2d = 1 .. 12 run the batch kernels"
    assert src["pts_bytes"] == "((size_t)2 << log2d) * fkb_pad64(rows) * sizeof(G1Jac)"
    assert src["fr_bytes"] == "(rows * ((size_t)3 << log2d) + ((size_t)3 << log2d)) * sizeof(Fr)"
    assert src["batch_domains"] == "log2d >= 1 && log2d <= FKB_LOG2D_MAX" and src["fallback"] == "rows == 0"
    assert src["halve"] == "(rows + 1) / 2" and src["pass"] == "std::min(rows, m - r0)"
    assert src["reserve_request"] == "bytes + bytes / 8 + 256" and M.request(800) == 800 + 100 + 256
    # a row's share of a pass: two Jacobian points and three Fr per coefficient
    assert M.ROW_BYTES == 2 * M.JAC + 3 * M.FR
    for log2d in (1, 6, 12):
        rows = M.rows_per_pass(log2d, 1 << 30)
        assert rows % 64 == 0 and M.pts_bytes(log2d, rows) + rows * (3 << log2d) * M.FR <= max(M.PASS_BYTES, 64 * (M.ROW_BYTES << log2d))


def _case(log2d, m, stride_extra, seed):
    rnd = random.Random(seed)
    d = 1 << log2d
    stride = d + stride_extra
    srs = [rnd.randrange(Q) for _ in range(d)]
    data = [M.GARBAGE] * (m * stride)
    for j in range(m):
        data[j * stride:j * stride + d] = [rnd.randrange(Q) for _ in range(d)]
    return srs, data, stride


@pytest.mark.parametrize("log2d", range(1, 7))
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_open_batch_is_the_direct_opening(log2d, m):
    d = 1 << log2d
    srs, data, stride = _case(log2d, m, m % 3, 100 * log2d + m)
    got, coms = M.batch(srs, data, d, m, stride, log2d, vec=False)
    assert coms is None and len(got) == m * d
    for j in range(m):
        assert got[j * d:(j + 1) * d] == M.open_direct(srs, data[j * stride:j * stride + d], log2d), "row %d" % j


@pytest.mark.parametrize("log2d,m,n", [(1, 65, 2), (3, 2, 5), (4, 130, 1), (5, 64, 0), (6, 63, 64), (6, 3, 17)])
def test_vec_commit_batch_is_interpolation_then_opening(log2d, m, n):
    """the first n evaluations of a row, zeros behind them: the coefficients are the inverse transform, the commitment their MSM"""
    d = 1 << log2d
    srs, data, stride = _case(log2d, m, 1, 7 * log2d + m)
    stride = n + 2
    data = [x if i % stride < n else M.GARBAGE for i, x in enumerate((data * 2)[:m * stride])]
    got, coms = M.batch(srs, data, n, m, stride, log2d, vec=True)
    wd = pow(M.root(2 * d), 2, Q)
    for j in range(m):
        ev = data[j * stride:j * stride + n] + [0] * (d - n)
        coef = [x * pow(d, Q - 2, Q) % Q for x in M.dft(ev, pow(wd, Q - 2, Q))]
        assert [sum(c * pow(wd, i * k, Q) for k, c in enumerate(coef)) % Q for i in range(d)] == ev
        assert got[j * d:(j + 1) * d] == M.open_direct(srs, coef, log2d), "row %d" % j
        assert coms[j] == sum(c * s for c, s in zip(coef, srs)) % Q


@pytest.mark.parametrize("log2d,m", [(2, 130), (6, 130)])
def test_halved_passes_give_the_same_rows(log2d, m):
    d = 1 << log2d
    srs, data, stride = _case(log2d, m, 2, 5)
    lim = M.request(M.pts_bytes(log2d, 33))
    pl = M.plan(log2d, m, lim)
    assert pl["route"] == "batch" and pl["passes"] == [33, 33, 33, 31] and pl["halvings"] == 2
    assert M.batch(srs, data, d, m, stride, log2d, False, lim) == M.batch(srs, data, d, m, stride, log2d, False)
    assert M.batch(srs, data, d, m, stride, log2d, False, M.request(M.pts_bytes(log2d, 1)) - 1) == M.batch(srs, data, d, m, stride, log2d, False)


def test_route():
    assert M.plan(6, 0)["route"] == "none"
    assert M.plan(0, 3) == {"route": "rows", "passes": [1, 1, 1], "halvings": 0, "held": (0, 0)}
    assert M.plan(M.LOG2D_MAX, 2)["route"] == "batch" and M.plan(M.LOG2D_MAX + 1, 2)["route"] == "rows"
    # the cap: 256 MB of workspace in whole groups of 64 rows, and FKB_ROWS_MAX rows
    assert M.rows_per_pass(12, 1000) == 192 and M.rows_per_pass(12, 64) == 64 and M.rows_per_pass(8, 4096) == 3584
    assert M.rows_per_pass(1, 1 << 20) == M.ROWS_MAX
    assert M.plan(12, 400)["passes"] == [192, 192, 16]
    assert M.plan(1, M.ROWS_MAX + 66)["passes"] == [M.ROWS_MAX, 66]
    # halving stops at the first pass whose two workspaces are granted; what the context already holds is not asked for again
    lim = M.request(M.pts_bytes(6, 33))
    assert M.plan(6, 130, lim)["held"] == (lim, M.request(M.fr_bytes(6, 33)))
    assert M.plan(6, 130, 4096, held=(M.pts_bytes(6, 130), M.fr_bytes(6, 130)))["passes"] == [130]
    # below 64 rows the point workspace does not shrink any more (M stays 64): one byte less and no pass fits
    assert M.pad64(1) == M.pad64(64) == 64 and M.pad64(65) == 128 and M.pts_bytes(6, 33) == M.pts_bytes(6, 1)
    rows = M.plan(6, 130, lim - 1)
    assert rows["route"] == "rows" and rows["passes"] == [1] * 130 and rows["halvings"] == 8 and rows["held"] == (0, 0)
    assert M.plan(6, 64, lim)["passes"] == [64]


def _guard(cases):
    """what the case table must cover, as a list of failures"""
    bad = []
    reach = {k[0]: M.reach(k) for k in cases}
    kernels = set().union(*[r["kernels"] for r in reach.values()]) if reach else set()
    if kernels != M.launch_sites():
        bad.append("kernels not launched by any case: %s" % sorted(M.launch_sites() - kernels))

    def some(what, pred):
        if not any(pred(k, reach[k[0]]) for k in cases):
            bad.append("no case with " + what)
    some("one batch pass", lambda k, r: r["route"] == "batch" and len(r["passes"]) == 1 and k[4] is None)
    some("a split by the cap with a ragged last pass", lambda k, r: r["route"] == "batch" and r["halvings"] == 0 and len(r["passes"]) >= 2
         and r["passes"][-1] < r["passes"][0])
    some("a second pass found through stride > d", lambda k, r: r["route"] == "batch" and len(r["passes"]) >= 2 and k[3] > 1 << k[1])
    some("passes halved under an allocation limit", lambda k, r: r["route"] == "batch" and r["halvings"] >= 1 and len(r["passes"]) >= 3)
    some("the row-by-row route under an allocation limit", lambda k, r: r["route"] == "rows" and k[4] is not None and 1 <= k[1] <= M.LOG2D_MAX)
    some("the row-by-row route of a domain outside the batch kernels", lambda k, r: r["route"] == "rows" and k[4] is None)
    some("rows that are no multiple of 64 in more than one workgroup", lambda k, r: r["route"] == "batch" and any(p > 64 and p % 64 for p in r["passes"]))
    return bad


def test_gpu_cases_cover_kernels_and_routes():
    assert len({k[0] for k in M.GPU_CASES}) == len(M.GPU_CASES)
    assert M.launch_sites() == {"k_fkb_fr_load", "k_fkb_fr_stage", "k_fkb_fr_scale", "k_fkb_pointwise", "k_fkb_stage<true>", "k_fkb_stage<false>",
                                "k_fkb_twist", "k_fkb_finish"}
    assert _guard(M.GPU_CASES) == []
    for k in M.GPU_CASES:
        assert k[2] << k[1] <= 130 << 9 and k[3] >= 1 << k[1], "nothing larger than d = 2^9 with m = 130"
    assert M.reach(M.case("halved"))["passes"] == [33, 33, 33, 31]
    assert M.reach(M.case("rows_cap"))["passes"] == [M.ROWS_MAX, 66]
    # every launch of a pass, for the smallest and the largest batch domain
    assert len(M.launches(1, True)) == 3 + 4 + 5 and len(M.launches(12, False)) == (1 + 13 + 1) + (1 + 12 + 1 + 12 + 1)


@pytest.mark.parametrize("drop", ["batch+halved+rows_cap+rows_cap_stride", "rows_cap+rows_cap_stride", "rows_cap_stride", "halved", "row_by_row", "d1"])
def test_guard_notices_a_missing_case(drop):
    left = [k for k in M.GPU_CASES if k[0] not in drop.split("+")]
    assert len(left) < len(M.GPU_CASES) and _guard(left) != []
