"""CPU tests of the batched-MSM model (tests/msm_batch_model.py): the model against the sources' constants, the digit recoding, the order of
operations against plain scalar arithmetic, the route, the events the GPU test's adversarial rows are chosen for, and the case table of
tests/test_gpu_msm_batch_paths.py against the plans, boundaries and pass splits the sources have."""
import pytest

import msm_batch_model as M
import structured_inputs as S
from conftest_helpers import rand_fr_ints

R = M.R


def test_model_constants_are_the_sources():
    src = M.parse_sources()
    assert src["N_BATCH_MAX"] == src["MB_N_MAX"] == M.N_BATCH_MAX
    assert (src["C_MIN"], src["C_MAX"], src["THREADS"], src["PER_BUCKET"]) == (M.C_MIN, M.C_MAX, M.THREADS, M.PER_BUCKET)
    assert (src["CANON_BYTES"], src["ROWS_MAX"]) == (M.CANON_BYTES, M.ROWS_MAX)
    assert src["route_test"] == "n <= N_BATCH_MAX" and src["oom_falls_back"] == "batch = false" and src["fallback_call"] == "msm_g1_run"
    # the 2-byte sort entry: 14 index bits below the sign bit 15, and the pool holds the longest row
    assert M.N_BATCH_MAX <= 1 << 14 and src["PAIRS_MAX"] >= M.N_BATCH_MAX
    # open_batch_core's outer loop as open_rows restates it, and the request `reserve` makes of the allocator
    assert src["open_rows_start"] == "std::min(m, std::max<size_t>(1, MSM_BATCH_CANON_BYTES / (nq * 32)))"
    assert src["open_reserve"] == "reserve(ctx, ctx->mb_q, rows * nq * 32)" and src["open_halve"] == "(rows + 1) / 2"
    assert src["open_exit"] == "st != KEAKI_ERR_OOM || rows == 1" and src["open_pass"] == "std::min(rows, m - r0)"
    assert src["reserve_request"] == "bytes + bytes / 8 + 256" and M.request(800) == 800 + 100 + 256


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 135, 136, 255, 256, 257, 271, 272, 543, 544, 1000, 1087, 1088, 2048, 2175, 2176, 4096, M.N_BATCH_MAX])
def test_window_choice_and_lds_budget(n):
    ct = M.window_bits(n)
    c, W, k, widths, offsets = M.plan(ct)
    assert c == ct and M.C_MIN <= c <= M.C_MAX
    assert k < W, "the top window is c - 1 bits wide: 2^(c-1) unsigned buckets fit the B slots"
    assert offsets[-1] + widths[-1] == 254
    B = 1 << (c - 1)
    G = M.THREADS // B
    assert n * G <= M.parse_sources()["PAIRS_MAX"], "the digits of a workgroup fit its sort pool"
    if c < M.C_MAX:
        assert n // B <= M.PER_BUCKET
    if c > M.C_MIN:
        assert n // (B // 2) > M.PER_BUCKET, "the smallest such c"


_every_digit_carries = M._every_window_carries


@pytest.mark.parametrize("ct", range(M.C_MIN, M.C_MAX + 1))
def test_recoding_reconstructs(ct):
    c, W, _, widths, offsets = M.plan(ct)
    B = 1 << (c - 1)
    cases = [0, 1, R - 1, (1 << c) - 1, 1 << (c - 1), _every_digit_carries(ct)] + rand_fr_ints(50, 1000 + ct)
    for v in cases:
        ds = M.digits(v, ct)
        assert M.reconstruct(ds, ct) == v
        for w, d in enumerate(ds):
            half = 1 << (widths[w] - 1)
            if w < W - 1:
                assert -half <= d <= half - 1
            else:
                assert 0 <= d <= B, "top digit: bucket d - 1 < B"
            if d:
                wg, lane, neg = M.slot(w, d, ct)
                assert 0 <= lane < M.THREADS and wg == w // (M.THREADS // B) and neg == (d < 0)
    ev = _every_digit_carries(ct)
    assert M.carries(ev, ct) == [1] * (W - 1), "every signed window carries, the last one into the top window"
    assert M.digits(ev, ct)[-1] == 2
    assert M.carries(0, ct) == [0] * (W - 1)
    assert M.digits(0, ct)[:-1] == [-(1 << (widths[w] - 1)) + (1 << (widths[w] - 1)) for w in range(W - 1)] == [0] * (W - 1)
    # 2^(c-1) is the first value of window 0 that goes negative with a carry: digit -half, the next window sees one more
    ds = M.digits(1 << (c - 1), ct)
    assert ds[0] == -(1 << (c - 1)) and ds[1] == 1


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257])
@pytest.mark.parametrize("secret", ["one", "minus_one", "two", "random"])
def test_order_of_operations_is_the_msm(n, secret):
    tau = S.secrets()[secret]
    dl = S.powers(tau, n)
    for row in M.adversarial_rows(n, rand_fr_ints(n, 7 * n)):
        got, _ = M.msm_row(dl, row)
        assert (got or 0) == S.msm_dlog(dl, row)


def test_adversarial_rows_reach_the_branches():
    """what the GPU test relies on: tau = 1 meets equal operands in the bucket loop, tau = -1 opposite operands and an identity accumulator;
    both meet them in the tree or the close as well"""
    n = 65
    ev1, evm = M.Events(), M.Events()
    for row in M.adversarial_rows(n, rand_fr_ints(n, 11)):
        M.msm_row(S.powers(1, n), row, ev1)
        M.msm_row(S.powers(R - 1, n), row, evm)
    assert ev1.get("bucket_equal", 0) > 0
    assert evm.get("bucket_opposite", 0) > 0 and evm.get("bucket_identity_acc", 0) > 0
    assert ev1.get("tree_equal", 0) + ev1.get("close_equal", 0) > 0
    assert evm.get("tree_opposite", 0) + evm.get("close_opposite", 0) + evm.get("tree_equal", 0) > 0
    # the all-zero row is the identity on every SRS
    assert M.msm_row(S.powers(5, n), [0] * n)[0] is None


def test_route():
    NB = M.N_BATCH_MAX
    assert M.route(100, 0) == "none" and M.route(0, 5) == "identity"
    for tables in (False, True):
        assert M.route(1, 1, tables) == "batch" and M.route(NB, 2, tables) == "batch"
        assert M.route(NB + 1, 2, tables) == "fallback" and M.route(1 << 20, 1, tables) == "fallback"
    # an allocation limit below the first reservation: fallback, unless the context already holds the workspaces
    n, m = 257, 65
    req = M.workspace_requests(n, m)
    assert req[0] == 65 * 257 * 32 * 9 // 8 + 256
    assert M.route(n, m, alloc_limit=req[0] - 1) == "fallback"
    assert M.route(n, m, alloc_limit=max(req)) == "batch"
    assert M.route(n, m, alloc_limit=4096, held=(65 * 257 * 32, 65 * 64 * 128)) == "batch"
    assert M.route(n, m, alloc_limit=4096) == "fallback"
    # passes: at most 256 MB of canonical scalars and 16,384 rows at a time
    assert M.rows_per_pass(NB, 4096) == 512 and M.rows_per_pass(1, 100000) == M.ROWS_MAX and M.rows_per_pass(4096, 1024) == 1024


def test_open_rows():
    """the halving loop of open_batch_core: rows 65 -> 33 -> 17 under a limit between the requests of 17 and 33 rows, the workspaces held
    from one pass to the next, the inner route of every pass, and the refusal of a single row"""
    nq, m = 256, 65
    assert M.open_rows(nq, m) == {"rows": [65], "routes": ["batch"], "held": (M.request(65 * nq * 32),) + tuple(M.workspace_requests(nq, 65))}
    lim = M.request(17 * nq * 32)
    assert M.request(33 * nq * 32) > lim + 1000
    o = M.open_rows(nq, m, lim)
    assert o["rows"] == [17, 17, 17, 14] and o["routes"] == ["batch"] * 4
    assert o["held"] == (lim, lim, M.request(17 * M.plan(M.window_bits(nq))[1] * 128))
    assert M.open_rows(nq, m, lim - 1)["rows"] == [9] * 7 + [2]
    # a held quotient workspace is not asked for again; a held workspace that is too small is freed before the refusal
    assert M.open_rows(nq, m, 4096, held=(65 * nq * 32, 65 * nq * 32, 1 << 20))["rows"] == [65]
    assert M.open_rows(nq, m, lim, held=(64 * nq * 32, 0, 0))["rows"] == [17, 17, 17, 14]
    assert M.open_rows(nq, m, M.request(nq * 32) - 1) is None, "one row refused: KEAKI_ERR_OOM"
    assert M.open_rows(nq, m, M.request(nq * 32))["rows"] == [1] * 65
    # the window sums of a short row are larger than the row: the quotient fits, the batch MSM does not
    o = M.open_rows(33, 65, M.request(65 * 33 * 32))
    assert o["rows"] == [65] and o["routes"] == ["fallback"] and o["held"][2] == 0
    # the byte bound and the row above N_BATCH_MAX
    assert M.open_rows(M.N_BATCH_MAX, 600)["rows"] == [512, 88] and M.open_rows(M.N_BATCH_MAX + 1, 2)["routes"] == ["fallback"]
    assert M.inner_passes(1, M.ROWS_MAX + 1) == [M.ROWS_MAX, 1] and M.inner_passes(M.N_BATCH_MAX, 513) == [512, 1]


# ---- the case table of tests/test_gpu_msm_batch_paths.py ------------------------------------------------------------------------------------
def _guard(cases):
    """what the table must cover, as a list of failures (empty: covered). A function of the case list, so that the test below can also show
    that it notices a missing case."""
    bad = []
    reach = {k[0]: M.reach(k) for k in cases if k[6] != "branch"}          # the events are test_branch_rows_reach_every_event's
    commit = [k for k in cases if k[1] == "commit"]
    widths = {M.window_bits(k[2]) for k in commit}
    if widths != set(range(M.C_MIN, M.C_MAX + 1)):
        bad.append("widths run: %s" % sorted(widths))
    ns = {k[2] for k in commit if k[6] == "edge"}
    bounds = M.width_boundaries()
    if len(bounds) != M.C_MAX - M.C_MIN:
        bad.append("boundaries of window_bits: %s" % bounds)
    for lo, hi in bounds:
        for n in (lo, hi):
            if n not in ns:
                bad.append("no case at the width boundary n = %d" % n)
    for c in range(M.C_MIN, M.C_MAX + 1):
        for srs in ("one", "minus_one"):
            if not any(k[6] == "branch" and M.window_bits(k[2]) == c and k[5] == srs for k in commit):
                bad.append("no adversarial rows at c = %d on the SRS %r" % (c, srs))

    def some(what, pred):
        if not any(pred(k, reach[k[0]]) for k in cases if k[0] in reach):
            bad.append("no case with " + what)
    some("two inner passes by ROWS_MAX", lambda k, r: k[1] == "commit" and max(r["inner"]) >= 2 and k[3] > M.ROWS_MAX and k[2] * 32 * M.ROWS_MAX <= M.CANON_BYTES)
    some("two inner passes by CANON_BYTES", lambda k, r: k[1] == "commit" and max(r["inner"]) >= 2 and k[3] <= M.ROWS_MAX)
    some("a second inner pass reading stride > n", lambda k, r: k[1] == "commit" and max(r["inner"]) >= 2 and k[4] > k[2])
    some("three outer passes and a ragged last one", lambda k, r: k[1] == "open" and len(r["outer"]) >= 3 and r["outer"][-1] < r["outer"][0]
         and set(r["routes"]) == {"batch"})
    some("an open whose MSM falls back below N_BATCH_MAX", lambda k, r: k[1] == "open" and "fallback" in r["routes"] and k[2] - 1 <= M.N_BATCH_MAX)
    some("an open of N_BATCH_MAX quotient coefficients", lambda k, r: k[1] == "open" and k[2] - 1 == M.N_BATCH_MAX and r["routes"] == ["batch"])
    some("an open of N_BATCH_MAX + 1 quotient coefficients", lambda k, r: k[1] == "open" and k[2] - 1 == M.N_BATCH_MAX + 1 and r["routes"] == ["fallback"])
    some("an open with stride > n", lambda k, r: k[1] == "open" and k[4] > k[2])
    some("identity points in a large plan", lambda k, r: k[5] == "holes" and r["c"] >= 8)
    some("identity points in the smallest plan", lambda k, r: k[5] == "holes" and r["c"] == M.C_MIN)
    # the quotient's segments: L = ceil(n / 256) = 1 with the last lane idle and busy, and a step of L with a ragged tail
    qn = {k[2] for k in cases if k[1] == "open" and k[6] == "z01"}
    for n in (M.THREADS - 1, M.THREADS, 2 * M.THREADS, 2 * M.THREADS + 1):
        if n not in qn:
            bad.append("no quotient case at n = %d" % n)
    return bad


def test_gpu_cases_cover_the_batch_paths():
    assert len({k[0] for k in M.GPU_CASES}) == len(M.GPU_CASES)
    assert _guard(M.GPU_CASES) == []
    for k in M.GPU_CASES:
        assert k[4] >= k[2] and (k[1] == "open" or k[2] <= 2500 or k[5] == "random")
    # the plans as the issue of this table lists them: G windows a workgroup, tree depth c - 1
    r6, r8 = M.reach(M.case("plan[n=272]")), M.reach(M.case("plan[n=1088]"))
    assert (r6["c"], r6["G"], r6["depth"]) == (6, 8, 5) and (r8["c"], r8["G"], r8["depth"]) == (8, 2, 7)
    # the limits of the two limited opens do what the GPU test says they do
    a, b = M.reach(M.case("open_halving")), M.reach(M.case("open_fallback"))
    assert a["outer"] == [17, 17, 17, 14] and set(a["routes"]) == {"batch"}
    assert b["outer"] == [65] and b["routes"] == ["fallback"] and b["held"][1] > 0 and b["held"][2] == 0


@pytest.mark.parametrize("drop", ["plan[n=544]", "plan[n=1087]", "rows_max[n=3,stride]", "rows_max[n=*]", "canon_bytes", "open_halving", "open_fallback",
                                  "open_route[n=16385]", "open_route[n=16386]", "branches[n=400,minus_one]", "identity_points[n=1500]", "quotient[n=513]"])
def test_guard_notices_a_missing_case(drop):
    if drop == "rows_max[n=*]":
        left = [k for k in M.GPU_CASES if not k[0].startswith("rows_max")]
    elif drop == "rows_max[n=3,stride]":
        left = [k for k in M.GPU_CASES if not k[0].endswith(",stride]")]
    else:
        left = [k for k in M.GPU_CASES if k[0] != drop]
    assert len(left) < len(M.GPU_CASES) and _guard(left) != []


@pytest.mark.parametrize("n", M.BRANCH_N)
def test_branch_rows_reach_every_event(n):
    """for every width: the rows the GPU test runs on tau = 1 and tau = -1 meet equal operands, opposite operands and an identity accumulator in
    the bucket loop, and equal and opposite operands in the tree or the close"""
    assert M.window_bits(n) == M.C_MIN + M.BRANCH_N.index(n)
    ev = set(M.branch_events(n, "one")) | set(M.branch_events(n, "minus_one"))
    assert {"bucket_equal", "bucket_opposite", "bucket_identity_acc"} <= ev
    assert ev & {"tree_equal", "close_equal"} and ev & {"tree_opposite", "close_opposite"}
    # tau = 1 alone doubles in the bucket loop and meets both cases at the first tree level (the two-scalar rows of branch_rows)
    assert {"bucket_equal", "tree_equal", "tree_opposite"} <= set(M.branch_events(n, "one"))
    # ... and at the last one, the merge of the two halves of a window (level c - 2)
    assert {"tree_top_equal", "tree_top_opposite"} <= set(M.branch_events(n, "one"))
    assert {"bucket_opposite", "bucket_identity_acc"} <= set(M.branch_events(n, "minus_one"))
    rows = M.branch_rows(n, rand_fr_ints(n, 5 + n))
    assert len(rows) == M.case("branches[n=%d,one]" % n)[3]
    for tau in (1, R - 1):
        dl = S.powers(tau, n)
        for row in rows[4:]:
            got, _ = M.msm_row(dl, row)
            assert (got or 0) == S.msm_dlog(dl, row)


def test_edge_scalars():
    for n in M.BOUNDARY_N:
        ct = M.window_bits(n)
        e = M.edge_scalars(n)
        assert e[:3] == [0, 1, R - 1] and e[3] == 1 << (ct - 1) and M.carries(e[4], ct) == [1] * (M.plan(ct)[1] - 1)
