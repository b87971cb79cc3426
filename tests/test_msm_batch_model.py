"""CPU tests of the batched-MSM model (tests/msm_batch_model.py): the model against the sources' constants, the digit recoding, the order of
operations against plain scalar arithmetic, the route, and the events the GPU test's adversarial rows are chosen for."""
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


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 135, 136, 255, 256, 257, 271, 272, 1000, 2048, 2175, 2176, 4096, M.N_BATCH_MAX])
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


def _every_digit_carries(ct):
    _, W, _, widths, offsets = M.plan(ct)
    return (1 << offsets[-1]) - 1 + (1 << offsets[-1])          # all ones below the top window, one on top


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
