"""One verdict per set proof over arbitrary point sets on the GPU (keaki_hip_kzg_verify_sets_each, _dev) against the big-integer model
(tests/set_pairs_model.py: status_i = 0 <=> dl(A_i) == q_i dl(Z2_i), with the identity rule). Inputs have known discrete logs (an SRS of known tau), every
expected status comes from the model, and the neighbours that must agree are asked on the same items: keaki_hip_kzg_verify_multi per item,
keaki_hip_kzg_verify_sets on the whole batch, keaki_hip_kzg_verify_each at k = 1. Both routes of the pairing side run every case.
tests/test_set_pairs_model.py shows on the CPU that every corruption used here breaks the equation of exactly its item."""
import numpy as np
import pytest

import set_pairs_model as P
import verify_sets_model as M
from conftest import rand_fr_ints
from test_gpu_set_pairs import BAD_ARG, OOM, R, SENT, TAU, TOO_LARGE, Inputs, dev, env, g1_of, g2_of, handles, make_case, mont, small_tables  # noqa: F401

pytestmark = pytest.mark.gpu
ROUTES = (1, 2)


def each(hip, env, x, c=None, want_pairs=False, **kw):
    """the call on the arrays of x, with the proofs (and whatever kw replaces) -> its result"""
    a = dict(com=x.com, points=x.points, values=x.values, proofs=x.proofs, item_stride=None, omega=None)
    a.update(env)
    a.update(kw)
    return hip.kzg_verify_sets_each(a["srs1"], a["srs2"], a["com"], a["points"], a["values"], x.k, a["proofs"], item_stride=a["item_stride"], omega=a["omega"],
                                    want_pairs=want_pairs)


def check(got, want):
    status, n_bad, first = got[:3]
    assert status.tolist() == want
    assert n_bad == sum(want) and first == (want.index(1) if 1 in want else None)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k,n", [(1, 9), (2, 65), (3, 7), (5, 8), (8, 9), (9, 3), (17, 2), (64, 5)])
def test_valid_items_give_zeros_and_the_pairs(oc, hip, env, k, n, route):
    hip.set_option("set_each_route", route)
    x = Inputs(oc, make_case(n, k, 7000 + 100 * k + n))
    got = each(hip, env, x, want_pairs=True)
    check(got, [0] * n)
    x.check(got[3:])
    g = mont(oc, rand_fr_ints(n, 7001 + k))
    ok, _ = hip.kzg_verify_sets(env["srs1"], env["srs2"], x.com, x.points, x.values, k, x.proofs, g)
    assert ok                                                               # n_bad = 0 <=> verify_sets accepts


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_a_corruption_marks_exactly_its_items(oc, hip, env, k, route):
    hip.set_option("set_each_route", route)
    n = 8
    c = make_case(n, k, 7100 + k)
    g = mont(oc, rand_fr_ints(n, 7101 + k))
    for kind, items in (("proof", [0]), ("value", [n - 1]), ("point", [2, 5]), ("com", [3])):
        d = c
        for i in items:
            d = P.corrupt(d, kind, i, k - 1, delta=1 + i)
        want = P.statuses(d)
        assert want == [1 if i in items else 0 for i in range(n)]
        x = Inputs(oc, d)
        check(each(hip, env, x), want)
        # status = verify_multi's ok per item, and verify_sets rejects the batch
        for i in (items[0], (items[0] + 1) % n):
            ok = hip.kzg_verify_multi(env["srs1"], env["srs2"], x.com[i], x.points[i * k:(i + 1) * k], x.values[i * k:(i + 1) * k], x.proofs[i])
            assert ok == (want[i] == 0)
        assert not hip.kzg_verify_sets(env["srs1"], env["srs2"], x.com, x.points, x.values, k, x.proofs, g)[0]


def test_at_k_one_the_bytes_are_verify_eachs(oc, hip, env):
    n = 9
    c = P.corrupt(P.corrupt(make_case(n, 1, 7200), "proof", 4), "value", 8)
    x = Inputs(oc, c)
    tau_g2 = g2_of(oc, [TAU])[0]
    want = hip.kzg_verify_each(x.com, tau_g2, x.points, x.values, x.proofs)
    for route in ROUTES:
        hip.set_option("set_each_route", route)
        got = each(hip, env, x)
        assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
        check(got, P.statuses(c))


@pytest.mark.parametrize("route", ROUTES)
def test_bad_items_at_the_first_and_last_slot_of_a_launch_chunk(oc, hip, env, route):
    hip.set_option("set_each_route", route)
    k, n = 2, 70
    c = make_case(n, k, 7300, shared=True)
    bad = [0, 31, 32, 63, 64, 69]                                          # chunks of 32 items: [0, 32), [32, 64), [64, 70)
    for i in bad:
        c = P.corrupt(c, "proof", i, delta=3 + i)
    want = P.statuses(c)
    assert [i for i, s in enumerate(want) if s] == bad
    x = Inputs(oc, c)
    base = each(hip, env, x)
    check(base, want)
    hip.trim()
    # the final exponentiation's slots are 4,608 B per item: 70 and then 64 items are refused, 32 fit (set_rows_plan.h: se_chunk_halve)
    limit = 200000
    assert P.se_chunk_halve(70) == 64 and P.se_chunk_halve(64) == 32
    assert 64 * 4608 * 9 // 8 + 256 > limit > 32 * 4608 * 9 // 8 + 256
    hip.debug_set_alloc_limit(limit)
    got = each(hip, env, x)
    hip.debug_set_alloc_limit(0)
    assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:]


@pytest.mark.parametrize("route", ROUTES)
def test_the_identity_rule_case_by_case(oc, hip, env, route):
    hip.set_option("set_each_route", route)
    r = rand_fr_ints(6, 7400)
    in_set, off_set = [TAU, r[0]], [r[1], r[2]]
    rows = []
    for q, a_zero, z_zero in ((5, True, True), (0, True, True), (0, True, False), (5, True, False), (0, False, False), (5, False, True), (0, False, True)):
        zs = in_set if z_zero else off_set
        rows.append((zs, [11, 11] if a_zero else [12, 11], q))
    c = M.Case(TAU, 2, [11], [z for z, _, _ in rows], [y for _, y, _ in rows], [q for _, _, q in rows], [1] * len(rows))
    want = P.statuses(c)
    assert want == [0, 0, 0, 1, 1, 1, 1]
    x = Inputs(oc, c)
    got = each(hip, env, x, want_pairs=True)
    check(got, want)
    x.check(got[3:])
    assert not got[4][0].any() and not got[3][0].any() and got[4][2].any()       # Z2 and A as identities, and a Z2 that is none


@pytest.mark.parametrize("route", ROUTES)
def test_point_mode_one_a_stride_with_a_gap_and_the_resident_form_behind_other_work(oc, hip, env, route):
    import torch
    hip.set_option("set_each_route", route)
    k, n, d, stride = 3, 9, 32, 5
    w = pow(pow(5, (R - 1) >> 28, R), (1 << 28) // d, R)
    idx = [[(5 * i + 3 * j * j + j) % d for j in range(k)] for i in range(n)]
    assert all(len(set(row)) == k for row in idx)
    c = M.valid_case(TAU, [rand_fr_ints(7, 7500)], [[pow(w, e, R) for e in row] for row in idx], [1] * n)
    c = P.corrupt(c, "proof", 6)
    want = P.statuses(c)
    x = Inputs(oc, c)
    flat_idx = np.full(n * stride, 0x7FFFFFFF, np.uint32)
    vals = np.full((n * stride, 4), SENT, np.uint64)
    for i in range(n):
        flat_idx[i * stride:i * stride + k] = idx[i]
        vals[i * stride:i * stride + k] = x.values[i * k:(i + 1) * k]
    check(each(hip, env, x, points=flat_idx, values=vals, item_stride=stride, omega=mont(oc, [w])), want)
    # resident, queued behind other work on the context's stream: a set_pairs call of the same context, not waited for
    d_in = [dev(x.com), dev(flat_idx), dev(vals), dev(x.proofs)]
    d_status = torch.full((n,), 7, dtype=torch.uint8).cuda()
    d_a, d_z = torch.zeros(n * 8, dtype=torch.int64).cuda(), torch.zeros(n * 16, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    hip.kzg_set_pairs_dev(env["srs1"], env["srs2"], d_in[0], 0, d_in[1], 1, mont(oc, [w]), d_in[2], stride, k, n, d_a, d_z)
    n_bad, first = hip.kzg_verify_sets_each_dev(env["srs1"], env["srs2"], d_in[0], 0, d_in[1], 1, mont(oc, [w]), d_in[2], stride, k, d_in[3], n, d_status, d_a, d_z)
    assert (n_bad, first) == (1, 6) and d_status.cpu().numpy().tolist() == want
    x.check((d_a.cpu().numpy().view(np.uint64).reshape(n, 8), d_z.cpu().numpy().view(np.uint64).reshape(n, 16)))


def raw_each(hip, env, x, n=None, k=None, com_stride=1, point_mode=0, stride=None, proofs=True, status=True, n_bad=True, com=True, srs2=None):
    import ctypes as C
    n = x.n if n is None else n
    k = x.k if k is None else k
    st_arr = np.full(max(x.n, 1), 0xAB, np.uint8)
    a = np.full((max(x.n, 1), 8), SENT, np.uint64)
    z = np.full((max(x.n, 1), 16), SENT, np.uint64)
    bad, first = C.c_uint64(77), C.c_uint64(78)
    p = lambda arr, on: arr.ctypes.data if on else None
    st = hip.lib.keaki_hip_kzg_verify_sets_each(hip.ctx, env["srs1"].handle, (srs2 or env["srs2"]).handle, p(x.com, com), com_stride, p(x.points, True), point_mode, None,
                                                p(x.values, True), k if stride is None else stride, k, p(x.proofs, proofs), n, p(st_arr, status),
                                                C.byref(bad) if n_bad else None, C.byref(first), p(a, True), p(z, True))
    untouched = bool((st_arr == 0xAB).all() and (a == SENT).all() and (z == SENT).all())
    return st, untouched, bad.value, first.value


def test_empty_calls_and_refusals_write_nothing(oc, hip, env):
    x = Inputs(oc, make_case(4, 3, 7600))
    assert raw_each(hip, env, x, n=0) == (0, True, 0, 2 ** 64 - 1)
    for kw in (dict(proofs=False), dict(status=False), dict(n_bad=False), dict(com=False), dict(k=0), dict(k=65), dict(stride=2), dict(com_stride=-1),
               dict(point_mode=1), dict(n=1 << 31)):
        assert raw_each(hip, env, x, **kw) == (BAD_ARG, True, 77, 78), kw
    s1, s2 = handles(oc, hip, TAU, 3)
    try:
        assert raw_each(hip, env, x, srs2=s2) == (TOO_LARGE, True, 77, 78)
        y = Inputs(oc, make_case(3, 1, 7601))
        hip.set_option("set_rows_wb", 13)
        hip.debug_set_alloc_limit(100000)
        own = {"srs1": s1, "srs2": s2}
        assert raw_each(hip, own, y) == (OOM, True, 77, 78)                 # the table is refused at every width
        hip.debug_set_alloc_limit(0)
        hip.set_option("set_rows_wb", 8)
        check(each(hip, own, y), [0] * 3)                                   # the context and the handles stay usable
    finally:
        hip.debug_set_alloc_limit(0)
        s1.free()
        s2.free()
