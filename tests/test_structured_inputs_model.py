"""CPU half of the structured-input tests (tests/structured_inputs.py): (a) the models of the kernels' order of operations reach the
exceptional additions the GPU tests of tests/test_gpu_structured_srs.py are meant to exercise -- and the random control reaches none;
(b) the discrete-log references and the oracle agree with the pure-Python group arithmetic on small structured instances; (c) the
digit-edge scalars of tests/test_gpu_fb_digit_edges.py rebuild under the recoding model and reach every class in every non-top window."""
import random

import numpy as np
import pytest

import structured_inputs as S

R = S.R
FK_POLYS = ("rand", "ones", "const")


def fk_poly(kind, d, seed=0):
    if kind == "rand":
        rnd = random.Random(seed + d)
        return [rnd.randrange(R) for _ in range(d)]
    if kind == "ones":
        return [1] * d
    return [7] + [0] * (d - 1)


def test_catalogue_is_what_it_claims():
    assert (S.LAMBDA * S.LAMBDA + S.LAMBDA + 1) % R == 0
    sec = S.secrets(c=8, log2d=3)
    assert sec["half"] * 2 % R == 1 and sec["two_pow_c"] == 256
    assert pow(sec["omega_2d"], 16, R) == 1 and pow(sec["omega_2d"], 8, R) == R - 1
    assert sec["omega_d"] == sec["omega_2d"] ** 2 % R and (sec["omega_2d"] + sec["minus_omega_2d"]) % R == 0
    assert S.powers(R - 1, 4) == [1, R - 1, 1, R - 1]


@pytest.mark.parametrize("log2d", [2, 3, 6])
def test_fk_model_computes_the_proofs(log2d):
    """the model's pipeline is the FK23 of the reference: every proof equals the direct opening at omega_d^i"""
    d = 1 << log2d
    for name, tau in S.secrets(8, log2d).items():
        for kind in FK_POLYS:
            p = fk_poly(kind, d)
            out, _ = S.fk_model(tau, p, log2d)
            evals = S.ntt(p + [0] * (d - len(p)), S.root_of_unity(d)) if d > 1 else [sum(p) % R]
            assert out == S.fk_dlogs(tau, p, evals), (name, kind)
            wd = S.root_of_unity(d)
            assert out[1] == S.open_dlog(tau, p, wd), (name, kind)


# which exceptional branches each structured secret reaches in the FK23 transforms, at the domains of the GPU test
FK_TARGETS = {
    "one": ("hat_s_addsub_special", "fwd_addsub_special"),
    "minus_one": ("hat_s_addsub_special", "inv_addsub_special", "fwd_addsub_special"),
    "omega_2d": ("hat_s_addsub_special",),
    "omega_d": ("hat_s_addsub_special", "inv_addsub_special", "fwd_addsub_special"),
    "minus_omega_2d": ("hat_s_addsub_special",),
    "zero": ("inv_addsub_special", "fwd_addsub_special"),
}
FK_TARGETS_R4 = {                                                     # log2 d = 12: the only domain of the list with radix-4 passes
    "one": ("hat_s_r4_fallback", "fwd_r4_fallback"),
    "zero": ("inv_mul2_identity", "fwd_r4_fallback"),
    "omega_d": ("inv_mul2_identity", "hat_s_r4_fallback", "fwd_r4_fallback"),
}


@pytest.mark.parametrize("log2d", [2, 3, 6, 9])
def test_fk_model_reaches_the_exceptional_butterflies(log2d):
    d = 1 << log2d
    sec = S.secrets(8, log2d)
    for name, keys in FK_TARGETS.items():
        total = dict.fromkeys(keys, 0)
        for kind in FK_POLYS:
            _, ev = S.fk_model(sec[name], fk_poly(kind, d), log2d)
            for k in keys:
                total[k] += ev[k]
        for k in keys:
            if k.startswith("inv") and log2d < 3:
                continue                                      # d = 4: the inverse transform has no butterfly with a non-trivial twiddle
            assert total[k] > 0, (name, k, log2d)
    for kind in FK_POLYS:
        _, ev = S.fk_model(sec["random"], fk_poly(kind, d), log2d)
        assert not any(ev.values()), (kind, ev)


def test_fk_model_reaches_the_radix4_fallbacks():
    log2d = 12
    d = 1 << log2d
    sec = S.secrets(8, log2d)
    for name, keys in FK_TARGETS_R4.items():
        total = dict.fromkeys(keys, 0)
        for kind in FK_POLYS:
            _, ev = S.fk_model(sec[name], fk_poly(kind, d), log2d)
            for k in keys:
                total[k] += ev[k]
        assert all(v > 0 for v in total.values()), (name, total)
    _, ev = S.fk_model(sec["random"], fk_poly("ones", d), log2d)
    assert not any(ev.values()), ev
    _, ev = S.fk_model(sec["one"], fk_poly("rand", d), log2d, radix4=False)     # with fk_radix4 off no lane takes the radix-4 pass
    assert ev["hat_s_r4_fallback"] == 0 and ev["hat_s_addsub_special"] > 0


# secrets whose SRS holds two equal or opposite table entries whatever n and c (generic mode: two equal or opposite points)
MSM_COLLIDING = ("one", "minus_one", "two", "half", "two_pow_c", "lambda")
MSM_COLLIDING_GENERIC = ("one", "minus_one", "lambda")


@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("c,n", [(8, 64), (10, 1000), (13, 1 << 14), (16, (1 << 16) + 5)])
def test_msm_collision_scalars_meet_in_one_bucket(c, n, tables):
    sec = S.secrets(c, log2d=6)
    names = ("one", "minus_one", "two_pow_c", "random") if n > (1 << 16) else sec         # the secrets the GPU test runs at this size
    for name in names:
        tau = sec[name]
        dl = S.powers(tau, n)
        sc = S.collision_scalars(dl, c, tables)
        if name in (MSM_COLLIDING if tables else MSM_COLLIDING_GENERIC):
            assert sc is not None, name
        if sc is not None:
            ev = S.bucket_events(S.msm_buckets(dl, sc, c, tables))
            assert ev["same"] >= 1 and ev["opposite"] >= 1, (name, ev)
        if name in ("random", "zero"):
            assert sc is None, name
    # random scalars over the random control: no bucket with a colliding pair
    rnd = random.Random(c)
    dl = S.powers(sec["random"], n)
    assert S.bucket_events(S.msm_buckets(dl, [rnd.randrange(R) for _ in range(n)], c, tables)) == {"same": 0, "opposite": 0}


def test_msm_digits_rebuild_the_scalar():
    rnd = random.Random(5)
    for c in (3, 8, 13, 16):
        _, W, _, offs, _ = S.msm_plan(c)
        for s in [0, 1, R - 1, (1 << 253) + 7] + [rnd.randrange(R) for _ in range(20)]:
            v = sum((-(b + 1) if neg else b + 1) << offs[w] for w, b, neg in S.msm_digits(s, c))
            assert v == s, (c, s)


# (tau, r, z, wb, wide) -> the events the constructed item reaches in the ciphertext sum
ENCAP_CASES = [
    (1, 5, R - 1, 8, True, "equal"),           # lane 0: r [tau]_2 from table A meets the same point from table B
    (256, 5, R - 256, 8, True, "equal"),       # the partial sums of lanes 0 and 1 are equal: the tree doubles
    (7, 9, 7, 8, True, "opposite"),            # z = tau: ct = O
    (1, 5, R - 1, 16, False, "equal"),         # one lane, 16-bit tables: acc = the next entry
    (7, 9, 7, 16, False, "opposite"),
    (7, 9, 7, 16, True, "opposite"),
    (2, 3, R - 2, 16, False, "equal"),
    (3, 5, R - 3, 8, True, "equal"),           # the small-batch items of the GPU test (secrets no 256-item batch uses)
    (768, 5, R - 768, 8, True, "equal"),
    (11, 9, 11, 8, True, "opposite"),
]


@pytest.mark.parametrize("case", ENCAP_CASES)
def test_encap_model_reaches_equal_and_opposite_partial_sums(case):
    tau, r, z, wb, wide, kind = case
    ct, ev = S.encap_ct_events(tau, r, z, wb, wide)
    assert ct == r * (tau - z) % R
    assert ev[kind] > 0, ev


def test_encap_model_random_control():
    rnd = random.Random(9)
    for wb, wide in ((8, True), (16, True), (16, False)):
        for _ in range(20):
            tau, r, z = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
            ct, ev = S.encap_ct_events(tau, r, z, wb, wide)
            assert ct == r * (tau - z) % R and ev == {"equal": 0, "opposite": 0}


# ---- the digit-edge scalars of the fixed-base walks ----------------------------------------------------------------------------------
FB_WIDTHS = list(range(8, 23))


def test_fb_windows_is_the_window_count_of_both_table_shapes():
    """fb_shape (ec_batch.hip.h) and gt_shape (pairing.hip.h) count windows as fb_windows does, and hold 2^(wb-1) + 1 slots each"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "keaki_amd", "csrc")
    for fname, shape in (("ec_batch.hip.h", "FbShape fb_shape"), ("pairing.hip.h", "GtShape gt_shape")):
        with open(os.path.join(csrc, fname)) as f:
            m = re.search(r"inline %s\(u32 wb\) \{ return \{wb, ([^,]+), ([^,]+)\}; \}" % shape, f.read())
        assert m, fname
        c_int = lambda e, wb: eval(re.sub(r"(\d+)u", r"\1", e).replace("/", "//").replace("?", "and").replace(":", "or"), {"wb": wb})
        assert m.group(1) == "(254u + wb - 1u) / wb + ((254u % wb) == 0u ? 1u : 0u)", (fname, m.group(1))
        for wb in list(range(2, 32)) + [127, 254]:
            assert c_int(m.group(1), wb) == S.fb_windows(wb), (fname, wb)
            assert wb > 30 or c_int(m.group(2), wb) == (1 << (wb - 1)) + 1, (fname, wb)


@pytest.mark.parametrize("wb", FB_WIDTHS)
def test_fb_digits_rebuild_the_scalar(wb):
    """sum d_j 2^(wb j) == k with every digit in (-half, half] and no carry out of the last window"""
    rnd = random.Random(100 + wb)
    half = 1 << (wb - 1)
    for k in S.fb_edge_scalars(wb) + [rnd.randrange(R) for _ in range(200)] + [0]:
        digs = S.fb_digits(k, wb)
        assert len(digs) == S.fb_windows(wb)
        assert all(-half < d <= half for d in digs), (wb, k)
        assert sum(d << (wb * j) for j, d in enumerate(digs)) == k, (wb, k)       # a carry out of the top window would leave k - 2^(wb W)
        assert 0 <= digs[-1] <= half, (wb, k)


@pytest.mark.parametrize("wb", FB_WIDTHS)
def test_fb_edge_scalars_reach_every_class_in_every_window(wb):
    sc = S.fb_edge_scalars(wb)
    assert all(0 < k < R for k in sc) and len(set(sc)) == len(sc) <= 16, wb
    W = S.fb_windows(wb)
    need = S.fb_edge_required(wb)
    assert need == {(j, c) for j in range(W - 1) for c in S.FB_EDGE_CLASSES if (j, c) != (0, "full")}
    got = S.fb_edge_covered(sc, wb)
    assert got == need, (wb, sorted(need - got))
    # the classes are what they say, on the digits: window j of some scalar has each of these digits, with the stated carry out
    full, half, p = 1 << wb, 1 << (wb - 1), 1 << S.fb_edge_level(wb)
    assert 1 <= S.fb_edge_level(wb) <= wb - 2 and len({1, half, half - 1, p, p + 1}) == 5
    # class -> (bits + carry in, digit)
    want = {"one": (1, 1), "zero": (0, 0), "half": (half, half), "half-1": (half - 1, half - 1), "pow": (p, p), "neg_first": (half + 1, -(half - 1)),
            "full": (full, 0), "pow+1": (p + 1, p + 1), "minus_one": (full - 1, -1)}
    carried_tops = []
    for k in sc:
        digs = S.fb_digits(k, wb)
        # a carry enters window j iff the digits below it sum to (k mod 2^(wb j)) - 2^(wb j), i.e. to something negative
        cin = [1 if sum(d << (wb * i) for i, d in enumerate(digs[:j])) < 0 else 0 for j in range(W)]
        if cin[W - 1]:
            carried_tops.append(digs[-1])
        for j, c in S.fb_digit_classes(k, wb):
            if c in want:
                assert (((k >> (wb * j)) & (full - 1)) + cin[j], digs[j]) == want[c], (wb, k, j, c)
                if c == "zero":
                    assert (j == 0 or digs[j - 1]) and digs[j + 1]
                if j < W - 1:
                    assert cin[j + 1] == (1 if c in ("neg_first", "full", "minus_one") else 0)
    # the specials: r - 1, r - 2, 1; a carry chain through every non-top window; the largest top digit that takes a carry in
    assert {R - 1, R - 2, 1} <= set(sc)
    chain = (half + 1) + sum((full - 1) << (wb * j) for j in range(1, W - 1))
    assert any(k % (1 << (wb * (W - 1))) == chain and {(j, "full") for j in range(1, W - 1)} <= S.fb_digit_classes(k, wb) for k in sc), wb
    rep = S.fb_edge_report(wb)
    assert rep["pairs"] == rep["required"] == len(need)
    T = (R - 1) >> (wb * (W - 1))
    assert rep["top_limit"] == T and T <= rep["top_max_digit"] <= T + 1
    # no scalar below r has a larger top digit behind a carry: the top bits T need window W - 2 <= that of r - 1
    best = T + 1 if ((R - 1) >> (wb * (W - 2))) & (full - 1) > half else T
    assert max(carried_tops) == best, (wb, max(carried_tops), best)


def test_fb_edge_top_window_limits():
    """what a scalar below r leaves to the top window"""
    assert {wb: S.fb_edge_report(wb)["top_limit"] for wb in (8, 11, 13, 16, 20)} == {8: 48, 11: 1, 13: 96, 16: 12388, 20: 12388}
    assert all(254 % wb for wb in FB_WIDTHS)                 # no width of the range has an extra, empty top window


def test_fb_edge_batch_items_carry_their_scalars_on_every_side():
    """-(r point) and -(r value) are the chosen scalars, and each side's scalars cover every width it is built for"""
    items = S.fb_edge_batch((8, 13, 16), (8, 16), (16, 20))
    assert len(set(items)) == len(items) < 128
    rs, b2, b1 = S.fb_edge_sides(items)
    assert set(rs) == set(S.fb_edge_union((8, 13, 16))) and set(b2) == set(S.fb_edge_union((8, 16))) and set(b1) == set(S.fb_edge_union((16, 20)))
    for side, widths in ((rs, (8, 13, 16)), (b2, (8, 16)), (b1, (16, 20))):
        for wb in widths:
            assert S.fb_edge_covered(side, wb) == S.fb_edge_required(wb), wb
    # a random tau meets nothing: every sum of the GPU cases, in the lane and in the sixteen-lane order
    rnd = random.Random(77)
    tau, c = rnd.randrange(R), rnd.randrange(R)
    for r, z, v in items:
        for wb, wide in ((8, True), (16, True), (16, False)):
            ct, ev = S.encap_ct_events(tau, r, z, wb, wide)
            assert ct == r * (tau - z) % R and ev == {"equal": 0, "opposite": 0}
        k, ev = S.fb_sum_events(c, r, 13, 1, -(r * v) % R, 16, False)
        assert k == r * (c - v) % R and ev == {"equal": 0, "opposite": 0}


# ---- (b) the references against the pure-Python group arithmetic -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero", "one", "minus_one", "two", "half", "two_pow_c", "lambda", "omega_d", "random"])
def test_oracle_msm_equals_py_on_structured_srs(oc, py, name):
    n = 24
    tau = S.secrets(8, 3)[name]
    dl = S.powers(tau, n)
    g1, g2 = oc.generators()
    sc = S.collision_scalars(dl, 8, True) or [pow(3, i + 1, R) for i in range(n)]
    m = lambda v: oc.fr_to_mont(oc.ints_to_limbs(v))
    pts1 = oc.g1_mul_batch(g1, m(dl))
    assert oc.g1_to_ints(pts1) == [py.g1_mul(py.G1_GEN, k) for k in dl]
    exp = py.g1_mul(py.G1_GEN, S.msm_dlog(dl, sc))
    assert oc.g1_to_ints(oc.msm_g1(pts1, m(sc)))[0] == exp == py.msm_naive([py.g1_mul(py.G1_GEN, k) for k in dl], sc)
    k2 = dl[:6]
    pts2 = oc.g2_mul_batch(g2, m(k2))
    assert oc.g2_to_ints(oc.msm_g2(pts2, m(sc[:6])))[0] == py.g2_mul(py.G2_GEN, S.msm_dlog(k2, sc[:6]))


def test_oracle_kem_identity_results_equal_py(oc, py):
    """z = tau gives ct = O; a constant polynomial (C = v g1) gives GT one; decapsulation of O ciphertexts and O proofs is GT one"""
    g1, g2 = oc.generators()
    m = lambda v: oc.fr_to_mont(oc.ints_to_limbs(v))
    one = py.gt_serialize(py.F12_ONE)
    for tau, c, z, v, r in [(7, 11, 7, 3, 5), (7, 11, 2, 11, 5), (1, 0, 1, 0, R - 1), (R - 1, 2, 1, 2, 3)]:
        com = oc.g1_mul_batch(g1, m([c]))[0]
        tg2 = oc.g2_mul_batch(g2, m([tau]))[0]
        ct, gt, key = oc.encap_batch(com, tg2, m([z]), m([v]), m([r]))
        assert oc.g2_to_ints(ct)[0] == py.g2_mul(py.G2_GEN, r * (tau - z) % R)
        k = r * (c - v) % R
        assert gt[0].tobytes() == py.gt_serialize(py.pairing(py.g1_mul(py.G1_GEN, k), py.G2_GEN))
        if k == 0:
            assert gt[0].tobytes() == one
        assert key[0].tobytes() == oc.blake3_xof(gt[0].tobytes(), 32)
    gt, _ = oc.decap_batch(np.zeros((1, 8), np.uint64), oc.g2_mul_batch(g2, m([5])))
    assert gt[0].tobytes() == one
