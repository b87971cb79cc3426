"""CPU half of the structured-input tests (tests/structured_inputs.py): (a) the models of the kernels' order of operations reach the
exceptional additions the GPU tests of tests/test_gpu_structured_srs.py are meant to exercise -- and the random control reaches none;
(b) the discrete-log references and the oracle agree with the pure-Python group arithmetic on small structured instances."""
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
