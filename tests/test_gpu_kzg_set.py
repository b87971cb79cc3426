"""KZG set openings on the GPU (keaki_hip_kzg_set_polys / open_multi / aggregate / verify_multi and their _dev forms) against the big-integer model
(tests/kzg_set_model.py). The SRS comes from a KNOWN tau, so every group result has a known discrete log: expected points are (integer) x generator
from the oracle's scalar multiplication, expected quotients come from the model's LONG DIVISION (never from partial fractions, which is what the
kernel computes), and nothing expected comes from the library under test."""
import ctypes as C
import os

import numpy as np
import pytest

import kzg_set_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = M.R
BAD_ARG, TOO_LARGE = -1, -5
N_MAX = 32769
TAU = rand_fr_ints(1, 20261020)[0]
NS = [1, "k", "k+1", 32, 33, 1024, 1025, N_MAX]          # both sides of every level boundary of the 32-coefficient blocks, up to three levels
KS = [1, 2, 7, 8, 9, 17, 64]                             # both sides of the 8-point pass (and of its 1 / 2 / 4-point instantiations)
OMEGA64 = pow(5, (R - 1) // 64, R)


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def unmont(oc, a):
    return oc.limbs_to_ints(oc.fr_from_mont(np.ascontiguousarray(a, np.uint64).reshape(-1, 4)))


def g1_of(oc, dls):
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, dls), threads=NCPU)


def g2_of(oc, dls):
    return oc.g2_mul_batch(oc.generators()[1], mont(oc, dls), threads=NCPU)


def jac_to_aff(j):
    """normalised Jacobian u64[12] -> affine u64[8] ((0, 0) = identity); both forms are unique"""
    j = np.asarray(j, np.uint64)
    return np.zeros(8, np.uint64) if not j[8:].any() else j[:8].copy()


def points_for(k, seed, with_tau=False):
    """k distinct points: 0, 1, r - 1 and roots of unity first, random ones behind"""
    special = [0, 1, R - 1, OMEGA64, pow(OMEGA64, 5, R), pow(OMEGA64, 63, R)]
    pts = (special + rand_fr_ints(k, seed))[:k] if k >= 3 else rand_fr_ints(k, seed)
    if with_tau:
        pts[k // 2] = TAU
    assert len(set(pts)) == k
    return pts


@pytest.fixture(scope="module")
def env(oc, hip):
    """the powers of tau in both groups, uploaded once: a G1 handle with window tables and one without, and the G2 powers"""
    pw = [1]
    for _ in range(N_MAX - 1):
        pw.append(pw[-1] * TAU % R)
    g1 = g1_of(oc, pw)
    g2 = g2_of(oc, pw[:70])
    plain, tabled = hip.srs_g1_upload(g1), hip.srs_g1_upload(g1)
    hip.srs_g1_precompute(tabled)
    srs2 = hip.srs_g2_upload(g2)
    coeffs = rand_fr_ints(N_MAX, 4242)
    e = {"pw": pw, "g1": g1, "g2": g2, "plain": plain, "tabled": tabled, "srs2": srs2, "coeffs": coeffs, "coeffs_m": mont(oc, coeffs), "cache": {}}
    yield e
    for h in (plain, tabled, srs2):
        h.free()


def expected(oc, env, n, k, with_tau=False):
    """(points, values, discrete log of the proof) for the first n coefficients and the k points of this (n, k); computed once"""
    key = (n, k, with_tau)
    if key not in env["cache"]:
        zs = points_for(k, 1000 * k + n % 997, with_tau)
        q, ys = M.quotient_long_division(env["coeffs"][:n], zs)
        env["cache"][key] = (zs, ys, M.poly_eval(q, TAU))
    return env["cache"][key]


def dev(arr):
    """a device copy, complete before the context's own (non-blocking) stream may read it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_zeros(words):
    import torch
    t = torch.zeros(words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint64)


# ---- set_polys -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 64, 1024])
def test_set_polys_every_word(oc, hip, k):
    zs = points_for(k, 31 * k)
    ys = rand_fr_ints(k, 17 * k + 1)
    zc, w, ic = hip.kzg_set_polys(mont(oc, zs), mont(oc, ys))
    assert unmont(oc, zc) == M.vanishing(zs)
    assert unmont(oc, w) == M.weights(zs)
    if k <= 64:
        assert unmont(oc, ic) == M.interpolant(zs, ys)
    else:                                                 # the O(k^3) Lagrange sum of the model is too slow at 1,024: I is THE polynomial of degree < k through the points
        got = unmont(oc, ic)
        assert all(M.poly_eval(got, z) == y for z, y in list(zip(zs, ys))[::37] + [(zs[-1], ys[-1])])
    zc2, w2, none = hip.kzg_set_polys(mont(oc, zs))
    assert none is None and np.array_equal(zc2, zc) and np.array_equal(w2, w)
    # _dev form: the same words
    dz, dy, o_z, o_w, o_i = dev(mont(oc, zs)), dev(mont(oc, ys)), dev_zeros(4 * (k + 1)), dev_zeros(4 * k), dev_zeros(4 * k)
    hip.kzg_set_polys_dev(dz.data_ptr(), dy.data_ptr(), k, o_z.data_ptr(), o_w.data_ptr(), o_i.data_ptr())
    hip.synchronize()
    assert np.array_equal(host(o_z).reshape(-1, 4), zc) and np.array_equal(host(o_w).reshape(-1, 4), w) and np.array_equal(host(o_i).reshape(-1, 4), ic)


# ---- open_multi ----------------------------------------------------------------------------------------------------------------------------
def sizes(n, k):
    return k if n == "k" else k + 1 if n == "k+1" else n


@pytest.mark.parametrize("n_spec", NS, ids=[str(n) for n in NS])
def test_open_multi_against_long_division(oc, hip, env, n_spec):
    for k in KS:
        n = sizes(n_spec, k)
        zs, ys, dl = expected(oc, env, n, k)
        want = g1_of(oc, [dl])[0]
        zm, cm = mont(oc, zs), env["coeffs_m"][:n]
        seen = []
        for srs in (env["plain"], env["tabled"]):
            proof, vals = hip.kzg_open_multi(srs, cm, zm)
            assert unmont(oc, vals) == ys, (n, k)
            assert np.array_equal(jac_to_aff(proof), want), (n, k)
            if n <= k:
                assert not proof[8:].any(), "n <= k: the proof is the identity"
            seen.append(proof)
            d_c, d_z, d_p, d_v = dev(cm), dev(zm), dev_zeros(12), dev_zeros(4 * k)
            hip.kzg_open_multi_dev(srs, d_c.data_ptr(), n, d_z.data_ptr(), k, d_p.data_ptr(), d_v.data_ptr())
            hip.synchronize()
            assert np.array_equal(host(d_p), proof) and np.array_equal(host(d_v).reshape(-1, 4), vals), (n, k)
        assert np.array_equal(seen[0], seen[1]), "with and without window tables: the same bytes"
        if k == 1:
            p1, v1 = hip.kzg_open(env["plain"], cm, zm[0])
            assert np.array_equal(p1, seen[0]) and np.array_equal(v1, vals[0]), "k = 1 is byte for byte keaki_hip_kzg_open"


def test_open_multi_ordinary_special_inputs(oc, hip, env):
    """a point equal to tau (Z(tau) = 0), p = const, and the empty polynomial"""
    for n, k in [(100, 9), (1025, 2)]:
        zs, ys, dl = expected(oc, env, n, k, with_tau=True)
        proof, vals = hip.kzg_open_multi(env["tabled"], env["coeffs_m"][:n], mont(oc, zs))
        assert unmont(oc, vals) == ys and np.array_equal(jac_to_aff(proof), g1_of(oc, [dl])[0])
    zs = points_for(9, 5)
    proof, vals = hip.kzg_open_multi(env["plain"], mont(oc, [12345]), mont(oc, zs))
    assert unmont(oc, vals) == [12345] * 9 and not proof[8:].any()
    proof, vals = hip.kzg_open_multi(env["plain"], np.zeros((0, 4), np.uint64), mont(oc, zs))
    assert not vals.any() and not proof[8:].any()


# ---- aggregate -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 9, 64])
def test_aggregate_equals_open_multi(oc, hip, env, k):
    n = 200
    zs, ys, dl = expected(oc, env, n, k)
    zm, cm = mont(oc, zs), env["coeffs_m"][:n]
    singles, vals = hip.kzg_open_batch(env["tabled"], np.broadcast_to(cm, (k, n, 4)), zm)
    singles_aff = np.stack([jac_to_aff(p) for p in singles])
    want, _ = hip.kzg_open_multi(env["tabled"], cm, zm)
    got = hip.kzg_aggregate(zm, singles_aff)
    assert np.array_equal(got, want), "byte for byte"
    assert np.array_equal(jac_to_aff(got), g1_of(oc, [dl])[0])
    d_z, d_p, d_o = dev(zm), dev(singles_aff), dev_zeros(12)
    hip.kzg_aggregate_dev(d_z.data_ptr(), d_p.data_ptr(), k, d_o.data_ptr())
    hip.synchronize()
    assert np.array_equal(host(d_o), want)


# ---- verify_multi --------------------------------------------------------------------------------------------------------------------------
def commitment(oc, env, n):
    return g1_of(oc, [M.poly_eval(env["coeffs"][:n], TAU)])[0]


@pytest.mark.parametrize("k", KS)
def test_verify_multi_accepts_and_rejects(oc, hip, env, k):
    n = 1025
    zs, ys, dl = expected(oc, env, n, k)
    com, proof = commitment(oc, env, n), g1_of(oc, [dl])[0]
    zm, ym = mont(oc, zs), mont(oc, ys)
    ok, a, zq = hip.kzg_verify_multi(env["tabled"], env["srs2"], com, zm, ym, proof, want_pair=True)
    assert ok
    i_tau = M.poly_eval(M.interpolant(zs, ys), TAU)
    assert np.array_equal(a, g1_of(oc, [M.poly_eval(env["coeffs"][:n], TAU) - i_tau])[0]), "C - [I]_1"
    assert np.array_equal(zq, g2_of(oc, [M.poly_eval(M.vanishing(zs), TAU)])[0]), "[Z]_2"
    assert hip.kzg_verify_multi(env["plain"], env["srs2"], com, zm, ym, proof)
    bad_y = list(ys); bad_y[k // 2] = (bad_y[k // 2] + 1) % R
    assert not hip.kzg_verify_multi(env["tabled"], env["srs2"], com, zm, mont(oc, bad_y), proof), "one changed value"
    bad_z = list(zs); bad_z[-1] = (bad_z[-1] + 12345) % R
    assert not hip.kzg_verify_multi(env["tabled"], env["srs2"], com, mont(oc, bad_z), ym, proof), "one changed point"
    assert not hip.kzg_verify_multi(env["tabled"], env["srs2"], com, zm, ym, g1_of(oc, [dl + 1])[0]), "a proof off by G"
    if k > 1:
        dl2 = expected(oc, env, n, k - 1)[2]
        assert not hip.kzg_verify_multi(env["tabled"], env["srs2"], com, zm, ym, g1_of(oc, [dl2])[0]), "a proof for a different set"
    if k <= 9:                                            # agrees with k single verifications of the single proofs
        for z, y in zip(zs, ys):
            q, v = M.divide_linear(env["coeffs"][:n], z)
            assert v == y and hip.kzg_verify(com, env["g2"][1], mont(oc, [z])[0], mont(oc, [y])[0], g1_of(oc, [M.poly_eval(q, TAU)])[0])


def test_verify_multi_every_honest_opening(oc, hip, env):
    """the proofs open_multi returns verify, at the sizes around the block and pass boundaries, a set that contains tau included"""
    for n, k, with_tau in [(1, 1, False), (2, 2, False), (9, 8, False), (33, 9, False), (1024, 17, False), (N_MAX, 64, False), (100, 9, True)]:
        zs, ys, dl = expected(oc, env, n, k, with_tau)
        proof, vals = hip.kzg_open_multi(env["tabled"], env["coeffs_m"][:n], mont(oc, zs))
        assert hip.kzg_verify_multi(env["tabled"], env["srs2"], commitment(oc, env, n), mont(oc, zs), vals, jac_to_aff(proof)), (n, k, with_tau)


# ---- the set ciphertext: ct = r [Z]_2, key = KDF(e(r (C - [I]_1), g2)), opened by the unchanged decapsulation with the set proof ------------------
@pytest.mark.parametrize("msg_len", [1, 32, 100])
def test_set_ciphertext_is_opened_by_the_set_proof(oc, hip, env, msg_len):
    n, k = 1025, 9
    zs, ys, dl = expected(oc, env, n, k)
    com = commitment(oc, env, n)
    zm, ym = mont(oc, zs), mont(oc, ys)
    ok, a, zq = hip.kzg_verify_multi(env["tabled"], env["srs2"], com, zm, ym, g1_of(oc, [dl])[0], want_pair=True)
    r = rand_fr_ints(1, 99 + msg_len)
    ct = hip.g2_mul_batch(zq, mont(oc, r))
    p_enc = hip.g1_mul_batch(a, mont(oc, r))
    _, key = hip.decap_batch(p_enc, oc.generators()[1].reshape(1, 16), msg_len)
    i_tau = M.poly_eval(M.interpolant(zs, ys), TAU)
    want_p = g1_of(oc, [r[0] * (M.poly_eval(env["coeffs"][:n], TAU) - i_tau)])
    _, want_key = oc.decap_batch(want_p, oc.generators()[1].reshape(1, 16), msg_len)
    assert np.array_equal(key, want_key), "the sender's key against the oracle's KDF of e(r (C - I(tau) G), g2)"
    proof, _ = hip.kzg_open_multi(env["tabled"], env["coeffs_m"][:n], zm)
    _, got = hip.decap_batch(jac_to_aff(proof).reshape(1, 8), ct, msg_len)
    assert np.array_equal(got, key), "decapsulate(pi_S, ct)"
    bad_y = list(ys); bad_y[3] = (bad_y[3] + 1) % R                       # the tuple a different vector would hold: its proof opens another key
    zc = M.vanishing(zs)
    dl_bad = (M.poly_eval(env["coeffs"][:n], TAU) - M.poly_eval(M.interpolant(zs, bad_y), TAU)) * M.inv(M.poly_eval(zc, TAU)) % R
    _, other = hip.decap_batch(g1_of(oc, [dl_bad]), ct, msg_len)
    assert not np.array_equal(other, key)


# ---- errors: nothing is written and the context stays usable ----------------------------------------------------------------------------------
def test_errors_write_nothing(oc, hip, env):
    from keaki_amd.hip import KeakiHipError, _ptr
    lib, ctx = hip.lib, hip.ctx
    zs = points_for(9, 1)
    zm, cm = mont(oc, zs), env["coeffs_m"][:100]
    big = mont(oc, rand_fr_ints(1025, 8))
    SENT = np.uint64(0xDEADBEEFDEADBEEF)
    out, vals = np.full(12, SENT), np.full((1025, 4), SENT)
    zc, w, ic = np.full((1026, 4), SENT), np.full((1025, 4), SENT), np.full((1025, 4), SENT)
    okv = C.c_int32(7)
    com = commitment(oc, env, 100)
    calls = [
        ("open_multi k = 0", BAD_ARG, lambda: lib.keaki_hip_kzg_open_multi(ctx, env["plain"].handle, _ptr(cm), 100, _ptr(zm), 0, _ptr(out), _ptr(vals))),
        ("open_multi k > 1024", BAD_ARG, lambda: lib.keaki_hip_kzg_open_multi(ctx, env["plain"].handle, _ptr(cm), 100, _ptr(big), 1025, _ptr(out), _ptr(vals))),
        ("open_multi null points", BAD_ARG, lambda: lib.keaki_hip_kzg_open_multi(ctx, env["plain"].handle, _ptr(cm), 100, None, 9, _ptr(out), _ptr(vals))),
        ("open_multi null srs", BAD_ARG, lambda: lib.keaki_hip_kzg_open_multi(ctx, None, _ptr(cm), 100, _ptr(zm), 9, _ptr(out), _ptr(vals))),
        ("set_polys k = 0", BAD_ARG, lambda: lib.keaki_hip_kzg_set_polys(ctx, _ptr(zm), None, 0, _ptr(zc), _ptr(w), None)),
        ("set_polys k > 1024", BAD_ARG, lambda: lib.keaki_hip_kzg_set_polys(ctx, _ptr(big), None, 1025, _ptr(zc), _ptr(w), None)),
        ("set_polys I without values", BAD_ARG, lambda: lib.keaki_hip_kzg_set_polys(ctx, _ptr(zm), None, 9, _ptr(zc), _ptr(w), _ptr(ic))),
        ("aggregate k = 0", BAD_ARG, lambda: lib.keaki_hip_kzg_aggregate(ctx, _ptr(zm), _ptr(env["g1"]), 0, _ptr(out))),
        ("set_polys null points", BAD_ARG, lambda: lib.keaki_hip_kzg_set_polys(ctx, None, None, 9, _ptr(zc), _ptr(w), None)),
        ("set_polys null weights", BAD_ARG, lambda: lib.keaki_hip_kzg_set_polys(ctx, _ptr(zm), None, 9, _ptr(zc), None, None)),
        ("aggregate k > 1024", BAD_ARG, lambda: lib.keaki_hip_kzg_aggregate(ctx, _ptr(big), _ptr(env["g1"]), 1025, _ptr(out))),
        ("verify_multi k > 1024", BAD_ARG, lambda: lib.keaki_hip_kzg_verify_multi(ctx, env["plain"].handle, env["srs2"].handle, _ptr(com), _ptr(big), _ptr(big), 1025,
                                                                                 _ptr(com), C.byref(okv), None)),
        ("verify_multi null proof", BAD_ARG, lambda: lib.keaki_hip_kzg_verify_multi(ctx, env["plain"].handle, env["srs2"].handle, _ptr(com), _ptr(zm), _ptr(zm), 9,
                                                                                   None, C.byref(okv), None)),
        ("verify_multi null G2 SRS", BAD_ARG, lambda: lib.keaki_hip_kzg_verify_multi(ctx, env["plain"].handle, None, _ptr(com), _ptr(zm), _ptr(zm), 9,
                                                                                    _ptr(com), C.byref(okv), None)),
        ("aggregate null proofs", BAD_ARG, lambda: lib.keaki_hip_kzg_aggregate(ctx, _ptr(zm), None, 9, _ptr(out))),
        ("verify_multi k = 0", BAD_ARG, lambda: lib.keaki_hip_kzg_verify_multi(ctx, env["plain"].handle, env["srs2"].handle, _ptr(com), _ptr(zm), _ptr(zm), 0,
                                                                              _ptr(com), C.byref(okv), None)),
        ("verify_multi short G2 SRS", TOO_LARGE, lambda: lib.keaki_hip_kzg_verify_multi(ctx, env["plain"].handle, env["srs2"].handle, _ptr(com), _ptr(big), _ptr(big),
                                                                                       70, _ptr(com), C.byref(okv), None)),
    ]
    short = hip.srs_g1_upload(env["g1"][:50])
    calls.append(("open_multi short SRS", TOO_LARGE, lambda: lib.keaki_hip_kzg_open_multi(ctx, short.handle, _ptr(cm), 100, _ptr(zm), 9, _ptr(out), _ptr(vals))))
    for what, code, call in calls:
        assert call() == code, what
        assert (out == SENT).all() and (vals == SENT).all() and (zc == SENT).all() and (w == SENT).all() and (ic == SENT).all() and okv.value == 7, what
        assert hip.lib.keaki_hip_last_error(ctx), what
    short.free()
    with pytest.raises(ValueError):
        hip.kzg_aggregate(zm, env["g1"][:3])
    with pytest.raises(KeakiHipError):
        hip.kzg_open_multi(env["plain"], cm, np.zeros((0, 4), np.uint64))
    # the context is still usable
    zs, ys, dl = expected(oc, env, 33, 9)
    proof, vals = hip.kzg_open_multi(env["plain"], env["coeffs_m"][:33], mont(oc, zs))
    assert unmont(oc, vals) == ys and np.array_equal(jac_to_aff(proof), g1_of(oc, [dl])[0])
