"""CPU suite: the model the GPU tests of keaki_hip_kzg_verify_batch compare with (tests/verify_batch_model.py) is itself checked -- the
discrete-log form against the point form, the verdict against the reference's own predicate -- and the new symbols exist in every layer."""
import ctypes
import os
import re

import pytest

import verify_batch_model as M
from conftest import rand_fr_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R


def make(n, degree, seed, shifts=False, roots=False, py=None):
    r = rand_fr_ints(3 * n + degree + 8, seed)
    tau, coeffs = r[0], r[1:degree + 2]
    zs = M.powers(py.fr_root_of_unity(1 << max(1, (n).bit_length())), n) if roots else r[degree + 2:degree + 2 + n]
    gammas = r[degree + 2 + n:degree + 2 + 2 * n]
    sh = r[degree + 2 + 2 * n:degree + 2 + 3 * n] if shifts else None
    return M.valid_case(tau, coeffs, zs, gammas, sh)


def as_points(py, c):
    g = py.G1_GEN
    return [py.g1_mul(g, x) for x in c.com], [py.g1_mul(g, x) for x in c.q]


@pytest.mark.parametrize("n,degree,shifts", [(1, 0, False), (2, 1, False), (3, 7, True), (17, 7, False), (64, 7, True)])
def test_discrete_log_model_equals_point_model(py, n, degree, shifts):
    c = make(n, degree, 100 + n, shifts)
    coms, proofs = as_points(py, c)
    assert M.combine(coms, c.z, c.y, proofs, c.gamma) == c.points()
    assert c.verdict()
    L, Rp = c.points()
    assert py.g1_mul(Rp, c.tau) == L                 # the verdict on points: tau R == L


def test_verdict_is_the_references_predicate_at_n_2(py):
    """e(L, g2) == e(R, [tau]_2) <=> tau R == L; against all(kzg_verify) of the reference's own form with the big-int pairing (slow: one case)"""
    c = make(2, 1, 7)
    g1_pow, tau_g2 = py.kzg_setup(c.tau, 2)
    coms, proofs = as_points(py, c)

    def ref_verify(com, z, y, proof):          # src/kzg.rs:135-148
        lhs = py.pairing(py.g1_add(com, py.g1_neg(py.g1_mul(py.G1_GEN, y))), py.G2_GEN)
        rhs = py.pairing(proof, py.g2_add(tau_g2, py.g2_neg(py.g2_mul(py.G2_GEN, z))))
        return lhs == rhs

    assert all(ref_verify(coms[0], c.z[i], c.y[i], proofs[i]) for i in range(2)) and c.verdict()
    bad = c.copy()
    bad.y[1] = (bad.y[1] + 1) % R
    assert not ref_verify(coms[0], bad.z[1], bad.y[1], proofs[1]) and not bad.verdict()
    L, Rp = c.points()
    assert py.pairing(L, py.G2_GEN) == py.pairing(Rp, tau_g2)


@pytest.mark.parametrize("degree", [0, 1, 7])
def test_valid_openings_accept_and_single_corruptions_reject(py, degree):
    c = make(12, degree, 40 + degree)
    assert c.verdict()
    if degree == 0:
        assert all(q == 0 for q in c.q) and c.sums() == (0, 0)        # every proof the identity, L = R = identity
    if degree == 1:
        assert len(set(c.q)) == 1                                     # all proofs the same point
    for field in ("y", "z", "q", "com"):
        bad = c.copy()
        getattr(bad, field)[0 if field == "com" else 5] += 1
        if degree == 0 and field == "z":
            assert bad.verdict()                                       # a constant opens to the same value everywhere
        else:
            assert not bad.verdict(), field
    swapped = c.copy()
    swapped.q[2], swapped.q[9] = swapped.q[9], swapped.q[2]
    assert swapped.verdict() == (degree <= 1)                          # degree <= 1: all quotients are equal, nothing changed


def test_cancelling_pair_is_accepted_at_equal_gammas_only():
    """the contract of the header: the call evaluates the combined equation for the gammas it is given"""
    c = make(6, 3, 77)
    d = 123456789
    c.y[0] = (c.y[0] + d) % R
    c.y[1] = (c.y[1] - d) % R
    c.gamma[1] = c.gamma[0]
    assert c.verdict()
    c.gamma[1] = (c.gamma[0] + 1) % R
    assert not c.verdict()
    z = c.copy()
    z.gamma = [0] * z.n                          # gamma = 0 accepts anything
    z.y[3] += 5
    assert z.verdict() and z.sums() == (0, 0)


def test_point_mode_1_is_point_mode_0_on_the_powers_of_omega(py):
    n = 13
    w = py.fr_root_of_unity(16)
    c = make(n, 7, 5, roots=True, py=py)
    assert c.z == [pow(w, i, R) for i in range(n)] and c.verdict()
    # the vector-commitment form: p(tau) by the barycentric formula from the evaluations alone
    evals = c.y + [rand_fr_ints(1, 9)[0]]
    ptau, inv = M.barycentric_at(evals, w, 16, c.tau)
    qs = [(ptau - evals[i]) * inv[i] % R for i in range(n)]
    v = M.Case(c.tau, [ptau], c.z, c.y, qs, c.gamma)
    assert v.verdict()


def test_symbols_exist_in_every_layer():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "keaki_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "keaki-hip-sys", "src", "lib.rs")).read()
    from keaki_amd import hip
    for s in ("keaki_hip_kzg_verify_batch", "keaki_hip_kzg_verify_batch_dev"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in hip.EXPORTS
        assert re.search(r"pub fn %s\(" % s, rs), s
    assert hasattr(hip.KeakiHip, "kzg_verify_batch") and hasattr(hip.KeakiHip, "kzg_verify_batch_dev")
    assert "sys::keaki_hip_kzg_verify_batch(" in open(os.path.join(ROOT, "rust", "keaki", "src", "hip.rs")).read()
    hip.load_library()
    lib = ctypes.CDLL(os.path.join(ROOT, "keaki_amd", "libkeaki_host.so"))
    for s in ("keaki_host_verify_batch", "keaki_host_vec_verify"):
        assert hasattr(lib, s), s
    from keaki_amd import keaki as K
    assert callable(K.verify_batch) and callable(K.vec_verify)
    # the header states the contract: the soundness bound needs independent uniform gammas
    full = open(os.path.join(ROOT, "include", "keaki_hip.h")).read()
    assert "independent, uniform" in full and "cancel" in full
