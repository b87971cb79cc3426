"""CPU suite: the model the GPU tests of keaki_hip_kzg_verify_cosets compare with (tests/coset_verify_model.py) is itself checked -- its
interpolant against Lagrange interpolation, its verdict on valid items and on every corruption the GPU tests use (so those are rejected by the
equation, not by luck), the l = 1 case against verify_batch_model -- and the new symbols exist in every layer."""
import ctypes
import os
import re

import pytest

import coset_verify_model as M
import fk_coset_model as FM
import kzg_set_model as SM
import verify_batch_model as VB
from conftest import rand_fr_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R


def make(n, l, degree, seed, shared=True):
    r = rand_fr_ints(1 + 2 * n + (degree + 1) * (1 if shared else n), seed)
    tau, hs, gammas, rest = r[0], r[1:1 + n], r[1 + n:1 + 2 * n], r[1 + 2 * n:]
    polys = [rest[i * (degree + 1):(i + 1) * (degree + 1)] for i in range(1 if shared else n)]
    return M.valid_case(tau, polys, hs, l, gammas)


def corruptions(c):
    """name -> corrupted copy: the list tests/test_gpu_verify_cosets.py runs on the device (n >= 3, l >= 2)"""
    out = {}
    for name, t in (("value at t = 0", 0), ("value at t = l - 1", c.l - 1)):
        b = c.copy()
        b.y[1][t] = (b.y[1][t] + 1) % R
        out[name] = b
    b = c.copy()
    b.q[0], b.q[2] = b.q[2], b.q[0]
    out["two proofs swapped"] = b
    b = c.copy()
    b.y[0], b.y[2] = b.y[2], b.y[0]
    out["two value rows swapped"] = b
    b = c.copy()
    b.h[1] = (b.h[1] + 1) % R
    out["a wrong shift"] = b
    return out


@pytest.mark.parametrize("l", [1, 2, 4, 8, 32])
def test_interpolant_is_lagrange_on_the_cosets_points(l):
    h, *ys = rand_fr_ints(1 + l, 300 + l)
    a = M.interpolant_coset(h, ys)
    zs = M.coset_points(h, l)
    assert a == SM.interpolant(zs, ys)
    assert [FM.poly_eval(a, z) for z in zs] == ys
    assert all((pow(z, l, R) - pow(h, l, R)) % R == 0 for z in zs)          # the coset is the solution set of x^l = h^l


@pytest.mark.parametrize("n,l,degree,shared", [(1, 1, 5, True), (3, 2, 9, True), (5, 4, 3, False), (4, 8, 20, False), (3, 16, 15, True), (2, 64, 70, True)])
def test_valid_items_accept_and_every_corruption_rejects(n, l, degree, shared):
    c = make(n, l, degree, 10 * n + l, shared)
    assert c.verdict() and all(c.single(k) for k in range(n))
    if degree < l:
        assert not any(c.q), "deg p < l: every proof is the identity"
    if n >= 3 and l >= 2 and degree >= l:
        for name, b in corruptions(c).items():
            assert not b.verdict(), name
            assert not all(b.single(k) for k in range(n)), name


@pytest.mark.parametrize("log2d,log2l", [(4, 1), (6, 2), (6, 6), (8, 3), (5, 0)])
def test_vector_cosets_with_the_proofs_of_the_opening_model(log2d, log2l):
    """proofs from fk_coset_model.proofs_direct (the model of keaki_hip_open_fk_cosets): coset i is {i + t r}, h = omega_d^i, c = omega_r^i"""
    d, l = 1 << log2d, 1 << log2l
    r = d // l
    rnd = rand_fr_ints(1 + r + d, 900 + 16 * log2d + log2l)
    c, evals = M.vector_case(rnd[0], rnd[1 + r:], log2d, log2l, rnd[1:1 + r])
    assert c.verdict() and all(c.single(i) for i in range(r))
    wr = M.omega(r) if r > 1 else 1
    assert [pow(h, l, R) for h in c.h] == [pow(wr, i, R) for i in range(r)]
    assert all(c.y[i][t] == evals[i + t * r] for i in range(r) for t in range(l))
    wrong_tau = c.copy()
    wrong_tau.tau_l = c.tau                      # [tau]_2 in place of [tau^l]_2
    assert wrong_tau.verdict() == (l == 1 or not any(c.q))
    if r >= 3 and l >= 2:
        for name, b in corruptions(c).items():
            assert not b.verdict(), name


def test_l_1_is_verify_batch():
    n = 9
    c = make(n, 1, 6, 4321)
    vb = VB.Case(c.tau, c.com, c.h, [row[0] for row in c.y], c.q, c.gamma)
    assert vb.verdict() and c.sums() == vb.sums()
    c.y[3][0] += 1
    vb.y[3] += 1
    assert c.sums() == vb.sums() and not c.verdict()


def test_cancelling_pair_is_accepted_at_equal_gammas_only():
    """the contract of the header: the call evaluates the combined equation for the gammas it is given"""
    c = make(4, 4, 11, 77, shared=False)
    h = c.h[0]
    polys_tau = rand_fr_ints(40, 5)
    c = M.valid_case(c.tau, [polys_tau[:12], polys_tau[12:24], polys_tau[24:36], polys_tau[28:40]], [h, h, c.h[2], c.h[3]], 4, c.gamma)
    assert c.verdict()
    d = 123456789
    c.y[0][2] = (c.y[0][2] + d) % R
    c.y[1][2] = (c.y[1][2] - d) % R
    c.gamma = [1] * c.n
    assert c.verdict() and not c.single(0) and not c.single(1)
    c.gamma = rand_fr_ints(c.n, 6)
    assert not c.verdict()
    z = c.copy()
    z.gamma = [0] * z.n                          # gamma = 0 accepts anything
    assert z.verdict() and z.sums() == (0, 0)


def test_tile_constants_match_the_sources():
    internal = open(os.path.join(ROOT, "keaki_amd", "csrc", "internal.h")).read()
    kernel = open(os.path.join(ROOT, "keaki_amd", "csrc", "kzg_cosets.hip")).read()
    assert re.search(r"VC_TILE_ELEMS = (\d+)", internal).group(1) == str(M.VC_TILE_ELEMS)
    assert re.search(r"VC_INV = (\d+)", kernel).group(1) == str(M.VC_INV)
    assert M.tile_items(1024) == 1 and M.tile_items(1) == 1024
    # ONE Fermat inversion in the library
    csrc = os.path.join(ROOT, "keaki_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hip.h")) and re.search(r"MOD\[0\] - 2u", open(os.path.join(csrc, f)).read())]
    assert defs == ["kzg_fr.hip.h"], defs


def test_symbols_exist_in_every_layer():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "keaki_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "keaki-hip-sys", "src", "lib.rs")).read()
    from keaki_amd import hip
    for s in ("keaki_hip_kzg_verify_cosets", "keaki_hip_kzg_verify_cosets_dev"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in hip.EXPORTS
        assert re.search(r"pub fn %s\(" % s, rs), s
    assert hasattr(hip.KeakiHip, "kzg_verify_cosets") and hasattr(hip.KeakiHip, "kzg_verify_cosets_dev")
    assert "sys::keaki_hip_kzg_verify_cosets(" in open(os.path.join(ROOT, "rust", "keaki", "src", "hip.rs")).read()
    hip.load_library()
    lib = ctypes.CDLL(os.path.join(ROOT, "keaki_amd", "libkeaki_host.so"))
    for s in ("keaki_host_verify_cosets", "keaki_host_vec_verify_cosets", "keaki_host_vec_verify_cosets_subset"):
        assert hasattr(lib, s), s
    from keaki_amd import keaki as K
    assert callable(K.verify_cosets) and callable(K.vec_verify_cosets) and callable(K.vec_verify_cosets_subset)
    full = open(os.path.join(ROOT, "include", "keaki_hip.h")).read()
    assert "tau^l" in full and "keaki_hip_kzg_verify_cosets" in full
