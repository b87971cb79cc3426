"""CPU suite: the model the GPU tests of keaki_hip_kzg_verify_each compare with (tests/verify_each_model.py) is itself checked against the
oracle's pairings -- in the rearranged form the kernel evaluates and in the reference's own form -- and the new symbols exist in every layer."""
import ctypes
import os
import re

import numpy as np
import pytest

import verify_each_model as M
from conftest import rand_fr_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def six_items():
    """valid | valid constant polynomial (proof = identity, C = y g1) | wrong value | wrong proof | wrong point | L = identity with a proof"""
    r = rand_fr_ints(40, 2718)
    c = M.valid_case(r[0], r[1:7], r[7:13], r[13:19])
    c.p[1] = 0
    c.y[1] = c.com[1]
    c.y[2] = (c.y[2] + 1) % R
    c.p[3] = (c.p[3] + 1) % R
    c.z[4] = (c.z[4] + 1) % R
    c.y[5] = (c.com[5] + c.z[5] * c.p[5]) % R
    assert c.status() == [0, 0, 1, 1, 1, 1] and c.lhs()[5] == 0 and c.lhs()[1] == 0
    return c


@pytest.fixture(scope="module")
def points(oc):
    c = six_items()
    g1, g2 = oc.generators()
    return c, g1, g2, oc.g2_mul_batch(g2, mont(oc, [c.s]))[0]


def test_model_agrees_with_the_oracles_pairings(oc, points):
    """valid_i <=> e(L_i, g2) e(-proof_i, [tau]_2) == 1 <=> e(L_i, g2) == e(proof_i, [tau]_2) (e(-P, Q) is the inverse of e(P, Q)),
    on the oracle's GT bytes"""
    c, g1, g2, tau_g2 = points
    L = oc.g1_mul_batch(g1, mont(oc, c.lhs()))
    proofs = oc.g1_mul_batch(g1, mont(oc, c.p))
    lhs, rhs = oc.pairing_batch(L, g2), oc.pairing_batch(proofs, tau_g2)
    assert [0 if np.array_equal(lhs[i], rhs[i]) else 1 for i in range(c.n)] == c.status()


def test_model_agrees_with_the_references_form(oc, points):
    """src/kzg.rs:135-148 as written: e(C - y g1, g2) == e(proof, tau g2 - z g2)"""
    c, g1, g2, tau_g2 = points
    a = oc.g1_mul_batch(g1, mont(oc, [c.com_of(i) - c.y[i] for i in range(c.n)]))
    q = oc.g2_mul_batch(g2, mont(oc, [c.s - z for z in c.z]))
    proofs = oc.g1_mul_batch(g1, mont(oc, c.p))
    lhs, rhs = oc.pairing_batch(a, g2), oc.pairing_batch(proofs, q)
    assert [0 if np.array_equal(lhs[i], rhs[i]) else 1 for i in range(c.n)] == c.status()


def test_identity_rules_are_the_equation():
    r = rand_fr_ints(8, 99)
    s, c0, z, p = r[0], r[1], r[2], r[3]
    assert M.Case(s, [c0], [z], [c0], [0]).status() == [0]                          # both identities
    assert M.Case(s, [c0], [z], [c0 + 1], [0]).status() == [1]                      # the proof alone
    assert M.Case(s, [c0], [z], [c0 + z * p], [p]).status() == [1]                  # L alone
    assert M.Case(0, [c0], [z], [c0 + z * p], [p]).status() == [0]                  # [tau]_2 = identity: valid <=> L = identity
    assert M.Case(0, [c0], [z], [c0 + z * p + 1], [p]).status() == [1]
    c = M.valid_case(s, r[4:6], r[6:8], [p, p + 1])
    assert c.status() == [0, 0] and c.counters() == (0, None)
    c.y[1] += 1
    assert c.counters() == (1, 1)


def test_symbols_exist_in_every_layer():
    """fails on a tree without keaki_hip_kzg_verify_each"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "keaki_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "keaki-hip-sys", "src", "lib.rs")).read()
    from keaki_amd import hip
    lib = hip.load_library()
    for s in ("keaki_hip_kzg_verify_each", "keaki_hip_kzg_verify_each_dev"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in hip.EXPORTS
        assert re.search(r"pub fn %s\(" % s, rs), s
    assert hasattr(hip.KeakiHip, "kzg_verify_each") and hasattr(hip.KeakiHip, "kzg_verify_each_dev")
    assert "sys::keaki_hip_kzg_verify_each(" in open(os.path.join(ROOT, "rust", "keaki", "src", "hip.rs")).read()
    host = ctypes.CDLL(os.path.join(ROOT, "keaki_amd", "libkeaki_host.so"))
    for s in ("keaki_host_verify_each", "keaki_host_locate_invalid", "keaki_host_vec_verify_each"):
        assert hasattr(host, s), s
    from keaki_amd import keaki as K
    assert callable(K.verify_each) and callable(K.locate_invalid) and callable(K.vec_verify_each)
