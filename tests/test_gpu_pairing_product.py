"""keaki_hip_pairing_product (_dev) on the GPU: prod_i e(P_i, Q_i) with ONE final exponentiation. With P_i = a_i g1 and Q_i = b_i g2 the product is
e(g1, g2)^(sum a_i b_i) = e((sum a_i b_i) g1, g2), which the oracle computes as ONE pairing of its own: nothing expected comes from the library."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

NCPU = min(os.cpu_count() or 1, 16)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BAD_ARG = -1
GT_ONE = np.zeros(384, np.uint8)
GT_ONE[0] = 1                                # serialize_uncompressed(1): c0.c0.c0 = 1 little-endian, every other coefficient zero


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


@pytest.fixture(scope="module")
def pairs(oc):
    """1,025 pairs (a_i g1, b_i g2) with their scalars, made once by the oracle"""
    n = 1025
    r = rand_fr_ints(2 * n, 20261022)
    a, b = r[:n], r[n:]
    g1, g2 = oc.generators()
    return {"a": a, "b": b, "p": oc.g1_mul_batch(g1, mont(oc, a), threads=NCPU), "q": oc.g2_mul_batch(g2, mont(oc, b), threads=NCPU)}


def expected(oc, a, b, skip=()):
    s = sum(x * y for i, (x, y) in enumerate(zip(a, b)) if i not in skip) % R
    g1, g2 = oc.generators()
    if s == 0:
        return GT_ONE
    return oc.pairing_batch(oc.g1_mul_batch(g1, mont(oc, [s]), threads=1), g2, threads=1)[0]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129, 1025])
def test_product_is_one_pairing_of_the_summed_exponent(oc, hip, pairs, n):
    """64 / 65: around the 32 lane pairs of a workgroup times two; 129: one element more than a single workgroup takes (two partial products and a
    second launch); 1,025: nine workgroups, the last with one element"""
    got = hip.pairing_product(pairs["p"][:n], pairs["q"][:n])
    assert got.shape == (384,) and np.array_equal(got, expected(oc, pairs["a"][:n], pairs["b"][:n]))
    if n == 1:
        assert np.array_equal(got, hip.pairing_batch(pairs["p"][:1], pairs["q"][:1])[0])


def test_identities_contribute_one(oc, hip, pairs):
    n = 70
    p, q = pairs["p"][:n].copy(), pairs["q"][:n].copy()
    p[3] = 0; p[64] = 0                       # identities in the G1 slot
    q[5] = 0; q[69] = 0                       # ... in the G2 slot
    p[7] = 0; q[7] = 0                        # ... in both
    got = hip.pairing_product(p, q)
    assert np.array_equal(got, expected(oc, pairs["a"][:n], pairs["b"][:n], skip=(3, 64, 5, 69, 7)))
    assert np.array_equal(hip.pairing_product(np.zeros((n, 8), np.uint64), q), GT_ONE)
    assert np.array_equal(hip.pairing_product(p, np.zeros((n, 16), np.uint64)), GT_ONE)
    assert np.array_equal(hip.pairing_product(np.zeros((3, 8), np.uint64), np.zeros((3, 16), np.uint64)), GT_ONE)


def test_empty_product_and_a_pair_with_its_negation(oc, hip, pairs):
    assert np.array_equal(hip.pairing_product(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64)), GT_ONE)
    g1 = oc.generators()[0]
    neg = oc.g1_mul_batch(g1, mont(oc, [R - pairs["a"][0]]), threads=1)[0]
    p = np.stack([pairs["p"][0], neg])
    q = np.stack([pairs["q"][0], pairs["q"][0]])
    assert np.array_equal(hip.pairing_product(p, q), GT_ONE)
    # ... among others: the rest of the product is what remains
    p3, q3 = np.concatenate([p, pairs["p"][1:4]]), np.concatenate([q, pairs["q"][1:4]])
    assert np.array_equal(hip.pairing_product(p3, q3), expected(oc, pairs["a"][1:4], pairs["b"][1:4]))


def test_dev_form_equals_the_host_form(oc, hip, pairs):
    import torch
    for n in (0, 5, 200):
        p, q = pairs["p"][:n], pairs["q"][:n]
        d_p = torch.from_numpy(np.ascontiguousarray(p).view(np.int64).copy().reshape(-1)).cuda() if n else torch.zeros(8, dtype=torch.int64, device="cuda:0")
        d_q = torch.from_numpy(np.ascontiguousarray(q).view(np.int64).copy().reshape(-1)).cuda() if n else torch.zeros(16, dtype=torch.int64, device="cuda:0")
        d_out = torch.full((400,), 255, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        hip.pairing_product_dev(d_p, d_q, n, d_out)
        hip.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:384], hip.pairing_product(p, q)) and (out[384:] == 255).all(), n


def test_errors_write_nothing(oc, hip, pairs):
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full(384, 0xAB, np.uint8)
    p, q = np.ascontiguousarray(pairs["p"][:2]), np.ascontiguousarray(pairs["q"][:2])
    lib = hip.lib
    assert lib.keaki_hip_pairing_product(hip.ctx, None, ptr(q), 2, ptr(out)) == BAD_ARG
    assert lib.keaki_hip_pairing_product(hip.ctx, ptr(p), None, 2, ptr(out)) == BAD_ARG
    assert lib.keaki_hip_pairing_product(hip.ctx, ptr(p), ptr(q), 2, None) == BAD_ARG
    assert lib.keaki_hip_pairing_product(hip.ctx, ptr(p), ptr(q), 1 << 31, ptr(out)) == BAD_ARG
    assert lib.keaki_hip_pairing_product_dev(hip.ctx, None, None, 2, ptr(out)) == BAD_ARG
    assert (out == 0xAB).all()
    assert np.array_equal(hip.pairing_product(p, q), expected(oc, pairs["a"][:2], pairs["b"][:2]))
