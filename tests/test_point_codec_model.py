"""CPU suite: the big-int model of the compressed point wire format (tests/point_codec_model.py) against known encodings, the reference's own
.ptau fixture, and -- for the subgroup test -- the fast form psi(Q) = [6 z^2]Q against the definition [r]Q = O."""
import json
import os
import random

import bn254_py as py
import point_codec_model as M

P, R = M.P, M.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_known_encodings():
    assert M.g1_compress(py.G1_GEN) == bytes([1]) + bytes(31)
    neg = M.g1_compress(py.g1_neg(py.G1_GEN))
    assert neg[31] == 0x80 and neg[:31] == bytes([1]) + bytes(30)
    assert M.g1_compress(None) == bytes(31) + bytes([0x40])
    assert M.g2_compress(None) == bytes(63) + bytes([0x40])
    # exactly one of P, -P carries the sign flag; x is the same
    a, b = M.g2_compress(py.G2_GEN), M.g2_compress(py.g2_neg(py.G2_GEN))
    assert a[:63] == b[:63] and {a[63] & 0xC0, b[63] & 0xC0} == {0, 0x80}
    assert int.from_bytes(a[:32], "little") == py.G2_GEN[0][0] and int.from_bytes(a[32:], "little") & ((1 << 254) - 1) == py.G2_GEN[0][1]


def test_round_trip_of_the_ptau_fixture():
    pts = py.ptau_points(open(os.path.join(GOLDEN, "ppot_0080_01.ptau.test"), "rb").read())
    assert len(pts["tau_g1"]) == 3 and len(pts["tau_g2"]) == 2
    for p in pts["tau_g1"]:
        assert py.g1_is_on_curve(p)
        for q in (p, py.g1_neg(p)):
            assert M.g1_decompress(M.g1_compress(q)) == (M.OK, q)
            assert M.g1_from_words(M.g1_words(q)) == q
    for p in pts["tau_g2"]:
        assert py.g2_is_on_curve(p)
        for q in (p, py.g2_neg(p)):
            assert M.g2_decompress(M.g2_compress(q), True) == (M.OK, q)
            assert M.g2_from_words(M.g2_words(q)) == q
    assert M.g1_decompress(M.g1_compress(None)) == (M.OK, None) and M.g2_decompress(M.g2_compress(None)) == (M.OK, None)


def test_fq_square_root():
    rnd = random.Random(1)
    roots = none = 0
    for _ in range(200):
        a = rnd.randrange(P)
        c = M.fq_sqrt(a)
        if c is None:
            assert pow(a, (P - 1) // 2, P) == P - 1          # Euler: a non-residue
            none += 1
        else:
            assert c * c % P == a
            roots += 1
    assert roots > 60 and none > 60
    assert M.fq_sqrt(0) == 0 and M.fq_sqrt(1) in (1, P - 1)


def test_fq2_square_root_branches():
    rnd = random.Random(2)
    # generic: every square has a root that squares back; a non-square (norm a non-residue of Fq) has none
    for _ in range(100):
        c = (rnd.randrange(P), rnd.randrange(P))
        a = py.f2_sqr(c)
        r = M.f2_sqrt(a)
        assert r is not None and py.f2_sqr(r) == a and r in (c, py.f2_neg(c))
    squares = nonsquares = 0
    for _ in range(100):
        a = (rnd.randrange(P), rnd.randrange(1, P))
        is_square = pow((a[0] * a[0] + a[1] * a[1]) % P, (P - 1) // 2, P) == 1
        assert (M.f2_sqrt(a) is not None) == is_square
        squares += is_square; nonsquares += not is_square
    assert squares > 25 and nonsquares > 25
    # a1 = 0: a0 a residue -> (sqrt(a0), 0); a0 a non-residue -> (0, sqrt(-a0)); zero -> zero
    res = next(a for a in range(2, 100) if M.fq_sqrt(a) is not None)
    non = next(a for a in range(2, 100) if M.fq_sqrt(a) is None)
    r = M.f2_sqrt((res, 0)); assert r[1] == 0 and r[0] * r[0] % P == res
    r = M.f2_sqrt((non, 0)); assert r[0] == 0 and (-r[1] * r[1]) % P == non
    assert M.f2_sqrt((0, 0)) == (0, 0)
    # both branches of the one-inversion complex method occur (delta a residue / a non-residue)
    seen = set()
    for _ in range(64):
        c = (rnd.randrange(P), rnd.randrange(1, P))
        a = py.f2_sqr(c)
        alpha = pow((a[0] * a[0] + a[1] * a[1]) % P, (P + 1) // 4, P)
        seen.add(M.fq_sqrt((a[0] + alpha) * py.TWO_INV % P) is not None)
        assert py.f2_sqr(M.f2_sqrt(a)) == a
    assert seen == {True, False}


def test_sign_order():
    assert not M.fq_is_neg(0) and not M.fq_is_neg(1) and M.fq_is_neg(P - 1) and not M.fq_is_neg((P - 1) // 2) and M.fq_is_neg((P + 1) // 2)
    # c1 decides; c0 only when c1 = 0
    assert M.f2_is_neg((1, P - 1)) and not M.f2_is_neg((P - 1, 1)) and M.f2_is_neg((P - 1, 0)) and not M.f2_is_neg((1, 0))
    for y in [(5, 7), (P - 5, 0), (0, P - 3), (123, (P + 1) // 2)]:
        assert M.f2_is_neg(y) != M.f2_is_neg(py.f2_neg(y))


def test_psi_is_multiplication_by_p_on_g2():
    for k in (1, 2, 0xC0FFEE):
        q = py.g2_mul(py.G2_GEN, k)
        assert py.g2_is_on_curve(M.psi(q))
        assert M.psi(q) == py.g2_mul(q, P % R)


def test_fast_subgroup_test_agrees_with_the_definition():
    rnd = random.Random(3)
    inside = [py.g2_mul(py.G2_GEN, rnd.randrange(1, R)) for _ in range(60)] + [py.G2_GEN, py.g2_neg(py.G2_GEN), py.g2_mul(py.G2_GEN, 2), py.g2_mul(py.G2_GEN, R - 2)]
    assert len(inside) >= 64
    for q in inside:
        assert M.in_subgroup_def(q) and M.in_subgroup_fast(q)
        assert M.ladder_events(q) == (0, 0, 0)           # the degenerate branches are unreachable inside G2
    outside = M.random_twist_points(64, 4)
    for q in outside:
        assert py.g2_is_on_curve(q)
        assert not M.in_subgroup_def(q) and not M.in_subgroup_fast(q)
    assert M.in_subgroup_def(None) and M.in_subgroup_fast(None)
    # what bn254_py.g2_mul answers is NOT the definition: it reduces the scalar
    assert py.g2_mul(outside[0], R) is None


def test_cofactor_cleared_points_are_members():
    for q in M.random_twist_points(8, 5):
        c = M.mul_unreduced(q, M.COFACTOR)
        assert c is not None and M.in_subgroup_def(c) and M.in_subgroup_fast(c)
        assert M.g2_decompress(M.g2_compress(c), True) == (M.OK, c)


def test_real_y_points_differ_in_c0_only():
    for q in M.g2_points_with_real_y(6, 6):
        assert py.g2_is_on_curve(q) and q[1][1] == 0
        a, b = M.g2_compress(q), M.g2_compress(py.g2_neg(q))
        assert a[:63] == b[:63] and (a[63] ^ b[63]) == 0x80
        assert M.g2_decompress(a, False) == (M.OK, q) and M.g2_decompress(b, False) == (M.OK, py.g2_neg(q))


def test_decoding_rule_rejections():
    x1 = bytes([1]) + bytes(31)
    enc = lambda v: int(v).to_bytes(32, "little")
    assert M.g1_decompress(bytes(31) + bytes([0xC0]))[0] == M.MALFORMED                     # both flags
    for v in (P, P + 1, (1 << 254) - 1):
        assert M.g1_decompress(enc(v))[0] == M.MALFORMED
    assert M.g1_decompress(x1[:31] + bytes([0x40]))[0] == M.MALFORMED                       # identity flag with x = 1
    assert M.g1_decompress(enc(4))[0] == M.NOT_ON_CURVE                                     # 4^3 + 3 = 67 is a non-residue
    assert M.fq_sqrt(67) is None
    assert M.g2_decompress(enc(P) + enc(1))[0] == M.MALFORMED and M.g2_decompress(enc(1) + enc(P))[0] == M.MALFORMED
    assert M.g2_decompress(enc(1 << 255) + enc(1))[0] == M.MALFORMED                        # c0 has no free bits
    assert M.g2_decompress(bytes(63) + bytes([0xC0]))[0] == M.MALFORMED
    assert M.g2_decompress(enc(1) + bytes(31) + bytes([0x40]))[0] == M.MALFORMED
    q = M.random_twist_points(1, 7)[0]
    assert M.g2_decompress(M.g2_compress(q), True) == (M.NOT_IN_SUBGROUP, None) and M.g2_decompress(M.g2_compress(q), False) == (M.OK, q)


def test_recorded_vectors_are_what_the_model_generates():
    want = json.load(open(os.path.join(GOLDEN, "point_codec_vectors.json")))
    assert want == M.golden_vectors()
    for e in want["g2"]:
        w = [int(v, 16) for v in e["words"]]
        q = M.g2_from_words(w)
        st, back = M.g2_decompress(bytes.fromhex(e["bytes"]), True)
        assert (st == M.OK) == e["in_subgroup"] and (back == q if e["in_subgroup"] else back is None)


def test_device_constants_are_the_models():
    """the literal constants of the kernels: (p + 1)/4 and (p - 1)/2 as little-endian words, 6 z^2 as two 64-bit halves"""
    import re
    csrc = os.path.join(os.path.dirname(GOLDEN), "..", "keaki_amd", "csrc")
    words = lambda text, name: [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", re.search(name + r"\[8\] = \{(.*?)\}", text).group(1))]
    value = lambda ws: sum(w << (32 * i) for i, w in enumerate(ws))
    sqrt_h = open(os.path.join(csrc, "fq_sqrt.hip.h")).read()
    codec = open(os.path.join(csrc, "point_codec.hip")).read()
    e = value(words(sqrt_h, "FQ_SQRT_EXP"))
    assert e == (P + 1) // 4 and e.bit_length() == int(re.search(r"FQ_SQRT_EXP_BITS = (\d+)", sqrt_h).group(1))
    assert value(words(codec, "FQ_HALF")) == (P - 1) // 2
    lo, hi = re.search(r"SIX_Z2_LO = 0x([0-9a-f]+)ull, SIX_Z2_HI = 0x([0-9a-f]+)ull", codec).groups()
    assert (int(hi, 16) << 64) | int(lo, 16) == M.SIX_Z2 == P % R and M.SIX_Z2.bit_length() == int(re.search(r"SIX_Z2_BITS = (\d+)", codec).group(1))
