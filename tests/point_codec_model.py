"""Model of the compressed point wire format (keaki_hip_g1/g2_compress, _decompress, keaki_hip_g2_subgroup_check) in plain big-int arithmetic
on oracle/bn254_py.py. Nothing here touches the library under test.

Wire format (ark-serialize 0.4.2 `serialize_compressed` of a short-Weierstrass affine point, restated from memory: DESIGN section 2):
  G1  32 B: x as a canonical little-endian integer; G2  64 B: x.c0 then x.c1. Flags in the top two bits of the LAST byte: bit 7 = y > -y
  (Fq: on canonical integers; Fq2: c1 decides, c0 when the c1 are equal, i.e. c1 = 0), bit 6 = identity (x = 0).
Decoding rule: status 0 ok, 1 malformed (both flags, a coordinate >= p, identity flag with x != 0), 2 x^3 + b has no root, 3 (G2 with the check
on) outside the order-r subgroup. A rejected item decodes to the identity placeholder None.

Square roots are the device's methods: a^((p+1)/4) in Fq (p = 3 mod 4) and the complex method in Fq2. Subgroup membership has two forms: the
DEFINITION [r]Q = O through `mul_unreduced` (a double-and-add of this file: bn254_py.g2_mul reduces its scalar mod r and so answers O for
every point), and the FAST form psi(Q) = [6 z^2]Q the device computes; tests/test_point_codec_model.py shows they agree.

Degenerate branches of the device ladder (left-to-right double-and-add over the 127 bits of 6 z^2, accumulator Jacobian, addend the affine Q):
  * Q = O never enters the ladder (the identity is a member by definition).
  * For Q in G2 \\ {O} the accumulator holds [k]Q with 1 <= k <= 6 z^2 < r, never O; an addition [k]Q + Q with equal or opposite operands would
    need (k -+ 1) Q = O with 0 < k -+ 1 < r: unreachable, as is [6 z^2]Q = +-Q.
  * For a twist point OUTSIDE G2 the order may be a small factor of the cofactor 2p - r, so the accumulator can become O and an addition can
    meet equal or opposite operands; the addition formulas branch on both, and `ladder_events` below counts them so that the tests can
    build inputs that do reach them (points of small order do not exist on this twist below 10069, so they use [c/m]-multiples)."""
import bn254_py as py

P, R, Z = py.P, py.R, py.Z
SIX_Z2 = 6 * Z * Z
COFACTOR = 2 * P - R                     # order of the twist = r (2p - r)
HALF = (P - 1) // 2
FLAG_NEG, FLAG_INF = 0x80, 0x40
OK, MALFORMED, NOT_ON_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3


# ---- square roots -----------------------------------------------------------------------------------------------------------------------------
def fq_sqrt(a):
    """a root of a in Fq or None: the candidate a^((p+1)/4) is checked by squaring it"""
    a %= P
    c = pow(a, (P + 1) // 4, P)
    return c if c * c % P == a else None


def f2_sqrt(a):
    """a root of a in Fq2 = Fq[u]/(u^2 + 1) or None. Complex method with ONE inversion: alpha = sqrt(a0^2 + a1^2), delta = (a0 + alpha)/2,
    x = delta^((p+1)/4). If x^2 = delta the root is (x, a1/(2x)); otherwise x^2 = -delta (-1 is a non-residue), the other choice
    delta' = (a0 - alpha)/2 = -a1^2/(4 delta) has the root a1/(2x), and the result is (a1/(2x), x). a1 = 0: (sqrt(a0), 0) or (0, sqrt(-a0))."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        x = pow(a0, (P + 1) // 4, P)
        c = (x, 0) if x * x % P == a0 else (0, x)
    else:
        alpha = pow((a0 * a0 + a1 * a1) % P, (P + 1) // 4, P)
        delta = (a0 + alpha) * py.TWO_INV % P
        x = pow(delta, (P + 1) // 4, P)
        t = a1 * pow(2 * x, P - 2, P) % P            # 0 for x = 0, as the device's inversion answers
        c = (x, t) if x * x % P == delta else (t, x)
    return c if py.f2_sqr(c) == (a0, a1) else None


def fq_is_neg(y):
    """the YIsNegative flag of ark-serialize: y > -y on canonical integers"""
    return y % P > HALF


def f2_is_neg(y):
    """Fq2 order: c1 first, then c0"""
    return fq_is_neg(y[1]) if y[1] % P else fq_is_neg(y[0])


# ---- encode / decode --------------------------------------------------------------------------------------------------------------------------
def g1_compress(pt):
    if pt is None:
        return bytes(31) + bytes([FLAG_INF])
    b = bytearray(int(pt[0]).to_bytes(32, "little"))
    if fq_is_neg(pt[1]):
        b[31] |= FLAG_NEG
    return bytes(b)


def g2_compress(pt):
    if pt is None:
        return bytes(63) + bytes([FLAG_INF])
    b = bytearray(int(pt[0][0]).to_bytes(32, "little") + int(pt[0][1]).to_bytes(32, "little"))
    if f2_is_neg(pt[1]):
        b[63] |= FLAG_NEG
    return bytes(b)


def _flags(last):
    return bool(last & FLAG_NEG), bool(last & FLAG_INF)


def g1_decompress(b):
    """-> (status, point or None)"""
    assert len(b) == 32
    neg, inf = _flags(b[31])
    x = int.from_bytes(b, "little") & ((1 << 254) - 1)
    if (neg and inf) or x >= P or (inf and x):
        return MALFORMED, None
    if inf:
        return OK, None
    y = fq_sqrt(x * x * x + py.B1)
    if y is None:
        return NOT_ON_CURVE, None
    if fq_is_neg(y) != neg:
        y = -y % P
    return OK, (x, y)


def g2_decompress(b, check_subgroup=True):
    assert len(b) == 64
    neg, inf = _flags(b[63])
    c0 = int.from_bytes(b[:32], "little")
    c1 = int.from_bytes(b[32:], "little") & ((1 << 254) - 1)
    if (neg and inf) or c0 >= P or c1 >= P or (inf and (c0 or c1)):
        return MALFORMED, None
    if inf:
        return OK, None
    x = (c0, c1)
    y = f2_sqrt(py.f2_add(py.f2_mul(py.f2_sqr(x), x), py.B2))
    if y is None:
        return NOT_ON_CURVE, None
    if f2_is_neg(y) != neg:
        y = py.f2_neg(y)
    if check_subgroup and not in_subgroup_fast((x, y)):
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


# ---- subgroup membership ----------------------------------------------------------------------------------------------------------------------
def mul_unreduced(pt, k):
    """[k]pt on the twist by double-and-add with the scalar AS GIVEN (no reduction mod r)"""
    acc = None
    while k:
        if k & 1:
            acc = py.g2_add(acc, pt)
        pt = py.g2_add(pt, pt)
        k >>= 1
    return acc


def psi(q):
    """untwist-Frobenius-twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)); psi(O) = O"""
    if q is None:
        return None
    return (py.f2_mul(py.f2_conj(q[0]), py.TWIST_MUL_BY_Q_X), py.f2_mul(py.f2_conj(q[1]), py.TWIST_MUL_BY_Q_Y))


def in_subgroup_def(q):
    return mul_unreduced(q, R) is None


def in_subgroup_fast(q):
    return q is None or psi(q) == mul_unreduced(q, SIX_Z2)


def ladder_events(q):
    """What the device ladder meets on Q: (accumulator became O, additions with equal operands, additions with opposite operands)"""
    acc, went_inf, equal, opposite = None, 0, 0, 0
    for i in range(SIX_Z2.bit_length() - 1, -1, -1):
        acc = py.g2_add(acc, acc)
        if (SIX_Z2 >> i) & 1:
            if acc is not None and acc[0] == q[0]:
                if acc[1] == q[1]: equal += 1
                else: opposite += 1
            acc = py.g2_add(acc, q)
            if acc is None: went_inf += 1
    return went_inf, equal, opposite


def twist_point_from_x(x, neg=False):
    """the twist point with this x and the y of that sign, or None when x^3 + b has no root"""
    y = f2_sqrt(py.f2_add(py.f2_mul(py.f2_sqr(x), x), py.B2))
    if y is None:
        return None
    return (x, py.f2_neg(y) if f2_is_neg(y) != neg else y)


def random_twist_points(count, seed):
    """`count` points of the twist from random x (a random twist point lies outside G2 except with probability 1/(2p - r))"""
    import random
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        q = twist_point_from_x((rnd.randrange(P), rnd.randrange(P)), bool(rnd.getrandbits(1)))
        if q is not None:
            out.append(q)
    return out


def g2_points_with_real_y(count, seed):
    """points of G2 whose y has c1 = 0, so that y and -y differ in c0 only: x^3 + b in Fq and a residue there. x = (x0, x1) with
    Im(x^3) = 3 x0^2 x1 - x1^3 = -Im(b), i.e. for a chosen x1 != 0: x0^2 = (x1^3 - Im(b)) / (3 x1). Cleared into G2 by the cofactor: the
    multiple of a point with real y need not have one, so these are TWIST points outside G2 unless returned through `cleared`."""
    import random
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        x1 = rnd.randrange(1, P)
        x0 = fq_sqrt((x1 ** 3 - py.B2[1]) * pow(3 * x1, P - 2, P))
        if x0 is None:
            continue
        x = (x0, x1)
        rhs = py.f2_add(py.f2_mul(py.f2_sqr(x), x), py.B2)
        assert rhs[1] == 0
        y0 = fq_sqrt(rhs[0])
        if y0 is None:
            continue
        out.append((x, (y0 if rnd.getrandbits(1) else -y0 % P, 0)))
    return out


# ---- the ABI's limb layout --------------------------------------------------------------------------------------------------------------------
def fq_words(x):
    return py.to_mont_limbs(x % P, P)


def g1_words(pt):
    """u64[8] Montgomery limbs, (0, 0) = identity"""
    return [0] * 8 if pt is None else fq_words(pt[0]) + fq_words(pt[1])


def g2_words(pt):
    return [0] * 16 if pt is None else fq_words(pt[0][0]) + fq_words(pt[0][1]) + fq_words(pt[1][0]) + fq_words(pt[1][1])


def g1_from_words(w):
    w = [int(v) for v in w]
    if not any(w):
        return None
    return (py.from_mont_limbs(w[:4], P), py.from_mont_limbs(w[4:], P))


def g2_from_words(w):
    w = [int(v) for v in w]
    if not any(w):
        return None
    f = lambda i: py.from_mont_limbs(w[4 * i:4 * i + 4], P)
    return ((f(0), f(1)), (f(2), f(3)))


# ---- the recorded vectors (tests/golden/point_codec_vectors.json) -----------------------------------------------------------------------------
def golden_vectors():
    """generated, never edited by hand: `python tests/point_codec_model.py > tests/golden/point_codec_vectors.json`"""
    g1 = [None, py.G1_GEN, py.g1_neg(py.G1_GEN)] + [py.g1_mul(py.G1_GEN, k) for k in (2, 3, 0xDEADBEEF, R - 2)]
    g2 = [None, py.G2_GEN, py.g2_neg(py.G2_GEN)] + [py.g2_mul(py.G2_GEN, k) for k in (2, 3, 0xDEADBEEF, R - 2)]
    outside = random_twist_points(4, 77)
    return {
        "g1": [{"words": ["%016x" % v for v in g1_words(p)], "bytes": g1_compress(p).hex()} for p in g1],
        "g2": [{"words": ["%016x" % v for v in g2_words(p)], "bytes": g2_compress(p).hex(), "in_subgroup": True} for p in g2]
              + [{"words": ["%016x" % v for v in g2_words(p)], "bytes": g2_compress(p).hex(), "in_subgroup": False} for p in outside],
    }


if __name__ == "__main__":
    import json
    print(json.dumps(golden_vectors(), indent=1))
