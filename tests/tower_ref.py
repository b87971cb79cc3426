"""Big-integer reference and operand families for the tower probe (keaki_hip_selftest_tower_ops, keaki_amd/csrc/tower_probe.hip and
tower_probe_wide.hip).

The host chooses the operands, the device runs ONE shipped function of the Fq12 tower per record -- in the lane-pair form of pair261.hip.h /
pairing.hip.h or in the twelve-lane form of pairing_wide.hip.h -- and returns all twelve Fq words; the functions here say what those words
must be, in Python integers on oracle/bn254_py.py, so every comparison is exact. tests/test_tower_ref_model.py checks this file against itself
on the CPU; tests/test_gpu_tower_ops.py runs the device.

A record is a dict of the areas its op reads (include/keaki_hip.h): "a", "b": 12 STORED residues (value x 2^261 mod p, below p) in the tower's
memory order c0.c0.c0 ... c1.c2.c1; "line": the six integers c0.c0, c0.c1, d0.c0, d0.c1, d1.c0, d1.c1 that travel as exact 29-bit limbs (c0, d0
below 2p, d1 below p); "t": 6 stored residues (X, Y, Z of the running point, or the three line coefficients of `ell`); "q": 4 stored residues;
"p": P.x, P.y as integers below p that travel as exact limbs. The families are chosen on the STORED values: the lazy sums inside the products are
bounded by what the words hold (p - 1 in every position is their worst case), not by what they stand for.
"""
import os
import random
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bn254_py as py  # noqa: E402
from field_ref import l29, w32  # noqa: E402

P, RFR = py.P, py.R
R261 = 1 << 261
R261I = pow(R261, -1, P)
REC_WORDS, OUT_FQ = 344, 12
OFF = {"a": 0, "b": 96, "line": 192, "t": 246, "q": 294, "p": 326}
# area -> (how many integers, words per integer, bound of each integer (exclusive), where the bound is stated)
AREAS = {
    "a": (12, 8, [P] * 12, "pair261.hip.h:38 'canonical (< p), 2^261-form'"),
    "b": (12, 8, [P] * 12, "pair261.hip.h:38"),
    "line": (6, 9, [2 * P] * 4 + [P] * 2, "pair261.hip.h:510-511 / pairing_wide.hip.h:111 'c0, d0 exact and < 2p, d1 exact and < p'"),
    "t": (6, 8, [P] * 6, "pair261.hip.h:38 (G2Hom / Line of pairing.hip.h:27-28 are Fq2d)"),
    "q": (4, 8, [P] * 4, "pair261.hip.h:38"),
    "p": (2, 9, [P] * 2, "pairing.hip.h:113 'cut(unpark_fq(park, 6))': exact limbs of a canonical residue"),
}


def enc(x):
    return x * R261 % P


def dec(x):
    return x * R261I % P


# ---- Fq12 <-> the twelve stored residues; flat <-> tower ------------------------------------------------------------------------------
def f12_of(st):
    c = [(dec(st[2 * m]), dec(st[2 * m + 1])) for m in range(6)]
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


def stored(f):
    return [enc(x) for f6 in f for f2 in f6 for x in f2]


def tower_pos(k):
    """Fq2 position in the tower's memory order of the flat coefficient of w^k (k = 2 j + e for c_e.c_j)"""
    return (k & 1) * 3 + (k >> 1)


def flat_pos(m):
    """the power of w that the Fq2 at memory position m = 3 e + j multiplies"""
    return 2 * (m % 3) + m // 3


def to_flat(f):
    c = [f[m // 3][m % 3] for m in range(6)]
    return [c[tower_pos(k)] for k in range(6)]


def from_flat(a):
    c = [a[flat_pos(m)] for m in range(6)]
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


F2 = py.F2_ZERO
F12_ZERO = (py.F6_ZERO, py.F6_ZERO)
F12_MINUS_ONE = ((((P - 1), 0), F2, F2), py.F6_ZERO)


def is_zero12(f):
    return all(x == 0 for f6 in f for f2 in f6 for x in f2)


def f12_inv0(f):
    """the library's convention: the inverse of 0 is 0 (fq_inv261(0) = 0 runs through fq2_inv, fq6_inv and fq12_inv)"""
    return F12_ZERO if is_zero12(f) else py.f12_inv(f)


def f6_inv0(a):
    return py.F6_ZERO if all(x == 0 for f2 in a for x in f2) else py.f6_inv(a)


# ---- Granger-Scott squaring, restated from pairing_wide.hip.h:144-146 (flat basis) ---------------------------------------------------
def gs_sqr(f):
    """(x, y) = (a0, a3), (a1, a4), (a2, a5); t_e = x^2 + xi y^2, t_o = 2 x y; 3 t - 2 a on the even powers of w, 3 t + 2 a on the odd ones,
    with xi on pair 1. Total; equal to the square on the cyclotomic subgroup only."""
    a = to_flat(f)
    add, sub, mul, xi = py.f2_add, py.f2_sub, py.f2_mul, py.f2_mul_xi

    def te(x, y): return add(mul(x, x), xi(mul(y, y)))
    def to(x, y): return py.f2_dbl(mul(x, y))
    def m3(t): return add(py.f2_dbl(t), t)
    o = [None] * 6
    o[0] = sub(m3(te(a[0], a[3])), py.f2_dbl(a[0]))
    o[3] = add(m3(to(a[0], a[3])), py.f2_dbl(a[3]))
    o[2] = sub(m3(te(a[1], a[4])), py.f2_dbl(a[2]))
    o[5] = add(m3(to(a[1], a[4])), py.f2_dbl(a[5]))
    o[4] = sub(m3(te(a[2], a[5])), py.f2_dbl(a[4]))
    o[1] = add(m3(xi(to(a[2], a[5]))), py.f2_dbl(a[1]))
    return from_flat(o)


# ---- the sparse product term by term (the model test holds py.f12_mul_by_034 against both) -------------------------------------------
def mul_by_034_tower_terms(f, c0, d0, d1):
    """pair261.hip.h:507-508"""
    (a0, a1, a2), (e0, e1, e2) = f
    add, mul, xi = py.f2_add, py.f2_mul, py.f2_mul_xi
    s3 = lambda x, y, z: add(add(x, y), z)
    r0 = (s3(mul(a0, c0), mul(e1, xi(d1)), mul(e2, xi(d0))), s3(mul(a1, c0), mul(e0, d0), mul(e2, xi(d1))), s3(mul(a2, c0), mul(e0, d1), mul(e1, d0)))
    r1 = (s3(mul(e0, c0), mul(a0, d0), mul(a2, xi(d1))), s3(mul(e1, c0), mul(a0, d1), mul(a1, d0)), s3(mul(e2, c0), mul(a1, d1), mul(a2, d0)))
    return (r0, r1)


def mul_by_034_flat_terms(f, c0, d0, d1):
    """pairing_wide.hip.h:110: c_k = a_k c0 + a_(k-1) d0 + a_(k-3) d1, indices mod 6, xi where they wrap (d0: k = 0; d1: k < 3)"""
    a = to_flat(f)
    add, mul, xi = py.f2_add, py.f2_mul, py.f2_mul_xi
    out = []
    for k in range(6):
        t = mul(a[k], c0)
        t = add(t, mul(a[(k - 1) % 6], d0 if k >= 1 else xi(d0)))
        t = add(t, mul(a[(k - 3) % 6], d1 if k >= 3 else xi(d1)))
        out.append(t)
    return from_flat(out)


# ---- references: record -> twelve stored residues --------------------------------------------------------------------------------------
def _line(rec):
    v = [dec(x) for x in rec["line"]]
    return (v[0], v[1]), (v[2], v[3]), (v[4], v[5])


def _f2s(st):
    return [(dec(st[2 * i]), dec(st[2 * i + 1])) for i in range(len(st) // 2)]


def _six(*f2s):
    return [enc(x) for f2 in f2s for x in f2]


def _ref_line_double(rec):
    t, l = py._line_double(tuple(_f2s(rec["t"])))
    return _six(*t, *l)


def _ref_line_add(rec):
    t, l = py._line_add(tuple(_f2s(rec["t"])), tuple(_f2s(rec["q"])))
    return _six(*t, *l)


def _ref_ell(rec):
    px, py_ = (dec(x) for x in rec["p"])
    return stored(py._ell(f12_of(rec["a"]), tuple(_f2s(rec["t"])), (px, py_)))


_MUL = lambda r: stored(py.f12_mul(f12_of(r["a"]), f12_of(r["b"])))
_INV = lambda r: stored(f12_inv0(f12_of(r["a"])))
_CYC = lambda r: stored(gs_sqr(f12_of(r["a"])))
_034 = lambda r: stored(py.f12_mul_by_034(f12_of(r["a"]), *_line(r)))
_CONJ = lambda r: stored(py.f12_conj(f12_of(r["a"])))


def _frob(k):
    return lambda r: stored(py.f12_frob(f12_of(r["a"]), k))


REF = {
    "FQ12_MUL": _MUL, "FQ12_MUL_LD": _MUL, "W12_MUL": _MUL,
    "FQ12_SQR": lambda r: stored(py.f12_sqr(f12_of(r["a"]))),
    "FQ12_INV": _INV, "FQ12_INV_PARKED": _INV, "W12_INV": _INV,
    "FQ12_CONJ": _CONJ, "W12_CONJ": _CONJ,
    "FQ12_CYC_SQR": _CYC, "W12_CYC_SQR": _CYC,
    "FQ12_MUL_BY_034": _034, "W12_MUL_034": _034,
    "ELL": _ref_ell,
    "FQ6_INV": lambda r: [enc(x) for f2 in f6_inv0(f12_of(r["a"])[0]) for x in f2] + [0] * 6,
    "LINE_DOUBLE": _ref_line_double, "W_LINE_DOUBLE": _ref_line_double,
    "LINE_ADD": _ref_line_add, "W_LINE_ADD": _ref_line_add,
    "W12_GATHER_OWN": lambda r: list(r["a"]),
}
for _k in (1, 2, 3):
    REF["FQ12_FROB%d" % _k] = REF["FQ12_FROB_PARKED%d" % _k] = REF["W12_FROB%d" % _k] = _frob(_k)

# the areas an op reads
USES = {n: ("a",) for n in REF}
for _n in ("FQ12_MUL", "FQ12_MUL_LD", "W12_MUL"):
    USES[_n] = ("a", "b")
for _n in ("FQ12_MUL_BY_034", "W12_MUL_034"):
    USES[_n] = ("a", "line")
USES["ELL"] = ("a", "t", "p")
for _n in ("LINE_DOUBLE", "W_LINE_DOUBLE"):
    USES[_n] = ("t",)
for _n in ("LINE_ADD", "W_LINE_ADD"):
    USES[_n] = ("t", "q")


def in_bounds(name, rec):
    """every integer of every area the op reads lies below the bound its callee states"""
    return all(len(rec[k]) == AREAS[k][0] and all(0 <= x < b for x, b in zip(rec[k], AREAS[k][2])) for k in USES[name])


# ---- operand families ------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return random.Random(0x746f7772 ^ zlib.crc32(name.encode()))


def dense(rng):
    return [rng.randrange(P) for _ in range(12)]


def unit(i, v=None):
    e = [0] * 12
    e[i] = enc(1) if v is None else v
    return e


def structured(with_zero=True):
    """(tag, twelve stored residues): zero, one, -1, the twelve unit vectors, every word p - 1, (p - 1) / 2, (p + 1) / 2"""
    out = [("zero", [0] * 12)] if with_zero else []
    out += [("one", stored(py.F12_ONE)), ("-1", stored(F12_MINUS_ONE))]
    out += [("unit%d" % i, unit(i)) for i in range(12)]
    out += [("all p-1", [P - 1] * 12), ("all (p-1)/2", [(P - 1) // 2] * 12), ("all (p+1)/2", [(P + 1) // 2] * 12)]
    return out


def subfields(rng):
    """elements of Fq, Fq2, Fq6 (c1 = 0) and of the pure-w part (c0 = 0)"""
    d = dense(rng)
    return [("in Fq", d[:1] + [0] * 11), ("in Fq2", d[:2] + [0] * 10), ("in Fq6", d[:6] + [0] * 6), ("pure w", [0] * 6 + d[6:])]


def sparse(rng):
    m = rng.randrange(1, 1 << 12)
    if rng.random() < 0.5:
        m &= rng.randrange(1, 1 << 12)
    return [rng.randrange(P) if (m >> i) & 1 else 0 for i in range(12)]


_CACHE = {}


def gt_generator():
    """e(G1, G2)"""
    if "gt" not in _CACHE:
        _CACHE["gt"] = py.pairing(py.G1_GEN, py.G2_GEN)
    return _CACHE["gt"]


def unitary_of(f):
    """f^((p^6 - 1)(p^2 + 1)): the easy part of the final exponentiation lands in the cyclotomic subgroup (order p^4 - p^2 + 1)"""
    g = py.f12_mul(py.f12_conj(f), py.f12_inv(f))
    return py.f12_mul(py.f12_frob(g, 2), g)


def gen_binary(name):
    rng, out = _rng(name), []
    allmax = [P - 1] * 12
    for tag, s in structured():
        out += [("structured:%s x dense" % tag, s, dense(rng)), ("structured:dense x %s" % tag, dense(rng), s), ("structured:%s squared" % tag, s, list(s)),
                ("structured:%s x all p-1" % tag, s, allmax), ("structured:all p-1 x %s" % tag, allmax, s)]
    for i in range(12):          # single terms of the schoolbook sum: w^i times w^j, every wrap of every pair
        for j in range(12):
            out.append(("unit%d x unit%d" % (i, j), unit(i, P - 1), unit(j, P - 1)))
    subs = subfields(rng)
    for ta, a in subs:
        out += [("subfield:%s x dense" % ta, a, dense(rng)), ("subfield:dense x %s" % ta, dense(rng), a)]
        out += [("subfield:%s x %s" % (ta, tb), a, b) for tb, b in subfields(rng)]
    for _ in range(16):
        out += [("sparse x dense", sparse(rng), dense(rng)), ("dense x sparse", dense(rng), sparse(rng)), ("sparse x sparse", sparse(rng), sparse(rng))]
    for _ in range(8):
        a = dense(rng)
        f = f12_of(a)
        out += [("related:b=a", a, list(a)), ("related:b=conj(a)", a, stored(py.f12_conj(f))), ("related:b=1/a", a, stored(py.f12_inv(f)))]
    out += [("random", dense(rng), dense(rng)) for _ in range(256)]
    return [(t, {"a": a, "b": b}) for t, a, b in out]


def gen_unary(name):
    rng = _rng(name)
    out = [("structured:" + t, s) for t, s in structured()]
    out += [("unit%d=p-1" % i, unit(i, P - 1)) for i in range(12)]
    for _ in range(4):
        out += [("subfield:" + t, s) for t, s in subfields(rng)]
    out += [("sparse", sparse(rng)) for _ in range(32)]
    out += [("random", dense(rng)) for _ in range(256)]
    return [(t, {"a": a}) for t, a in out]


def gen_inverse(name):
    rng = _rng(name)
    d = dense(rng)
    out = [("0", [0] * 12), ("one", stored(py.F12_ONE)), ("c1=0", d[:6] + [0] * 6), ("c0=0", [0] * 6 + d[6:]), ("in Fq", d[:1] + [0] * 11), ("all p-1", [P - 1] * 12)]
    out += [("structured:" + t, s) for t, s in structured(False)]
    out += [("sparse", sparse(rng)) for _ in range(16)]
    out += [("random", dense(rng)) for _ in range(256)]
    if name == "FQ6_INV":          # the op reads c0 alone: the same classes inside Fq6
        out += [("f6:c0 only", d[:2] + [0] * 10), ("f6:c1 only", [0, 0] + d[2:4] + [0] * 8), ("f6:c2 only", [0] * 4 + d[4:6] + [0] * 6), ("f6:all p-1, c1 ignored", [P - 1] * 6 + d[6:])]
    return [(t, {"a": a}) for t, a in out]


def gen_cyclotomic(name):
    """-> families; the tag says whether the record lies in the cyclotomic subgroup, where the formula is the square (the model test checks both
    kinds against py.f12_sqr)"""
    rng = _rng(name)
    gt = gt_generator()
    out = [("cyclotomic:one", stored(py.F12_ONE)), ("cyclotomic:e(G1,G2)", stored(gt)), ("cyclotomic:conj e(G1,G2)", stored(py.f12_conj(gt)))]
    out += [("cyclotomic:easy part of random", stored(unitary_of(f12_of(dense(rng))))) for _ in range(128)]
    # -1 is unitary (a conj(a) = 1) but NOT in the cyclotomic subgroup (its order 2 does not divide the odd p^4 - p^2 + 1): the formula gives 5 there
    out += [("general:" + t, s) for t, s in structured()]
    out += [("general:unit%d=p-1" % i, unit(i, P - 1)) for i in range(12)]
    out += [("general:" + t, s) for t, s in subfields(rng)]
    out += [("general:sparse", sparse(rng)) for _ in range(32)]
    out += [("general:random", dense(rng)) for _ in range(192)]
    return [(t, {"a": a}) for t, a in out]


LINE_EDGES = [("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2p-1", 2 * P - 1)]
D1_EDGES = [("0", 0), ("1", 1), ("p-1", P - 1)]


def gen_sparse_product(name):
    rng, out = _rng(name), []
    fs = [("dense", None), ("all p-1", [P - 1] * 12)] + [("unit%d" % i, unit(i)) for i in range(12)] + [("unit%d=p-1" % i, unit(i, P - 1)) for i in range(12)]

    def f_of(v):
        return dense(rng) if v is None else list(v)
    n = 0
    for tf, f in fs:
        for tv, v in LINE_EDGES:          # c0 = d0 = (v, v), d1 walking through its own edges
            td, d = D1_EDGES[n % 3]
            n += 1
            out.append(("edge:f %s, c0=d0=(%s,%s), d1=%s" % (tf, tv, tv, td), f_of(f), [v, v, v, v, d, d]))
        for tag, lo, hi in (("(0,2p-1)", 0, 2 * P - 1), ("(2p-1,0)", 2 * P - 1, 0)):          # one component 0, the other at the bound
            out.append(("mixed:f %s, c0=d0=%s, d1=p-1" % (tf, tag), f_of(f), [lo, hi, lo, hi, P - 1, P - 1]))
            out.append(("mixed:f %s, c0=%s, d0 swapped, d1=(p-1,0)" % (tf, tag), f_of(f), [lo, hi, hi, lo, P - 1, 0]))
    for tv, v in LINE_EDGES:          # every pairing of the edges between the two components, f at its bound
        for tw, w in LINE_EDGES:
            out.append(("grid:f all p-1, c0=(%s,%s), d0=(%s,%s), d1=p-1" % (tv, tw, tw, tv), [P - 1] * 12, [v, w, w, v, P - 1, P - 1]))
    for td, d in D1_EDGES:          # the line's terms one at a time
        out.append(("single:c0 only", dense(rng), [2 * P - 1, 2 * P - 1, 0, 0, 0, 0]))
        out.append(("single:d0 only", dense(rng), [0, 0, 2 * P - 1, 2 * P - 1, 0, 0]))
        out.append(("single:d1=%s only" % td, dense(rng), [0, 0, 0, 0, d, d]))
    out.append(("zero line", dense(rng), [0] * 6))
    out.append(("zero f", [0] * 12, [2 * P - 1] * 4 + [P - 1] * 2))
    for _ in range(256):
        out.append(("random", dense(rng), [rng.randrange(2 * P) for _ in range(4)] + [rng.randrange(P) for _ in range(2)]))
    return [(t, {"a": a, "line": l}) for t, a, l in out]


def g2_points(rng):
    """(tag, affine Q = k G2 as two Fq2) for k = 1, 2, r - 1 and seeded random scalars"""
    if "g2" not in _CACHE:
        _CACHE["g2"] = {k: py.g2_mul(py.G2_GEN, k) for k in (1, 2, RFR - 1)}
    pts = [("G2", _CACHE["g2"][1]), ("2 G2", _CACHE["g2"][2]), ("(r-1) G2", _CACHE["g2"][RFR - 1])]
    pts += [("k G2", py.g2_mul(py.G2_GEN, rng.randrange(1, RFR))) for _ in range(3)]
    return pts


def _scaled(q, z):
    """the homogeneous projective point (x z, y z, z)"""
    return (py.f2_mul(q[0], z), py.f2_mul(q[1], z), z)


def gen_line(name):
    rng, out = _rng(name), []
    add = name.endswith("LINE_ADD")
    pts = g2_points(rng)

    def rec(t, q=None):
        r = {"t": _six(*t)}
        if add:
            r["q"] = _six(*(q if q is not None else pts[rng.randrange(len(pts))][1]))
        return r
    for i, (tag, q) in enumerate(pts):
        other = pts[(i + 1) % len(pts)][1]
        z = (rng.randrange(1, P), rng.randrange(P))
        out.append(("point:T=(%s, 1)" % tag, rec((q[0], q[1], py.F2_ONE), other)))
        out.append(("point:T=%s, random Z" % tag, rec(_scaled(q, z), other)))
        if add:
            out.append(("point:Q = T = %s" % tag, rec((q[0], q[1], py.F2_ONE), q)))
            out.append(("point:Q = T = %s, random Z" % tag, rec(_scaled(q, z), q)))
            out.append(("point:Q = -T = -%s" % tag, rec((q[0], q[1], py.F2_ONE), py.g2_neg(q))))
            out.append(("point:Q = -T = -%s, random Z" % tag, rec(_scaled(q, z), py.g2_neg(q))))
    zero3, zero2 = (F2, F2, F2), (F2, F2)
    out.append(("identity:T = 0", rec(zero3, pts[0][1])))
    if add:
        out.append(("identity:Q = 0", rec((pts[0][1][0], pts[0][1][1], py.F2_ONE), zero2)))
        out.append(("identity:T = 0 and Q = 0", rec(zero3, zero2)))
    # stored words at their bound, whatever they stand for
    top = {"t": [P - 1] * 6}
    if add:
        top["q"] = [P - 1] * 4
    out.append(("bound:every coordinate p-1", top))
    for v_tag, v in (("1", 1), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2)):
        r = {"t": [v] * 6}
        if add:
            r["q"] = [v] * 4
        out.append(("bound:every coordinate %s" % v_tag, r))
    for _ in range(256):
        r = {"t": [rng.randrange(P) for _ in range(6)]}
        if add:
            r["q"] = [rng.randrange(P) for _ in range(4)]
        out.append(("random", r))
    return out


def gen_ell(name):
    rng, out = _rng(name), []
    words = [("0", 0), ("1", 1), ("one", enc(1)), ("p-1", P - 1)]
    g1 = py.g1_mul(py.G1_GEN, rng.randrange(1, RFR))
    for tf, f in (("dense", None), ("all p-1", [P - 1] * 12), ("one", stored(py.F12_ONE)), ("zero", [0] * 12)):
        for tl, l in words:
            for tp, pc in words:
                out.append(("edge:f %s, line words %s, P words %s" % (tf, tl, tp), {"a": dense(rng) if f is None else list(f), "t": [l] * 6, "p": [pc, pc]}))
    for i in range(12):
        out.append(("unit%d, line p-1, P p-1" % i, {"a": unit(i, P - 1), "t": [P - 1] * 6, "p": [P - 1, P - 1]}))
    q = py.g2_mul(py.G2_GEN, rng.randrange(1, RFR))
    _, l = py._line_double((q[0], q[1], py.F2_ONE))
    out.append(("point:a doubling line at a G1 point", {"a": dense(rng), "t": _six(*l), "p": [enc(g1[0]), enc(g1[1])]}))
    out.append(("identity:P = 0", {"a": dense(rng), "t": _six(*l), "p": [0, 0]}))
    out.append(("identity:line = 0", {"a": dense(rng), "t": [0] * 6, "p": [enc(g1[0]), enc(g1[1])]}))
    for _ in range(256):
        out.append(("random", {"a": dense(rng), "t": [rng.randrange(P) for _ in range(6)], "p": [rng.randrange(P), rng.randrange(P)]}))
    return out


def generate(name):
    """-> (tags, records), in the order the device gets them"""
    if name in ("FQ12_MUL", "FQ12_MUL_LD", "W12_MUL"):
        fam = gen_binary(name)
    elif name in ("FQ12_INV", "FQ12_INV_PARKED", "W12_INV", "FQ6_INV"):
        fam = gen_inverse(name)
    elif name.endswith("CYC_SQR"):
        fam = gen_cyclotomic(name)
    elif name in ("FQ12_MUL_BY_034", "W12_MUL_034"):
        fam = gen_sparse_product(name)
    elif name == "ELL":
        fam = gen_ell(name)
    elif "LINE_" in name:
        fam = gen_line(name)
    else:
        fam = gen_unary(name)
    return [t for t, _ in fam], [r for _, r in fam]


def expected(name, recs):
    """the twelve result Fq of every record as 8 words each: list of 12 x 8"""
    return [[w32(x) for x in REF[name](r)] for r in recs]


def pack_records(recs):
    """records -> the n x 344 uint32 array of keaki_hip_selftest_tower_ops"""
    import numpy as np
    a = np.zeros((len(recs), REC_WORDS), np.uint32)
    for i, r in enumerate(recs):
        for k, vals in r.items():
            _, words, _, _ = AREAS[k]
            for j, v in enumerate(vals):
                a[i, OFF[k] + words * j:OFF[k] + words * (j + 1)] = l29(v) if words == 9 else w32(v)
    return a
