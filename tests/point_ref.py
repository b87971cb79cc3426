"""Big-integer reference, bounds table and operand families for the point probe (keaki_hip_selftest_point_ops, keaki_amd/csrc/point_probe.hip and
point_probe_g2.hip).

The host chooses every limb, the device runs ONE shipped function of the lazy-limb group law per record, and the functions here say what the
result must be -- in plain Python integers. A lazy result is not unique (any representative of the right residue inside the documented bound
is right), so the verdict is a predicate, not an array: `judge(name, rec, out)` returns the list of what is wrong with one record's output

  * the affine image of the device's point (X/ZZ, Y/ZZZ or X/Z^2, Y/Z^3, Montgomery factor removed) must equal the chord-and-tangent sum of the
    affine images of the operands on y^2 = x^3 + b (a = 0; the formulas never read b, so operands need not lie on the curve: any residue in
    any coordinate, only ZZ^3 = ZZZ^2 must hold for XYZZ), flags / `special` / return values must equal the reference's, *ratio == Z3 / Z1;
  * every limb 0..7 is at most 2^29 + 8, every value is below the bound its header states (BOUNDS: file, line and the words on that line),
    stored results are canonical;
  * tables: entry m (or 2i + 1) is m P as an affine point of the curve isomorphic by zfix, xb == beta x, a pair's tables share one curve;
  * GLV: bit-exact with the header's definition on integers, and the contract itself (recombination mod r, magnitudes < 2^127, digit ranges,
    reconstruction, the byte encoding);
  * ladders: (k log) mod r times G, the bool false exactly for the identity.

tests/test_point_ref_model.py checks this file against itself and against the limb-exact models on the CPU; tests/test_gpu_point_ops.py runs
the device. Constants come from keaki_amd/csrc/gen_constants.py through field_ref (the text it prints).

Tightened bounds. A coordinate that is subtracted against a biased multiple K = m p cannot go all the way to m p: the field probe showed that
the subtrahend must stay 2^233 (6e-7 p) below K (field_ref.SUB_SLACK), or limb 8 of the difference underflows. Where a header states `<= 4 p`
or `< 4 (X < 2)` for such a coordinate (j29_madd's Y1, the G2 mixed addition's accumulator) the families stop 2^233 short: rows `*.tight`
of BOUNDS, each with the argument why no shipped call site comes near. The hashed sources are left alone, as field_ref does.
"""
import os
import random
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402

ROOT = fr.ROOT
P, RFR = fr.P, fr.RFR
R256, R261 = fr.R256, fr.R261
R256I, R261I = pow(R256, -1, P), pow(R261, -1, P)
L29_8, SLACK = fr.L29_8, fr.SUB_SLACK
SLOTS, SW, FLAG_SLOT, OUT_SLOTS, OUT_FLAG_SLOT, MAX_RECORDS = 17, 9, 16, 50, 49, 4096
DIG_STRIDE = 132

OPS = ["X29_ADD", "X29_DBL", "X29_STORE", "X29_LOAD_STORE", "J29_DBL", "J29_MADD", "J29_ADDSUB", "J29_SAT_ROUNDTRIP", "J29_BUILD_TABLE",
       "J29_BUILD_TABLE_ODD", "J29_BUILD_PAIR", "GLV_DECOMPOSE", "GLV_FIXED_DIGITS", "GLV_UNIFORM_DIGITS", "LADDER_FIXED", "LADDER_GTAB",
       "LADDER_UNIFORM", "LADDER_MUL2", "XYZZ_ADD_MIXED_FQ", "XYZZ_ADD_FQ", "XYZZ_DBL_FQ", "XYZZ_DBL_AFF_FQ", "JAC_ADD_FQ", "JAC_ADD_MIXED_FQ",
       "JAC_DBL_FQ", "X29G2_ADD_MIXED", "X29G2_ADD", "X29G2_DBL", "X29G2_DBL_OF_ACC", "X29G2_STORE", "XYZZ_ADD_MIXED_FQ2", "XYZZ_ADD_FQ2",
       "XYZZ_DBL_FQ2", "XYZZ_DBL_AFF_FQ2", "JAC_ADD_FQ2", "JAC_ADD_MIXED_FQ2", "JAC_DBL_FQ2"]
UNIFORM_OPS = ("GLV_UNIFORM_DIGITS", "LADDER_UNIFORM", "LADDER_MUL2")          # the wave's first record decides the scalars
LADDER_OPS = ("LADDER_FIXED", "LADDER_GTAB", "LADDER_UNIFORM", "LADDER_MUL2")
ONE_PER_FILE = ("X29_ADD", "J29_MADD", "X29G2_ADD", "XYZZ_ADD_FQ")            # the every-record-its-own-answer test: one op per source file

# ---- the bounds table: key -> (bound as a multiple of p (exclusive), tightening in units of 2^233, file, line, words on that line) ---------
_X, _G, _J, _M = "keaki_amd/csrc/xyzz29.hip.h", "keaki_amd/csrc/xyzz29_g2.hip.h", "keaki_amd/csrc/jac29.hip.h", "keaki_amd/csrc/models/model_jac29.py"
BOUNDS = {
    "x29.in":        (32, 0, _X, 2, "below 32 p"),
    "x29.add.x":     (10.4, 0, _X, 5, "X3 < 10.4"),
    "x29.add.y":     (4.6, 0, _X, 6, "Y3 < 4.6"),
    "x29.add.zz":    (1.1, 0, _X, 6, "ZZ3, ZZZ3 < 1.1"),
    "x29.dbl.x":     (19.7, 0, _X, 7, "X3 < 19.7"),
    "x29.dbl.y":     (9.7, 0, _X, 7, "Y3 < 9.7"),
    "x29.dbl.zz":    (5.8, 0, _X, 7, "ZZ3 < 5.8"),
    "x29.dbl.zzz":   (3, 0, _X, 7, "ZZZ3 < 3"),
    "j29.run.x":     (17.6, 0, _J, 7, "X < 17.6"),
    "j29.run.y":     (3.8, 0, _J, 7, "Y < 3.8"),
    "j29.run.z":     (2.1, 0, _J, 7, "Z < 2.1"),
    "j29.madd.x1":   (19, 0, _J, 173, "X < 19 p"),
    # Y1 is subtracted against K4 (rr = S2 - Y1 + 4p, jac29.hip.h:191): with S2 below 2^232 the literal bound 4p underflows limb 8 (tests/test_point_ref_model.py
    # shows it on the integer model). No call site comes near: a running Y is a dual stream's output (< 3.8 p, jac29.hip.h:7) and a ladder's first
    # point has Y = 4p - y with y a table entry's product output of a point of odd order, i.e. y >= 1 and within 2^233 of 0 with probability 2^-21 per
    # entry AND S2 < 2^232 (2^-22) at the same addition.
    "j29.madd.y1.tight": (4, 1, _J, 173, "Y <= 4 p"),
    "j29.madd.x2":   (9.3, 0, _J, 246, "st.fin(7, run.x, run.y)"),          # a table x: rescaled (< 4.3 p) or, the last entry, a raw j29_madd output (< 9.3 p)
    "j29.madd.y2":   (4, 1, _J, 331, "u29_sub(zero, e.y, Q29::K4)"),          # a table y (< 2 p) or its negation 4p - y: below 4p, and product operands need no more
    "j29.madd.out.x": (9.3, 0, _M, 170, '"madd.x"'),
    "j29.madd.out.y": (1.8, 0, _M, 174, '"madd.y"'),
    "j29.madd.out.z": (1.5, 0, _M, 175, '"madd.z"'),
    # a ladder's result is its running point: Y a dual stream's output (< 3.8 p) or, when the last step was the first addition, a table y or its negation 4p - y
    "j29.ladder.y":  (4, 0, _J, 501, "the negation may become the running point's y (<= 4 p)"),
    "j29.addsub.in": (32, 0, _J, 54, "every coordinate below 32 p"),
    "j29.addsub.x":  (9.2, 0, _M, 146, '"as.x"'),
    "j29.addsub.y":  (1.45, 0, _M, 148, '"as.y"'),
    "j29.addsub.z":  (1.3, 0, _M, 136, '"as.z"'),
    "j29.tab.x":     (4.3, 0, _M, 215, '"tab.x", out[i][0], 4.3'),
    "j29.tab.y":     (2, 0, _M, 215, '"tab.y", out[i][1], 2.0'),
    "j29.pair.x":    (2, 0, _M, 243, '"pair.x"'),
    "j29.pair.y":    (2, 0, _M, 243, '"pair.y"'),
    "j29.product":   (2, 0, _M, 9, "value < (sum of products) / 2^261 + p"),      # zfix, beta x, a ladder's final Z: outputs of one product of values below 34 p and 2 p
    # the G2 mixed addition subtracts acc.x against K2 and acc.y against K4 (xyzz29_g2.hip.h:82) and hands K4 - zz.im, K4 - zzz.im raw to a dual stream
    # (xyzz29_g2.hip.h:109-110, limb 8 must not go negative): 2^233 short of the stated multiples. The accumulator a kernel holds is an output of this
    # function or a table point times `one`: below 1.5 p in every coordinate (xyzz29_g2.hip.h:13).
    "g2.acc.x.tight": (2, 1, _G, 11, "accumulator < 4 (X < 2)"),
    "g2.acc.tight":  (4, 1, _G, 11, "accumulator < 4 (X < 2)"),
    "g2.table":      (32, 0, _G, 12, "table coordinates < 32"),
    "g2.mixed.x":    (1.1, 0, _G, 13, "after < 1.1"),
    "g2.mixed.y":    (1.5, 0, _G, 13, "Y3 < 1.5"),
    "g2.mixed.zz":   (1.1, 0, _G, 13, "ZZ3, ZZZ3 < 1.1"),
    "g2.tail":       (1.2, 0, _G, 116, "< 1.2p"),
    "canon":         (1, 0, "keaki_amd/csrc/bn254_curve.hip.h", 8, "representation-independent"),      # saturated words: canonical residues
}


def bound(key):
    m, t, *_ = BOUNDS[key]
    return int(m * 1000) * P // 1000 - t * SLACK


# ---- fields: an element is a tuple of residues, (a,) in Fq and (a0, a1) in Fq2 -------------------------------------------------------------
def f_add(a, b): return tuple((x + y) % P for x, y in zip(a, b))
def f_sub(a, b): return tuple((x - y) % P for x, y in zip(a, b))
def f_neg(a): return tuple(-x % P for x in a)
def f_is0(a): return not any(a)
def f_int(a, k): return tuple(x * k % P for x in a)


def f_mul(a, b):
    if len(a) == 1:
        return (a[0] * b[0] % P,)
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f_inv(a):
    if len(a) == 1:
        return (pow(a[0], -1, P),)
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f_div(a, b): return f_mul(a, f_inv(b))


def ct_add(p, q):
    """chord and tangent on y^2 = x^3 + b, b never read. None: the identity. A doubling with y == 0 gives the identity (a point of order two)."""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if f_is0(f_add(y1, y2)):
            return None
        lam = f_div(f_int(f_mul(x1, x1), 3), f_int(y1, 2))
    else:
        lam = f_div(f_sub(y2, y1), f_sub(x2, x1))
    x3 = f_sub(f_sub(f_mul(lam, lam), x1), x2)
    return (x3, f_sub(f_mul(lam, f_sub(x1, x3)), y1))


def ct_neg(p): return None if p is None else (p[0], f_neg(p[1]))


def _jmul(k, x, y):
    """k (x, y) over Fq by Jacobian doublings and mixed additions, one inversion at the end (the ladders' reference runs thousands of these)"""
    X, Y, Z = 0, 1, 0
    for bit in bin(k)[2:] if k else "":
        if Z:
            A, B = X * X % P, Y * Y % P
            C = B * B % P
            D = 2 * ((X + B) ** 2 - A - C) % P
            E = 3 * A % P
            X3 = (E * E - 2 * D) % P
            X, Y, Z = X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P
        if bit == "1":
            if not Z:
                X, Y, Z = x, y, 1
            else:
                zz = Z * Z % P
                h, rr = (x * zz - X) % P, (y * Z * zz - Y) % P
                if h == 0:          # the running point meets the base: by the affine rule
                    q = ct_add(((X * pow(zz, -1, P) % P,), (Y * pow(Z * zz, -1, P) % P,)), ((x,), (y,)))
                    X, Y, Z = (q[0][0], q[1][0], 1) if q else (0, 1, 0)
                else:
                    hh = h * h % P
                    hhh, v = h * hh % P, X * hh % P
                    X3 = (rr * rr - hhh - 2 * v) % P
                    X, Y, Z = X3, (rr * (v - X3) - Y * hhh) % P, Z * h % P
    if not Z:
        return None
    zi = pow(Z, -1, P)
    return ((X * zi * zi % P,), (Y * zi * zi * zi % P,))


def ct_mul(k, p):
    if p is not None and len(p[0]) == 1 and p[1][0]:
        return _jmul(k, p[0][0], p[1][0])
    return ct_mul_generic(k, p)


def ct_mul_generic(k, p):
    """double and add by ct_add alone (any field; tests/test_point_ref_model.py ties it, ct_add and _jmul to oracle/bn254_py.py)"""
    r = None
    while k:
        if k & 1:
            r = ct_add(r, p)
        p = ct_add(p, p)
        k >>= 1
    return r


G1 = ((1,), (2,))
_MULG = {}


def mul_g(k):
    """k G on the curve"""
    k %= RFR
    if k not in _MULG:
        _MULG[k] = _jmul(k, 1, 2)
    return _MULG[k]


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def dl(s): return fr.val(s) * R261I % P          # lazy slot -> residue
def ds(s): return fr.wval(s) * R256I % P         # saturated slot -> residue
def lz(res, m=0): return fr.l29(res * R261 % P + m * P)          # residue -> exact limbs of (its 2^261 form + m p)
def sat(res): return fr.w32(res * R256 % P)
def sh5(res): return fr.l29((res * R256 % P) << 5)              # u29_from_sat_shift5 of the saturated word: the loaders' form, 32 v


def record(slots, flags=()):
    r = [[0] * SW for _ in range(SLOTS)]
    for i, s in enumerate(slots):
        r[i][:len(s)] = s
    r[FLAG_SLOT][:len(flags)] = [int(f) for f in flags]
    return r


def pack_records(recs):
    import numpy as np
    return np.array(recs, dtype=np.uint32).reshape(len(recs), SLOTS, SW)


def unpack_records(arr):
    return [[[int(w) for w in s] for s in r] for r in arr.reshape(-1, SLOTS, SW)]


def _rng(name):
    return random.Random(0x706f696e ^ zlib.crc32(name.encode()))


def lazy_below(rng, b):
    """arbitrary limbs of the carried class (0..7 from the edge set, up to 2^29 + 8) with the value within 2^232 below b"""
    return fr.lazy_limbs(rng, L29_8, L29_8, b)


def fel(rng, deg):
    return tuple(rng.randrange(1, P) for _ in range(deg))


# ---- decoding -------------------------------------------------------------------------------------------------------------------------------
def el_lazy(slots, i, deg): return tuple(dl(slots[i + j]) for j in range(deg))
def el_sat(slots, i, deg): return tuple(ds(slots[i + j]) for j in range(deg))


def img_xyzz(c):
    x, y, zz, zzz = c
    return None if f_is0(zz) else (f_div(x, zz), f_div(y, zzz))


def img_jac(c):
    x, y, z = c
    if f_is0(z):
        return None
    zi = f_inv(z)
    zi2 = f_mul(zi, zi)
    return (f_mul(x, zi2), f_mul(y, f_mul(zi, zi2)))


def img_aff(c):
    return None if f_is0(c[0]) and f_is0(c[1]) else (c[0], c[1])


class Verdict:
    def __init__(self, name):
        self.name, self.errors, self.maxima = name, [], {}

    def err(self, msg):
        self.errors.append(msg)

    def lazy(self, coord, limbs, key):
        v = fr.val(limbs)
        self.maxima[coord] = max(self.maxima.get(coord, 0.0), v / P)
        if any(x > L29_8 for x in limbs[:8]):
            self.err("%s: a limb above 2^29 + 8: %s" % (coord, [hex(x) for x in limbs]))
        if not v < bound(key):
            self.err("%s = %.4f p, not below %s (%s:%d)" % (coord, v / P, BOUNDS[key][0], BOUNDS[key][2], BOUNDS[key][3]))

    def canon(self, coord, words):
        if any(words[8:]) or not fr.wval(words) < P:
            self.err("%s: stored words not canonical" % coord)

    def same(self, what, got, want):
        if got != want:
            self.err("%s: device %s, reference %s" % (what, _show(got), _show(want)))


def _show(p):
    if p is None or isinstance(p, (int, bool)):
        return str(p)
    return "(" + ", ".join("%#x" % v for c in p for v in (c if isinstance(c, tuple) else (c,))) + ")"


# ---- judges ---------------------------------------------------------------------------------------------------------------------------------
def _x29_in(rec, s, flag, deg=1):
    c = [el_lazy(rec, s + deg * k, deg) for k in range(4)]
    return None if rec[FLAG_SLOT][flag] else img_xyzz(c)


def _x29_out(v, out, keys, deg=1, want=None):
    names = ("x", "y", "zz", "zzz")
    for k in range(4):
        for j in range(deg):
            v.lazy(names[k] + (".re", ".im")[j] if deg == 2 else names[k], out[deg * k + j], keys[k])
    c = [el_lazy(out, deg * k, deg) for k in range(4)]
    if f_is0(c[2]) or f_is0(c[3]):
        v.err("a finite result with ZZ or ZZZ == 0")
        return
    v.same("affine image", img_xyzz(c), want)


_ADDK = ("x29.add.x", "x29.add.y", "x29.add.zz", "x29.add.zz")
_DBLK = ("x29.dbl.x", "x29.dbl.y", "x29.dbl.zz", "x29.dbl.zzz")
_INK = ("x29.in",) * 4


def judge_x29(v, rec, out):
    a = _x29_in(rec, 0, 0)
    if v.name == "X29_ADD":
        b = _x29_in(rec, 4, 1)
        want = ct_add(a, b)
        passed = rec[4:8] if a is None else rec[0:4] if b is None else None
        keys = _INK if passed else _DBLK if a == b else _ADDK
    elif v.name == "X29_DBL":
        want, passed, keys = ct_add(a, a), (rec[0:4] if a is None else None), _DBLK
    if v.name in ("X29_ADD", "X29_DBL"):
        flag = out[OUT_FLAG_SLOT][0]
        if passed is not None:          # an identity operand: the other operand comes back limb for limb, with its flag
            v.same("passed-through operand", [list(s) for s in out[0:4]], [list(s) for s in passed])
            v.same("inf flag", flag, int(want is None))
            return
        v.same("inf flag", flag, int(want is None))
        if want is not None:
            _x29_out(v, out, keys, want=want)
        return
    # the stores: canonical words, the same point; the identity as xyzz_inf (1, 1, 0, 0)
    if v.name == "X29_LOAD_STORE":
        a = img_xyzz([el_sat(rec, k, 1) for k in range(4)])
    _judge_store(v, out, a, 1)


def _judge_store(v, out, want, deg):
    for k in range(4 * deg):
        v.canon("word slot %d" % k, out[k])
    c = [el_sat(out, deg * k, deg) for k in range(4)]
    one = (1,) + (0,) * (deg - 1)
    if want is None:
        v.same("stored identity", c, [one, one, (0,) * deg, (0,) * deg])
    else:
        v.same("affine image", img_xyzz(c) if not f_is0(c[3]) else None, want)


def _j29_out(v, out, s, keys, want, tag=""):
    for k, n in enumerate("xyz"):
        v.lazy(tag + n, out[s + k], keys[k])
    v.same(tag + "affine image", img_jac([el_lazy(out, s + k, 1) for k in range(3)]), want)


_RUNK = ("j29.run.x", "j29.run.y", "j29.run.z")


def judge_j29(v, rec, out):
    a = img_jac([el_lazy(rec, k, 1) for k in range(3)])
    if v.name == "J29_DBL":
        _j29_out(v, out, 0, _RUNK, ct_add(a, a))
    elif v.name == "J29_MADD":
        b = (el_lazy(rec, 3, 1), el_lazy(rec, 4, 1))
        special = 1 if a == b else 2 if a == ct_neg(b) else 0
        v.same("special", out[OUT_FLAG_SLOT][0], special)
        if special:
            v.same("returned operand", [list(s) for s in out[0:3]], [list(s) for s in rec[0:3]])
            v.same("ratio left alone", out[3], [0] * SW)
        else:
            _j29_out(v, out, 0, ("j29.madd.out.x", "j29.madd.out.y", "j29.madd.out.z"), ct_add(a, b))
            # the result stays in the running point's set (jac29.hip.h:442 'map the running point's bound set into itself')
            _j29_out(v, out, 0, _RUNK, ct_add(a, b), "running set: ")
            v.same("ratio == Z3 / Z1", dl(out[3]) * dl(rec[2]) % P, dl(out[2]))
    elif v.name == "J29_ADDSUB":
        b = img_jac([el_lazy(rec, 3 + k, 1) for k in range(3)])
        ok = not (a[0] == b[0])
        v.same("return value", out[OUT_FLAG_SLOT][0], int(ok))
        if ok:
            keys = ("j29.addsub.x", "j29.addsub.y", "j29.addsub.z")
            _j29_out(v, out, 0, keys, ct_add(a, b), "sum ")
            _j29_out(v, out, 3, keys, ct_add(a, ct_neg(b)), "diff ")
        else:
            v.same("results left alone", [list(s) for s in out[0:6]], [[0] * SW] * 6)
    elif v.name == "J29_SAT_ROUNDTRIP":
        for k in range(3):
            v.canon("word slot %d" % k, out[k])
            v.same("coordinate %d" % k, out[k], rec[k])


BETA = None          # set with the GLV constants below


def _judge_table(v, out, s, base, odd, zfix, keys, tag):
    """entry e at s + 3e: (x, xb, y); (x zfix^2... ) the entry as a point of E: (x / zfix^2, y / zfix^3)"""
    zi = f_inv(zfix)
    zi2, zi3 = f_mul(zi, zi), f_mul(zi, f_mul(zi, zi))
    for e in range(8):
        x, xb, y = (out[s + 3 * e + k] for k in range(3))
        raw = e == 7 and keys[0] != "j29.pair.x"          # the chain's last entry stays as j29_madd left it (jac29.hip.h:246)
        v.lazy("%s[%d].x" % (tag, e), x, "j29.madd.out.x" if raw else keys[0]); v.lazy("%s[%d].xb" % (tag, e), xb, "j29.product")
        v.lazy("%s[%d].y" % (tag, e), y, "j29.madd.out.y" if raw else keys[1])
        m = 2 * e + 1 if odd else e + 1
        v.same("%s entry %d = %d P" % (tag, e, m), (f_mul((dl(x),), zi2), f_mul((dl(y),), zi3)), ct_mul(m, base))
        v.same("%s entry %d: xb == beta x" % (tag, e), dl(xb), BETA * dl(x) % P)


def judge_table(v, rec, out):
    a = img_jac([el_sat(rec, k, 1) for k in range(3)])
    if v.name == "J29_BUILD_PAIR":
        b = img_jac([el_sat(rec, 3 + k, 1) for k in range(3)])
        v.lazy("zfix", out[48], "j29.product")
        z = (dl(out[48]),)
        _judge_table(v, out, 0, a, True, z, ("j29.pair.x", "j29.pair.y"), "TA")
        _judge_table(v, out, 24, b, True, z, ("j29.tab.x", "j29.tab.y"), "TB")
    else:
        v.lazy("zfix", out[24], "j29.product")
        _judge_table(v, out, 0, a, v.name == "J29_BUILD_TABLE_ODD", (dl(out[24]),), ("j29.tab.x", "j29.tab.y"), "T")


# ---- GLV ------------------------------------------------------------------------------------------------------------------------------------
def _words(text, name, n):
    return sum(w << (32 * i) for i, w in enumerate(fr._arr(text, name, n)))


_GLV = fr._struct(fr._TXT, "GlvParams")
GLV_G1, GLV_G2, GLV_A1, GLV_A2, GLV_NB1 = (_words(_GLV, n, k) for n, k in (("G1", 3), ("G2", 5), ("A1", 2), ("A2", 4), ("NB1", 4)))
GLV_B1, GLV_B2 = -GLV_NB1, GLV_A1
LAMBDA = GLV_A1 * pow(GLV_NB1, -1, RFR) % RFR          # a1 + b1 lambda == 0 (mod r)
BETA = fr.val(fr._arr(_GLV, "BETA29", 9)) * R261I % P
assert pow(LAMBDA, 3, RFR) == 1 and LAMBDA != 1 and pow(BETA, 3, P) == 1 and BETA != 1 and (GLV_A2 + GLV_B2 * LAMBDA) % RFR == 0
assert ct_mul(LAMBDA, G1) == (f_int(G1[0], BETA), G1[1])         # phi(x, y) = (beta x, y) = lambda (x, y)


def glv_ref(k):
    """the header's definition on integers (jac29.hip.h:89): signed k1, k2"""
    c1, c2 = (k * GLV_G1) >> 256, (k * GLV_G2) >> 256
    return k - c1 * GLV_A1 - c2 * GLV_A2, -c1 * GLV_B1 - c2 * GLV_B2


def fixed_ref(mag):
    """glv_fixed_digits on integers -> (33 signed digits, packed dig[5], sg[2])"""
    d, car, dig, sg = [], 0, [0] * 5, [0] * 2
    for j in range(33):
        n = ((mag >> (4 * j)) & 15 if j < 32 else 0) + car
        car = int(n > 8)
        d.append(n - 16 if car else n)
        dig[j >> 3] |= abs(d[-1]) << ((j & 7) * 4)
        sg[j >> 5] |= car << (j & 31)          # the sign bit is the carry: also set on a digit 16 - 16 = 0, where the ladders never look
    return d, dig, sg


def wnaf5_ref(mag):
    """width-5 NAF, least significant first, 129 positions"""
    d = []
    for _ in range(129):
        if mag & 1:
            m = mag & 31
            x = m if m < 16 else m - 32
            mag -= x
        else:
            x = 0
        d.append(x)
        mag >>= 1
    assert mag == 0
    return d


def naf_bytes(d):
    return [0 if x == 0 else ((abs(x) + 1) >> 1) | (0x80 if x < 0 else 0) for x in d]


def val32(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def _scalar_of(rec, slot, mont=True):
    k = fr.wval(rec[slot])
    return k * pow(R256, -1, RFR) % RFR if mont else k


def fr_mont(k): return fr.w32(k * R256 % RFR)


def judge_glv(v, rec, out, first=None):
    if v.name == "GLV_DECOMPOSE":
        k = fr.wval(rec[0])
        k1, k2 = glv_ref(k)
        g1, g2 = val32(out[0][:5]), val32(out[1][:5])
        n1, n2 = out[OUT_FLAG_SLOT][0], out[OUT_FLAG_SLOT][1]
        v.same("k1", (g1, n1), (abs(k1), int(k1 < 0)))
        v.same("k2", (g2, n2), (abs(k2), int(k2 < 0)))
        if ((-g1 if n1 else g1) + (-g2 if n2 else g2) * LAMBDA - k) % RFR:
            v.err("+-k1 +- k2 lambda != k (mod r)")
        if g1 >> 127 or g2 >> 127:
            v.err("a magnitude of 2^127 or more")
    elif v.name == "GLV_FIXED_DIGITS":
        mag = val32(rec[0][:5])
        d, dig, sg = fixed_ref(mag)
        v.same("dig", out[0][:5], dig)
        v.same("sg", out[1][:2], sg)
        got = [(-1 if (out[1][j >> 5] >> (j & 31)) & 1 else 1) * ((out[0][j >> 3] >> ((j & 7) * 4)) & 15) for j in range(33)]
        if any(abs(x) > 8 for x in got) or sum(x << (4 * j) for j, x in enumerate(got)) != mag or got[32] not in (0, 1):
            v.err("digits outside [-8, 8] or not the magnitude: %s" % got)
    else:
        k = _scalar_of(first if first is not None else rec, 0)
        k1, k2 = glv_ref(k)
        raw = [(out[w // SW][w % SW] >> (8 * b)) & 0xFF for w in range(2 * DIG_STRIDE // 4) for b in range(4)]
        v.same("signs", (out[OUT_FLAG_SLOT][0], out[OUT_FLAG_SLOT][1]), (int(k1 < 0), int(k2 < 0)))
        for h, mag in enumerate((abs(k1), abs(k2))):
            got = raw[h * DIG_STRIDE:h * DIG_STRIDE + 129]          # bytes 129..131 of a half are never written
            v.same("half %d bytes" % h, got, naf_bytes(wnaf5_ref(mag)))
            dec = [(-1 if b & 0x80 else 1) * (2 * (b & 0x7F) - 1) if b else 0 for b in got]
            nz = [i for i, x in enumerate(dec) if x]
            if any(abs(x) > 15 for x in dec) or any(j - i < 5 for i, j in zip(nz, nz[1:])) or sum(x << i for i, x in enumerate(dec)) != mag:
                v.err("half %d: not a width-5 NAF of the magnitude" % h)


def judge_ladder(v, rec, out, first=None):
    f = first if first is not None else rec
    a = img_jac([el_sat(rec, k, 1) for k in range(3)])
    if v.name == "LADDER_MUL2":
        b = img_jac([el_sat(rec, 3 + k, 1) for k in range(3)])
        kA, kB = _scalar_of(f, 6), _scalar_of(f, 7)
        tb = ct_mul(kB, b)
        want = ct_add(ct_mul(kA, a), ct_neg(tb) if f[FLAG_SLOT][2] else tb)
    else:
        want = ct_mul(_scalar_of(f, 3), a) if a is not None else None
    v.same("return value", out[OUT_FLAG_SLOT][0], int(want is not None))
    if want is not None:
        _j29_out(v, out, 0, ("j29.run.x", "j29.ladder.y", "j29.product"), want)


def judge_sat(v, rec, out):
    deg = 2 if v.name.endswith("FQ2") else 1
    kind = v.name[:-4] if deg == 2 else v.name[:-3]

    def X(s): return img_xyzz([el_sat(rec, s + deg * k, deg) for k in range(4)])
    def J(s): return img_jac([el_sat(rec, s + deg * k, deg) for k in range(3)])
    def A(s): return img_aff([el_sat(rec, s + deg * k, deg) for k in range(2)])
    a = A(0) if kind == "XYZZ_DBL_AFF" else X(0) if kind.startswith("XYZZ") else J(0)
    b = {"XYZZ_ADD_MIXED": lambda: A(4 * deg), "XYZZ_ADD": lambda: X(4 * deg), "JAC_ADD": lambda: J(3 * deg), "JAC_ADD_MIXED": lambda: A(3 * deg)}.get(kind, lambda: a)()
    want = ct_add(a, b)
    n = 4 if kind.startswith("XYZZ") else 3
    for k in range(n * deg):
        v.canon("word slot %d" % k, out[k])
    c = [el_sat(out, deg * k, deg) for k in range(n)]
    v.same("affine image", img_xyzz(c) if n == 4 else img_jac(c), want)


def judge_g2(v, rec, out):
    a = _x29_in(rec, 0, 0, 2)
    if v.name == "X29G2_STORE":
        return _judge_store(v, out, a, 2)
    tail = ("g2.tail",) * 4
    if v.name == "X29G2_ADD_MIXED":
        b = img_aff([el_sat(rec, 8 + 2 * k, 2) for k in range(2)])
        want = ct_add(a, b)
        keys = tail if (a is None or a == b) else ("g2.mixed.x", "g2.mixed.y", "g2.mixed.zz", "g2.mixed.zz")
        if b is None:          # nothing to add: the accumulator as it was
            v.same("accumulator left alone", ([list(s) for s in out[0:8]], out[OUT_FLAG_SLOT][0]), ([list(s) for s in rec[0:8]], rec[FLAG_SLOT][0]))
            return
    elif v.name == "X29G2_ADD":
        b = _x29_in(rec, 8, 1, 2)
        want, keys = ct_add(a, b), tail
        if a is None or b is None:
            v.same("passed-through operand", [list(s) for s in out[0:8]], [list(s) for s in (rec[8:16] if a is None else rec[0:8])])
            v.same("empty flag", out[OUT_FLAG_SLOT][0], int(want is None))
            return
    else:
        want, keys = ct_add(a, a), tail
        if a is None:
            v.same("empty flag", out[OUT_FLAG_SLOT][0], 1)
            return
    v.same("empty flag", out[OUT_FLAG_SLOT][0], int(want is None))
    if want is not None:
        _x29_out(v, out, keys, 2, want)


def judge(name, rec, out, first=None):
    """-> Verdict of one record (rec, out: slot lists). `first`: the wave's first record, for the wave-uniform ops."""
    v = Verdict(name)
    if name.startswith("X29G2"):
        judge_g2(v, rec, out)
    elif name.startswith("X29"):
        judge_x29(v, rec, out)
    elif name in ("J29_BUILD_TABLE", "J29_BUILD_TABLE_ODD", "J29_BUILD_PAIR"):
        judge_table(v, rec, out)
    elif name.startswith("J29"):
        judge_j29(v, rec, out)
    elif name.startswith("GLV"):
        judge_glv(v, rec, out, first)
    elif name.startswith("LADDER"):
        judge_ladder(v, rec, out, first)
    else:
        judge_sat(v, rec, out)
    return v


# ---- which bound every operand slot answers to: op -> [(slot, key)] (lazy operands; saturated ones are canonical) ---------------------------
IN_ROWS = {
    "X29_ADD": [(s, "x29.in") for s in range(8)], "X29_DBL": [(s, "x29.in") for s in range(4)], "X29_STORE": [(s, "x29.in") for s in range(4)],
    "J29_DBL": list(zip(range(3), _RUNK)),
    "J29_MADD": [(0, "j29.madd.x1"), (1, "j29.madd.y1.tight"), (2, "j29.run.z"), (3, "j29.madd.x2"), (4, "j29.madd.y2")],
    "J29_ADDSUB": [(s, "j29.addsub.in") for s in range(6)],
    "X29G2_ADD_MIXED": [(0, "g2.acc.x.tight"), (1, "g2.acc.x.tight")] + [(s, "g2.acc.tight") for s in range(2, 8)],
    "X29G2_ADD": [(s, "g2.tail") for s in range(16)], "X29G2_DBL": [(s, "g2.tail") for s in range(8)],
    "X29G2_DBL_OF_ACC": [(0, "g2.acc.x.tight"), (1, "g2.acc.x.tight")] + [(s, "g2.acc.tight") for s in range(2, 8)],
    "X29G2_STORE": [(0, "g2.acc.x.tight"), (1, "g2.acc.x.tight")] + [(s, "g2.acc.tight") for s in range(2, 8)],
}
SAT_SLOTS = {"X29_LOAD_STORE": 4, "J29_SAT_ROUNDTRIP": 3, "J29_BUILD_TABLE": 3, "J29_BUILD_TABLE_ODD": 3, "J29_BUILD_PAIR": 6, "LADDER_FIXED": 3,
             "LADDER_GTAB": 3, "LADDER_UNIFORM": 3, "LADDER_MUL2": 6, "XYZZ_ADD_MIXED_FQ": 6, "XYZZ_ADD_FQ": 8, "XYZZ_DBL_FQ": 4, "XYZZ_DBL_AFF_FQ": 2,
             "JAC_ADD_FQ": 6, "JAC_ADD_MIXED_FQ": 5, "JAC_DBL_FQ": 3, "XYZZ_ADD_MIXED_FQ2": 12, "XYZZ_ADD_FQ2": 16, "XYZZ_DBL_FQ2": 8,
             "XYZZ_DBL_AFF_FQ2": 4, "JAC_ADD_FQ2": 12, "JAC_ADD_MIXED_FQ2": 10, "JAC_DBL_FQ2": 6}
SAT_EXTRA = {"X29G2_ADD_MIXED": range(8, 12)}          # saturated slots beside lazy ones


def operand_errors(name, rec):
    """what of this record lies outside its callee's documented bound"""
    bad = []
    for s, key in IN_ROWS.get(name, []):
        if any(x > L29_8 for x in rec[s][:8]) or not fr.val(rec[s]) < bound(key):
            bad.append("slot %d outside %s" % (s, key))
    for s in list(range(SAT_SLOTS.get(name, 0))) + list(SAT_EXTRA.get(name, [])):
        if rec[s][8] or not fr.wval(rec[s]) < P:
            bad.append("slot %d not canonical" % s)
    if name in LADDER_OPS or name == "GLV_UNIFORM_DIGITS":
        for s in {"LADDER_MUL2": (6, 7), "GLV_UNIFORM_DIGITS": (0,)}.get(name, (3,)):
            if rec[s][8] or not fr.wval(rec[s]) < RFR:
                bad.append("scalar slot %d not below r" % s)
    if name == "GLV_DECOMPOSE" and not fr.wval(rec[0]) < RFR:
        bad.append("k not below r")
    if name == "GLV_FIXED_DIGITS" and val32(rec[0][:5]) >> 128:
        bad.append("magnitude of 2^128 or more")
    return bad


# ---- families ---------------------------------------------------------------------------------------------------------------------------------
Z_KINDS = ("z=1", "z=p-1", "z=rand")


def _z(rng, kind, deg=1):
    return {"z=1": (1,) + (0,) * (deg - 1), "z=p-1": (P - 1,) + (0,) * (deg - 1)}.get(kind) or fel(rng, deg)


def xyzz_of(pt, z):
    """(x z^2, y z^3, z^2, z^3) as field elements"""
    z2 = f_mul(z, z)
    z3 = f_mul(z, z2)
    return [f_mul(pt[0], z2), f_mul(pt[1], z3), z2, z3]


def jac_of(pt, z):
    z2 = f_mul(z, z)
    return [f_mul(pt[0], z2), f_mul(pt[1], f_mul(z, z2)), z]


def lazy_pt(coords, mults):
    """field elements -> lazy slots, component by component, residue + m p in exact limbs"""
    out, i = [], 0
    for c in coords:
        for comp in c:
            out.append(lz(comp, mults[i % len(mults)]))
            i += 1
    return out


def sat_pt(coords):
    return [sat(comp) for c in coords for comp in c]


# A family entry is (tag, record) or (tag, record, logs): the discrete logs (base G, mod r) of the op's result points in the order of result_images, where the
# operands are multiples of G that the generator knows. tests/test_gpu_point_ops.py checks those against (log) G computed with oracle/bn254_py.py.
def _log_pts(rng, n):
    """points of the curve with known logs"""
    logs = [1, 2, 3, RFR - 1, RFR - 2] + [rng.randrange(1, RFR) for _ in range(n)]
    return [(k, mul_g(k)) for k in logs[:n]]


def gen_xyzz_lazy(name):
    """X29_ADD, X29_DBL, X29_STORE and the X29G2 ops: [(tag, record)]"""
    rng, out = _rng(name), []
    g2 = name.startswith("X29G2")
    deg = 2 if g2 else 1
    mixed, two = name == "X29G2_ADD_MIXED", name in ("X29_ADD", "X29G2_ADD")
    if g2:
        acc = name in ("X29G2_ADD_MIXED", "X29G2_DBL_OF_ACC", "X29G2_STORE")
        top = [1, 1, 3, 3, 3, 3, 3, 3] if acc else [0] * 8          # the largest multiple of p to add in each slot (values stay below 2 / 4 / 1.2 p)
        keys = [k for _, k in IN_ROWS[name]][:8]
    else:
        top, keys = [31] * 4, ["x29.in"] * 4
    nsl = 4 * deg

    def A(coords, mults, flag=0):
        return lazy_pt(coords, mults), flag

    def second(pt, z, mults):
        """the second operand of the op in its own form -> (slots, flag)"""
        if mixed:
            return sat_pt(list(pt) if pt is not None else [(0,) * deg] * 2), 0
        if pt is None:
            return [lazy_below(rng, bound(k)) for k in keys], 1          # arbitrary limbs behind a set flag
        return lazy_pt(xyzz_of(pt, z), mults), 0

    def rec(a, b=None):
        slots = list(a[0])
        flags = [a[1]]
        if b is not None:
            slots += b[0]
            flags.append(b[1])
        return record(slots, flags)

    def randpt():
        return (fel(rng, deg), fel(rng, deg))

    def mults(kind):
        if kind == "0":
            return [0]
        if kind == "top":
            return top
        return [rng.randrange(t + 1) for t in top]
    inf_a = lambda: ([lazy_below(rng, bound(k)) for k in keys], 1)

    # canonical operands as the loaders produce them
    if not g2:
        for tag, vals in (("canonical:p-1 in x", (P - 1, None, None)), ("canonical:p-1 in y", (None, P - 1, None)), ("canonical:z=p-1", (None, None, P - 1)),
                          ("canonical:all p-1", (P - 1, P - 1, P - 1))) + tuple(("canonical:random", (None, None, None)) for _ in range(256)):
            pts = []
            for _ in range(2):
                x, y, z = (((v * R256I) % P,) if v is not None else fel(rng, 1) for v in vals)          # the saturated WORD is p - 1
                c = [x, y, f_mul(z, z), f_mul(z, f_mul(z, z))]
                pts.append(([sh5(e[0]) for e in c], 0))
            out.append((tag, rec(pts[0], pts[1] if two else None)))
    else:
        for _ in range(256):          # l2_from_fq2 / the product by `one`: reduced values, exact limbs, below 1.2 p
            a = A(xyzz_of(randpt(), fel(rng, deg)), [0])
            out.append(("canonical:random", rec(a, second(randpt(), fel(rng, deg), [0]) if (two or mixed) else None)))
        if mixed:
            for tag, w in (("canonical:table words p-1", P - 1), ("canonical:table words 1", 1)):
                q = [tuple(w * R256I % P for _ in range(deg))] * 2
                out.append((tag, rec(A(xyzz_of(randpt(), fel(rng, deg)), [0]), (sat_pt(q), 0))))
    # bound corners: each coordinate alone at its bound minus one, then all; exact limbs and limbs 0..7 up to 2^29 + 8
    for style in ("exact", "lazy"):
        for which in list(range(nsl)) + ["all"]:
            pt, z = randpt(), fel(rng, deg)
            c = xyzz_of(pt, z)
            slots = lazy_pt(c, [0])
            for s in range(nsl):
                if which == "all" or which == s:
                    free = s < 2 * deg          # X and Y take any residue; ZZ and ZZZ are tied by ZZ^3 == ZZZ^2: the top multiple of p above the residue
                    if free:
                        slots[s] = fr.l29(bound(keys[s]) - 1) if style == "exact" else lazy_below(rng, bound(keys[s]))
                    else:
                        res = fr.val(slots[s])
                        m = (bound(keys[s]) - 1 - res) // P
                        slots[s] = fr.l29(res + m * P)
            tag = "corner:%s:%s" % (style, which)
            out.append((tag, rec((slots, 0), second(randpt(), fel(rng, deg), top if not mixed else [0]) if (two or mixed) else None)))
            if two:          # the corner on the second operand too
                out.append((tag + ":b", rec(A(xyzz_of(randpt(), fel(rng, deg)), [0]), (slots, 0))))
    if mixed:          # accumulator at its bound against table coordinates 32 (p - 1)
        q = [tuple((P - 1) * R256I % P for _ in range(deg))] * 2
        for style in ("exact", "lazy"):
            c = xyzz_of(randpt(), fel(rng, deg))
            slots = lazy_pt(c, top)
            for s in range(4):
                slots[s] = fr.l29(bound(keys[s]) - 1) if style == "exact" else lazy_below(rng, bound(keys[s]))
            out.append(("corner:%s:acc at bound, table 32(p-1)" % style, rec((slots, 0), (sat_pt(q), 0))))
    if name == "X29_DBL":
        for style in ("exact", "lazy"):
            slots = lazy_pt(xyzz_of(randpt(), fel(rng, 1)), [31])
            slots[1] = fr.l29(32 * P - 1) if style == "exact" else lazy_below(rng, 32 * P)
            out.append(("corner:%s:Y=32p-1" % style, rec((slots, 0))))
    # every branch in more than one representation
    if two or mixed:
        for zk1 in Z_KINDS:
            for zk2 in (Z_KINDS if not mixed else ("z=1",)):
                for mk in ("0", "top", "rand", "rand"):
                    pt = randpt()
                    z1, z2 = _z(rng, zk1, deg), _z(rng, zk2, deg)
                    a = A(xyzz_of(pt, z1), mults(mk))
                    sfx = ":%s:%s:m=%s" % (zk1, zk2, mk)
                    out.append(("branch:equal" + sfx, rec(a, second(pt, z2, mults(mk)))))
                    out.append(("branch:opposite" + sfx, rec(a, second(ct_neg(pt), z2, mults(mk)))))
                    out.append(("branch:P+2P" + sfx, rec(a, second(ct_add(pt, pt), z2, mults(mk)))))
                    out.append(("branch:2P+P" + sfx, rec(A(xyzz_of(ct_add(pt, pt), z1), mults(mk)), second(pt, z2, mults(mk)))))
        out += zero_test_sweep(name, rng, rec, A, second, randpt, top, deg)
        for mk in ("0", "top"):
            pt = randpt()
            out.append(("identity:a:m=" + mk, rec(inf_a(), second(pt, fel(rng, deg), mults(mk)))))
            out.append(("identity:b:m=" + mk, rec(A(xyzz_of(pt, fel(rng, deg)), mults(mk)), second(None, None, None))))
            out.append(("identity:both:m=" + mk, rec(inf_a(), second(None, None, None))))
        # coordinates == 0 where the formula is defined
        for tag, pa, pb in (("zero:x1", ((0,) * deg, fel(rng, deg)), randpt()), ("zero:x2", randpt(), ((0,) * deg, fel(rng, deg))),
                            ("zero:y1", (fel(rng, deg), (0,) * deg), randpt()), ("zero:y2", randpt(), (fel(rng, deg), (0,) * deg)),
                            ("zero:x1=x2=0,y1=-y2", ((0,) * deg, (5,) + (0,) * (deg - 1)), ((0,) * deg, (P - 5,) + (0,) * (deg - 1)))):
            for mk in ("0", "top"):
                out.append((tag + ":m=" + mk, rec(A(xyzz_of(pa, fel(rng, deg)), mults(mk)), second(pb, fel(rng, deg), mults(mk)))))
    else:
        for zk in Z_KINDS:
            for mk in ("0", "top", "rand"):
                out.append(("point:%s:m=%s" % (zk, mk), rec(A(xyzz_of(randpt(), _z(rng, zk, deg)), mults(mk)))))
        out.append(("identity:a", rec(inf_a())))
        out.append(("zero:x", rec(A(xyzz_of(((0,) * deg, fel(rng, deg)), fel(rng, deg)), top))))
    # points of the curve with known logs
    if not g2:
        lp = _log_pts(rng, 12)
        for i, (ka, pa) in enumerate(lp):
            kb, pb = lp[(5 * i + 1) % len(lp)]
            out.append(("logs:%d,%d" % (ka, kb), rec(A(xyzz_of(pa, fel(rng, 1)), mults("rand")), second(pb, fel(rng, 1), mults("rand")) if two else None),
                        [ka + kb if two else 2 * ka if name == "X29_DBL" else ka]))
    for _ in range(128):
        out.append(("random", rec(A(xyzz_of(randpt(), fel(rng, deg)), mults("rand")), second(randpt(), fel(rng, deg), mults("rand")) if (two or mixed) else None)))
    return out


def zero_test_multiples(name, rec):
    """the multiple of p that the argument of the op's first zero test holds on this record (None: not a multiple), by the limb-exact column model of
    field_ref -- x29_add: P = U2 - U1 + 8p; j29_addsub: H = U2 - U1 + 4p; j29_madd: H = U2 - X1 + 32p; the G2 additions: both components of P"""
    mc = lambda a, b: fr.mont_closed([(a, b)])[0]
    sub = lambda a, b, k: fr.sub_model(a, b, fr.K[k])[0]
    if name == "X29_ADD":
        args = [sub(mc(rec[4], rec[2]), mc(rec[0], rec[6]), "K8")]
    elif name == "J29_ADDSUB":
        args = [sub(mc(rec[3], mc(rec[2], rec[2])), mc(rec[0], mc(rec[5], rec[5])), "K4")]
    elif name == "J29_MADD":
        args = [sub(mc(rec[3], mc(rec[2], rec[2])), rec[0], "K32")]
    else:
        return None
    ks = [fr.val(a) // P if fr.val(a) % P == 0 else None for a in args]
    return ks[0]


# the multiples of p each zero test's argument can take on equal x: its bias plus the span of the two sides
#   x29_add     P = U2 - U1 + 8p, both sides products below 7.1 p of one residue: 8 - 7 .. 8 + 7
#   j29_addsub  H = U2 - U1 + 4p, both sides below 2.35 p: 4 - 2 .. 4 + 2
#   j29_madd    H = U2 - X1 + 32p, X1 below 19 p, U2 a product below 1.1 p: 32 - 18 .. 32 + 1
ZERO_TEST_RANGE = {"X29_ADD": range(1, 16), "J29_ADDSUB": range(2, 7), "J29_MADD": range(14, 34)}


def zero_test_sweep(name, rng, rec, A, second, randpt, top, deg):
    """equal and opposite points over a grid of lazy multiples, so that the zero test's argument takes every multiple of p its bound allows"""
    out = []
    if name != "X29_ADD":
        for ma in range(max(top) + 1):
            pt = randpt()
            z1, z2 = fel(rng, deg), fel(rng, deg)
            lo, hi = [min(t, ma) for t in top], [t - min(t, ma) for t in top]
            out.append(("zerotest:equal:m=%d" % ma, rec(A(xyzz_of(pt, z1), lo), second(pt, z2, hi))))
            out.append(("zerotest:opposite:m=%d" % ma, rec(A(xyzz_of(pt, z1), hi), second(ct_neg(pt), z2, lo))))
        return out
    seen = {}
    for _ in range(6000):
        if len(seen) == len(ZERO_TEST_RANGE[name]):
            break
        pt = randpt()
        z1, z2 = fel(rng, deg), fel(rng, deg)
        ms = [rng.choice([0, 0, 4, 12, 20, 28, 31, 31]) for _ in range(4)]
        r = rec(A(xyzz_of(pt, z1), ms), second(pt, z2, [rng.choice([0, 0, 4, 12, 20, 28, 31, 31]) for _ in range(4)]))
        k = zero_test_multiples(name, r)
        if k is not None and k not in seen:
            seen[k] = r
    for swap in (False, True):          # P = p and P = 15p: one side 7p above the other, which a draw does not find
        for _ in range(40):
            r = _x29_extreme(rng, swap)
            k = zero_test_multiples(name, r) if r else None
            if k in (1, 15):
                seen.setdefault(k, r)
                break
    for k in sorted(seen):
        out.append(("zerotest:equal:P=%dp" % k, seen[k]))
        r2 = [list(s) for s in seen[k]]
        r2[5] = lz((-dl(r2[5])) % P, fr.val(r2[5]) // P)          # the opposite point with the same x products
        out.append(("zerotest:opposite:P=%dp" % k, r2))
    return out


def _x29_extreme(rng, swap):
    """equal points with U1 = u + 7p and U2 = u (swap: the other way round): the residues of a.x and b.zz just below p at the multiple 31, their product's
    residue u small"""
    for _ in range(400):
        z2 = rng.randrange(1, P)
        rz = z2 * z2 * R261 % P
        if rz > 97 * P // 100:
            break
    else:
        return None
    for _ in range(4000):
        rx = rng.randrange(97 * P // 100, P)
        u = rx * rz * R261I % P
        if P // 150 < u < P // 50:
            break
    else:
        return None
    z1 = rng.randrange(1, P)
    x = rx * R261I * pow(z1 * z1, -1, P) % P
    pt = ((x,), (rng.randrange(1, P),))
    a, b = lazy_pt(xyzz_of(pt, (z1,)), [31, 0, 0, 0]), lazy_pt(xyzz_of(pt, (z2,)), [0, 0, 31, 0])
    return record(b + a if swap else a + b)


def gen_j29(name):
    rng, out = _rng(name), []
    randpt = lambda: (fel(rng, 1), fel(rng, 1))
    bx, by, bz = (bound(k) for k in (("j29.madd.x1", "j29.madd.y1.tight", "j29.run.z") if name == "J29_MADD" else _RUNK if name == "J29_DBL" else ("j29.addsub.in",) * 3))
    tops = [(b - P) // P for b in (bx, by, bz)]          # residue + m p stays below the bound for m <= tops

    def J(pt, z, ms):
        return lazy_pt(jac_of(pt, z), ms)

    def aff2(pt, mx=0, my=0):
        return [lz(pt[0][0], mx), lz(pt[1][0], my)]

    def rnd_m():
        return [rng.randrange(t + 1) for t in tops]

    def second(pt, z, ms):
        return aff2(pt, ms[0] % 9, ms[1] % 3) if name == "J29_MADD" else J(pt, z, ms) if name == "J29_ADDSUB" else []
    two = name != "J29_DBL"
    # canonical operands as the loaders produce them (j29_from_sat: 32 v; the addend of j29_madd: u29_from_fq-like, exact limbs below 2p)
    if name != "J29_MADD":
        for tag, vals in (("canonical:p-1 in x", (P - 1, None, None)), ("canonical:p-1 in y", (None, P - 1, None)), ("canonical:p-1 in z", (None, None, P - 1)),
                          ("canonical:all p-1", (P - 1,) * 3)) + tuple(("canonical:random", (None,) * 3) for _ in range(256)):
            pts = [[sh5((v * R256I) % P if v is not None else rng.randrange(1, P)) for v in vals] for _ in range(2)]
            if name == "J29_DBL":          # the running point's set is narrower than the loaders' 32 v: the same residues, reduced
                pts = [[lz(dl(s)) for s in p] for p in pts]
            out.append((tag, record(pts[0] + (pts[1] if two else []))))
    else:
        for _ in range(256):
            out.append(("canonical:random", record(J(randpt(), fel(rng, 1), [0]) + aff2(randpt()))))
    # bound corners
    for style in ("exact", "lazy"):
        for which in (0, 1, 2, "all"):
            slots = J(randpt(), fel(rng, 1), [0])
            for s, b in enumerate((bx, by, bz)):
                if which in (s, "all"):
                    slots[s] = fr.l29(b - 1) if style == "exact" else lazy_below(rng, b)
            tag = "corner:%s:%s" % (style, which)
            out.append((tag, record(slots + second(randpt(), fel(rng, 1), tops))))
            if name == "J29_ADDSUB":
                out.append((tag + ":v", record(J(randpt(), fel(rng, 1), [0]) + slots)))
                out.append((tag + ":both", record(slots + [list(s) for s in reversed(slots)])))
    if name == "J29_MADD":
        for style in ("exact", "lazy"):
            for tag, y2 in (("S2==0", 0), ("S2 small", 1)):
                # Y1 at its bound with S2 == 0 (y2 == 0: S2 is the product of the limbs 0) and with S2 small (y2 the residue that makes y2 Z^3 == 1 / 2^261... small)
                z = fel(rng, 1)
                slots = J(randpt(), z, [0])
                slots[1] = fr.l29(by - 1) if style == "exact" else lazy_below(rng, by)
                x2 = lz(rng.randrange(1, P))
                if y2 == 0:
                    ys = [0] * 9
                else:          # S2 = y2 Z^3 / 2^261 as a residue: choose it 1, so that the product's value is 1 or p + 1
                    zl = fr.val(slots[2])
                    ys = fr.l29(pow(zl, -3, P) * R261 * R261 * R261 % P)
                out.append(("corner:%s:Y1 at bound, %s" % (style, tag), record(slots + [x2, ys])))
            for mx2 in (0, 3):
                slots = [fr.l29(bx - 1) if style == "exact" else lazy_below(rng, bx), lazy_below(rng, by), lazy_below(rng, bz)]
                p2 = randpt()
                out.append(("corner:%s:running set, addend m=%d" % (style, mx2), record(slots + [fr.l29(bound("j29.madd.x2") - 1) if mx2 else lz(p2[0][0]), fr.l29(bound("j29.madd.y2") - 1) if mx2 else lz(p2[1][0])])))
    # branches
    if two:
        for zk1 in Z_KINDS:
            for zk2 in Z_KINDS:
                for mk in ("0", "top", "rand"):
                    ms = lambda: [0] * 3 if mk == "0" else tops if mk == "top" else rnd_m()
                    pt, z1, z2 = randpt(), _z(rng, zk1), _z(rng, zk2)
                    sfx = ":%s:%s:m=%s" % (zk1, zk2, mk)
                    out.append(("branch:equal" + sfx, record(J(pt, z1, ms()) + second(pt, z2, ms()))))
                    out.append(("branch:opposite" + sfx, record(J(pt, z1, ms()) + second(ct_neg(pt), z2, ms()))))
                    out.append(("branch:P+2P" + sfx, record(J(pt, z1, ms()) + second(ct_add(pt, pt), z2, ms()))))
                    out.append(("branch:2P+P" + sfx, record(J(ct_add(pt, pt), z1, ms()) + second(pt, z2, ms()))))
        # the zero test's argument on every multiple of p its bound allows
        seen = {}
        for _ in range(4000):
            if len(seen) == len(ZERO_TEST_RANGE[name]):
                break
            pt, z1, z2 = randpt(), fel(rng, 1), fel(rng, 1)
            if name == "J29_MADD":
                r = record(J(pt, z1, [rng.randrange(tops[0] + 1), rng.randrange(tops[1] + 1), rng.randrange(2)]) + aff2(pt, rng.randrange(9), rng.randrange(3)))
            else:
                r = record(J(pt, z1, [rng.choice([0, 8, 31]) for _ in range(3)]) + J(pt, z2, [rng.choice([0, 8, 31]) for _ in range(3)]))
            k = zero_test_multiples(name, r)
            if k is not None and k not in seen:
                seen[k] = r
        if name == "J29_MADD":          # H = 33p: X1 so small that the product U2 of the same residue comes out one p higher
            for _ in range(40):
                z = fel(rng, 1)
                v = rng.randrange(1, P // 5000)
                pt = ((v * R261I * pow(z[0] * z[0], -1, P) % P,), fel(rng, 1))
                r = record(J(pt, z, [0, 0, 1]) + aff2(pt, 8, 0))
                if zero_test_multiples(name, r) == 33:
                    seen[33] = r
                    break
        for k in sorted(seen):
            out.append(("zerotest:equal:H=%dp" % k, seen[k]))
            r2 = [list(s) for s in seen[k]]
            s = 4
            r2[s] = lz((-dl(r2[s])) % P, min(fr.val(r2[s]) // P, 2))
            out.append(("zerotest:opposite:H=%dp" % k, r2))
        for tag, pa, pb in (("zero:x1", ((0,), fel(rng, 1)), randpt()), ("zero:x2", randpt(), ((0,), fel(rng, 1))), ("zero:y1", (fel(rng, 1), (0,)), randpt()),
                            ("zero:y2", randpt(), (fel(rng, 1), (0,)))):
            out.append((tag, record(J(pa, fel(rng, 1), rnd_m()) + second(pb, fel(rng, 1), rnd_m()))))
    else:
        for zk in Z_KINDS:
            for mk in range(3):
                out.append(("point:%s:m=%d" % (zk, mk), record(J(randpt(), _z(rng, zk), [0] * 3 if mk == 0 else tops if mk == 1 else rnd_m()))))
        out.append(("zero:x", record(J(((0,), fel(rng, 1)), fel(rng, 1), tops))))
    lp = _log_pts(rng, 12)
    for i, (ka, pa) in enumerate(lp):
        kb, pb = lp[(5 * i + 1) % len(lp)]
        out.append(("logs:%d,%d" % (ka, kb), record(J(pa, fel(rng, 1), rnd_m()) + second(pb, fel(rng, 1), rnd_m())),
                    {"J29_DBL": [2 * ka], "J29_MADD": [ka + kb], "J29_ADDSUB": [ka + kb, ka - kb]}[name]))
    for _ in range(128):
        out.append(("random", record(J(randpt(), fel(rng, 1), rnd_m()) + second(randpt(), fel(rng, 1), rnd_m()))))
    return out


def gen_sat(name):
    """the saturated formulas and the round trips: canonical operands"""
    rng, out = _rng(name), []
    deg = 2 if name.endswith("FQ2") else 1
    kind = name[:-4] if deg == 2 else name[:-3] if name.endswith("_FQ") else name
    randpt = lambda: (fel(rng, deg), fel(rng, deg))
    form = {"XYZZ_ADD_MIXED": ("X", "A"), "XYZZ_ADD": ("X", "X"), "XYZZ_DBL": ("X",), "XYZZ_DBL_AFF": ("A",), "JAC_ADD": ("J", "J"), "JAC_ADD_MIXED": ("J", "A"),
            "JAC_DBL": ("J",), "X29_LOAD_STORE": ("X",), "J29_SAT_ROUNDTRIP": ("J",)}[kind]

    def enc(f, pt, z):
        if pt is None:
            junk = [fel(rng, deg), fel(rng, deg)]
            return sat_pt({"X": junk + [(0,) * deg] * 2, "J": junk + [(0,) * deg], "A": [(0,) * deg] * 2}[f])
        return sat_pt({"X": xyzz_of, "J": jac_of}[f](pt, z) if f != "A" else list(pt))

    def R(a, b=None, za=None, zb=None):
        s = enc(form[0], a, za or fel(rng, deg))
        if len(form) == 2:
            s += enc(form[1], b, zb or fel(rng, deg))
        return record(s)
    for _ in range(256):
        out.append(("canonical:random", R(randpt(), randpt())))
    w = lambda v: tuple(v * R256I % P for _ in range(deg))          # the saturated WORDS hold v
    for tag, v in (("p-1", P - 1), ("1", 1)):
        a, b = (w(v), fel(rng, deg)), (fel(rng, deg), w(v))
        out.append(("corner:words %s in x | y" % tag, R(a, b, (1,) + (0,) * (deg - 1), (1,) + (0,) * (deg - 1))))
        out.append(("corner:words %s in z" % tag, R(randpt(), randpt(), w(v), w(v))))
    if len(form) == 2:
        for zk1 in Z_KINDS:
            for zk2 in Z_KINDS:
                pt, z1, z2 = randpt(), _z(rng, zk1, deg), _z(rng, zk2, deg)
                sfx = ":%s:%s" % (zk1, zk2)
                out += [("branch:equal" + sfx, R(pt, pt, z1, z2)), ("branch:opposite" + sfx, R(pt, ct_neg(pt), z1, z2)),
                        ("branch:P+2P" + sfx, R(pt, ct_add(pt, pt), z1, z2)), ("branch:2P+P" + sfx, R(ct_add(pt, pt), pt, z1, z2))]
        pt = randpt()
        out += [("identity:b", R(pt, None)), ("identity:both", R(None, None))]
        if form[0] != "A":
            out.append(("identity:a", R(None, pt)))
        out += [("zero:x1", R(((0,) * deg, fel(rng, deg)), randpt())), ("zero:x2", R(randpt(), ((0,) * deg, fel(rng, deg)))),
                ("zero:y1", R((fel(rng, deg), (0,) * deg), randpt()))]
    else:
        for zk in Z_KINDS:
            out.append(("point:" + zk, R(randpt(), None, _z(rng, zk, deg))))
        if form[0] != "A":
            out.append(("identity:a", R(None)))
        out.append(("zero:x", R(((0,) * deg, fel(rng, deg)))))
    if deg == 1:
        lp = _log_pts(rng, 10)
        for i, (ka, pa) in enumerate(lp):
            kb, pb = lp[(3 * i + 1) % len(lp)]
            out.append(("logs:%d,%d" % (ka, kb), R(pa, pb), [ka + kb if len(form) == 2 else 2 * ka if "DBL" in kind else ka]))
    return out


# ---- GLV scalars ------------------------------------------------------------------------------------------------------------------------------
G1MUL_CONSTANTS = (9931322734385697763, 147946756881789319010696353538189108491, 147946756881789319000765030803803410728)


def half_scalars():
    """magnitudes below 2^127 for the built scalars: 0, 1, 2^127 - 1, the nibble patterns of the fixed recoding's carry chains (ending in the carry digit 32),
    runs that make the width-5 NAF carry through every position"""
    top = (1 << 127) - 1
    hs = [("0", 0), ("1", 1), ("2^127-1", top)]
    for nib in (7, 8, 9, 0xF):
        v = int("%x" % nib * 32, 16)
        hs.append(("nibbles %x" % nib, v & top))
        hs.append(("nibbles %x, top 7" % nib, (v & ((1 << 124) - 1)) | (7 << 124)))
    hs.append(("nibbles 8 then 7s", int("7" * 31 + "8", 16) & top))
    hs.append(("nibbles 9 low, 8s", int("7" + "8" * 30 + "9", 16)))
    for d in range(1, 9):
        hs.append(("nibbles all %d" % d, int("%x" % d * 31, 16)))
        hs.append(("nibbles all %x" % (16 - d), int("7" + "%x" % (16 - d) * 31, 16)))          # the digit -d in every window, the carry into the top nibble
    for d in range(1, 16, 2):
        hs.append(("naf +%d" % d, sum(d << (6 * i) for i in range(20))))
        hs.append(("naf -%d" % d, sum((32 - d) << (6 * i) for i in range(20)) & top))
    for s in range(5):
        hs.append(("ones from bit %d" % s, (top >> s) << s))
        hs.append(("runs of 5 ones, shift %d" % s, sum(31 << (7 * i + s) for i in range(17)) & top))
    hs.append(("alternating", int("5" * 31, 16)))
    return hs


def glv_scalars():
    """[(tag, k)]: named scalars, both sides of the rounding steps of c1 and c2, and scalars built from chosen half-scalars (kept only when the integer
    reference of glv_decompose gives the chosen pair back) -> (list, built, dropped)"""
    named = [("0", 0), ("1", 1), ("2", 2), ("r-1", RFR - 1), ("r-2", RFR - 2), ("lambda", LAMBDA), ("lambda+1", LAMBDA + 1), ("lambda-1", LAMBDA - 1),
             ("r-lambda", RFR - LAMBDA), ("2lambda", 2 * LAMBDA % RFR), ("lambda^2", LAMBDA * LAMBDA % RFR), ("2^127", 1 << 127), ("2^128-1", (1 << 128) - 1),
             ("2^128", 1 << 128), ("2^253+5", (1 << 253) + 5)] + [("g1_mul_batch constant %d" % i, c) for i, c in enumerate(G1MUL_CONSTANTS)]
    for i, g in ((1, GLV_G1), (2, GLV_G2)):
        mmax = ((RFR - 1) * g) >> 256
        for m in sorted({1, 2, 3, mmax // 2, mmax - 1, mmax}):
            k = -((-m << 256) // g)          # ceil(m 2^256 / g): the first k with c_i = m
            if 0 < k < RFR:
                named += [("c%d steps to %d" % (i, m), k), ("c%d one below the step to %d" % (i, m), k - 1)]
    # c_i is a FLOOR of a product with a floored constant, not a rounding: (k1, k2) = f1 (a1, b1) + f2 (a2, b2) with f1 in [e1, 1 + e1), f2 in [e2, 1 + e2), where
    # e_i = k frac(g_i) / 2^256 < 0.09 | 0.13. So k1 = f1 a1 + f2 a2 is never negative, k2 = f1 b1 + f2 b2 is positive only below b2 < 2^64, and a chosen pair
    # (+h1, -h2) is what the decomposition returns when f1 ~ h2 / |b1| and f2 ~ h1 / a2 lie in [0.13, 1): both magnitudes from 2^125 to 2^126. The patterns keep their
    # low 31 nibbles and get the top nibble 2 or 3; (+h, 0) is the decomposition of k = h itself. What the edges of the cell still drop is counted.
    built, dropped = [], 0
    pats = half_scalars()
    hs = [(t, (h & ((1 << 124) - 1)) | ((2 + (i & 1)) << 124)) for i, (t, h) in enumerate(pats)]
    for i, (t1, h1) in enumerate(hs):
        for (t2, h2), s2 in ((hs[(3 * i + 1) % len(hs)], -1), (hs[(7 * i + 2) % len(hs)], -1), ((t1, h1), -1), (("0", 0), 1)):
            if not h2:
                h1 = pats[i][1] & ((1 << 126) - 1)
            k = (h1 + s2 * h2 * LAMBDA) % RFR
            if glv_ref(k) == (h1, s2 * h2):
                built.append(("built:+%s %s%s" % (t1, "+-"[s2 < 0], t2), k))
            else:
                dropped += 1
    seen, uniq = set(), []
    for t, k in built:
        if k not in seen:
            seen.add(k)
            uniq.append((t, k))
    return named, uniq, dropped


def gen_glv(name):
    rng = _rng(name)
    named, built, _ = glv_scalars()
    named = [("named:" + t if i < 18 else "rounding:" + t, k) for i, (t, k) in enumerate(named)]
    ks = named + built + [("random", rng.randrange(RFR)) for _ in range(256)]
    if name == "GLV_DECOMPOSE":
        return [(t, record([fr.w32(k)])) for t, k in ks]
    if name == "GLV_FIXED_DIGITS":
        mags = [("pattern:" + t, h) for t, h in half_scalars()] + [("random", rng.randrange(1 << 127)) for _ in range(256)]
        mags += [("half:" + t, abs(h)) for t, k in ks[:len(named) + len(built)] for h in glv_ref(k)]
        # The header promises digit 32 as 'the carry' of a 127-bit magnitude; below 2^127 the top nibble is at most 7, 7 + 1 is not above 8, and the carry never
        # comes. The function reads 128 bits, and on those the carry digit is what makes the sum come out: the magnitudes from 2^127 on reach it.
        mags += [("128 bits:" + t, m) for t, m in (("2^127", 1 << 127), ("2^128-1", (1 << 128) - 1), ("nibbles 8, top 8", int("8" * 32, 16)), ("top 9", 9 << 124),
                                                   ("top 8, carry in", (8 << 124) | int("9" * 31, 16)), ("top f", int("f" + "0" * 31, 16)))]
        return [(t, record([[(m >> (32 * i)) & 0xFFFFFFFF for i in range(5)]])) for t, m in mags]
    # wave-uniform: one record per scalar stands for its wave; generate() lays the waves out
    pick = named[:18] + named[18::3] + built[::max(1, len(built) // 30)]
    return [(t, record([fr_mont(k)])) for t, k in pick[:58] + ks[-2:]]


def gen_tables(name):
    rng, out = _rng(name), []
    lp = _log_pts(rng, 40)
    pair = name == "J29_BUILD_PAIR"
    odd = name != "J29_BUILD_TABLE"
    entries = lambda k: [(k, 2 * e + 1 if odd else e + 1) for e in range(8)]          # (log, m): m times the oracle's (log) G, one full multiplication per table
    for i, (ka, pa) in enumerate(lp):
        for zk in Z_KINDS if i < 8 else ("z=rand",):
            slots = sat_pt(jac_of(pa, _z(rng, zk)))
            tag, logs = "logs:%d:%s" % (ka, zk), entries(ka)
            if pair:
                kb, pb = lp[(7 * i + 3) % len(lp)] if i % 4 else (ka, pa) if i % 8 else (RFR - ka, ct_neg(pa))          # B = A and B = -A among them
                slots += sat_pt(jac_of(pb, _z(rng, zk)))
                tag += ",%d" % kb
                logs += entries(kb)
            out.append((tag, record(slots), logs))
    # canonical corners: the saturated WORDS that u29_from_fq reads at p - 1 and at 1, in x, in y, in z and in all three (both points of a pair)
    npts = 2 if pair else 1
    for tag, v in (("p-1", P - 1), ("1", 1)):
        for which in (0, 1, 2, "all"):
            slots = []
            for _ in range(npts):
                words = [rng.randrange(1, P) for _ in range(3)]
                for c in range(3):
                    if which in (c, "all"):
                        words[c] = v
                slots += [fr.w32(w) for w in words]
            out.append(("corner:words %s in %s" % (tag, "xyz"[which] if which != "all" else "all"), record(slots)))
    # seeded random fill: random Jacobian points, off the curve (the builds never read b)
    for _ in range(256):
        out.append(("random", record([fr.w32(rng.randrange(1, P)) for _ in range(3 * npts)])))
    return out


def ladder_scalars():
    named, built, _ = glv_scalars()
    # r - 2d and (r - 2d) lambda: where a plain windowed ladder would find the running point on the entry it adds last (jac29.hip.h:175 names r - 2). After the
    # GLV split it does not: the last digit e of either half would have to satisfy k == 2e, and such a k decomposes into one digit. fixed_ladder_meetings runs the
    # ladder on integers and finds no meeting for any scalar of this list; inside a ladder `special` fires only in the two-term form, on related points.
    meet = [("candidate:r-%d" % (2 * d), RFR - 2 * d) for d in range(1, 9)] + [("candidate:(r-%d)lambda" % (2 * d), (RFR - 2 * d) * LAMBDA % RFR) for d in (1, 2)]
    return [("named:" + t if i < 18 else "rounding:" + t, k) for i, (t, k) in enumerate(named)] + meet + built[::5]


def fixed_ladder_meetings(k):
    """the fixed-window ladder of jac_scalar_mul_u29_j on integers: the running point as a multiple n of P; -> the list of `special` values (1: the entry added is
    the running point, 2: its negative) its additions meet"""
    k1, k2 = glv_ref(k)
    d = [fixed_ref(abs(k1))[0], fixed_ref(abs(k2))[0]]
    n, empty, met = 0, True, []
    for j in range(32, -1, -1):
        if not empty:
            n = 16 * n % RFR
        for which, (h, dig) in enumerate(zip((k1, k2), d)):
            if dig[j]:
                e = (dig[j] if h >= 0 else -dig[j]) * (LAMBDA if which else 1) % RFR
                if empty:
                    n, empty = e, False
                elif n == e:
                    met.append(1)
                    n = 2 * n % RFR
                elif (n + e) % RFR == 0:
                    met.append(2)
                    empty = True
                else:
                    n = (n + e) % RFR
    assert (0 if empty else n) == k % RFR
    return met


def gen_ladder(name):
    """[(tag, record, logs)] -- the uniform forms: 64 points per scalar (generate() keeps the waves whole)"""
    rng, out = _rng(name), []
    uniform = name in UNIFORM_OPS
    ks = ladder_scalars()
    base = [("G", 1, (1,)), ("G z", 1, None), ("7G z", 7, None)] + [("rand z", rng.randrange(1, RFR), None) for _ in range(3)] + [("identity", 0, None)]

    def jac(log, z):
        pt = mul_g(log)
        return sat_pt(jac_of(pt, z or fel(rng, 1))) if pt is not None else sat_pt([fel(rng, 1), fel(rng, 1), (0,)])
    if name == "LADDER_MUL2":
        ks16 = [ks[i] for i in (1, 3, 4, 5, 8, 10, 11, 14)] + ks[len(ks) - 8:]
        for w, (t, kA) in enumerate(ks16):
            tB, kB = ks16[(5 * w + 3) % 16]
            for negB in (w & 1,):
                for lane in range(64):
                    la = rng.randrange(1, RFR)
                    rel = ("B=A", la) if lane == 1 else ("B=-A", RFR - la) if lane == 2 else ("B=lambda A", la * LAMBDA % RFR) if lane == 3 else None
                    if lane == 4 and kB:          # kA A + kB B = identity: B = -(kA / kB) A
                        rel = ("sum=identity", (-kA * pow(kB, -1, RFR) * la * (-1 if negB else 1)) % RFR)
                    lb = rel[1] if rel and rel[1] % RFR else rng.randrange(1, RFR)
                    out.append(("%s:kB=%s,negB=%d:%s" % (t, tB, negB, rel[0] if rel else "random"),
                                record(jac(la, None) + jac(lb, None) + [fr_mont(kA), fr_mont(kB)], [0, 0, negB]), [kA * la + (-kB if negB else kB) * lb]))
        assert len(out) == 1024
        return out
    if uniform:
        sel = [ks[i] for i in (0, 1, 4, 5, 8, 11, 14, 15)] + ks[len(ks) - 8:]
        for t, k in sel:
            for lane in range(64):
                if lane == 0:
                    log, z, pt = 1, (1,), "G"
                elif lane == 1:
                    log, z, pt = 0, None, "identity"
                else:
                    log, z, pt = rng.randrange(1, RFR), None, "rand z"
                out.append(("%s:%s" % (t, pt), record(jac(log, z) + [fr_mont(k)]), [k * log]))
        assert len(out) == 1024
        return out
    for t, k in ks:          # every point, the identity included, with every scalar
        for pt, log, z in base:
            out.append(("%s:%s" % (t, pt), record(jac(log, z) + [fr_mont(k)]), [k * log]))
    for _ in range(64):
        log, k = rng.randrange(1, RFR), rng.randrange(RFR)
        out.append(("random", record(jac(log, None) + [fr_mont(k)]), [k * log]))
    assert len(out) <= 1024, len(out)
    return out


LOGS = {}          # op -> per record: None, or the logs of its result points (see _log_pts)


def generate(name):
    """-> (tags, records) in the order the device gets them"""
    if name.startswith(("X29_ADD", "X29_DBL", "X29_STORE", "X29G2")):
        fam = gen_xyzz_lazy(name)
    elif name in ("J29_DBL", "J29_MADD", "J29_ADDSUB"):
        fam = gen_j29(name)
    elif name.startswith("GLV"):
        fam = gen_glv(name)
        if name == "GLV_UNIFORM_DIGITS":          # every scalar leads a wave of its own; the other 63 lanes hold another scalar, which must not count
            other = record([fr_mont(0x1234567)])
            fam = [x for t, r in fam[:60] for x in [(t, r)] + [(t + " (a lane behind the first)", other)] * 63]
    elif name.startswith("J29_BUILD"):
        fam = gen_tables(name)
    elif name.startswith("LADDER"):
        fam = gen_ladder(name)
    else:
        fam = gen_sat(name)
    assert len(fam) <= MAX_RECORDS, (name, len(fam))
    LOGS[name] = [[k if isinstance(k, tuple) else k % RFR for k in f[2]] if len(f) == 3 else None for f in fam]
    return [f[0] for f in fam], [f[1] for f in fam]


def result_images(name, out):
    """the affine images of the points in one record's output, in the order the families' logs are given: one point, sum and difference for J29_ADDSUB, the eight
    entries of a table (sixteen of a pair) as points of E"""
    lazy_j = lambda s: img_jac([el_lazy(out, s + k, 1) for k in range(3)])
    if name in ("X29_ADD", "X29_DBL"):
        return [None if out[OUT_FLAG_SLOT][0] else img_xyzz([el_lazy(out, k, 1) for k in range(4)])]
    if name in ("X29_STORE", "X29_LOAD_STORE") or name.startswith("XYZZ"):
        return [img_xyzz([el_sat(out, k, 1) for k in range(4)])]
    if name == "J29_SAT_ROUNDTRIP" or name.startswith("JAC"):
        return [img_jac([el_sat(out, k, 1) for k in range(3)])]
    if name in ("J29_DBL", "J29_MADD"):
        return [lazy_j(0)]
    if name == "J29_ADDSUB":
        return [lazy_j(0), lazy_j(3)]
    if name.startswith("J29_BUILD"):
        pair = name == "J29_BUILD_PAIR"
        zi = f_inv((dl(out[48 if pair else 24]),))
        zi2 = f_mul(zi, zi)
        zi3 = f_mul(zi, zi2)
        return [(f_mul((dl(out[s + 3 * e]),), zi2), f_mul((dl(out[s + 3 * e + 2]),), zi3)) for s in ((0, 24) if pair else (0,)) for e in range(8)]
    if name.startswith("LADDER"):
        return [lazy_j(0) if out[OUT_FLAG_SLOT][0] else None]
    raise KeyError(name)


def family_kinds(tags):
    return {t.split(":")[0] for t in tags}


def distinct_records(name, n, seed=12):
    """n records of ordinary additions that all differ (tests/test_gpu_point_ops.py: every record gets its own answer)"""
    rng = random.Random(seed)
    deg = 2 if name in ("X29G2_ADD",) else 1
    pt = lambda: (fel(rng, deg), fel(rng, deg))
    if name == "X29_ADD":
        return [record(lazy_pt(xyzz_of(pt(), fel(rng, 1)), [rng.randrange(32) for _ in range(4)]) + lazy_pt(xyzz_of(pt(), fel(rng, 1)), [rng.randrange(32) for _ in range(4)])) for _ in range(n)]
    if name == "X29G2_ADD":
        return [record(lazy_pt(xyzz_of(pt(), fel(rng, 2)), [0]) + lazy_pt(xyzz_of(pt(), fel(rng, 2)), [0])) for _ in range(n)]
    if name == "J29_MADD":
        return [record(lazy_pt(jac_of(pt(), fel(rng, 1)), [rng.randrange(19), rng.randrange(3), rng.randrange(2)]) + lazy_pt(list(pt()), [rng.randrange(9), rng.randrange(3)])) for _ in range(n)]
    if name == "XYZZ_ADD_FQ":
        return [record(sat_pt(xyzz_of(pt(), fel(rng, 1))) + sat_pt(xyzz_of(pt(), fel(rng, 1)))) for _ in range(n)]
    raise KeyError(name)


_ORACLE, _ORACLE_PTS = [], {}


def oracle_point(k):
    """(k mod r) G -- for k = (log, m): m times (log) G -- by oracle/bn254_py.py (affine double and add, nothing shared with this file), in this file's point form"""
    if not _ORACLE:
        import importlib.util
        spec = importlib.util.spec_from_file_location("bn254_py", os.path.join(ROOT, "oracle", "bn254_py.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        assert m.P == P and m.R == RFR
        _ORACLE.append(m)
    m = _ORACLE[0]
    k, small = k if isinstance(k, tuple) else (k, 1)
    if k % RFR not in _ORACLE_PTS:
        if len(_ORACLE_PTS) > 4096:
            _ORACLE_PTS.clear()
        _ORACLE_PTS[k % RFR] = m.g1_mul(m.G1_GEN, k % RFR)
    pt = m.g1_mul(_ORACLE_PTS[k % RFR], small)
    return None if pt is None else ((pt[0],), (pt[1],))


def oracle_errors(name, out, logs):
    """the device's result points against (log) G of the oracle, for a record whose operands are known multiples of G"""
    got = result_images(name, out)
    assert len(got) == len(logs)
    return ["result point %d: device %s, oracle (%s) G = %s" % (i, _show(g), k, _show(oracle_point(k))) for i, (g, k) in enumerate(zip(got, logs)) if g != oracle_point(k)]


def oracle_sample(name, n):
    """which records of a family with logs go to the oracle: all of them, except for the ladders, where one oracle multiplication costs 10 ms and every record
    has a log: the first eight lanes of every wave of the uniform forms (G, the identity, the related points of the two-term form among them), every fourth
    record of the per-lane forms. Every record is judged against this file's reference in any case; tests/test_point_ref_model.py ties that to the oracle."""
    if name in ("LADDER_UNIFORM", "LADDER_MUL2"):
        return [i for i in range(n) if i % 64 < 8]
    if name in LADDER_OPS:
        return list(range(0, n, 4))
    return list(range(n))
