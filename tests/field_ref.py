"""Big-integer reference and operand families for the field probe (keaki_hip_selftest_field_ops, keaki_amd/csrc/field_probe.hip).

The host chooses the operands, the device runs ONE shipped field function per record and returns the raw limbs, and the functions here say
what those limbs must be -- in plain Python integers, so every comparison is exact. tests/test_field_ref_model.py checks this file against
itself on the CPU (bounds respected, column model == closed form, no bias difference negative); tests/test_gpu_field_ops.py runs the device.

Constants come from keaki_amd/csrc/gen_constants.py (its module values and the text it PRINTS), never from a generated header.

BOUNDS is the list a reviewer reads: one row per operand class, with the source line that documents it. A record is a list of up to 12
slots; a slot is 9 limbs (lazy) or 8 words (saturated).
"""
import contextlib
import importlib.util
import io
import os
import random
import re
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_gen_constants():
    spec = importlib.util.spec_from_file_location("keaki_gen_constants", os.path.join(ROOT, "keaki_amd", "csrc", "gen_constants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    texts = []
    for fn in (mod.main, mod.main_pair261):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fn()
        texts.append(buf.getvalue())
    return mod, texts


GC, (_TXT, _TXT261) = _load_gen_constants()
P, RFR = GC.P, GC.R
M29 = (1 << 29) - 1
R256, R261 = 1 << 256, 1 << 261
PINV261 = pow(P, -1, R261)
U32 = 1 << 32


def _arr(text, name, n):
    m = re.search(r"uint32_t %s\[%d\] = \{([^}]*)\}" % (name, n), text)
    return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]


def _struct(text, name):
    return text.split("struct %s {" % name, 1)[1].split("\n};", 1)[0]


_Q29 = _struct(_TXT, "Fq29Params")
K = {k: _arr(_Q29, k, 9) for k in ("K2", "K4", "K4W", "K8", "K16", "K16W", "K32", "K64", "K128", "K8W")}
K_MULT = {"K2": 2, "K4": 4, "K4W": 4, "K8": 8, "K16": 16, "K16W": 16, "K32": 32, "K64": 64, "K128": 128, "K8W": 8}
Q29_MOD, Q29_ONE, Q29_R256 = _arr(_Q29, "MOD", 9), _arr(_Q29, "ONE", 9), _arr(_Q29, "R256", 9)
Q29_INV = int(re.search(r"INV = 0x([0-9a-f]+)u", _Q29).group(1), 16)
Q29_PINV = int(re.search(r"PINV = 0x([0-9a-f]+)u", _Q29).group(1), 16)
C266, C783, PLAIN_ONE = (_arr(_TXT261, n, 9) for n in ("C266", "C783", "PLAIN_ONE"))


# ---- limbs and words -----------------------------------------------------------------------------------------------------------
def l29(v):
    """exact 29-bit limbs, limb 8 = the rest"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def w32(v):
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wval(w):
    return sum(x << (32 * i) for i, x in enumerate(w[:8]))


assert val(Q29_MOD) == P and val(Q29_ONE) == R261 % P and val(Q29_R256) == R256 % P and (Q29_INV * P + 1) % (1 << 29) == 0
assert all(val(K[k]) == K_MULT[k] * P for k in K) and val(C266) == (1 << 266) % P and val(C783) == (1 << 783) % P and val(PLAIN_ONE) == 1

L29_8, L30_16, L15_30, L31 = (1 << 29) + 8, (1 << 30) + 16, 3 << 29, (1 << 31) - 1

# ---- the bounds table ----------------------------------------------------------------------------------------------------------
# row -> (largest limb 0..7, largest limb 8, value bound (exclusive; None: whatever the limbs allow), source)
BOUNDS = {
    "mul.wide":   (L30_16, L30_16, None, "fq29_asm.hip.h:4 'Limbs at most 2^30 + 16 on one side'; fq29_core.hip.h:75"),
    "mul.narrow": (L29_8, L29_8, None, "fq29_asm.hip.h:4 '2^29 + 8 on the other'; fq29_core.hip.h:75"),
    "sqr":        (L29_8, L29_8, None, "fq29_asm.hip.h:11 'Limbs of a at most 2^29 + 8'; fq29_core.hip.h:106"),
    "mul2.abd":   (L29_8, L29_8, None, "fq29_asm.hip.h:19 'a, b, d at most 2^29 + 8'"),
    "mul2.c":     (L15_30, L15_30, None, "fq29_asm.hip.h:19 'c at most 1.5 * 2^30'"),
    "dot":        (L29_8, L29_8, None, "fq29_dot_asm.hip.h:4,11,18 'All limbs at most 2^29 + 8' (dot6: 63 terms in a column)"),
    "carry.in":   (U32 - 1, U32 - 8, None, "fq29_core.hip.h:162 'inputs: any u32 limbs' (limb 8 + carry 7 must fit a u32)"),
    "sub.a":      (L30_16, L29_8, 20 * P, "fq29_core.hip.h:12 'x < ~20p'; a_i + K_i < 2^32 for every K (gen_constants.py:126 biased)"),
    "subraw.a":   (L29_8, L29_8, 20 * P, "fq29_core.hip.h:178 'limbs below 2^31' holds for a carried minuend: a_i + K_i < 2^31; fq29_core.hip.h:12 'x < ~20p'"),
    "sub3.c":     (L29_8, L29_8, 2 * P, "fq29_core.hip.h:186 'a - b - 2c + 8p': b + 2c < 8p, limbs b_i + 2 c_i < 2^31"),
    "sub3.b":     (L29_8, L29_8, 4 * P - (1 << 233), "fq29_core.hip.h:186 'a - b - 2c + 8p': b + 2c < 8p - 2^233 (SUB_SLACK below)"),
    "mz18":       (U32 - 1, U32 - 1, 18 * P, "fq29_core.hip.h:193 'x < 18p and limb 0 is exact'"),
    "mz35":       (U32 - 1, U32 - 1, 35 * P, "fq29_core.hip.h:195 'the same for x < 35p'"),
    "is_zero":    (L30_16, L29_8, 101 * P, "fq29.hip.h:14 'a lazy value below ~100p'; limbs: the wide side of u29_mul (fq29_asm.hip.h:4)"),
    "pack":       (M29, M29, 2 * P, "fq29_core.hip.h:198 't < 2p with exact limbs'"),
    "sat":        (None, None, 1 << 256, "fq29_core.hip.h:40,54: any 8 x 32-bit words"),
    "canon":      (None, None, P, "bn254_field.hip.h:98 (operands below p: 'a+b < 2^255'); pair261.hip.h:38 'canonical (< p), 2^261-form'"),
    "canon_fr":   (None, None, RFR, "bn254_field.hip.h:98 (the portable templates: operands below the modulus r)"),
    "lt2p":       (None, None, 2 * P, "bn254_field.hip.h:73 'a < 2*MOD'"),
    "to_sat":     (L29_8, L29_8, 169 * P, "fq29_core.hip.h:216-218: a product by R256 < p must come out below 2p: value < 169p = 2^261"),
}
# Value bound of the subtrahend: "at least the value bound of b" (fq29_core.hip.h:171) is short by a hair. The carried result keeps up to 2^232 + 2^207
# in its limbs 0..7 (each up to 2^29 + 7), so a - b + K must be at least that much or limb 8 comes out as -1: with a = 0 the value of b has to
# stay 2^233 (6e-7 p) below K. The model test shows the failure just above this bound (a = 0, b = K - 1 in lazy limbs) and none below; the
# shipped call sites leave whole multiples of p. The comment in the kernel source is left alone (the file is hashed into the committed profiles).
SUB_SLACK = 1 << 233
for _k, _m in K_MULT.items():
    if _k == "K8W":
        continue
    _wide = _k.endswith("W")
    # b of a - b + K: limbs below the bias (carried class 2^29 + 8 for bias 2^30, the uncarried class 'below 2^31' for bias 2^31), value below K
    BOUNDS["sub.b." + _k] = (L31 if _wide else L29_8, L29_8, _m * P - SUB_SLACK,
                             "fq29_core.hip.h:171 'K a biased multiple of p that is at least the value bound of b'; gen_constants.py:%d (%s); "
                             "fq29_core.hip.h:178 'limbs below 2^31'" % (141 + list(K).index(_k), _k))
# u29_sub_raw has no carry pass to bring the 2^bias / 2^29 taken out of K's limb 8 back: limb 8 itself must not go negative, so with a_8 = 0 the value
# of b must stay below K[8] 2^232 (2 2^232 ~ 6e-7 p short of 'the value bound of b'). The shipped call sites are far inside (xyzz29.hip.h:51,72).
for _k in ("K16", "K32"):
    BOUNDS["subraw.b." + _k] = (L29_8, L29_8, K[_k][8] << 232, "fq29_core.hip.h:178-180, tightened to limb 8 of %s (gen_constants.py:126): see the comment above" % _k)


def in_row(slot, row):
    lim, lim8, vb, _ = BOUNDS[row]
    if lim is None:
        return len(slot) == 8 and all(0 <= x < U32 for x in slot) and wval(slot) < vb
    return len(slot) == 9 and all(0 <= x <= lim for x in slot[:8]) and 0 <= slot[8] <= lim8 and (vb is None or val(slot) < vb)


# ---- references ----------------------------------------------------------------------------------------------------------------
def mont_closed(pairs):
    """(sum a_k b_k + m p) / 2^261 with m = -T / p mod 2^261: the unique Montgomery result; limbs 0..7 its 29-bit digits, limb 8 the rest"""
    t = sum(val(a) * val(b) for a, b in pairs)
    m = (-t * PINV261) % R261
    out = (t + m * P) >> 261
    assert (t + m * P) % R261 == 0
    return l29(out), m


def mont_columns(pairs):
    """the column algorithm of u29_mul_ref / u29_sqr_ref (and of the asm streams: the same columns with more products) in unbounded
    integers -> (limbs, largest value a column accumulator held, quotient digits)"""
    acc, peak, m, r = 0, 0, [0] * 9, [0] * 9
    for k in range(17):
        lo = max(0, k - 8)
        for a, b in pairs:
            for i in range(lo, min(k, 8) + 1):
                acc += a[i] * b[k - i]
        if k < 9:
            for i in range(k):
                acc += m[i] * Q29_MOD[k - i]
            m[k] = ((acc & 0xFFFFFFFF) * Q29_INV) & M29
            acc += m[k] * Q29_MOD[0]
        else:
            for i in range(k - 8, 9):
                acc += m[i] * Q29_MOD[k - i]
            r[k - 9] = acc & M29
        peak = max(peak, acc)
        acc >>= 29
    r[8] = acc
    return r, peak, sum(d << (29 * i) for i, d in enumerate(m))


def carry_model(t):
    """u29_carry on integer limbs -> (result limbs as integers, every intermediate)"""
    r = [t[0] & M29] + [(t[i] & M29) + (t[i - 1] >> 29) for i in range(1, 8)] + [t[8] + (t[7] >> 29)]
    return r, list(t[:8]) + r


def sub_model(a, b, k, c=None, carried=True):
    """a - b (- 2c) + K limb-wise, then the carry pass -> (limbs, intermediates that must lie in [0, 2^32))"""
    t = [a[i] - b[i] - (2 * c[i] if c else 0) + k[i] for i in range(9)]
    if not carried:
        return t, t
    r, mid = carry_model(t)      # limb 8 BEFORE the carry may dip below zero by the 2 (4) taken out of K[8]: the u32 wrap is exact, r[8] is what counts
    return r, mid


def _u(l):
    return [x % U32 for x in l] + [0] * (9 - len(l))


def ref_product(n):
    def f(s):
        pairs = [(s[0], s[0])] if n == 0 else [(s[2 * k], s[2 * k + 1]) for k in range(n)]
        return _u(mont_closed(pairs)[0])
    return f


def _mul_const(a, c):
    return mont_closed([(a, c)])[0]


def _pack(t):
    return w32(val(t) % P if val(t) < 2 * P else val(t) - P)


def _fq(fn, mod=P):
    return lambda s: _u(w32(fn(*[wval(x) for x in s]) % mod))


def _inv(x, mod=P):
    return pow(x, -1, mod) if x % mod else 0


def ref_sub(kname, carried=True):
    return lambda s: _u(sub_model(s[0], s[1], K[kname], carried=carried)[0])


R256I, R261I = pow(R256, -1, P), pow(R261, -1, P)
REF = {
    "U29_MUL": ref_product(1), "U29_MUL_REF": ref_product(1), "U29_SQR": ref_product(0), "U29_SQR_REF": ref_product(0),
    "U29_MUL2": ref_product(2), "U29_DOT3": ref_product(3), "U29_DOT4": ref_product(4), "U29_DOT6": ref_product(6),
    "U29_CARRY": lambda s: _u(carry_model(s[0])[0]),
    "U29_SUB_RAW_K16": ref_sub("K16", False), "U29_SUB_RAW_K32": ref_sub("K32", False),
    "U29_SUB3": lambda s: _u(sub_model(s[0], s[1], K["K8W"], c=s[2])[0]),
    "U29_MAYBE_ZERO": lambda s: _u([int(((s[0][0] * Q29_PINV) & M29) <= 17)]),
    "U29_MAYBE_ZERO34": lambda s: _u([int(((s[0][0] * Q29_PINV) & M29) <= 34)]),
    "U29_IS_ZERO": lambda s: _u([int(val(s[0]) % P == 0)]),
    "U29_PACK_CANONICAL": lambda s: _u(_pack(s[0])),
    "U29_FROM_SAT_SHIFT5": lambda s: _u(l29(wval(s[0]) << 5)),
    "U29_FROM_SAT_PLAIN": lambda s: _u(l29(wval(s[0]))),
    "U29_FROM_FQ": lambda s: _u(_mul_const(l29(wval(s[0]) << 5), Q29_ONE)),
    "U29_TO_FQ": lambda s: _u(_pack(_mul_const(s[0], Q29_R256))),
    "U29_TO_SAT": lambda s: _u(_pack(_mul_const(s[0], Q29_R256))),
    "FQ_MUL": _fq(lambda a, b: a * b * R256I), "FQ_SQR": _fq(lambda a: a * a * R256I), "FQ_ADD": _fq(lambda a, b: a + b),
    "FQ_SUB": _fq(lambda a, b: a - b), "FQ_NEG": _fq(lambda a: -a), "FQ_DBL": _fq(lambda a: 2 * a), "FQ_HALF": _fq(lambda a: a * _inv(2)),
    "FQ_REDUCE_ONCE": lambda s: _u(w32(wval(s[0]) - P if wval(s[0]) >= P else wval(s[0]))),
    # Montgomery form in, Montgomery form out: (a R)^-1 R^2 = a^-1 R; 0 -> 0
    "FQ_INV_XGCD": _fq(lambda a: _inv(a) * R256 * R256), "FQ_INV_SAFEGCD": _fq(lambda a: _inv(a) * R256 * R256),
    "FQ_INV_FERMAT": _fq(lambda a: _inv(a) * R256 * R256), "FQ_INV": _fq(lambda a: _inv(a) * R256 * R256),
    "FR_FROM_MONT": _fq(lambda a: a * _inv(R256, RFR), RFR), "FR_MUL": _fq(lambda a, b: a * b * _inv(R256, RFR), RFR),
    "FR_ADD": _fq(lambda a, b: a + b, RFR), "FR_SUB": _fq(lambda a, b: a - b, RFR),
    "TO261": _fq(lambda a: a * 32), "TO256": _fq(lambda a: a * _inv(32)), "CANON_WORDS": _fq(lambda a: a * R261I),
    "FQ_INV261": _fq(lambda a: _inv(a) * R261 * R261),
}
for _k in K_MULT:
    if _k != "K8W":
        REF["U29_SUB_" + _k] = ref_sub(_k)

# ---- the lane-pair tower: records 2r, 2r + 1 are c0, c1 of one Fq2 element; reference over PAIRS of records, in the 2^261 form -----------
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def f2_add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def f2_xi(a): return ((9 * a[0] - a[1]) % P, (9 * a[1] + a[0]) % P)
def f2_inv(a):
    n = _inv(a[0] * a[0] + a[1] * a[1])
    return (a[0] * n % P, -a[1] * n % P)
def f6_mul(a, b):
    m = f2_mul
    return (f2_add(m(a[0], b[0]), f2_xi(f2_add(m(a[1], b[2]), m(a[2], b[1])))), f2_add(f2_add(m(a[0], b[1]), m(a[1], b[0])), f2_xi(m(a[2], b[2]))),
            f2_add(f2_add(m(a[0], b[2]), m(a[1], b[1])), m(a[2], b[0])))


def _pair(fn):
    """fn over plain Fq2 tuples (one per slot) -> the two records' results: operands leave the 2^261 form, the result enters it"""
    def f(s0, s1):
        n = min(len(s0), 6)
        e = [((wval(s0[k]) * R261I) % P, (wval(s1[k]) * R261I) % P) for k in range(n)]
        r = fn(*e)
        return _u(w32(r[0] * R261 % P)), _u(w32(r[1] * R261 % P))
    return f


PAIR_ARITY = {"FQ2_MUL": 2, "FQ2_SQR": 1, "FQ2_MUL_XI": 1, "FQ2_MUL_FQ": 2, "FQ2_INV": 1, "FQ2_CONJ": 1, "FQ2_NEG": 1, "FQ4_SQR_T0": 2, "FQ4_SQR_T1": 2,
              "FQ6_MUL_C0": 6, "FQ6_MUL_C1": 6, "FQ6_MUL_C2": 6}
PAIR_REF = {
    "FQ2_MUL": _pair(f2_mul), "FQ2_SQR": _pair(lambda a: f2_mul(a, a)), "FQ2_MUL_XI": _pair(f2_xi),
    "FQ2_MUL_FQ": _pair(lambda a, k: (a[0] * k[0] % P, a[1] * k[1] % P)),     # each lane multiplies by the factor in ITS slot 1
    "FQ2_INV": _pair(f2_inv), "FQ2_CONJ": _pair(lambda a: (a[0], -a[1] % P)), "FQ2_NEG": _pair(lambda a: (-a[0] % P, -a[1] % P)),
    "FQ4_SQR_T0": _pair(lambda x, y: f2_add(f2_mul(x, x), f2_xi(f2_mul(y, y)))), "FQ4_SQR_T1": _pair(lambda x, y: f2_add(f2_mul(x, y), f2_mul(x, y))),
    "FQ6_MUL_C0": _pair(lambda *e: f6_mul(e[0:3], e[3:6])[0]), "FQ6_MUL_C1": _pair(lambda *e: f6_mul(e[0:3], e[3:6])[1]),
    "FQ6_MUL_C2": _pair(lambda *e: f6_mul(e[0:3], e[3:6])[2]),
}

# slot -> bounds row, per op
PRODUCT_ROWS = {"U29_MUL": ["mul.wide", "mul.narrow"], "U29_MUL_REF": ["mul.wide", "mul.narrow"], "U29_SQR": ["sqr"], "U29_SQR_REF": ["sqr"],
                "U29_MUL2": ["mul2.abd", "mul2.abd", "mul2.c", "mul2.abd"], "U29_DOT3": ["dot"] * 6, "U29_DOT4": ["dot"] * 8, "U29_DOT6": ["dot"] * 12}
ROWS = dict(PRODUCT_ROWS)
ROWS.update({"U29_CARRY": ["carry.in"], "U29_SUB3": ["sub.a", "sub3.b", "sub3.c"], "U29_SUB_RAW_K16": ["subraw.a", "subraw.b.K16"],
             "U29_SUB_RAW_K32": ["subraw.a", "subraw.b.K32"], "U29_MAYBE_ZERO": ["mz18"], "U29_MAYBE_ZERO34": ["mz35"], "U29_IS_ZERO": ["is_zero"],
             "U29_PACK_CANONICAL": ["pack"], "U29_FROM_SAT_SHIFT5": ["sat"], "U29_FROM_SAT_PLAIN": ["sat"], "U29_FROM_FQ": ["canon"],
             "U29_TO_FQ": ["to_sat"], "U29_TO_SAT": ["to_sat"], "FQ_REDUCE_ONCE": ["lt2p"]})
for _k in K_MULT:
    if _k != "K8W":
        ROWS["U29_SUB_" + _k] = ["sub.a", "sub.b." + _k]
for _n, _a in (("FQ_MUL", 2), ("FQ_SQR", 1), ("FQ_ADD", 2), ("FQ_SUB", 2), ("FQ_NEG", 1), ("FQ_DBL", 1), ("FQ_HALF", 1), ("FQ_INV_XGCD", 1),
               ("FQ_INV_SAFEGCD", 1), ("FQ_INV_FERMAT", 1), ("FQ_INV", 1), ("TO261", 1), ("TO256", 1), ("CANON_WORDS", 1), ("FQ_INV261", 1)):
    ROWS[_n] = ["canon"] * _a
for _n, _a in (("FR_FROM_MONT", 1), ("FR_MUL", 2), ("FR_ADD", 2), ("FR_SUB", 2)):
    ROWS[_n] = ["canon_fr"] * _a
for _n, _a in PAIR_ARITY.items():
    ROWS[_n] = ["canon"] * _a


# ---- operand families ----------------------------------------------------------------------------------------------------------
REDRAW_CAP = 200
redraws_peak = [0]          # the most draws any chosen-quotient record needed (the model test asserts the cap is never hit)


def _rng(name):
    return random.Random(0x6b65616b ^ zlib.crc32(name.encode()))


def canonical_edges(mod=P):
    """(tag, residue) list: the canonical edge family"""
    e = [("0", 0), ("1", 1), ("2", 2), ("p-1", mod - 1), ("p-2", mod - 2), ("(p-1)/2", (mod - 1) // 2), ("(p+1)/2", (mod + 1) // 2),
         ("R256", R256 % mod), ("R256^2", R256 * R256 % mod), ("R261", R261 % mod), ("R261^2", R261 * R261 % mod)]
    for k in sorted({29 * i for i in range(1, 9)} | {32 * j for j in range(1, 8)}):
        e += [("2^%d" % k, 1 << k), ("2^%d-1" % k, (1 << k) - 1)]
    e += [("limb%d" % i, M29 << (29 * i)) for i in range(8)] + [("limb8", ((mod >> 232) - 1) << 232)]
    e += [("word%d" % j, 0xFFFFFFFF << (32 * j)) for j in range(7)] + [("word7", ((mod >> 224) - 1) << 224)]
    e.append(("ones29", val([M29] * 8 + [(mod >> 232) - 1])))

    def once(v):
        v &= (1 << 254) - 1
        return v - mod if v >= mod else v
    e += [("pick3", once(wval([0xFFFFFFFF] * 7 + [0x2FFFFFFF]))), ("pick4", 3), ("pick5", once(wval([0, 0xFFFFFFFF] * 3 + [0, 0x1FFFFFFF])))]
    assert all(0 <= v < mod for _, v in e)
    return e


def rand_canon(rng, mod=P):
    return rng.randrange(mod)


def lazy_limbs(rng, lim, lim8, bound, extra=()):
    """limbs 0..7 from the edge set (not by reduction), limb 8 so that the value lies just below `bound` (within 2^232 of it)"""
    pool = [0, 1, M29, 1 << 29, L29_8] + list(extra)
    low = [min(lim, rng.choice(pool) if rng.random() < 0.7 else rng.randrange(lim + 1)) for _ in range(8)]
    top = lim8 if bound is None else min(lim8, max(0, (bound - 1 - val(low + [0])) >> 232))
    return low + [top]


def _value_bounds(row):
    lim, lim8, vb, _ = BOUNDS[row]
    allowed = (lim8 + 1) << 232
    want = [vb] if vb is not None else [2 * P, 20 * P, 32 * P, None]      # product output | the lazy class | from_sat_shift5 | limb 8 at its budget
    return [b for b in want if b is None or b <= allowed] or [None]


def gen_product(name):
    """families of the product streams -> [(tag, slots)]"""
    rows, rng, out = PRODUCT_ROWS[name], _rng(name), []
    nslots, sqr = len(rows), len(rows) == 1
    edges = canonical_edges()
    extra = {"mul.wide": [L30_16], "mul2.c": [L15_30]}

    def lazy(row, bound="cycle"):
        lim, lim8, _, _ = BOUNDS[row]
        bs = _value_bounds(row)
        return lazy_limbs(rng, lim, lim8, rng.choice(bs) if bound == "cycle" else bound, extra.get(row, ()))

    # canonical edges: every edge in every slot once, the other slots random residues or other edges
    for j, (tag, v) in enumerate(edges):
        for s in range(nslots if nslots <= 2 else 1):
            slots = [l29(edges[(j * 7 + 3 * t) % len(edges)][1]) if (j + t) % 3 == 0 else l29(rand_canon(rng)) for t in range(nslots)]
            slots[(s + j) % nslots] = l29(v)
            out.append(("edge:%s@%d" % (tag, (s + j) % nslots), slots))
    # lazy representations at the documented limb classes and value bounds
    for _ in range(192):
        out.append(("lazy", [lazy(r) for r in rows]))
    # column budget: every limb of every operand at its maximum at once (all nine; and with limb 8 at the class's largest value bound)
    out.append(("budget", [[BOUNDS[r][0]] * 8 + [BOUNDS[r][1]] for r in rows]))
    out.append(("budget-low8", [[BOUNDS[r][0]] * 8 + [0] for r in rows]))
    # chosen quotient digits
    if sqr:
        out.append(("m=0", [l29(rng.randrange(1 << 100) << 131)]))
    else:
        last_row = rows[-1]
        b_bound = min(20 * P, (BOUNDS[last_row][1] + 1) << 232)
        for kind in ["m=0"] * 4 + ["m=ones"] * 24:
            for draw in range(1, REDRAW_CAP + 1):
                slots = [l29(rand_canon(rng) + rng.randrange(2) * P) for _ in range(nslots)]
                a = val(slots[-2]) | 1
                slots[-2] = l29(a)
                if kind == "m=0":
                    m = 0
                else:
                    m = (R261 - 1) - ((M29 - rng.randrange(1 << 29)) << (29 * rng.randrange(9)))
                rest = sum(val(slots[2 * k]) * val(slots[2 * k + 1]) for k in range(nslots // 2 - 1))
                b = ((-m * P - rest) * pow(a, -1, R261)) % R261
                if b < b_bound:
                    break
            else:
                draw = REDRAW_CAP + 1
            redraws_peak[0] = max(redraws_peak[0], draw)
            if draw > REDRAW_CAP:
                continue
            slots[-1] = l29(b)
            pairs = [(slots[2 * k], slots[2 * k + 1]) for k in range(nslots // 2)]
            assert mont_closed(pairs)[1] == m
            out.append((kind, slots))
        # m = 0 without a search: a b == 0 (mod 2^261) by the powers of two (every other product zero)
        z = [[0] * 9 for _ in range(nslots)]
        z[-2], z[-1] = l29(rng.randrange(1, 1 << 100) << 130), l29(rng.randrange(1, 1 << 100) << 131)
        out.append(("m=0:pow2", z))
    # chosen results: 0, p - 1, p, and within 2^29 of the output bound 2p
    if sqr:
        out += [("result=0", [[0] * 9]), ("result=p", [l29(P)])]
        near = [2 * P - 1 - rng.randrange(1 << 29) for _ in range(64)]
        near = [v for v in near if pow(v * R261 % P, (P - 1) // 2, P) == 1][:2]          # the targets that are squares (about half)
        for tag, target in [("result=p-1", P - 1)] + [("result~2p", v) for v in near]:
            # a^2 == target 2^261 (mod p) when that is a square (p == 3 mod 4), a lifted by multiples of p until the window holds the target
            rhs = target * R261 % P
            a0 = pow(rhs, (P + 1) // 4, P)
            if a0 * a0 % P != rhs:
                continue
            for j in range(40):
                for a in (a0 + j * P, P - a0 + j * P):
                    if a < 20 * P and mont_closed([(l29(a), l29(a))])[0] == l29(target):
                        out.append((tag, [l29(a)]))
                        break
                else:
                    continue
                break
    else:
        out += [("result=0", [[0] * 9 for _ in range(nslots)]), ("result=p", [l29(P) if t >= nslots - 2 else [0] * 9 for t in range(nslots)])]
        for tag, target in (("result=p-1", P - 1), ("result=p", P), ("result~2p", 2 * P - 1 - rng.randrange(1 << 29)), ("result~2p'", 2 * P - 1 - rng.randrange(1 << 29))):
            slots = [l29(rand_canon(rng)) for _ in range(nslots)]
            a = (rand_canon(rng) + 13 * P) | 1          # a b / 2^261 must reach up to 2p: a ~ 13p .. 14p, b up to 20p
            slots[-2] = l29(a)
            rest = sum(val(slots[2 * k]) * val(slots[2 * k + 1]) for k in range(nslots // 2 - 1))
            b0 = ((target * R261 - rest) * pow(a, -1, P)) % P
            for j in range(20):
                slots[-1] = l29(b0 + j * P)
                if mont_closed([(slots[2 * k], slots[2 * k + 1]) for k in range(nslots // 2)])[0] == l29(target):
                    out.append((tag, [list(x) for x in slots]))
                    break
    # random fill
    for _ in range(256):
        out.append(("random", [l29(rng.randrange(2 * P)) for _ in rows]))
    return out


def gen_sub(name):
    rows, rng, out = ROWS[name], _rng(name), []
    three = name == "U29_SUB3"
    (alim, alim8, abound, _), (blim, blim8, bbound, _) = BOUNDS[rows[0]], BOUNDS[rows[1]]
    zero = [0] * 9

    def top(low, bound, lim8):
        return low + [min(lim8, max(0, (bound - 1 - val(low + [0])) >> 232))]
    cs = [zero, l29(2 * P - 1), top([BOUNDS["sub3.c"][0]] * 8, 2 * P, L29_8)] if three else [None]
    for c in cs:
        tail = [c] if three else []
        sfx = "" if not three else ":c=%d" % cs.index(c)
        eq = lazy_limbs(rng, min(alim, blim), min(alim8, blim8), min(abound, bbound))
        out.append(("a=b" + sfx, [eq, list(eq)] + tail))
        out.append(("a=0,b=bound" + sfx, [zero, l29(bbound - 1)] + tail))
        out.append(("a=0,b=bound,limbs max" + sfx, [zero, top([blim] * 8, bbound, blim8)] + tail))
        out.append(("a=bound,b=0" + sfx, [l29(abound - 1), zero] + tail))
        out.append(("a limbs max,b=0" + sfx, [top([alim] * 8, abound, alim8), zero] + tail))
        out.append(("a=0,b limbs max" + sfx, [zero, top([blim] * 8, bbound, blim8)] + tail))
        out.append(("both limbs max" + sfx, [top([alim] * 8, abound, alim8), top([blim] * 8, bbound, blim8)] + tail))
    for tag, v in canonical_edges():
        out.append(("edge:" + tag, [l29(v), l29(rand_canon(rng))] + ([l29(rand_canon(rng))] if three else [])))
        out.append(("edge:b=" + tag, [l29(rand_canon(rng)), l29(v)] + ([l29(v)] if three else [])))
    for _ in range(192):
        a = lazy_limbs(rng, alim, alim8, rng.choice([2 * P, abound]), [L30_16])
        b = lazy_limbs(rng, blim, blim8, rng.choice([min(2 * P, bbound), bbound]), [blim, blim - 1])
        out.append(("lazy", [a, b] + ([lazy_limbs(rng, L29_8, L29_8, 2 * P)] if three else [])))
    for _ in range(128):
        out.append(("random", [l29(rng.randrange(2 * P)) for _ in rows]))
    return out


def gen_misc(name):
    rng, out, row = _rng(name), [], ROWS[name][0]
    if name == "U29_CARRY":
        out.append(("all max", [[U32 - 1] * 8 + [U32 - 8]]))
        out.append(("zero", [[0] * 9]))
        for i in range(8):
            out += [("limb%d=2^32-1" % i, [[U32 - 1 if j == i else 0 for j in range(9)]]), ("limb%d=2^29" % i, [[1 << 29 if j == i else M29 for j in range(9)]])]
        for _ in range(256):
            out.append(("random", [[rng.choice([0, M29, 1 << 29, L31, U32 - 1, rng.randrange(U32)]) for _ in range(8)] + [rng.randrange(U32 - 8)]]))
    elif name in ("U29_MAYBE_ZERO", "U29_MAYBE_ZERO34"):
        kmax = 17 if name == "U29_MAYBE_ZERO" else 34
        for k in range(kmax + 1):
            v = k * P
            out.append(("%dp exact" % k, [l29(v)]))
            # other limb representations of the same value with limb 0 exact: move 2^29 between neighbouring limbs, and limbs 1.. as one carry-free dump
            l = l29(v)
            for i in range(1, 8):
                if l[i + 1] > 0:
                    m = list(l); m[i] += 1 << 29; m[i + 1] -= 1
                    out.append(("%dp lazy limb %d" % (k, i), [m]))
        for _ in range(128):
            out.append(("random", [l29(rng.randrange(BOUNDS[row][2]))]))
    elif name == "U29_IS_ZERO":
        for k in range(101):
            for d in (0, 1, -1):
                if k * P + d >= 0:
                    out.append(("%dp%+d" % (k, d), [l29(k * P + d)]))
        for k in (0, 1, 2, 50, 100):      # the same multiples with uncarried limbs
            l = l29(k * P)
            for i in range(0, 8):
                if l[i + 1] > 0:
                    m = list(l); m[i] += 1 << 29; m[i + 1] -= 1
                    out.append(("%dp lazy limb %d" % (k, i), [m]))
        for _ in range(64):
            out.append(("random", [l29(rng.randrange(100 * P))]))
    elif name == "U29_PACK_CANONICAL":
        for t in (0, 1, P - 1, P, P + 1, 2 * P - 1):
            out.append(("t=%s" % {0: "0", 1: "1", P - 1: "p-1", P: "p", P + 1: "p+1", 2 * P - 1: "2p-1"}[t], [l29(t)]))
        out += [("edge:" + tag, [l29(v)]) for tag, v in canonical_edges()] + [("edge+p:" + tag, [l29(v + P)]) for tag, v in canonical_edges()]
        out += [("random", [l29(rng.randrange(2 * P))]) for _ in range(512)]
    elif name in ("U29_FROM_SAT_SHIFT5", "U29_FROM_SAT_PLAIN"):
        out += [("edge:" + tag, [w32(v)]) for tag, v in canonical_edges()]
        out += [("all ones", [[0xFFFFFFFF] * 8]), ("top bit", [w32(1 << 255)])] + [("word%d ones" % j, [w32(0xFFFFFFFF << (32 * j))]) for j in range(8)]
        out += [("random", [w32(rng.randrange(1 << 256))]) for _ in range(256)]
    elif name in ("U29_TO_FQ", "U29_TO_SAT"):
        lim, lim8, vb, _ = BOUNDS[row]
        out += [("edge:" + tag, [l29(v)]) for tag, v in canonical_edges()]
        out += [("kp", [l29(k * P)]) for k in (1, 2, 31, 32, 168)] + [("kp-1", [l29(k * P - 1)]) for k in (1, 2, 32, 169)]
        out += [("lazy", [lazy_limbs(rng, lim, lim8, rng.choice([2 * P, 20 * P, 32 * P, vb]))]) for _ in range(192)]
        out.append(("limbs max", [[lim] * 8 + [(vb - 1 - val([lim] * 8 + [0])) >> 232]]))
        out += [("random", [l29(rng.randrange(2 * P))]) for _ in range(128)]
    elif name == "FQ_REDUCE_ONCE":
        out += [("edge:" + tag, [w32(v)]) for tag, v in canonical_edges()] + [("edge+p:" + tag, [w32(v + P)]) for tag, v in canonical_edges()]
        out += [("random", [w32(rng.randrange(2 * P))]) for _ in range(256)]
    else:
        raise KeyError(name)
    return out


_SLOW = {"FQ_INV_XGCD", "FQ_INV_SAFEGCD", "FQ_INV_FERMAT", "FQ_INV", "FQ_INV261", "FQ2_INV"}


def gen_saturated(name):
    rows, rng, out = ROWS[name], _rng(name), []
    mod = RFR if rows[0] == "canon_fr" else P
    edges = canonical_edges(mod)
    for j, (tag, v) in enumerate(edges):
        for s in range(len(rows)):
            slots = [w32(edges[(5 * j + 3) % len(edges)][1] if j % 2 else rand_canon(rng, mod)) for _ in rows]
            slots[s] = w32(v)
            out.append(("edge:%s@%d" % (tag, s), slots))
    if len(rows) == 2:      # edge against edge: sums and differences that land on 0, p - 1, p
        for tag, x, y in (("x+y=p", 5, mod - 5), ("x+y=p-1", 5, mod - 6), ("x+y=p+1", 6, mod - 5), ("x=y", mod - 7, mod - 7), ("x-y=-1", 8, 9), ("x-y=1", 9, 8),
                          ("(p-1)^2", mod - 1, mod - 1), ("half+half", (mod + 1) // 2, (mod + 1) // 2), ("half+half'", (mod - 1) // 2, (mod + 1) // 2)):
            out.append((tag, [w32(x), w32(y)]))
    out += [("random", [w32(rand_canon(rng, mod)) for _ in rows]) for _ in range(128 if name in _SLOW else 512)]
    return out


def gen_pair(name):
    """lane-pair ops -> [(tag, slots of the c0 record, slots of the c1 record)]"""
    n, rng, out = PAIR_ARITY[name], _rng(name), []
    edges = canonical_edges()
    r = lambda: w32(rand_canon(rng))
    for j, (tag, v) in enumerate(edges):
        for comp in (0, 1):
            s = [[r() for _ in range(n)], [r() for _ in range(n)]]
            s[comp][j % n] = w32(v)
            out.append(("edge:%s@c%d.%d" % (tag, comp, j % n), s[0], s[1]))
        out.append(("edge both:" + tag, [w32(v)] * n, [w32(edges[(3 * j + 1) % len(edges)][1])] * n))
    z = w32(0)
    out.append(("zero", [z] * n, [z] * n))
    out.append(("c1=0", [r() for _ in range(n)], [z] * n))
    out.append(("c0=0", [z] * n, [r() for _ in range(n)]))
    out.append(("c0=c1", *(lambda s: (s, [list(x) for x in s]))([r() for _ in range(n)])))
    out.append(("all p-1", [w32(P - 1)] * n, [w32(P - 1)] * n))
    for _ in range(64 if name in _SLOW else 192):
        a, b = [r() for _ in range(n)], [r() for _ in range(n)]
        if name == "FQ2_MUL_FQ" and rng.random() < 0.5:
            b[1] = list(a[1])          # the tower's use: the same Fq factor in both lanes
        out.append(("random", a, b))
    return out


def generate(name):
    """-> (tags, records): one tag and one list of slots per record, in the order the device gets them"""
    if name in PAIR_REF:
        tags, recs = [], []
        for tag, s0, s1 in gen_pair(name):
            tags += [tag + " (c0)", tag + " (c1)"]
            recs += [s0, s1]
        return tags, recs
    if name in PRODUCT_ROWS:
        fam = gen_product(name)
    elif name.startswith("U29_SUB"):
        fam = gen_sub(name)
    elif ROWS[name][0] in ("canon", "canon_fr"):
        fam = gen_saturated(name)
    else:
        fam = gen_misc(name)
    return [t for t, _ in fam], [s for _, s in fam]


def expected(name, recs):
    """the nine output words of every record"""
    if name in PAIR_REF:
        out = []
        for i in range(0, len(recs), 2):
            out += list(PAIR_REF[name](recs[i], recs[i + 1]))
        return out
    return [REF[name](s) for s in recs]


def pack_records(recs):
    """records -> the n x 12 x 9 uint32 array of keaki_hip_selftest_field_ops"""
    import numpy as np
    a = np.zeros((len(recs), 12, 9), np.uint32)
    for i, slots in enumerate(recs):
        for s, limbs in enumerate(slots):
            a[i, s, :len(limbs)] = limbs
    return a


ALL_OPS = sorted(set(REF) | set(PAIR_REF))
