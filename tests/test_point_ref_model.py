"""CPU checks of tests/point_ref.py: the reference, bounds table and operand families that tests/test_gpu_point_ops.py feeds to
keaki_hip_selftest_point_ops. Nothing here touches the device code; what is pinned is that the GPU test asks the right question: every op has a
reference and families of several kinds, every operand lies inside its callee's documented bound (BOUNDS names an existing source line for each),
the named corners are there, the zero tests' arguments take every multiple of p they can, the GLV list reaches every digit class. The limb-exact
models of the tree (keaki_amd/csrc/models/model_jac29.py, model_g2_add29.py) and a limb-exact statement of xyzz29.hip.h written here from
field_ref's column model stand in for the device: their results on the same family operands, corners included, must pass point_ref.judge without
tripping a model's own overflow assertions -- and three deliberately wrong variants must fail it."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402
import point_ref as pr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

P = pr.P
CODES = khip.point_op_codes()
GEOMETRY = ("COUNT", "SLOTS", "SLOT_WORDS", "FLAG_SLOT", "OUT_SLOTS", "OUT_FLAG_SLOT", "MAX_RECORDS", "FIRST_G2")
_FAM = {}


def family(name):
    if name not in _FAM:
        _FAM[name] = pr.generate(name)
    return _FAM[name]


def _model(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(pr.ROOT, "keaki_amd", "csrc", "models", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.ONE = m.limbs(m.R261 % m.P)
    return m


def test_op_list_is_the_headers():
    ops = sorted((k for k in CODES if k not in GEOMETRY), key=lambda k: CODES[k])
    assert ops == pr.OPS and [CODES[k] for k in ops] == list(range(CODES["COUNT"])) and CODES["COUNT"] == 37
    assert (CODES["SLOTS"], CODES["SLOT_WORDS"], CODES["FLAG_SLOT"], CODES["OUT_SLOTS"], CODES["OUT_FLAG_SLOT"], CODES["MAX_RECORDS"]) == \
        (pr.SLOTS, pr.SW, pr.FLAG_SLOT, pr.OUT_SLOTS, pr.OUT_FLAG_SLOT, pr.MAX_RECORDS)
    assert CODES["FIRST_G2"] == CODES["X29G2_ADD_MIXED"] and all(n.startswith("X29G2") or n.endswith("FQ2") for n in ops[CODES["FIRST_G2"]:])
    # the two older probes keep their enums
    assert khip.field_op_codes()["COUNT"] == 62 and khip.tower_op_codes()["COUNT"] == 29


def test_bounds_rows_name_existing_source_lines():
    for key, (mult, tight, path, line, words) in pr.BOUNDS.items():
        text = open(os.path.join(pr.ROOT, path)).read().split("\n")
        assert words in text[line - 1], (key, path, line, words, text[line - 1])
        assert 0 < pr.bound(key) <= 32 * P and (tight in (0, 1))
    assert pr.bound("j29.madd.y1.tight") == 4 * P - fr.SUB_SLACK and pr.bound("g2.acc.x.tight") == 2 * P - fr.SUB_SLACK


@pytest.mark.parametrize("name", pr.OPS)
def test_every_op_has_families_inside_its_bounds(name):
    tags, recs = family(name)
    assert 1 <= len(recs) <= (1024 if name in pr.LADDER_OPS else pr.MAX_RECORDS)
    kinds = pr.family_kinds(tags)
    assert len(kinds) >= 2, kinds
    for t, r in zip(tags, recs):
        assert not pr.operand_errors(name, r), (t, pr.operand_errors(name, r))
    if name in pr.UNIFORM_OPS:
        assert len(recs) % 64 == 0 and len(recs) // 64 >= 16
    if name in ("LADDER_UNIFORM", "LADDER_MUL2"):
        assert len(recs) == 16 * 64
        for w in range(0, len(recs), 64):          # 64 different points per scalar
            assert len({tuple(map(tuple, r[0:3])) for r in recs[w:w + 64]}) == 64
    elif name not in pr.LADDER_OPS and name != "GLV_UNIFORM_DIGITS":          # the ladders' 1,024 records and the uniform forms' 16 to 60 waves go to the scalar list
        assert 256 <= sum(t == "random" or t == "canonical:random" for t in tags) <= 512
    assert len(pr.LOGS[name]) == len(recs)


def test_named_corners_are_present():
    def has(name, *parts):
        return any(all(p in t for p in parts) for t in family(name)[0])
    for name in ("X29_ADD", "X29_DBL", "J29_DBL", "J29_MADD", "J29_ADDSUB", "X29G2_ADD_MIXED", "X29G2_ADD", "X29G2_DBL"):
        for style in ("exact", "lazy"):
            assert has(name, "corner:" + style, ":all") and has(name, "corner:" + style, ":0")
    assert has("X29_DBL", "Y=32p-1") and has("J29_MADD", "Y1 at bound", "S2==0") and has("J29_MADD", "running set")
    assert has("X29G2_ADD_MIXED", "acc at bound, table 32(p-1)") and has("X29_ADD", "canonical:all p-1")
    for name in ("J29_BUILD_TABLE", "J29_BUILD_TABLE_ODD", "J29_BUILD_PAIR"):          # the saturated WORDS at p - 1 and 1, as u29_from_fq reads them
        tags, recs = family(name)
        for v, t in ((P - 1, "p-1"), (1, "1")):
            for c in range(3):
                r = recs[tags.index("corner:words %s in %s" % (t, "xyz"[c]))]
                assert fr.wval(r[c]) == v and (name != "J29_BUILD_PAIR" or fr.wval(r[3 + c]) == v)
            r = recs[tags.index("corner:words %s in all" % t)]
            assert all(fr.wval(r[c]) == v for c in range(6 if name == "J29_BUILD_PAIR" else 3))
    for name in ("LADDER_FIXED", "LADDER_GTAB"):          # every point, the identity included, with every scalar
        tags = family(name)[0]
        for t, _ in pr.ladder_scalars():
            for pt in ("G", "G z", "7G z", "rand z", "identity"):
                assert "%s:%s" % (t, pt) in tags
    for name in ("X29_ADD", "J29_MADD", "J29_ADDSUB", "X29G2_ADD", "X29G2_ADD_MIXED"):
        for br in ("equal", "opposite", "P+2P", "2P+P"):
            for zk in pr.Z_KINDS:
                assert has(name, "branch:" + br, zk)
    for name in ("X29_ADD", "X29G2_ADD", "X29G2_ADD_MIXED"):
        assert has(name, "identity:a") and has(name, "identity:b") and has(name, "identity:both")
    # the corner records really sit at the bound: value within 2^232 of it, and for the lazy style some limb above 2^29
    tags, recs = family("J29_MADD")
    i = tags.index("corner:lazy:1")
    assert pr.bound("j29.madd.y1.tight") - fr.val(recs[i][1]) <= 1 << 232 and max(recs[i][1][:8]) > fr.M29
    tags, recs = family("X29_ADD")
    assert fr.val(recs[tags.index("corner:exact:0")][0]) == 32 * P - 1


@pytest.mark.parametrize("name", sorted(pr.ZERO_TEST_RANGE))
def test_zero_test_arguments_take_every_multiple(name):
    tags, recs = family(name)
    for kind in ("equal", "opposite"):
        got = sorted({pr.zero_test_multiples(name, r) for t, r in zip(tags, recs) if t.startswith("zerotest:" + kind)})
        assert got == list(pr.ZERO_TEST_RANGE[name]), (kind, got)


def test_glv_list_reaches_every_digit_class():
    named, built, dropped = pr.glv_scalars()
    assert len(built) >= 100 and dropped * 4 <= len(built) + dropped
    names = {t for t, _ in named}
    assert {"0", "1", "2", "r-1", "r-2", "lambda", "lambda+1", "lambda-1", "r-lambda", "2lambda", "lambda^2", "2^127", "2^128-1", "2^128", "2^253+5"} <= names
    assert sum(t.startswith("c1 ") for t in names) >= 8 and sum(t.startswith("c2 ") for t in names) >= 8
    for i, g in ((1, pr.GLV_G1), (2, pr.GLV_G2)):          # the two sides of a step differ by one in c_i
        steps = [k for t, k in named if t.startswith("c%d steps" % i)]
        assert steps and all(((k * g) >> 256) == (((k - 1) * g) >> 256) + 1 for k in steps)
    fixed, naf, top = set(), set(), set()
    for _, k in built:
        for h in pr.glv_ref(k):
            assert abs(h) < 1 << 127
            d = pr.fixed_ref(abs(h))[0]
            fixed |= set(d[:31]); top.add(d[32]); naf |= set(pr.wnaf5_ref(abs(h)))
    # the recoding takes n > 8 to n - 16: the digits are -7 .. 8, never -8 (the header's [-8, 8] is an enclosure). Below 2^127 the top nibble is at most 7 and
    # 7 + 1 is not above 8: digit 32 stays clear on every magnitude glv_decompose can return; GLV_FIXED_DIGITS reaches it on 128-bit words.
    assert fixed == set(range(-7, 9)) and top == {0}
    assert naf == set(range(-15, 16, 2)) | {0}
    assert all(pr.fixed_ref(m)[0][32] == 0 for m in ((1 << 127) - 1, int("7" + "9" * 31, 16)))
    tags, recs = family("GLV_FIXED_DIGITS")
    assert {pr.fixed_ref(pr.val32(r[0][:5]))[0][32] for r in recs} == {0, 1}
    # the worst magnitudes stay below 2^127 (the floors in g1, g2 widen the cell by at most 13 %)
    for _, k in named + built:
        k1, k2 = pr.glv_ref(k)
        assert (k1 + k2 * pr.LAMBDA - k) % pr.RFR == 0 and abs(k1) < 1 << 127 and abs(k2) < 1 << 127


def test_no_scalar_makes_a_single_ladder_meet_its_table():
    """jac29.hip.h:175 expects `special` inside a ladder 'only for k = r - 2'. That was the plain ladder: after the GLV split the running point never lands on the
    entry being added, for r - 2, for the other candidates r - 2d and for everything else in the list (the ladder on integers says so). The branch is reached
    by J29_MADD itself and, inside a ladder, by LADDER_MUL2's lanes with B = A, B = -A and kA A + kB B = identity."""
    ks = dict(pr.ladder_scalars())
    assert ks["named:r-2"] == pr.RFR - 2 and sum(t.startswith("candidate:") for t in ks) == 10
    for t, k in ks.items():
        assert pr.fixed_ladder_meetings(k) == [], t
    rng = pr._rng("meet")
    assert not any(pr.fixed_ladder_meetings(rng.randrange(pr.RFR)) for _ in range(200))
    tags = family("LADDER_MUL2")[0]
    assert all(any(t.endswith(rel) for t in tags) for rel in ("B=A", "B=-A", "B=lambda A", "sum=identity"))
    assert {r[pr.FLAG_SLOT][2] for r in family("LADDER_MUL2")[1]} == {0, 1}          # negB both ways


def test_digit_references_reconstruct():
    rng = pr._rng("digits")
    for _ in range(300):
        m = rng.randrange(1 << 127)
        d = pr.fixed_ref(m)[0]
        assert sum(x << (4 * j) for j, x in enumerate(d)) == m and all(-7 <= x <= 8 for x in d)
        w = pr.wnaf5_ref(m)
        nz = [i for i, x in enumerate(w) if x]
        assert sum(x << i for i, x in enumerate(w)) == m and all(x % 2 and abs(x) <= 15 for x in w if x) and all(j - i >= 5 for i, j in zip(nz, nz[1:]))


def test_packing_round_trips():
    for name in ("X29_ADD", "X29G2_ADD_MIXED", "LADDER_MUL2", "GLV_DECOMPOSE"):
        recs = family(name)[1][:40]
        a = pr.pack_records(recs)
        assert a.shape == (len(recs), pr.SLOTS, pr.SW) and a.dtype == np.uint32
        assert pr.unpack_records(a) == recs
    assert pr.dl(pr.lz(12345, 7)) == 12345 and pr.ds(pr.sat(P - 1)) == P - 1 and pr.dl(pr.sh5(77)) == 77


def test_reference_agrees_with_the_oracle():
    """ct_add (the reference behind every addition op), the generic double-and-add, the Jacobian _jmul and mul_g against oracle/bn254_py.py, which shares nothing
    with point_ref; and the logs the families carry: the judge's own expectation of a record with known logs is (log) G of the oracle"""
    pr.oracle_point(1)
    m = pr._ORACLE[0]
    wrap = lambda pt: None if pt is None else ((pt[0],), (pt[1],))
    rng = pr._rng("oracle")
    logs = [1, 2, 3, pr.RFR - 1, pr.RFR - 2, pr.LAMBDA] + [rng.randrange(1, pr.RFR) for _ in range(10)]
    pts = {k: wrap(m.g1_mul(m.G1_GEN, k)) for k in logs}
    assert pts[1] == pr.G1 and all(m.g1_is_on_curve((p[0][0], p[1][0])) for p in pts.values())
    for i, ka in enumerate(logs):
        kb = logs[(5 * i + 1) % len(logs)]
        for a, b in ((ka, kb), (ka, ka), (ka, -ka), (ka, 0), (0, kb)):
            pa = pts[ka] if a else None
            pb = None if not b else pts[kb] if b == kb else pts[ka] if b == ka else pr.ct_neg(pts[ka])
            assert pr.ct_add(pa, pb) == wrap(m.g1_add(None if pa is None else (pa[0][0], pa[1][0]), None if pb is None else (pb[0][0], pb[1][0])))
            assert pr.ct_add(pa, pb) == pr.oracle_point(a + b)
        s = rng.randrange(pr.RFR) if i % 2 else rng.randrange(1 << 20)
        assert pr.ct_mul_generic(s, pts[ka]) == pr.ct_mul(s, pts[ka]) == pr.oracle_point(s * ka) and pr.mul_g(ka) == pts[ka]
    assert pr.mul_g(pr.RFR) is None and pr.ct_mul_generic(pr.RFR, pr.G1) is None and pr.oracle_point(0) is None
    # the families' logs: what the judge expects of the record is what the oracle says
    for name in pr.OPS:
        tags, recs = family(name)
        have = [i for i, l in enumerate(pr.LOGS[name]) if l is not None]
        assert bool(have) == (name in pr.LADDER_OPS or name.startswith("J29_BUILD") or any(t.startswith("logs:") for t in tags)), name
        for i in have[::max(1, len(have) // 12)]:
            r, lg = recs[i], pr.LOGS[name][i]
            if name in pr.LADDER_OPS:
                first = recs[i // 64 * 64] if name in pr.UNIFORM_OPS else r
                a = pr.img_jac([pr.el_sat(r, k, 1) for k in range(3)])
                if name == "LADDER_MUL2":
                    b = pr.ct_mul(pr._scalar_of(first, 7), pr.img_jac([pr.el_sat(r, 3 + k, 1) for k in range(3)]))
                    want = pr.ct_add(pr.ct_mul(pr._scalar_of(first, 6), a), pr.ct_neg(b) if first[pr.FLAG_SLOT][2] else b)
                else:
                    want = pr.ct_mul(pr._scalar_of(first, 3), a)
                assert [want] == [pr.oracle_point(k) for k in lg], (name, tags[i])
            elif name.startswith("J29_BUILD"):
                a = pr.img_jac([pr.el_sat(r, k, 1) for k in range(3)])
                assert pr.ct_mul(3, a) == pr.oracle_point(lg[1] if name != "J29_BUILD_TABLE" else lg[2]), (name, tags[i])


# ---- the limb-exact models in the device's place --------------------------------------------------------------------------------------------
def _out(slots, flags=()):
    o = [[0] * pr.SW for _ in range(pr.OUT_SLOTS)]
    for i, s in enumerate(slots):
        o[i][:len(s)] = s
    o[pr.OUT_FLAG_SLOT][:len(flags)] = [int(f) for f in flags]
    return o


def _judge_all(name, run, skip=lambda t: False, least=300):
    tags, recs = family(name)
    n = 0
    for t, r in zip(tags, recs):
        if skip(t):
            continue
        o = run(r)
        v = pr.judge(name, r, o)
        assert not v.errors, (name, t, v.errors)
        lg = pr.LOGS[name][tags.index(t)] if t.startswith("logs:") else None
        if lg is not None:
            assert not pr.oracle_errors(name, o, lg), (name, t)
        n += 1
    assert n > least


def test_model_jac29_agrees_with_the_reference_on_the_families():
    """a corner that trips one of the model's overflow assertions is a finding before any GPU run"""
    m = _model("model_jac29")
    zero = lambda r, i: fr.val(r[i]) % P == 0

    def dbl(r):
        return _out(m.j29_dbl(tuple(r[0:3])))

    def madd(r):
        a = pr.img_jac([pr.el_lazy(r, k, 1) for k in range(3)])
        b = (pr.el_lazy(r, 3, 1), pr.el_lazy(r, 4, 1))
        res = m.j29_madd(tuple(r[0:3]), r[3], r[4])
        if res is None:
            return _out(r[0:3], [1 if a == b else 2])
        return _out(list(res[0]) + [res[1]], [0])

    def addsub(r):
        res = m.j29_addsub(tuple(r[0:3]), tuple(r[3:6]))
        return _out([], [0]) if res is None else _out(list(res[0]) + list(res[1]), [1])
    _judge_all("J29_DBL", dbl)
    _judge_all("J29_MADD", madd)
    _judge_all("J29_ADDSUB", addsub)
    # the table builds: the model's tables (it has no beta x: one more product by beta)
    beta = fr._arr(pr._GLV, "BETA29", 9)

    def from_fq(r, s):
        return tuple(m.limbs(fr.wval(r[s + k]) * 32 % P) for k in range(3))          # u29_from_fq: the reduced 2^261 form, exact limbs

    def flat(tab):
        return [c for x, y in tab for c in (x, m.mul(x, beta), y)]

    def table(odd):
        def run(r):
            tab, zfix = (m.table_odd if odd else m.table_multiples)(from_fq(r, 0))
            return _out(flat(tab) + [zfix])
        return run

    def pair(r):
        ta, tb, zfix = m.tables_pair(from_fq(r, 0), from_fq(r, 3))
        return _out(flat(ta) + flat(tb) + [zfix])
    def thin():          # every log point and corner, one in four of the random fill (the model is slow)
        seen = [0]

        def skip(t):
            seen[0] += t == "random"
            return t == "random" and seen[0] % 4 != 0
        return skip
    _judge_all("J29_BUILD_TABLE", table(False), thin(), 120)
    _judge_all("J29_BUILD_TABLE_ODD", table(True), thin(), 120)
    _judge_all("J29_BUILD_PAIR", pair, thin(), 120)


def test_model_g2_add29_agrees_with_the_reference_on_the_families():
    m = _model("model_g2_add29")
    pair = lambda r, s: tuple((r[s + 2 * k], r[s + 2 * k + 1]) for k in range(4))
    flat = lambda p: [c for co in p for c in co]

    def mixed(r):
        q = tuple((fr.l29(fr.wval(r[8 + 2 * k]) << 5), fr.l29(fr.wval(r[9 + 2 * k]) << 5)) for k in range(2))
        return _out(flat(m.add_mixed(pair(r, 0), q)), [0])
    ordinary = lambda t: t.startswith(("branch:equal", "branch:opposite", "zerotest", "identity", "zero:x1=x2"))          # the model has the ordinary addition only
    _judge_all("X29G2_ADD_MIXED", mixed, ordinary)
    _judge_all("X29G2_ADD", lambda r: _out(flat(m.add_full(pair(r, 0), pair(r, 8))), [0]), ordinary)
    _judge_all("X29G2_DBL", lambda r: _out(flat(m.dbl_full(pair(r, 0))), [0]), lambda t: t.startswith("identity"))


# xyzz29.hip.h statement by statement on the column model of field_ref (its header cites a model that is not in the tree)
def _mc(a, b): return fr.mont_closed([(a, b)])[0]
def _carry(t): return [x % fr.U32 for x in fr.carry_model([x % fr.U32 for x in t])[0]]
def _sub(a, b, k): return _carry([a[i] - b[i] + fr.K[k][i] for i in range(9)])


def x29_dbl_stmt(a):
    x, y, zz, zzz = a
    U = _carry([2 * v for v in y])
    V = _mc(U, U); W = _mc(U, V); S = _mc(x, V); XX = _mc(x, x)
    M = _carry([3 * v for v in XX])
    M2 = _mc(M, M)
    x3 = _carry([M2[i] - 2 * S[i] + fr.K["K16W"][i] for i in range(9)])
    T = [S[i] - x3[i] + fr.K["K32"][i] for i in range(9)]
    assert all(0 <= v < fr.U32 for v in T)
    return [x3, _sub(_mc(M, T), _mc(W, y), "K4"), _mc(V, zz), _mc(W, zzz)]


def x29_add_stmt(r, bias="K8", equal_returns_a=False):
    a, b = r[0:4], r[4:8]
    if r[pr.FLAG_SLOT][0]:
        return _out(b, [r[pr.FLAG_SLOT][1]])
    if r[pr.FLAG_SLOT][1]:
        return _out(a, [0])
    U1, U2, S1, S2 = _mc(a[0], b[2]), _mc(b[0], a[2]), _mc(a[1], b[3]), _mc(b[1], a[3])
    Pd, R = _sub(U2, U1, bias), _sub(S2, S1, "K8")
    if fr.val(Pd) % P == 0:
        if fr.val(R) % P == 0:
            return _out(a if equal_returns_a else x29_dbl_stmt(a), [0])
        return _out([], [1])
    PP = _mc(Pd, Pd); PPP = _mc(Pd, PP); Q = _mc(U1, PP)
    x3 = _carry([_mc(R, R)[i] - PPP[i] - 2 * Q[i] + fr.K["K8W"][i] for i in range(9)])
    T = [Q[i] - x3[i] + fr.K["K16"][i] for i in range(9)]
    assert all(0 <= v < fr.U32 for v in T)
    return _out([x3, _sub(_mc(R, T), _mc(S1, PPP), "K2"), _mc(_mc(a[2], b[2]), PP), _mc(_mc(a[3], b[3]), PPP)], [0])


def test_statement_model_of_xyzz29_agrees_with_the_reference():
    _judge_all("X29_ADD", x29_add_stmt)
    _judge_all("X29_DBL", lambda r: _out(r[0:4], [1]) if r[pr.FLAG_SLOT][0] else _out(x29_dbl_stmt(r[0:4]), [0]))


def _first_failure(name, run):
    for t, r in zip(*family(name)):
        try:
            if pr.judge(name, r, run(r)).errors:
                return t
        except AssertionError:
            return t
    return None


def test_wrong_variants_fail_the_judge():
    """the verdict is sensitive where the device code could be subtly wrong: a bias too small for P, an equal-point branch that forgets to double, a
    `special` that confuses equal with opposite"""
    assert _first_failure("X29_ADD", lambda r: x29_add_stmt(r, bias="K4")) is not None
    assert _first_failure("X29_ADD", lambda r: x29_add_stmt(r, equal_returns_a=True)).startswith(("branch:equal", "canonical:all p-1"))          # all words p - 1: the same point twice
    m = _model("model_jac29")

    def madd_wrong(r):
        res = m.j29_madd(tuple(r[0:3]), r[3], r[4])
        return _out(r[0:3], [2]) if res is None else _out(list(res[0]) + [res[1]], [0])
    assert _first_failure("J29_MADD", madd_wrong).startswith("branch:equal")


def test_literal_bound_of_madd_y1_underflows_limb_8():
    """why `Y <= 4 p` (jac29.hip.h:173) is tightened by 2^233 in BOUNDS: rr = S2 - Y1 + 4p with S2 == 0 and Y1 = 4p - 1 in lazy limbs leaves limb 8 at -1"""
    r, _ = fr.sub_model([0] * 9, fr.l29(4 * P - 1), fr.K["K4"])
    assert r[8] == -1 and fr.val(r) == 1
    rng = pr._rng("y1")
    for y in [fr.l29(pr.bound("j29.madd.y1.tight") - 1)] + [pr.lazy_below(rng, pr.bound("j29.madd.y1.tight")) for _ in range(50)]:
        r, _ = fr.sub_model([0] * 9, y, fr.K["K4"])
        assert r[8] >= 0 and fr.val(r) == 4 * P - fr.val(y)
