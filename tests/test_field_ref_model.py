"""CPU suite: tests/field_ref.py against itself -- the reference, the bounds table and the operand families that tests/test_gpu_field_ops.py
feeds to keaki_hip_selftest_field_ops. Nothing here touches the device code; what is pinned is that the GPU test asks the right question:
  * every op code of include/keaki_hip.h has a reference, a bounds row per operand and at least one family;
  * every emitted operand respects its row, and every row names its source line;
  * the column algorithm of u29_mul_ref / u29_sqr_ref, restated in unbounded integers, agrees with the closed form (T + m p) / 2^261 on every
    emitted record and no column reaches 2^64 -- the stated per-limb budgets included;
  * no limb of a biased difference goes negative or past 32 bits inside the documented bounds (what the K constants exist for), the result
    is congruent to a - b (- 2c) and its limbs 0..7 are at most 2^29 + 7;
  * the search for chosen quotient digits never hits its redraw cap."""
import os
import re
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

CODES = khip.field_op_codes()
GEOMETRY = {"COUNT", "FIRST_PAIR", "SLOTS", "SLOT_WORDS", "MAX_RECORDS"}
OPS = sorted(k for k in CODES if k not in GEOMETRY)


@pytest.fixture(scope="module")
def families():
    return {name: fr.generate(name) for name in OPS}


def test_every_op_code_has_a_reference_rows_and_a_family(families):
    assert sorted(CODES[k] for k in OPS) == list(range(CODES["COUNT"])) and CODES["COUNT"] >= 60
    assert OPS == fr.ALL_OPS, (sorted(set(OPS) - set(fr.ALL_OPS)), sorted(set(fr.ALL_OPS) - set(OPS)))
    assert (CODES["SLOTS"], CODES["SLOT_WORDS"], CODES["MAX_RECORDS"]) == (12, 9, 65536)
    for name in OPS:
        assert (name in fr.PAIR_REF) == (CODES[name] >= CODES["FIRST_PAIR"]), name
        tags, recs = families[name]
        assert 0 < len(recs) == len(tags) <= 4096 and len({t.split(":")[0].split(" ")[0] for t in tags}) >= 2, name
        assert all(len(s) == len(fr.ROWS[name]) for s in recs), name
        if name in fr.PAIR_REF:
            assert len(recs) % 2 == 0
    # the difference ops cover every K constant that the generator emits, and each K a shipped call site passes has an op
    csrc = os.path.join(fr.ROOT, "keaki_amd", "csrc")
    used = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hip.h")) and not f.startswith(("selftest", "field_probe", "bn254_constants")):
            used |= set(re.findall(r"Q29::(K\d+W?)\b", open(os.path.join(csrc, f)).read()))
    assert used and used <= set(fr.K), used
    for k in used - {"K8W"}:
        assert "U29_SUB_" + k in CODES, k
    assert "K8W" in used and "U29_SUB3" in CODES
    raw = set(re.findall(r"u29_sub_raw\([^;]*?Q29::(K\d+W?)\)", "".join(open(os.path.join(csrc, f)).read() for f in ("xyzz29.hip.h", "xyzz29_g2.hip.h", "jac29.hip.h", "msm.hip.h"))))
    assert raw == {"K16", "K32"}


def test_bounds_table_names_a_source_line_for_every_row():
    for row, (lim, lim8, vb, src) in fr.BOUNDS.items():
        m = re.findall(r"([\w.]+\.(?:h|py)):(\d+)", src)
        assert m, row
        for f, line in m:
            path = os.path.join(fr.ROOT, "keaki_amd", "csrc", f)
            assert os.path.exists(path) and int(line) <= len(open(path).read().splitlines()), (row, f, line)
    assert {r for rows in fr.ROWS.values() for r in rows} == set(fr.BOUNDS)


def test_every_emitted_operand_respects_its_row(families):
    for name in OPS:
        tags, recs = families[name]
        for tag, slots in zip(tags, recs):
            for s, (slot, row) in enumerate(zip(slots, fr.ROWS[name])):
                assert fr.in_row(slot, row), "%s [%s] slot %d outside row %s: %s" % (name, tag, s, row, [hex(x) for x in slot])


def test_families_reach_the_documented_bounds(families):
    """the edge families are there: budget records put every limb at its row's maximum, lazy records come within 2^232 of a value bound"""
    for name, rows in fr.PRODUCT_ROWS.items():
        tags, recs = families[name]
        b = recs[tags.index("budget")]
        assert all(slot == [fr.BOUNDS[r][0]] * 8 + [fr.BOUNDS[r][1]] for slot, r in zip(b, rows)), name
        assert any(t.startswith("m=ones") for t in tags) or len(rows) == 1, name
        assert {"result=0", "result=p"} <= set(tags) and any(t.startswith("result~2p") for t in tags), name
        near = [fr.val(s[-1]) for t, s in zip(tags, recs) if t == "lazy"]
        assert any(2 * fr.P - (1 << 232) <= v < 2 * fr.P for v in near), name
    for name in OPS:
        if name.startswith("U29_SUB"):
            tags, recs = families[name]
            vb = fr.BOUNDS[fr.ROWS[name][1]][2]
            assert any(fr.val(s[1]) == vb - 1 for s in recs) and any(s[0] == s[1] for s in recs), name


def test_column_model_agrees_with_the_closed_form_and_stays_below_2_64(families):
    peak = {}
    for name, rows in fr.PRODUCT_ROWS.items():
        tags, recs = families[name]
        top = 0
        for tag, s in zip(tags, recs):
            pairs = [(s[0], s[0])] if len(rows) == 1 else [(s[2 * k], s[2 * k + 1]) for k in range(len(rows) // 2)]
            limbs, col, m = fr.mont_columns(pairs)
            want, m_closed = fr.mont_closed(pairs)
            assert col < 1 << 64, "%s [%s]: a column reaches %d bits" % (name, tag, col.bit_length())
            assert limbs == want and m == m_closed, (name, tag)
            assert want[8] < 1 << 32, (name, tag)
            if not tag.startswith("budget"):
                assert fr.val(want) < 4 * fr.P or tag == "lazy", (name, tag)
            top = max(top, col)
        peak[name] = top.bit_length()
    # the budgets are tight where the headers say so: the dot6 and mul2 budget records fill a column to within two bits of 64
    assert peak["U29_DOT6"] >= 63 and peak["U29_MUL2"] >= 62, peak


def test_no_biased_difference_leaves_32_bits(families):
    for name in OPS:
        if not name.startswith("U29_SUB") and name != "U29_CARRY":
            continue
        tags, recs = families[name]
        for tag, s in zip(tags, recs):
            if name == "U29_CARRY":
                r, mid = fr.carry_model(s[0])
                want = fr.val(s[0])
            elif name == "U29_SUB3":
                r, mid = fr.sub_model(s[0], s[1], fr.K["K8W"], c=s[2])
                want = fr.val(s[0]) - fr.val(s[1]) - 2 * fr.val(s[2]) + 8 * fr.P
            else:
                k = name.split("_")[-1]
                r, mid = fr.sub_model(s[0], s[1], fr.K[k], carried="RAW" not in name)
                want = fr.val(s[0]) - fr.val(s[1]) + fr.K_MULT[k] * fr.P
            assert all(0 <= x < 1 << 32 for x in mid), "%s [%s]: an intermediate limb leaves [0, 2^32): %s" % (name, tag, [hex(x) for x in mid])
            assert fr.val(r) == want and want >= 0, (name, tag)
            if "RAW" in name:
                assert all(x < 1 << 31 for x in r[:8]), (name, tag)       # 'limbs below 2^31' (fq29_core.hip.h:178)
            else:
                assert all(x <= (1 << 29) + 7 for x in r[:8]), (name, tag)
            assert fr.REF[name](s) == r, (name, tag)


def test_subtrahend_bound_is_tight_to_the_slack_the_table_states():
    """Why the rows of the subtrahends stop 2^233 below K: with a = 0 and the subtrahends summing to K - 3 in these limbs the carried result
    would need limb 8 = -1 (the device would return 2^32 - 1 there); one slack lower, the same limb shapes come out right."""
    c = fr.l29(2 * fr.P - 1)
    r, mid = fr.sub_model([0] * 9, fr.l29(4 * fr.P - 1), fr.K["K8W"], c=c)
    assert r[8] == -1 and fr.val(r) == 3
    r, mid = fr.sub_model([0] * 9, fr.l29(4 * fr.P - fr.SUB_SLACK - 1), fr.K["K8W"], c=c)
    assert all(0 <= x < 1 << 32 for x in mid) and fr.val(r) == fr.SUB_SLACK + 3
    for k, mult in fr.K_MULT.items():          # and no representation below the bound can do it: limbs 0..7 of a carried result hold less than 2^233
        assert sum(((1 << 29) + 7) << (29 * i) for i in range(8)) < fr.SUB_SLACK


def test_predicate_and_pack_families_cover_their_stated_ranges(families):
    for name, kmax in (("U29_MAYBE_ZERO", 17), ("U29_MAYBE_ZERO34", 34)):
        tags, recs = families[name]
        for k in range(kmax + 1):
            reps = [s for t, s in zip(tags, recs) if t.startswith("%dp " % k)]
            assert len(reps) >= (2 if k else 1) and all(fr.val(s[0]) == k * fr.P and fr.REF[name](s)[0] == 1 for s in reps), (name, k)
        assert fr.REF[name]([fr.l29((kmax + 1) * fr.P)])[0] == 0          # the filter is sharp: the first multiple past the range is refused
    tags, recs = families["U29_IS_ZERO"]
    for k in range(101):
        for d in (0, 1, -1):
            if k or d >= 0:
                assert fr.REF["U29_IS_ZERO"](recs[tags.index("%dp%+d" % (k, d))])[0] == int(d == 0)
    tags, recs = families["U29_PACK_CANONICAL"]
    assert [fr.val(s[0]) for s in recs[:6]] == [0, 1, fr.P - 1, fr.P, fr.P + 1, 2 * fr.P - 1]
    assert [fr.wval(fr.REF["U29_PACK_CANONICAL"](s)) for s in recs[:6]] == [0, 1, fr.P - 1, 0, 1, fr.P - 1]
    for name in ("FQ_INV_XGCD", "FQ_INV_SAFEGCD", "FQ_INV_FERMAT", "FQ_INV", "FQ_INV261"):
        assert fr.REF[name]([fr.w32(0)])[:8] == [0] * 8          # every inverse maps 0 -> 0
        x = fr.REF[name]([fr.w32(12345)])
        rr = (fr.R261 if name == "FQ_INV261" else fr.R256)
        assert fr.wval(x) * 12345 % fr.P == rr * rr % fr.P


def test_tower_reference_is_the_oracles(py):
    import random
    rng = random.Random(7)
    e = [(rng.randrange(fr.P), rng.randrange(fr.P)) for _ in range(6)]
    assert fr.f2_mul(e[0], e[1]) == py.f2_mul(e[0], e[1]) and fr.f2_xi(e[2]) == py.f2_mul_xi(e[2]) and fr.f2_inv(e[3]) == py.f2_inv(e[3])
    assert fr.f6_mul(tuple(e[:3]), tuple(e[3:])) == py.f6_mul(tuple(e[:3]), tuple(e[3:]))
    # through the record layer: words in the 2^261 form in, words in the 2^261 form out
    s0 = [fr.w32(x[0] * fr.R261 % fr.P) for x in e]
    s1 = [fr.w32(x[1] * fr.R261 % fr.P) for x in e]
    want = py.f6_mul(tuple(e[:3]), tuple(e[3:]))
    for j, name in enumerate(("FQ6_MUL_C0", "FQ6_MUL_C1", "FQ6_MUL_C2")):
        r0, r1 = fr.PAIR_REF[name](s0, s1)
        assert (fr.wval(r0), fr.wval(r1)) == (want[j][0] * fr.R261 % fr.P, want[j][1] * fr.R261 % fr.P)
    x, y = e[0], e[1]
    r0, r1 = fr.PAIR_REF["FQ4_SQR_T0"](s0[:2], s1[:2])
    t0 = py.f2_add(py.f2_sqr(x), py.f2_mul_xi(py.f2_sqr(y)))
    assert (fr.wval(r0), fr.wval(r1)) == (t0[0] * fr.R261 % fr.P, t0[1] * fr.R261 % fr.P)


def test_redraw_cap_is_never_hit_and_the_reference_is_quick(families):
    assert 0 < fr.redraws_peak[0] <= fr.REDRAW_CAP, fr.redraws_peak
    slowest = 0.0
    for name in OPS:
        t0 = time.perf_counter()
        out = fr.expected(name, families[name][1])
        slowest = max(slowest, time.perf_counter() - t0)
        assert len(out) == len(families[name][1]) and all(len(o) == 9 and all(0 <= w < 1 << 32 for w in o) for o in out), name
    assert slowest < 5.0, slowest        # meant: well under a second per op; the bound only catches a family that grew by mistake
