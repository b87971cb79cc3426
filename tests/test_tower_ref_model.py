"""CPU suite: tests/tower_ref.py against itself -- the references and the operand families that tests/test_gpu_tower_ops.py feeds to
keaki_hip_selftest_tower_ops. Nothing here touches the device code; what is pinned is that the GPU test asks the right question: every op has
a reference and families, every operand stays inside the bounds its callee documents, the restated Granger-Scott squaring is the square exactly
where it should be, the sparse product is the sum of the terms the headers list, and the flat <-> tower permutation is a permutation."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_ref as tr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

CODES = khip.tower_op_codes()
GEOMETRY = ("COUNT", "FIRST_WIDE", "REC_WORDS", "OUT_WORDS", "MAX_RECORDS")
OPS = sorted((k for k in CODES if k not in GEOMETRY), key=lambda k: CODES[k])
P = tr.P


@pytest.fixture(scope="module")
def families():
    out, seconds = {}, {}
    for name in OPS:
        t0 = time.perf_counter()
        tags, recs = tr.generate(name)
        want = tr.expected(name, recs)
        seconds[name] = time.perf_counter() - t0
        out[name] = (tags, recs, want)
    return out, seconds


def test_geometry_and_op_codes_match_the_header():
    assert [CODES[k] for k in OPS] == list(range(CODES["COUNT"])) and CODES["COUNT"] == 29
    assert (CODES["REC_WORDS"], CODES["OUT_WORDS"], CODES["MAX_RECORDS"]) == (tr.REC_WORDS, 8 * tr.OUT_FQ, 4096)
    assert CODES["FIRST_WIDE"] == CODES["W12_MUL"] and all((CODES[k] >= CODES["FIRST_WIDE"]) == k.startswith("W") for k in OPS)
    # the areas tile the record
    end = 0
    for k in ("a", "b", "line", "t", "q", "p"):
        assert tr.OFF[k] == end
        end += tr.AREAS[k][0] * tr.AREAS[k][1]
    assert end == tr.REC_WORDS
    # the field probe's enum and record are not touched
    f = khip.field_op_codes()
    assert (f["COUNT"], f["SLOTS"], f["SLOT_WORDS"]) == (62, 12, 9) and not any(k.startswith("KEAKI_TOP") for k in f)


def test_every_op_has_a_reference_and_families(families):
    fam, _ = families
    assert sorted(tr.REF) == sorted(OPS) and sorted(tr.USES) == sorted(OPS)
    for name in OPS:
        tags, recs, want = fam[name]
        kinds = {t.split(":")[0].split(" ")[0] for t in tags}
        assert len(kinds) >= 2, (name, kinds)
        assert 256 <= tags.count("random") + tags.count("general:random") + tags.count("cyclotomic:easy part of random") <= 512, name
        assert len(recs) <= CODES["MAX_RECORDS"] and len(want) == len(recs)
        assert all(len(w) == 12 and all(len(x) == 8 for x in w) for w in want)
        # a lane-pair op and its twelve-lane counterpart are asked the same kind of question
    for a, b in (("FQ12_MUL", "W12_MUL"), ("FQ12_CYC_SQR", "W12_CYC_SQR"), ("FQ12_MUL_BY_034", "W12_MUL_034"), ("FQ12_INV", "W12_INV"), ("LINE_ADD", "W_LINE_ADD")):
        assert [t for t in fam[a][0]] == [t for t in fam[b][0]]


def test_every_operand_respects_its_row(families):
    fam, _ = families
    for name in OPS:
        tags, recs, _ = fam[name]
        for t, r in zip(tags, recs):
            assert set(r) == set(tr.USES[name]), (name, t)
            assert tr.in_bounds(name, r), (name, t)
    # the bounds the families reach: a line at 2p - 1 / p - 1, words at p - 1
    for name in ("FQ12_MUL_BY_034", "W12_MUL_034"):
        recs = fam[name][1]
        assert any(r["line"] == [2 * P - 1] * 4 + [P - 1] * 2 and r["a"] == [P - 1] * 12 for r in recs)
        assert any(r["line"][:4] == [0, 2 * P - 1, 0, 2 * P - 1] for r in recs) and any(r["line"][:4] == [2 * P - 1, 0, 2 * P - 1, 0] for r in recs)
    # packing: words and limbs round-trip
    for name in ("FQ12_MUL", "W12_MUL_034", "ELL", "LINE_ADD"):
        recs = fam[name][1][:40]
        a = tr.pack_records(recs)
        assert a.shape == (len(recs), tr.REC_WORDS) and a.dtype == np.uint32
        for row, r in zip(a, recs):
            for k, vals in r.items():
                n, words, _, _ = tr.AREAS[k]
                for j, v in enumerate(vals):
                    w = [int(x) for x in row[tr.OFF[k] + words * j:tr.OFF[k] + words * (j + 1)]]
                    if words == 9:
                        assert all(x < (1 << 29) for x in w[:8]) and sum(x << (29 * i) for i, x in enumerate(w)) == v
                    else:
                        assert sum(x << (32 * i) for i, x in enumerate(w)) == v
            untouched = set(range(tr.REC_WORDS)) - {tr.OFF[k] + i for k in r for i in range(tr.AREAS[k][0] * tr.AREAS[k][1])}
            assert not row[sorted(untouched)].any()


def test_granger_scott_is_the_square_on_the_cyclotomic_subgroup_only(families, py):
    """The kernels call the formula on outputs of the easy part, f^((p^6 - 1)(p^2 + 1)): elements of order dividing p^4 - p^2 + 1. There it is the
    square; elsewhere it is not, and the probe holds the device to the formula itself. -1 is unitary (a conj(a) = 1) yet outside that subgroup
    (p^4 - p^2 + 1 is odd): the formula sends it to 5, so "unitary" is not the condition."""
    fam, _ = families
    for name in ("FQ12_CYC_SQR", "W12_CYC_SQR"):
        tags, recs, _ = fam[name]
        inside = differ = 0
        for t, r in zip(tags, recs):
            f = tr.f12_of(r["a"])
            same = tr.gs_sqr(f) == py.f12_sqr(f)
            if t.startswith("cyclotomic"):
                f2 = py.f12_frob(f, 2)
                assert py.f12_mul(py.f12_frob(f2, 2), f) == f2, t          # f^(p^4) f = f^(p^2)
                assert py.f12_mul(f, py.f12_conj(f)) == py.F12_ONE, t
                assert same, t
                inside += 1
            else:
                differ += not same
        assert inside >= 131 and differ >= 100, (inside, differ)
        assert "general:all p-1" in tags and "general:-1" in tags
    m1 = tr.F12_MINUS_ONE
    assert py.f12_mul(m1, py.f12_conj(m1)) == py.F12_ONE and (py.P**4 - py.P**2 + 1) % 2 == 1
    assert tr.gs_sqr(m1) == (((5, 0), py.F2_ZERO, py.F2_ZERO), py.F6_ZERO) != py.f12_sqr(m1)
    gt = tr.gt_generator()
    assert py.f12_pow(gt, py.R) == py.F12_ONE and gt != py.F12_ONE


def test_sparse_product_is_the_sum_of_the_terms_the_headers_list(families, py):
    fam, _ = families
    tags, recs, want = fam["FQ12_MUL_BY_034"]
    for t, r, w in list(zip(tags, recs, want))[::3]:
        f, (c0, d0, d1) = tr.f12_of(r["a"]), tr._line(r)
        ref = py.f12_mul_by_034(f, c0, d0, d1)
        assert tr.mul_by_034_tower_terms(f, c0, d0, d1) == ref, t
        assert tr.mul_by_034_flat_terms(f, c0, d0, d1) == ref, t
        assert [tr.w32(x) for x in tr.stored(ref)] == w
    # the unit-vector records select single terms: with f = w^i the result has at most three non-zero Fq2 coefficients
    for t, r, w in zip(tags, recs, want):
        if t.startswith("edge:f unit") or t.startswith("mixed:f unit"):
            nz = {m // 2 for m in range(12) if any(w[m])}
            assert len(nz) <= 3, t


def test_flat_and_tower_orders_are_permutations_of_each_other(py):
    assert sorted(tr.tower_pos(k) for k in range(6)) == list(range(6))
    assert all(tr.flat_pos(tr.tower_pos(k)) == k for k in range(6)) and all(tr.tower_pos(tr.flat_pos(m)) == m for m in range(6))
    assert [tr.tower_pos(k) for k in range(6)] == [0, 3, 1, 4, 2, 5]          # pairing_wide.hip.h:193 'c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 = flat 0, 2, 4, 1, 3, 5'
    import random
    rng = random.Random(5)
    f = tr.f12_of(tr.dense(rng))
    assert tr.from_flat(tr.to_flat(f)) == f and tr.to_flat(f) == py._f12_to_w(f) and tr.f12_of(tr.stored(f)) == f
    # w itself: flat coefficient 1 is c1.c0
    w = ((py.F2_ZERO,) * 3, (py.F2_ONE, py.F2_ZERO, py.F2_ZERO))
    assert tr.to_flat(w) == [py.F2_ZERO, py.F2_ONE] + [py.F2_ZERO] * 4


def test_references_hold_their_own_identities(families, py):
    fam, _ = families
    # inverses: a * a^-1 = 1, and 0 -> 0
    tags, recs, want = fam["FQ12_INV"]
    assert tags[0] == "0" and want[0] == [[0] * 8] * 12
    for r in recs[1:60]:
        f = tr.f12_of(r["a"])
        assert py.f12_mul(f, tr.f12_inv0(f)) == py.F12_ONE
    tags, recs, want = fam["FQ6_INV"]
    assert want[0] == [[0] * 8] * 12 and all(w[6:] == [[0] * 8] * 6 for w in want)
    # b = 1 / a gives one
    tags, recs, want = fam["W12_MUL"]
    one = [tr.w32(x) for x in tr.stored(py.F12_ONE)]
    assert sum(w == one for t, w in zip(tags, want) if t == "related:b=1/a") == 8
    # line functions: Q = T doubles to nothing (the chord degenerates: lam = theta = 0), T = 0 stays 0
    tags, recs, want = fam["LINE_ADD"]
    for t, w in zip(tags, want):
        if t.startswith("point:Q = T") or t.startswith("identity:T = 0 and"):
            assert w == [[0] * 8] * 12, t
    # a doubling step of T = (Q, 1) lands on 2 Q
    tags, recs, want = fam["LINE_DOUBLE"]
    i = tags.index("point:T=(G2, 1)")
    x, y, z = tr._f2s([sum(v << (32 * j) for j, v in enumerate(w)) for w in want[i][:6]])
    zi = py.f2_inv(z)
    assert (py.f2_mul(x, zi), py.f2_mul(y, zi)) == py.g2_mul(py.G2_GEN, 2)


def test_the_references_are_quick(families):
    _, seconds = families
    slow = {k: round(v, 2) for k, v in seconds.items() if v > 5.0}
    assert not slow, slow
