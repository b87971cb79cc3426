"""GPU suite: the shipped functions of the pairing's Fq12 tower on host-chosen operands against Python integers (keaki_hip_selftest_tower_ops).

Each op of keaki_tower_op (include/keaki_hip.h) -- the Fq12 operations and line functions of the lane-pair form, and the twelve-lane form with
its own product code -- runs on the operand families of tests/tower_ref.py: zero, one, -1, the unit vectors, every word at p - 1, subfield and
sparse elements, related pairs, line coefficients at 0 / p / 2p - 1 as exact limbs, points with known logs, the identity path's zeros, the
inverse of 0. Every one of the 96 result words of every record must equal the big-integer reference. No tolerance.
tests/test_tower_ref_model.py checks the reference and the families themselves on the CPU."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_ref as tr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

pytestmark = pytest.mark.gpu

CODES = khip.tower_op_codes()
OPS = sorted((k for k in CODES if k not in ("COUNT", "FIRST_WIDE", "REC_WORDS", "OUT_WORDS", "MAX_RECORDS")), key=lambda k: CODES[k])
WIDE = [k for k in OPS if CODES[k] >= CODES["FIRST_WIDE"]]
PAIR = [k for k in OPS if CODES[k] < CODES["FIRST_WIDE"]]
KEAKI_ERR_BAD_ARG = -1
_FAMILIES = {}


def family(name):
    """(tags, records, expected words n x 12 x 8), computed once per op and left unchanged"""
    if name not in _FAMILIES:
        tags, recs = tr.generate(name)
        _FAMILIES[name] = (tags, recs, np.array(tr.expected(name, recs), dtype=np.uint32))
    return _FAMILIES[name]


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def _report(name, tags, recs, got, want, bad):
    lines = ["%s: %d of %d records differ" % (name, len(bad), len(recs))]
    for i in bad[:4]:
        lines.append("  record %d, family [%s]" % (i, tags[i]))
        for area, vals in recs[i].items():
            for j, v in enumerate(vals):
                lines.append("    %s[%d] = %#x" % (area, j, v))
        for m in range(12):
            mark = " " if (got[i, m] == want[i, m]).all() else "*"
            lines.append("   %s Fq %2d device:    %s" % (mark, m, _hex(got[i, m])))
            lines.append("   %s       reference: %s" % (mark, _hex(want[i, m])))
    return "\n".join(lines)


def _check(hip, name, tags, recs, want):
    got = hip.tower_ops(CODES[name], tr.pack_records(recs))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0].tolist()
    if bad:
        print(_report(name, tags, recs, got, want, bad))
    assert not bad, "%s: first mismatch in family [%s] (record %d of %d)" % (name, tags[bad[0]], bad[0], len(recs))


@pytest.mark.parametrize("name", OPS)
def test_tower_op_matches_big_integers(hip, name):
    tags, recs, want = family(name)
    _check(hip, name, tags, recs, want)


@pytest.mark.parametrize("name", WIDE)
def test_wide_op_with_partial_rows_and_waves(hip, name):
    """n = 1 .. 5: one to three idle rows of a wave, then a second wave with one row; every lane of both runs (the pairs of a row meet in the
    exchange area, the lanes of a pair by DPP) and only the first n records may be stored"""
    tags, recs, want = family(name)
    for n in (1, 2, 3, 4, 5):
        lo = len(recs) - 7 - n          # the seeded random fill
        _check(hip, name, tags[lo:lo + n], recs[lo:lo + n], want[lo:lo + n])


@pytest.mark.parametrize("name", PAIR)
def test_lane_pair_op_with_a_padded_tail(hip, name):
    """n = 1, 31, 32, 33: one pair of a wave, one short of a wave, a whole wave, a wave and one pair"""
    tags, recs, want = family(name)
    for n in (1, 31, 32, 33):
        lo = len(recs) - 40
        _check(hip, name, tags[lo:lo + n], recs[lo:lo + n], want[lo:lo + n])


@pytest.mark.parametrize("name", ["FQ12_MUL", "W12_MUL"])
def test_every_record_gets_its_own_answer(hip, name):
    """4,096 records that all differ, against the reference, and the first and the last of them alone: a lane pair or a row that read or wrote
    another record's words shows"""
    rng = random.Random(12)
    n = CODES["MAX_RECORDS"]
    recs = [{"a": tr.dense(rng), "b": tr.dense(rng)} for _ in range(n)]
    a = tr.pack_records(recs)
    big = hip.tower_ops(CODES[name], a)
    small = hip.tower_ops(CODES[name], a[[0, n - 1]].copy())
    assert np.array_equal(small, big[[0, n - 1]])
    want = np.array(tr.expected(name, recs), dtype=np.uint32)
    bad = np.nonzero((big != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "records %s... got another answer than their own" % bad[:5].tolist()


def test_bad_arguments_are_refused(hip):
    lib, ctx = hip.lib, hip.ctx
    a = tr.pack_records(family("FQ12_CONJ")[1][:2])
    out = np.full((2, 96), 0xA5A5A5A5, np.uint32)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    conj, wide = CODES["FQ12_CONJ"], CODES["W12_CONJ"]
    assert lib.keaki_hip_selftest_tower_ops(ctx, conj, pa, 2, po) == 0
    out[:] = 0xA5A5A5A5
    for op, p_in, n, p_out in ((CODES["COUNT"], pa, 2, po), (0xFFFFFFFF, pa, 2, po), (conj, pa, 0, po), (conj, pa, CODES["MAX_RECORDS"] + 1, po),
                               (wide, pa, 0, po), (wide, pa, CODES["MAX_RECORDS"] + 1, po), (conj, None, 2, po), (conj, pa, 2, None), (wide, None, 2, po)):
        assert lib.keaki_hip_selftest_tower_ops(ctx, op, p_in, n, p_out) == KEAKI_ERR_BAD_ARG, (op, n)
        assert b"bad argument" in lib.keaki_hip_last_error(ctx)
    assert (out == 0xA5A5A5A5).all()          # nothing was launched, nothing written
    assert lib.keaki_hip_selftest_tower_ops(None, conj, pa, 2, po) == KEAKI_ERR_BAD_ARG
    with pytest.raises(khip.KeakiHipError):
        hip.tower_ops(CODES["COUNT"], a)
    # the context is as usable as before, in both forms
    assert lib.keaki_hip_selftest_tower_ops(ctx, wide, pa, 2, po) == 0
    assert np.array_equal(out.reshape(2, 12, 8), hip.tower_ops(conj, a))
