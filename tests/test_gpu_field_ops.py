"""GPU suite: the shipped field streams on host-chosen operands against Python integers (keaki_hip_selftest_field_ops).

Each op of include/keaki_hip.h runs on the operand families of tests/field_ref.py -- canonical edges, lazy limb representations at the
documented limb and value bounds, every limb at a product stream's column budget, chosen Montgomery quotient digits and results, the edges
of the biased differences -- and every one of the nine result words of every record must equal the big-integer reference. No tolerance.
tests/test_field_ref_model.py checks the reference and the families themselves on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

pytestmark = pytest.mark.gpu

CODES = khip.field_op_codes()
OPS = sorted((k for k in CODES if k not in ("COUNT", "FIRST_PAIR", "SLOTS", "SLOT_WORDS", "MAX_RECORDS")), key=lambda k: CODES[k])
KEAKI_ERR_BAD_ARG = -1


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def _report(name, tags, recs, got, want, bad):
    lines = ["%s: %d of %d records differ" % (name, len(bad), len(recs))]
    for i in bad[:5]:
        lines.append("  record %d, family [%s]" % (i, tags[i]))
        for s, slot in enumerate(recs[i]):
            lines.append("    operand %d: %s" % (s, _hex(slot)))
        lines.append("    device:    %s" % _hex(got[i]))
        lines.append("    reference: %s" % _hex(want[i]))
    return "\n".join(lines)


@pytest.mark.parametrize("name", OPS)
def test_field_op_matches_big_integers(hip, name):
    tags, recs = fr.generate(name)
    want = np.array(fr.expected(name, recs), dtype=np.uint32)
    got = hip.field_ops(CODES[name], fr.pack_records(recs))
    bad = np.nonzero((got != want).any(axis=1))[0].tolist()
    if bad:
        print(_report(name, tags, recs, got, want, bad))
    assert not bad, "%s: first mismatch in family [%s] (record %d of %d)" % (name, tags[bad[0]], bad[0], len(recs))
    if name.startswith("U29_SUB") or name == "U29_CARRY":
        # what the device returned, read as integers: congruent to the difference, limbs 0..7 carried (the raw class: below 2^31)
        top = (1 << 31) - 1 if "RAW" in name else (1 << 29) + 7
        assert int(got[:, :8].max()) <= top
        for s, g in zip(recs, got):
            v = fr.val([int(x) for x in g])
            d = fr.val(s[0]) - (fr.val(s[1]) if len(s) > 1 else 0) - (2 * fr.val(s[2]) if len(s) > 2 else 0)
            assert (v - d) % fr.P == 0


def test_every_lane_gets_its_own_record(hip):
    """the same two records alone and as the first and last of a full 65,536-record call whose other records all differ: a lane that read
    or wrote another lane's record shows"""
    import random
    rng = random.Random(11)
    n = CODES["MAX_RECORDS"]
    a = np.zeros((n, 12, 9), np.uint32)
    vals = []
    for i in range(n):
        x, y = rng.randrange(2 * fr.P), rng.randrange(2 * fr.P)
        vals.append((x, y))
        a[i, 0, :], a[i, 1, :] = fr.l29(x), fr.l29(y)
    op = CODES["U29_MUL"]
    big = hip.field_ops(op, a)
    small = hip.field_ops(op, a[[0, n - 1]].copy())
    assert np.array_equal(small, big[[0, n - 1]])
    pinv, r = fr.PINV261, fr.R261
    want = np.array([fr.l29((x * y + ((-x * y * pinv) % r) * fr.P) >> 261) for x, y in vals], dtype=np.uint32)
    bad = np.nonzero((big != want).any(axis=1))[0]
    assert bad.size == 0, "records %s... got another answer than their own" % bad[:5].tolist()


def test_bad_arguments_are_refused(hip):
    lib, ctx = hip.lib, hip.ctx
    a = np.zeros((2, 12, 9), np.uint32)
    out = np.full((2, 9), 0xA5A5A5A5, np.uint32)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    mul, pair = CODES["U29_MUL"], CODES["FQ2_MUL"]
    assert lib.keaki_hip_selftest_field_ops(ctx, mul, pa, 2, po) == 0
    out[:] = 0xA5A5A5A5
    for op, p_in, n, p_out in ((CODES["COUNT"], pa, 2, po), (0xFFFFFFFF, pa, 2, po), (mul, pa, 0, po), (mul, pa, CODES["MAX_RECORDS"] + 1, po),
                               (mul, None, 2, po), (mul, pa, 2, None), (pair, pa, 1, po), (CODES["FQ6_MUL_C2"], pa, 65535, po)):
        assert lib.keaki_hip_selftest_field_ops(ctx, op, p_in, n, p_out) == KEAKI_ERR_BAD_ARG, (op, n)
        assert b"bad argument" in lib.keaki_hip_last_error(ctx)
    assert (out == 0xA5A5A5A5).all()          # nothing was launched, nothing written
    assert lib.keaki_hip_selftest_field_ops(None, mul, pa, 2, po) == KEAKI_ERR_BAD_ARG
    with pytest.raises(khip.KeakiHipError):
        hip.field_ops(pair, a[:1])
    # the context is as usable as before
    assert lib.keaki_hip_selftest_field_ops(ctx, pair, pa, 2, po) == 0


def test_binary_gcd_inverse_refuses_what_it_cannot_finish(hip):
    """fq_inv_xgcd loops for ever on a multiple of p: the probe answers an operand that is not below p with all-ones words and does not
    run it; canonical neighbours in the same call are inverted as usual"""
    vals = [fr.P - 1, fr.P, fr.P + 1, 2 * fr.P, (1 << 256) - 1, 0, 1]
    got = hip.field_ops(CODES["FQ_INV_XGCD"], fr.pack_records([[fr.w32(v)] for v in vals]))
    for v, g in zip(vals, got):
        if v < fr.P:
            assert [int(x) for x in g] == fr.REF["FQ_INV_XGCD"]([fr.w32(v)]), v
        else:
            assert (g == 0xFFFFFFFF).all(), v


@pytest.mark.parametrize("name", ["FQ2_MUL", "FQ2_SQR", "FQ6_MUL_C0"])
def test_lane_pair_op_with_a_padded_tail(hip, name):
    """n = 2 (62 padded lanes) and n = 66 (one full wave and a wave of one pair): the DPP exchange needs every lane of a wave active, and
    only the first n records may be stored"""
    tags, recs = fr.generate(name)
    for n in (2, 66):
        sub = recs[-n:]
        want = np.array(fr.expected(name, sub), dtype=np.uint32)
        got = hip.field_ops(CODES[name], fr.pack_records(sub))
        assert got.shape == (n, 9) and np.array_equal(got, want), (name, n)
