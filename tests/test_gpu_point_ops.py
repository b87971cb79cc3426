"""GPU suite: the shipped functions of the lazy-limb group law on host-chosen operands against Python integers (keaki_hip_selftest_point_ops).

Each op of keaki_point_op (include/keaki_hip.h) -- x29_add / x29_dbl and the stores of xyzz29.hip.h, the G2 additions of xyzz29_g2.hip.h, j29_dbl /
j29_madd / j29_addsub, the table builds, glv_decompose and the two digit recoders, the four ladders of jac29.hip.h, and the saturated formulas of
bn254_curve.hip.h over Fq and Fq2 -- runs on the operand families of tests/point_ref.py: canonical operands as the loaders produce them, every
coordinate at its documented bound (exact limbs, and limbs 0..7 up to 2^29 + 8), equal / opposite / P against 2P in several representations with
the zero tests' arguments on every multiple of p they can hold, the identity on either side behind arbitrary limbs, GLV scalars at the rounding
steps of c1 and c2 and on the carry chains of both recodings, ladders over points with known logs. point_ref.judge gives the verdict on every
record: affine image, flags, `special`, *ratio, limb and value bounds, canonical stores, tables entry by entry, digits bit for bit. No tolerance.
Where the operands are multiples of G that the generator knows (the `logs` families, the table builds' log points, every ladder record), the device's
result is additionally compared with (log) G computed by oracle/bn254_py.py (point_ref.oracle_errors; the ladders on the sample of oracle_sample).
tests/test_point_ref_model.py checks the reference and the families themselves on the CPU.

Measured on an MI355X (pytest --durations=0 of this file): 80 cases in 16 s; the slowest are the ladders, whose reference is a Python scalar
multiplication per record plus the oracle's on the sample (LADDER_MUL2 3.5 s, LADDER_UNIFORM 1.9 s, LADDER_FIXED 1.0 s, LADDER_GTAB 0.8 s), then the four
4,096-record cases (0.7 - 1.0 s); every other case is below 0.5 s. profiles/point_probe_maxima.txt holds the largest values observed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_ref as pr  # noqa: E402
from keaki_amd import hip as khip  # noqa: E402

pytestmark = pytest.mark.gpu

CODES = khip.point_op_codes()
OPS = list(pr.OPS)
PER_LANE = [k for k in OPS if k not in pr.UNIFORM_OPS]
KEAKI_ERR_BAD_ARG = -1
_FAMILIES = {}
MAXIMA = {}          # (op, coordinate) -> largest value observed in a result, as a multiple of p


def family(name):
    """(tags, records), computed once per op and left unchanged"""
    if name not in _FAMILIES:
        _FAMILIES[name] = pr.generate(name)
    return _FAMILIES[name]


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def _report(name, tags, recs, outs, verdicts, bad):
    lines = ["%s: %d of %d records fail" % (name, len(bad), len(recs))]
    for i in bad[:4]:
        lines.append("  record %d, family [%s]" % (i, tags[i]))
        for e in verdicts[i].errors:
            lines.append("    ! " + e)
        for s, slot in enumerate(recs[i]):
            if any(slot):
                lines.append("    operand slot %2d: %s" % (s, _hex(slot)))
        for s, slot in enumerate(outs[i]):
            if any(slot):
                lines.append("    device  slot %2d: %s" % (s, _hex(slot)))
    return "\n".join(lines)


def _check(hip, name, tags, recs, note=True, logs=None):
    out = hip.point_ops(CODES[name], pr.pack_records(recs))
    assert out.shape == (len(recs), pr.OUT_SLOTS, pr.SW)
    outs = out.tolist()
    verdicts, bad = [], []
    sample = set(pr.oracle_sample(name, len(recs))) if logs is not None else ()
    for i, (rec, o) in enumerate(zip(recs, outs)):
        v = pr.judge(name, rec, o, recs[i // 64 * 64] if name in pr.UNIFORM_OPS else None)
        verdicts.append(v)
        if logs is not None and logs[i] is not None and i in sample:          # operands with known logs: additionally (log) G of oracle/bn254_py.py
            v.errors += pr.oracle_errors(name, o, logs[i])
        if v.errors:
            bad.append(i)
        if note:
            for coord, m in v.maxima.items():
                key = (name, re.sub(r"\[\d\]", "[]", coord))
                MAXIMA[key] = max(MAXIMA.get(key, 0.0), m)
    if bad:
        print(_report(name, tags, recs, outs, verdicts, bad))
    assert not bad, "%s: first failure in family [%s] (record %d of %d): %s" % (name, tags[bad[0]], bad[0], len(recs), verdicts[bad[0]].errors[0])


@pytest.mark.parametrize("name", OPS)
def test_point_op_matches_big_integers(hip, name):
    tags, recs = family(name)
    _check(hip, name, tags, recs, logs=pr.LOGS[name])


@pytest.mark.parametrize("name", PER_LANE)
def test_per_lane_op_with_partial_waves(hip, name):
    """n = 1, 63, 64, 65: one lane of a wave, one short of a wave, a whole wave, a wave and one lane; all 64 lanes of every wave run and only the
    first n records come back"""
    tags, recs = family(name)
    lo = len(recs) - 70
    for n in (1, 63, 64, 65):
        _check(hip, name, tags[lo:lo + n], recs[lo:lo + n], note=False)


@pytest.mark.parametrize("name", pr.UNIFORM_OPS)
def test_uniform_op_with_one_and_two_waves(hip, name):
    """one wave, two waves with different scalars (a wave that read the other wave's digits in LDS would show), and a second wave of one lane, whose
    scalar is then its own"""
    tags, recs = family(name)
    for lo, n in ((0, 64), (64, 128), (128, 65), (192, 1)):
        _check(hip, name, tags[lo:lo + n], recs[lo:lo + n], note=False)


@pytest.mark.parametrize("name", pr.ONE_PER_FILE)
def test_every_record_gets_its_own_answer(hip, name):
    """4,096 records that all differ, against the reference, and the first and the last of them alone: a lane that read or wrote another record's
    words shows"""
    n = CODES["MAX_RECORDS"]
    recs = pr.distinct_records(name, n)
    a = pr.pack_records(recs)
    assert len({r.tobytes() for r in a}) == n
    big = hip.point_ops(CODES[name], a)
    small = hip.point_ops(CODES[name], a[[0, n - 1]].copy())
    assert np.array_equal(small, big[[0, n - 1]])
    bad = [i for i, (rec, o) in enumerate(zip(recs, big.tolist())) if pr.judge(name, rec, o).errors]
    assert not bad, "records %s... got another answer than their own" % bad[:5]


def test_bad_arguments_are_refused(hip):
    lib, ctx = hip.lib, hip.ctx
    a = pr.pack_records(family("J29_DBL")[1][:2])
    out = np.full((2, pr.OUT_SLOTS, pr.SW), 0xA5A5A5A5, np.uint32)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    dbl, g2, gtab = CODES["J29_DBL"], CODES["X29G2_DBL"], CODES["LADDER_GTAB"]
    assert lib.keaki_hip_selftest_point_ops(ctx, dbl, pa, 2, po) == 0
    good = out.copy()
    out[:] = 0xA5A5A5A5
    for op, p_in, n, p_out in ((CODES["COUNT"], pa, 2, po), (0xFFFFFFFF, pa, 2, po), (dbl, pa, 0, po), (dbl, pa, CODES["MAX_RECORDS"] + 1, po),
                               (g2, pa, 0, po), (g2, pa, CODES["MAX_RECORDS"] + 1, po), (gtab, pa, 0, po), (dbl, None, 2, po), (dbl, pa, 2, None), (g2, None, 2, po)):
        assert lib.keaki_hip_selftest_point_ops(ctx, op, p_in, n, p_out) == KEAKI_ERR_BAD_ARG, (op, n)
        assert b"bad argument" in lib.keaki_hip_last_error(ctx)
    assert (out == 0xA5A5A5A5).all()          # nothing was launched, nothing written
    assert lib.keaki_hip_selftest_point_ops(None, dbl, pa, 2, po) == KEAKI_ERR_BAD_ARG
    with pytest.raises(khip.KeakiHipError):
        hip.point_ops(CODES["COUNT"], a)
    # the context is as usable as before
    assert np.array_equal(hip.point_ops(dbl, a), good)


def test_report_observed_maxima(hip):
    """the largest value every result coordinate took in the runs above, as a multiple of p: a record beside the headers' stated bounds
    (profiles/point_probe_maxima.txt), not a threshold. KEAKI_POINT_MAXIMA_OUT names a file to write the table to."""
    if not MAXIMA:
        for name in OPS:
            _check(hip, name, *family(name), logs=pr.LOGS[name])
    lines = ["%-22s %-24s %10.4f" % (op, coord, m) for (op, coord), m in sorted(MAXIMA.items(), key=lambda kv: (OPS.index(kv[0][0]), kv[0][1]))]
    print("\n".join(lines))
    path = os.environ.get("KEAKI_POINT_MAXIMA_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert lines
