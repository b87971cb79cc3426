"""The group offsets of encap_multi / encrypt_multi and the split of the groups between the two routes (keaki_amd/csrc/encap_multi_plan.h:
encap_multi_offsets_ok, encap_multi_plan) are integer work on the offsets and one option. keaki_amd/host/encap_multi_plan_main.cpp includes
that header and nothing of HIP and checks, under AddressSanitizer + UBSan, for random and adversarial offset arrays (all groups empty, one
huge group, m = 1, alternating empty groups and single items) and thresholds 0 / 1 / a group's exact size / size + 1: the runs and single
groups partition [0, m) in order, their item ranges partition [0, n), a single piece is exactly a group at or above the threshold and runs
are maximal, every bad array (first word not 0, a decreasing word, a last word that is not n, n or m of 2^31) is refused, and the
item-to-group search of the kernel, restated in the program, returns for every item the j with offsets[j] <= i < offsets[j + 1]. The
default of the option is held against struct Tuning, the option table and the header here."""
import os
import re
import shutil
import subprocess

import pytest

import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "keaki_amd", "host")


def test_offsets_and_routes_hold_their_invariants_under_the_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", HOST, "encap_multi_plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(HOST, "encap_multi_plan_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) offset arrays, (\d+) searches", r.stdout)
    assert m and int(m.group(1)) >= 400 and int(m.group(2)) >= 100000, r.stdout


def test_the_search_of_the_program_is_the_search_of_the_kernel():
    """the program RESTATES the kernel's binary search: the two loops must be the same text"""
    loop = r"u32 lo = 0, hi = m;\s*while \(hi - lo > 1u\) \{\s*const u32 mid = lo \+ \(\(hi - lo\) >> 1\);\s*if \(offsets\[mid\] <= gi\) lo = mid; else hi = mid;\s*\}"
    kernel = open(os.path.join(V.CSRC, "kem_multi.hip")).read()
    program = open(os.path.join(HOST, "encap_multi_plan_main.cpp")).read().replace("uint32_t", "u32")
    assert len(re.findall(loop, kernel)) == 1 and len(re.findall(loop, program)) == 1


def test_the_threshold_option_is_declared_once_everywhere():
    default, diag = V.tuning_members()["encap_multi_single_min"]
    assert default >= 0 and not diag
    assert [n for n, _ in V.table_options()].count("encap_multi_single_min") == 1
    # the default the header tells callers is the default of the struct
    hdr = open(os.path.join(ROOT, "include", "keaki_hip.h")).read()
    told = re.search(r'"encap_multi_single_min" \(.*?default ([\d,]+)', hdr, re.S)
    assert told and int(told.group(1).replace(",", "")) == default
    # the library and the checker share ONE plan: api.hip includes the header and restates none of it
    api = V._src("api.hip")
    assert '#include "encap_multi_plan.h"' in api and api.count("encap_multi_plan(") == 2 and "struct EncapMultiPiece" not in api
