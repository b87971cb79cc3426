"""The chunk plans of the host-array MSM and kzg_open (keaki_amd/csrc/host_plan.h: msm_pipe_bounds, open_plan) are integer work on the tuning
and the length alone. keaki_amd/host/host_plan_main.cpp includes that header and nothing of HIP and checks, under AddressSanitizer + UBSan:
for growth 50 .. 1000 percent, 2 .. 1000 forced chunks and every n in 0 .. 399 and around 2^16, 2^20, 2^21, 2^22, 2^24 -- the bounds run
from 0 to n, strictly increasing, in at most 64 pieces, whole pages from 65,536 scalars on; the coefficient chunks of open partition [0, n)
top first and their MSM ranges are non-empty and partition [0, n - 1); and the automatic bounds at 2^20, 2^21, 2^22 and 2^24. It also drives
reserve_shrinking, the shrinking reservation of the KZG verdict calls (api_kzg.hip), with each of its four shrink rules against a reservation that
refuses above a byte limit, from 1, floor, floor + 1, 33, 64, 65, 70 and 4,096 items with a limit for every count from the floor to the start: the
counts tried decrease strictly and stay at or above the floor, the first that fits is accepted and is the last try, another failure returns after
one try with the error not cleared, and a refusal at the floor comes back as a refusal. The program
restates the defaults of the four chunking options (struct Tuning lives in internal.h, which needs HIP) and prints them; they are held
against the struct here."""
import os
import shutil
import subprocess

import pytest

import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "keaki_amd", "host")


def test_chunk_plans_hold_their_invariants_under_the_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", HOST, "host_plan_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(HOST, "host_plan_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    members = V.tuning_members()
    assert "defaults: " + " ".join("%s=%d" % (k, members[k][0]) for k in ("msm_pipe_chunks", "pipe_chunks", "msm_pipe_min", "msm_pipe_growth")) in r.stdout, r.stdout
