"""The host plan of kzg set_pairs (keaki_amd/csrc/set_rows_plan.h: window width of the G2 table, its bytes, slices per item, launch chunks of the
rows and of the pairing side) is integer work. keaki_amd/host/set_rows_plan_main.cpp includes that header and nothing of HIP and prints the plan;
this test compiles it with the host compiler and holds every line against the plan restated in tests/set_pairs_model.py, and the restated plan
against the figures the header states (a G2 entry is 128 B: 10,488,320 / 1,707,264 / 528,384 B per base at 13 / 10 / 8 bits; 13 bits up to k = 51,
10 bits up to 64: the widest table under 512 MiB)."""
import os
import shutil
import subprocess

import pytest

import set_pairs_model as P
import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "keaki_amd", "host")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("set_rows_plan") / "plan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HOST, "set_rows_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_table_shape_for_every_k(lines):
    rows = {int(x[1]): [int(v) for v in x[2:]] for x in lines if x[0] == "table"}
    assert sorted(rows) == list(range(1, 65))
    for k, (wb, windows, entries, nbytes, log2kp) in rows.items():
        assert wb == P.sr_wb(k) and windows == P.sr_windows(wb) and entries == P.sr_entries(wb) and nbytes == P.sr_table_bytes(k, wb)
        assert nbytes == 128 * k * windows * entries and windows * wb >= 255      # the top window takes the last carry
        assert wb == (13 if k <= 51 else 10)
        assert nbytes <= P.SR_TABLE_BYTES_MAX
        assert log2kp == P.sr_log2kp(k) and (1 << log2kp) >= k and (log2kp == 0 or (1 << (log2kp - 1)) < k)
    assert (P.sr_windows(13), P.sr_windows(10), P.sr_windows(8)) == (20, 26, 32)
    assert (P.sr_table_bytes(1, 13), P.sr_table_bytes(1, 10), P.sr_table_bytes(1, 8)) == (10488320, 1707264, 528384)
    assert P.sr_table_bytes(52, 13) > P.SR_TABLE_BYTES_MAX >= P.sr_table_bytes(51, 13) and rows[64][3] == 109264896
    # additions per row: k x windows
    assert (2 * 20, 8 * 20, 64 * 20, 64 * 26, 64 * 32) == (40, 160, 1280, 1664, 2048)
    seen = 0
    for x in lines:
        if x[0] == "bytes":
            assert int(x[3]) == P.sr_table_bytes(int(x[1]), int(x[2]))
            seen += 1
        elif x[0] == "item":
            k, pm, msm, b = (int(v) for v in x[1:])
            assert b == P.sr_item_bytes(k, P.sr_log2kp(k), pm, msm)
            seen += 1
        elif x[0] == "narrower":
            assert int(x[2]) == P.sr_wb_narrower(int(x[1]))
            seen += 1
    assert seen == 64 * 3 + 64 * 4 + 3
    assert [P.sr_wb_narrower(w) for w in (13, 10, 8)] == [10, 8, 0]


def test_slices_on_both_sides_of_the_threshold(lines):
    seen = 0
    for x in lines:
        if x[0] != "slices":
            continue
        log2kp, n, opt, S = (int(v) for v in x[1:])
        assert S == P.sr_slices(n, log2kp, opt)
        assert S & (S - 1) == 0 and S <= min(1 << log2kp, 64)
        lanes_min = opt or P.SR_MIN_LANES
        assert n * S >= lanes_min or S == min(1 << log2kp, 64)           # enough lanes, or no further split
        assert S == 1 or n * (S // 2) < lanes_min                          # never split further than needed
        seen += 1
    assert seen == 7 * 12 * 5
    assert P.sr_slices(1024, 6) == 64 and P.sr_slices(65536, 6) == 1 and P.sr_slices(65535, 6) == 2 and P.sr_slices(5, 0) == 1
    # what the GPU tests force: one slice, two, and kp
    assert P.sr_slices(9, 3, 1) == 1 and P.sr_slices(9, 3, 18) == 2 and P.sr_slices(9, 3, 1 << 31) == 8


def test_chunks_and_constants(lines):
    seen = 0
    for x in lines:
        if x[0] == "chunk":
            log2kp, n, ch = (int(v) for v in x[1:])
            assert ch == P.sr_chunk_items(n, log2kp) and 1 <= ch <= n and (ch << log2kp) <= P.SR_CHUNK_VALUES
        elif x[0] == "halve":
            assert int(x[2]) == (int(x[1]) + 1) // 2
        elif x[0] == "each":
            n, ch, half = (int(v) for v in x[1:])
            assert ch == P.se_chunk_items(n, 1 << 17) == min(n, 1 << 16) and half == P.se_chunk_halve(ch)
            assert half % 32 == 0 and half >= P.SE_CHUNK_MIN and (half <= ch or ch <= P.SE_CHUNK_MIN)
        elif x[0] == "eachbytes":
            assert [int(v) for v in x[1:]] == [64, 128 + 256 + 768 + 384 + 384]
        elif x[0] == "route":
            assert int(x[3]) == P.se_route(int(x[1]), int(x[2])) == (1 if int(x[1]) == 1 else 2)
        elif x[0] == "consts":
            assert [int(v) for v in x[1:]] == [P.SR_TABLE_BYTES_MAX, P.SR_MIN_LANES, P.SR_CHUNK_VALUES, P.SE_CHUNK_MIN]
        else:
            continue
        seen += 1
    assert seen == 7 * 8 + 5 + 7 + 1 + 1 + 6


def test_the_options_are_declared_and_the_library_shares_the_plan():
    m = V.tuning_members()
    assert m["set_rows_wb"] == (0, False) and m["set_rows_min_lanes"] == (0, False) and m["set_each_route"] == (0, False)
    names = [n for n, _ in V.table_options()]
    assert names.count("set_rows_wb") == 1 and names.count("set_rows_min_lanes") == 1 and names.count("set_each_route") == 1
    api = V._src("api_kzg.hip")
    assert '#include "set_rows_plan.h"' in api and "sr_wb(" in api and "sr_slices(" in api and "sr_chunk_items(" in api and "se_chunk_items(" in api and "se_route(" in api
