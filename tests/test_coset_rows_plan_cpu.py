"""The host plan of kzg coset_pairs (keaki_amd/csrc/coset_rows_plan.h: window width, table bytes, slices per item, launch chunks, route) is
integer work. keaki_amd/host/coset_rows_plan_main.cpp includes that header and nothing of HIP and prints the plan; this test compiles it with the
host compiler and holds every line against the plan restated in tests/coset_pairs_model.py, and the restated plan against the figures the
header states (13 bits up to l = 64, 10 bits up to l = 512, 8 bits at l = 1,024: the widest table under 512 MiB; 270 MB at l = 1,024)."""
import os
import shutil
import subprocess

import pytest

import coset_pairs_model as P
import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "keaki_amd", "host")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("coset_rows_plan") / "plan")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HOST, "coset_rows_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_table_shape_for_every_l(lines):
    rows = {int(x[1]): [int(v) for v in x[2:]] for x in lines if x[0] == "table"}
    assert sorted(rows) == list(range(11))
    for log2l, (wb, windows, entries, nbytes) in rows.items():
        assert wb == P.cr_wb(log2l) and windows == P.cr_windows(wb) and entries == P.cr_entries(wb) and nbytes == P.cr_table_bytes(log2l, wb)
        assert nbytes == 64 * (1 << log2l) * windows * entries and windows * wb >= 255      # the top window takes the last carry
        assert wb == (13 if log2l <= 6 else 10 if log2l <= 9 else 8)
        assert nbytes <= P.CR_TABLE_BYTES_MAX
    assert (P.cr_windows(13), P.cr_windows(10), P.cr_windows(8)) == (20, 26, 32)
    assert rows[10][3] == 270532608 and rows[6][3] == 335626240 and rows[2][3] == 20976640 and P.cr_table_bytes(6, 10) == 54632448
    # additions per row: l x windows
    assert 64 * rows[6][1] == 1280 and 4 * rows[2][1] == 80 and 64 * P.cr_windows(10) == 1664
    for x in lines:
        if x[0] == "bytes":
            assert int(x[3]) == P.cr_table_bytes(int(x[1]), int(x[2]))


def test_slices_on_both_sides_of_the_threshold(lines):
    seen = 0
    for x in lines:
        if x[0] != "slices":
            continue
        log2l, n, opt, S = (int(v) for v in x[1:])
        assert S == P.cr_slices(n, log2l, opt)
        assert S & (S - 1) == 0 and S <= min(1 << log2l, 64)
        lanes_min = opt or P.CR_MIN_LANES
        assert n * S >= lanes_min or S == min(1 << log2l, 64)           # enough lanes, or no further split
        assert S == 1 or n * (S // 2) < lanes_min                        # never split further than needed
        seen += 1
    assert seen == 11 * 12 * 5
    assert P.cr_slices(2048, 6) == 64 and P.cr_slices(2049, 6) == 64 and P.cr_slices(131072, 6) == 1 and P.cr_slices(131071, 6) == 2


def test_chunks_routes_and_constants(lines):
    for x in lines:
        if x[0] == "chunk":
            log2l, n, ch = (int(v) for v in x[1:])
            assert ch == P.cr_chunk_items(n, log2l) and 1 <= ch <= n and (ch << log2l) <= P.CR_CHUNK_VALUES
        elif x[0] == "route":
            assert int(x[3]) == (2 if int(x[2]) == 2 else 1)
        elif x[0] == "halve":
            assert int(x[2]) == (int(x[1]) + 1) // 2
        elif x[0] == "consts":
            assert [int(v) for v in x[1:]] == [P.CR_TABLE_BYTES_MAX, P.CR_MIN_LANES, P.CR_CHUNK_VALUES]


def test_the_options_are_declared_and_the_library_shares_the_plan():
    m = V.tuning_members()
    assert m["coset_rows_min_lanes"] == (0, False) and m["coset_rows_route"] == (0, False) and m["coset_rows_wb"] == (0, False)
    names = [n for n, _ in V.table_options()]
    assert names.count("coset_rows_min_lanes") == 1 and names.count("coset_rows_route") == 1
    api = V._src("api_kzg.hip")
    assert '#include "coset_rows_plan.h"' in api and "cr_wb(" in api and "cr_slices(" in api and "cr_chunk_items(" in api and "cr_route(" in api
