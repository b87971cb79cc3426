"""CPU suite: the tuning options of a context are declared once. Tuning (csrc/internal.h) holds them, TUNE_OPTIONS (csrc/api.hip) is the
one table that keaki_hip_ctx_set_option and the environment (KEAKI_<NAME>, read by tune_from_env) both go through, and the comment of
keaki_hip_ctx_set_option in include/keaki_hip.h names them for callers. The three must agree."""
import os
import re

import variant_cases as V


def test_table_and_tuning_members_match_one_to_one():
    members = V.tuning_members()
    table = V.table_options()
    names = [n for n, _ in table]
    assert len(names) == len(set(names)), "an option is declared twice: %s" % names
    # every member is an option of its own name, except the allocation limit (keaki_hip_debug_set_alloc_limit)
    assert set(names) == set(members) - {"alloc_limit"}
    # the diagnostic switch exists in the diagnostic build only, in the struct and in the table alike
    assert {n for n, diag in table if diag} == {n for n, (_, diag) in members.items() if diag} == {"diag_row_mask"}
    # ... and through set_option only: its entry keeps it out of the environment
    entry = [line for line in V._src("api.hip").splitlines() if "TUNE_OPTION(diag_row_mask" in line]
    assert len(entry) == 1 and "nullptr, nullptr, false)" in entry[0], entry


def test_every_shipped_option_is_named_in_the_header():
    hdr = open(os.path.join(V.ROOT, "include", "keaki_hip.h")).read()
    doc = re.search(r"/\* Tuning / A-B switches of a context.*?\*/\s*keaki_status keaki_hip_ctx_set_option\(", hdr, re.S).group(0)
    missing = [n for n in V.shipped_options() if '"%s"' % n not in doc]
    assert not missing, "options the set_option comment of keaki_hip.h does not name: %s" % missing


def test_getenv_is_called_once_in_the_library():
    calls = []
    for dirpath, dirnames, files in os.walk(V.CSRC):
        dirnames[:] = [d for d in dirnames if not d.startswith("build")]
        for f in files:
            if f.endswith((".hip", ".h", ".cpp", ".c")):
                text = open(os.path.join(dirpath, f)).read()
                calls += [(f, m.start()) for m in re.finditer(r"\bgetenv\s*\(", text)]
    assert len(calls) == 1 and calls[0][0] == "api.hip", calls
    api = V._src("api.hip")
    assert api.index("void tune_from_env(") < calls[0][1] < api.index("struct BufClass")

