"""tests/workspace_cases.py against include/keaki_hip.h, on a CPU: every keaki_hip_* function the header declares is covered by a row of the
call table of tests/test_gpu_workspace_poison.py or stands in the exemption list with its reason -- so an entry point added without a row fails
here -- and the table holds the rows and shapes the poison test was specified with."""
import os
import re

import workspace_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "keaki_hip.h")


def test_table_and_exemptions_partition_the_header():
    fns = W.header_functions()
    assert len(fns) >= 140
    assert W.check_against_header() == []
    assert set(W.covered()) | set(W.EXEMPT) == set(fns)


def test_a_removed_row_is_noticed():
    for family in ("kzg_quotient", "g2_subgroup_check", "msm_g1"):
        table = {f: fam for f, fam in W.covered().items() if fam != family}
        bad = W.check_against_header(table=table)
        assert bad and all("neither in a row" in b for b in bad), family


def test_a_new_declaration_is_noticed(tmp_path):
    hdr = open(HEADER).read()
    new = "keaki_status keaki_hip_kzg_brand_new_dev(keaki_hip_ctx* ctx, const void* d_in, size_t n, void* d_out);\n"
    marker = "#ifdef __cplusplus\n}"
    assert hdr.count(marker) == 1
    scratch = tmp_path / "keaki_hip.h"
    scratch.write_text(hdr.replace(marker, new + marker))
    assert W.check_against_header(str(scratch)) == ["keaki_hip_kzg_brand_new_dev: neither in a row of the table nor exempt"]
    # a declaration inside a comment is not one
    scratch.write_text(hdr.replace(marker, "/* " + new + " */\n" + marker))
    assert W.check_against_header(str(scratch)) == []


def test_a_function_that_left_the_header_is_noticed(tmp_path):
    hdr = open(HEADER).read()
    cut = re.sub(r"keaki_status keaki_hip_kzg_quotient\(.*?\);", "", hdr, flags=re.S)
    assert cut != hdr
    scratch = tmp_path / "keaki_hip.h"
    scratch.write_text(cut)
    assert W.check_against_header(str(scratch)) == ["keaki_hip_kzg_quotient: not a function of the header"]


def test_every_dev_form_stands_beside_its_host_form():
    """a row that covers f_dev covers f: the footprint step runs the resident form of the row's own call"""
    for r in W.rows():
        for f in r.functions:
            if f.endswith("_dev"):
                assert f[:-4] in r.functions, (r.family, f)
    cov = W.covered()
    for f in W.header_functions():
        if f.endswith("_dev") and f[:-4] in cov:
            assert f in cov, "%s: its host form has a row" % f


def test_rows_are_well_formed():
    fams = [r.family for r in W.rows()]
    assert len(fams) == len(set(fams))
    ids = ["%s-%s" % (r.family, s[0]) for r, s in W.case_ids()]
    assert len(ids) == len(set(ids))
    for r in W.rows():
        assert r.functions and 1 <= len(r.shapes) and r.reference.strip(), r.family
        assert len(r.shapes) <= 3 or r.family in ("msm_g1", "msm_g2", "kzg_open", "kzg_quotient", "open_fk_poly", "pairing_batch"), r.family
        for sid, small, large in r.shapes:
            assert isinstance(small, dict) and isinstance(large, dict) and small != large, (r.family, sid)
        # a reference that names a test names one that exists
        for path, name in re.findall(r"(tests/test_\w+\.py)::(test_\w+)", r.reference):
            assert re.search(r"^def %s\(" % name, open(os.path.join(ROOT, path)).read(), re.M), (r.family, path, name)
        for path in re.findall(r"tests/\w+\.py", r.reference):
            assert os.path.exists(os.path.join(ROOT, path)), (r.family, path)


def _shapes(family):
    return {r.family: r for r in W.rows()}[family].shapes


def test_the_specified_shapes_are_in_the_table():
    import heavy_cases as H
    import variant_cases as V
    for g in ("msm_g1", "msm_g2"):
        plain = {(s["n"], s["tables"]) for _, s, _ in _shapes(g) if "tables" in s}
        assert plain == {(n, t) for n in (1, 33, 257, 5000) for t in (False, True)}, g
    g1 = [s for _, s, _ in _shapes("msm_g1")]
    assert {"n": 5000, "chunks": V.PIPE_CHUNKS} in g1 and V.PIPE_CHUNKS == 3
    assert {"n": 5000, "opts": {"msm_c": H.C_STATIC}} in g1 and {"n": 5000, "opts": {"msm_c": H.C_WALK}} in g1 and (H.C_STATIC, H.C_WALK) == (16, 12)
    lbs = V.switch_lbs(5000)
    assert [s["opts"]["part_shift"] for s in g1 if "part_shift" in s.get("opts", {})] == sorted({lbs[0], lbs[-1]})
    assert {"heavy": True} in g1
    assert {(s["n"], s["chunks"]) for _, s, _ in _shapes("kzg_open")} == {(n, c) for n in (1, 2, 33, 1025) for c in (0, 3)}
    assert [s["n"] for _, s, _ in _shapes("kzg_quotient")] == [1, 2, 33, 1025]
    for f in ("msm_g1_batch", "kzg_open_batch"):
        assert [(s["m"], s["n"]) for _, s, _ in _shapes(f)] == [(3, 33), (65, 64)]
    assert {(s["log2d"], s["gtab"]) for _, s, _ in _shapes("open_fk_poly")} == {(3, 1), (3, 0), (9, 1), (9, 0)}
    for f in ("open_fk_poly_batch", "vec_commit_batch"):
        assert [(s["log2d"], s["m"]) for _, s, _ in _shapes(f)] == [(3, 65)]
    assert [(s["log2d"], s["log2l"]) for _, s, _ in _shapes("open_fk_cosets_poly")] == [(6, 2)]
    import vec_update_model as UM
    assert [len(UM.passes(s["k"], 8)) for _, s, _ in _shapes("vec_update")] == [1, 2]
    assert [s["log2n"] for _, s, _ in _shapes("fr_fft")] == [5]
    for f in ("g1_mul_batch", "g2_mul_batch"):
        assert [s["n"] for _, s, _ in _shapes(f)] == [1, 65]
    assert {(s["n"], s["wide"]) for _, s, _ in _shapes("pairing_batch")} == {(n, w) for n in (1, 3, 65) for w in (0, 1 << 20)}
    assert [s["n"] for _, s, _ in _shapes("pairing_product")] == [1, 129]
    for f in ("encap_batch", "decap_batch", "encrypt_batch", "decrypt_batch"):
        assert [s["n"] for _, s, _ in _shapes(f)] == [1, 65, 300]
    assert [s["sizes"] for _, s, _ in _shapes("encap_multi")] == [[0, 1, 62, 65]]
    for f in ("kzg_verify_sets", "kzg_verify_sets_each", "kzg_set_pairs"):
        assert [(s["k"], s["n"]) for _, s, _ in _shapes(f)] == [(3, 65), (17, 2)]
    for f in ("g1_compress", "g2_compress", "g1_decompress", "g2_decompress", "g2_subgroup_check"):
        assert [s["n"] for _, s, _ in _shapes(f)] == [1, 65, 300]
    fams = {r.family for r in W.rows()}
    assert {"kzg_verify", "kzg_verify_batch", "kzg_verify_each", "kzg_verify_cosets", "kzg_verify_cosets_each", "kzg_coset_pairs", "kzg_set_polys", "kzg_open_multi",
            "kzg_aggregate", "kzg_verify_multi", "vec_commit"} <= fams


def test_the_larger_call_is_larger():
    """the residue step's call is strictly larger in the size that sizes the family's workspaces"""
    for r, (sid, small, large) in W.case_ids():
        if "heavy" in small or r.family == "kzg_verify":
            assert large.get("larger"), (r.family, sid)
            continue
        if "sizes" in small:
            assert sum(large["sizes"]) > sum(small["sizes"]) and len(large["sizes"]) > len(small["sizes"])
            continue
        keys = [k for k in ("n", "m", "k", "log2d", "log2n", "l") if k in small]
        assert keys, (r.family, sid)
        assert all(large[k] >= small[k] for k in keys) and any(large[k] > small[k] for k in keys), (r.family, sid, small, large)


def test_synthetic_division_is_division():
    p, z = [5, 0, 7, 11, 3], 12345
    q, v = W.synthetic_division(p, z)
    ev = lambda c, x: sum(a * pow(x, i, W.R) for i, a in enumerate(c)) % W.R
    assert v == ev(p, z)
    for x in (0, 1, 99):                                  # p(x) - p(z) = q(x) (x - z)
        assert (ev(p, x) - v) % W.R == ev(q, x) * (x - z) % W.R
    assert W.synthetic_division([9], 4) == ([], 9) and W.synthetic_division([], 4) == ([], 0)


def test_the_hook_is_declared_beside_the_allocation_limit():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"keaki_hip_debug_set_alloc_limit\([^;]*;\s*keaki_status keaki_hip_debug_poison_workspaces\(keaki_hip_ctx\* ctx, uint32_t byte, int32_t also_new\);", hdr)
    # the scratch list of the hook is the list of DevBufs declared directly in keaki_hip_ctx: kem's caches are not in it
    src = open(os.path.join(ROOT, "keaki_amd", "csrc", "internal.h")).read()
    ctx = src[src.index("struct keaki_hip_ctx {"):]
    ctx = ctx[:ctx.index("// instrumentation")]
    declared = set()
    for line in ctx.splitlines():
        m = re.match(r"\s*keaki_internal::DevBuf ([^;]+);", line)
        if m:
            declared |= {n.strip() for n in m.group(1).split(",")}
    scratch = ctx[ctx.index("void for_each_scratch"):]
    listed = set(re.findall(r"&(\w+)", scratch))
    assert declared and declared == listed, (declared ^ listed)
