"""CPU suite: the variant model of tests/variant_cases.py against the sources. Every instantiation the host code can launch must be reached
by a case of tests/test_gpu_variants.py (or be listed as unreachable, with the model's reason); the digit-edge scalars must drive every
window of every plan through each branch of the digit walk; the model must reproduce the operating points the repository records."""
import os
import re

import structured_inputs as S
import variant_cases as V

R = S.R


def _src(name):
    return V._src(name)


def launchable():
    """the instantiations the host code launches, parsed from the launch sites"""
    out = set()
    host = _src("msm_host.hip.h")
    out |= {"k_tile_sort<%s>" % w for w in re.findall(r"KEAKI_TILE_SORT\((\d+)\);", host)}
    m = re.search(r"#define KEAKI_CHUNK_SORT\(L, R, Q\).*", host).group(0)
    masks = re.findall(r"KEAKI_CHUNK_SORT1\(L, R, Q, (true|false)\)", m)
    assert sorted(masks) == ["false", "true"], m
    for geom in re.findall(r"KEAKI_CHUNK_SORT\((\d+, \d+, \d+)\);", host):
        for mk in masks:
            out.add("k_chunk_sort<%s,%s>" % (geom.replace(" ", ""), mk))
    for nt, mode in re.findall(r"KEAKI_ACC\((\d), (ACC_\w+)\);", host):
        out.add(V.acc_g1_name(int(nt), mode))
    for nt, mode, pf in re.findall(r"k_msm_accumulate_g1_u29<(\d), (ACC_\w+), (\d)>", host):
        out.add(V.acc_g1_name(int(nt), mode, int(pf)))
    assert "k_msm_accumulate<F>" in host
    out.add("k_msm_accumulate<Fq>")
    fft = _src("fft_g1.hip")
    body = re.search(r"static void launch_stage3\(.*?\n}\n", fft, re.S).group(0)
    as29 = re.findall(r"k_g1_fft_stage_map<DIT, UNI, GT, (true|false)>", body)
    assert sorted(as29) == ["false", "true"]
    for dit, uni, gt in re.findall(r"launch_stage3<(true|false), (true|false), (true|false)>", fft):
        for a in as29:
            out.add("k_g1_fft_stage_map<%s,%s,%s,%s>" % (dit, uni, gt, a))
    for dit, a in re.findall(r"k_g1_fft_stage4<(true|false), (true|false)>\)", fft):
        out.add("k_g1_fft_stage4<%s,%s>" % (dit, a))
    for occ in re.findall(r"k_encap_fixed<Fq2, (\d)>", _src("ec_batch_g2.hip")):
        out.add("k_encap_fixed<Fq2,%s>" % occ)
    for occ in re.findall(r"k_encap_fixed<Fq, (\d)>", _src("ec_batch_g1.hip")):
        out.add("k_encap_fixed<Fq,%s>" % occ)
    out.add("k_encap_fixed_g2_wide" if "hipLaunchKernelGGL(k_encap_fixed_g2_wide," in _src("ec_batch_g2.hip") else "?")
    # the GT exponentiation: the kernels gt_encap_exp_run launches, and the forms its callers ask for (both tables; B alone into an
    # accumulator; A alone from it)
    run = re.search(r"keaki_status gt_encap_exp_run\(.*?\n}\n", _src("pairing.hip"), re.S).group(0)
    out |= set(re.findall(r"hipLaunchKernelGGL\(((?:pw::)?k_gt_encap_exp\w*),", run))
    for args in re.findall(r"gt_encap_exp_run\(ctx, ([^;]*)\)\);", _src("api.hip")):
        a = [x.strip() for x in args.split(",")]
        assert len(a) in (8, 10), args                   # tab_a, wb_a, tab_b, wb_b, betas, rs, n, gt [, acc_in, acc_out]
        acc_in, acc_out = (a + ["nullptr", "nullptr"])[8:10]
        assert (a[0] == "nullptr") == (acc_out != "nullptr") and (a[2] == "nullptr") == (acc_in != "nullptr"), args
        if acc_in != "nullptr" or acc_out != "nullptr":
            out.add("k_gt_encap_exp[%s]" % ("acc_in" if acc_in != "nullptr" else "acc_out"))
    return out


def test_the_launch_sites_parse_into_the_expected_families():
    ls = launchable()
    fam = lambda p: {k for k in ls if k.startswith(p)}
    assert len(fam("k_tile_sort<")) == 7
    assert len(fam("k_chunk_sort<")) == 8
    assert len(fam("k_msm_accumulate_g1_u29<")) == 7
    assert len(fam("k_g1_fft_stage_map<")) == 12
    assert len(fam("k_g1_fft_stage4<")) == 4
    assert fam("k_encap_fixed<") == {"k_encap_fixed<Fq2,1>", "k_encap_fixed<Fq2,2>", "k_encap_fixed<Fq,1>"}
    assert fam("k_encap_fixed_g2") == {"k_encap_fixed_g2_wide"}
    assert fam("k_gt_encap_exp") | fam("pw::k_gt_encap_exp") == {"k_gt_encap_exp", "pw::k_gt_encap_exp_wide", "k_gt_encap_exp[acc_in]",
                                                                 "k_gt_encap_exp[acc_out]"}


def test_the_case_table_reaches_every_launchable_instantiation():
    reached = set()
    for _, ks in V.cases():
        reached |= set(ks)
    ls = launchable()
    assert set(V.UNREACHABLE) <= ls
    assert not (set(V.UNREACHABLE) & reached)
    missing = ls - reached - set(V.UNREACHABLE)
    assert not missing, "instantiations no case of tests/test_gpu_variants.py reaches: %s" % sorted(missing)


def test_unreachable_instantiations_are_unreachable_for_every_accepted_width():
    """k_tile_sort<11>: the plan of 11 windows is c = 24 only, which neither path accepts"""
    for c in range(3, 25):
        W = V.plan(c)["W"]
        if W == 11:
            assert V.width_refused(c, False) and V.width_refused(c, True), c
    for n in [1 << k for k in range(0, 31)]:
        assert V.plan(V.choose_window(n))["W"] != 11 and V.plan(V.choose_window_shared(n))["W"] != 11


def test_refused_widths_match_the_plans_the_sort_cannot_take():
    """set_option's limits (internal.h) against the sort model: a width is refused iff part_make_shape refuses its plan at any n and
    bin count (generic: all buckets; window tables: the largest window)"""
    for c in range(3, 25):
        p = V.plan(c)
        for shared in (False, True):
            nb = p["max_b"] if shared else p["nb"]
            for n in (1, V.N_SMALL, V.N_LARGE, 1 << 24):
                for lb in (-1, 0, 11):
                    assert (V.part_make_shape(n, p["W"], nb, lb) is None) == V.width_refused(c, shared), (c, shared, n, lb)
    assert [c for c in range(3, 25) if V.width_refused(c, False)] == [20, 21, 22, 23, 24]
    assert [c for c in range(3, 25) if V.width_refused(c, True)] == [24]
    # the C side states the same rule once, checked by the compiler
    assert "static_assert(msm_c_limit_is(MSM_C_MAX, false) && msm_c_limit_is(MSM_C_SHARED_MAX, true)" in _src("msm_g2.hip")


def test_set_option_and_environment_apply_the_same_width_limits():
    """the option table (api.hip: TUNE_OPTIONS) states the limits once for both paths: set_option refuses and the environment
    (KEAKI_MSM_C, KEAKI_MSM_C_SHARED) ignores the widths msm_c_too_wide names, with MSM_C_MAX / MSM_C_SHARED_MAX"""
    api = _src("api.hip")
    assert "TUNE_OPTION(msm_c, msm_c_refuses<MSM_C_MAX>)" in api
    assert "TUNE_OPTION(msm_c_shared, msm_c_refuses<MSM_C_SHARED_MAX>)" in api
    check = re.search(r"template <int MX>\nbool msm_c_refuses\(keaki_hip_ctx\* ctx, const char\* name, long long v\) \{.*?\n\}\n", api, re.S).group(0)
    assert "if (!msm_c_too_wide(v, MX)) return false;" in check and "return true;" in check
    env = re.search(r"void tune_from_env\(Tuning& t\) \{\n.*?\n\}\n", api, re.S).group(0)
    assert "if (!o.refuses || !o.refuses(nullptr, o.name, v)) o.assign(t, v);" in env


def test_digit_edge_scalars_reach_every_branch_of_every_plan():
    need = {"zero", "one", "half", "neg_first", "neg", "full"}
    for c in range(3, 25):
        p = V.plan(c)
        sc = V.digit_edge_scalars(c)
        assert all(0 <= s < R for s in sc), c
        seen = set()
        for s in sc:
            seen |= V.digit_branches(s, c)
            # the digits restate the scalar: sum of +-(bucket + 1) 2^offset(w)
            tot = sum((-(b + 1) if neg else (b + 1)) << p["offs"][w] for w, b, neg in S.msm_digits(s, c))
            assert tot == s, (c, s)
        for w in range(p["W"] - 1):
            want = need - ({"full"} if w == 0 else set())        # no carry enters window 0
            got = {b for ww, b in seen if ww == w}
            assert want <= got, (c, w, want - got)
        assert (p["W"] - 1, "top_max") in seen, c
        assert all(1 << p["offs"][w] in sc for w in range(p["W"]))


def test_switch_matrix_covers_every_geometry_masked_and_unmasked():
    lbs = V.switch_lbs()
    p = V.plan(V.choose_window(V.N_LARGE))
    geoms = {V.part_make_shape(V.N_LARGE, p["W"], p["nb"], lb)["geom"] for lb in lbs}
    assert geoms == {0, 1, 2, 3}
    Ls = {V.reduce_len(p["max_b"], False, l) for l in V.REDUCE_L}
    assert any(p["max_b"] % L for L in Ls), "no ragged last chunk"
    assert V.reduce_len(p["max_b"], False, 4096) == V.reduce_len(p["max_b"]) or 4096 <= p["max_b"]
    runs = V.switch_runs()
    for sw in V.SWITCHES:
        for ss in V.SCALAR_SETS:
            mine = [r for r in runs if r[1] == ss and {k: v for k, v in r[0].items() if k not in ("part_shift", "reduce_l")} == sw]
            assert {r[0].get("part_shift") for r in mine if not r[2]} == set(lbs)
            assert {r[0].get("reduce_l") for r in mine if not r[2]} == set(V.REDUCE_L)
            assert any(r[2] for r in mine)


def test_operating_points_the_repository_records():
    # 2^24 points with tables: c = 22 (README; tests/test_gpu_baseline_sizes.py: test_headline_msm_2p24_with_tables), lb 10, geometry 1
    assert V.auto_shape(1 << 24, True) == (True, 22, 10, 1)
    # generic MSMs of 2^22 points or more: c = 19, 2048 bins, geometry 0
    for k in range(22, 27):
        assert V.auto_shape(1 << k, False) == (False, 19, 11, 0)
    # 2^22 points over tables: the shared path at >= 20 bits (tests/test_gpu_group.py: test_two_contexts_share_one_table_allocation)
    assert V.auto_shape(1 << 22, True)[1] >= 20
    # forced widths the GPU tests assert as window_bits: test_gpu_group.py (5, 9, 13), test_gpu_structured_srs.py (8, 10, 13, 16)
    for c in (5, 9, 13, 8, 10, 16):
        assert V.msm(3000, {"msm_c": c})["c"] == c
        assert V.msm(1000, {}, table_c=c)["c"] == c
    # a forced target is a plan target: 18 bits give the 15-window plan of 17, 21 / 23 those of 20 / 22
    assert V.plan(18)["c"] == 17 and V.plan(21)["c"] == 20 and V.plan(23)["c"] == 22


def test_every_automatic_shape_is_reached_by_a_test():
    """automatic (path, geometry) over 2^5 .. 2^26 points: the small cases reach geometry 3; the large ones are reached by existing tests,
    whose functions must still exist"""
    auto = {(s[0], s[3]) for k in range(5, 27) for s in (V.auto_shape(1 << k, False), V.auto_shape(1 << k, True))}
    reached = {(s[0], s[3]) for s in (V.auto_shape(V.N_LARGE, False), V.auto_shape(V.N_SMALL, False), V.auto_shape(V.N_LARGE, True))}
    for test, n, tables, passes in V.AUTO_LARGE:
        f, name = test.split("::")
        with open(os.path.join(V.ROOT, f)) as fh:
            assert re.search(r"def %s\(" % name, fh.read()), test
        reached.add((lambda s: (s[0], s[3]))(V.auto_shape(n, tables, passes)))
    assert auto <= reached, sorted(auto - reached)
    # geometries 0, 1, 2 are automatic only at 2^19 points or more
    assert {g for _, g in auto} == {0, 1, 2, 3}


def test_gt_exponentiation_model_restates_the_host_code_and_every_form_has_a_case():
    """gt_encap_exp_name against gt_encap_exp_run (pairing.hip) and the split of a_table (api.hip); each of the three forms -- two lanes
    per item, twelve lanes per item, and the two launches around an accumulator -- is reached by a listed case of
    tests/test_gpu_fb_digit_edges.py, whose functions must exist"""
    pairing, api = _src("pairing.hip"), _src("api.hip")
    assert "constexpr size_t GT_EXP_WIDE_AUTO = %d;" % V.GT_EXP_WIDE_AUTO in pairing
    assert "const size_t wide_max = ctx->tune.pair_wide_max < 0 ? GT_EXP_WIDE_AUTO : (size_t)ctx->tune.pair_wide_max;" in pairing
    assert "if (n <= wide_max && d_tab_a && d_tab_b && !d_acc_in && !d_acc_out)" in pairing
    body = re.search(r"static keaki_status a_table\(.*?\n}\n", api, re.S).group(0)
    assert "if (a.n > %d) {" % V.GT_SPLIT_ABOVE in body and body.index("if (!k.gt_a.holds(com_host)) {") < body.index("if (a.n > %d) {" % V.GT_SPLIT_ABOVE)
    assert "FB_TABLES_MIN = %d;" % V.FB_TABLES_MIN in api
    assert V.gt_encap_exp_name(2048) == V.gt_encap_exp_name(2048, split=True) == {"pw::k_gt_encap_exp_wide"}
    assert V.gt_encap_exp_name(2049) == V.gt_encap_exp_name(4096, split=True) == V.gt_encap_exp_name(5, 0) == {"k_gt_encap_exp"}
    assert V.gt_encap_exp_name(4097, split=True) == V.gt_encap_exp_name(4097, 1 << 20, True) == {"k_gt_encap_exp[acc_out]", "k_gt_encap_exp[acc_in]"}
    assert V.gt_encap_exp_name(4097) == {"k_gt_encap_exp"}
    edge = {cid: ks for cid, ks in V.cases() if cid.startswith("fb_edge[")}
    for want in ("k_gt_encap_exp", "pw::k_gt_encap_exp_wide", "k_gt_encap_exp[acc_in]", "k_gt_encap_exp[acc_out]", "k_encap_fixed_g2_wide",
                 "k_encap_fixed<Fq2,1>", "k_encap_fixed<Fq2,2>", "k_encap_fixed<Fq,1>"):
        assert any(want in ks for ks in edge.values()), want
    # the sizes sit where the cases say: 8-bit tables below FB_TABLES_MIN, the twelve-lane form up to GT_EXP_WIDE_AUTO, the split above it
    for wb in V.FB_EDGE_B_WIDTHS:
        assert V.fb_edge_small_n((wb,)) < V.FB_TABLES_MIN
    assert V.fb_edge_small_n() < V.FB_TABLES_MIN <= V.FB_EDGE_WIDE16_N <= V.GT_EXP_WIDE_AUTO < V.GT_SPLIT_ABOVE < V.FB_EDGE_SPLIT_N <= 65536
    assert V.FB_EDGE_WIDE16_N % 4 and V.FB_EDGE_WIDE16_N % 64 and V.FB_EDGE_SPLIT_N % 64          # a ragged last row and block
    with open(os.path.join(V.ROOT, "tests", "test_gpu_fb_digit_edges.py")) as f:
        text = f.read()
    assert "V.fb_edge_runs()" in text
    for name, _, _, _, _ in V.fb_edge_runs():
        assert 'run(h, b, "%s' % name.split("[")[0] in text or 'batches(), "%s"' % name in text, name
    # every width a case walks is covered in full by the side that walks it
    for b1 in [V.FB_EDGE_B1_WIDTHS] + [(wb,) for wb in V.FB_EDGE_B_WIDTHS]:
        rs, b2, b1s = S.fb_edge_sides(S.fb_edge_batch(V.FB_EDGE_R_WIDTHS, V.FB_EDGE_B2_WIDTHS, b1))
        for side, widths in ((rs, V.FB_EDGE_R_WIDTHS), (b2, V.FB_EDGE_B2_WIDTHS), (b1s, b1)):
            for wb in widths:
                assert S.fb_edge_covered(side, wb) == S.fb_edge_required(wb), (b1, wb)


def test_fk_and_encap_models_follow_the_switches():
    # fk_radix4 only acts under fk_uniform; fk_gtab only on the per-lane ladders
    for log2d in V.FK_LOG2D:
        base = V.fk_stage_kernels(log2d, {"fk_uniform": 0})
        assert base == V.fk_stage_kernels(log2d, {"fk_uniform": 0, "fk_radix4": 0})
        assert not any("stage4" in k for k in base)
    big = V.fk_stage_kernels(12, {})
    assert "k_g1_fft_stage4<true,true>" in big and "k_g1_fft_stage4<false,true>" in big
    assert V.encap_g2_fixed_name(V.ENCAP_N, True, 0) == V.encap_g2_fixed_name(V.ENCAP_N, False, 0) == "k_encap_fixed<Fq2,2>"
    assert V.encap_g2_fixed_name(V.ENCAP_N, True, 1) == "k_encap_fixed<Fq2,1>"
    assert 65536 < V.ENCAP_N < 2 * 65536                 # one launch: above 2^16 items, below the two-chunk pipeline
