"""CPU suite: the heavy-bucket model of tests/heavy_cases.py. Every case of tests/test_gpu_msm_heavy.py must put exactly the designed
number of pairs into its designed buckets in every pass -- counted over all scalars, fillers and carries included -- and those counts must
sit on the edges the model claims: the two places the threshold is written, the slice length and its multiples, the clamp of the size
sort, a slice cut by a chunk end under every arrival order, every mode of the combine kernel, the second trip of the segment search.
The tests print what they checked (pytest -s)."""
import functools
import re

import heavy_cases as H
import structured_inputs as S
import variant_cases as V

R = S.R
HM, HS, C2 = H.HM, H.HS, H.C2


@functools.lru_cache(maxsize=1 << 16)
def digits(s, c):
    return tuple(S.msm_digits(s, c))


def has(src, text):
    """`text` occurs in the source, whatever the white space between its tokens"""
    return re.search(r"\s*".join(re.escape(tok) for tok in text.split()), src) is not None


def show(case):
    print("\n".join(H.report(case)))


def bucket_logs(case, label, pas=0):
    """the signed dlogs of the points that designed bucket `label` receives in pass `pas`, scaled by the window's weight over tables"""
    p = V.plan(case["c"])
    w0, b0 = case["designed"][label]
    sizes = H.pass_sizes(case)
    lo = sum(sizes[:pas])
    out = []
    for k, s in zip(case["dlogs"][lo:lo + sizes[pas]], case["scalars"][lo:lo + sizes[pas]]):
        for w, b, neg in digits(s, case["c"]):
            if H.gid(p, case["tables"], w, b) == H.gid(p, case["tables"], w0, b0):
                e = (k << p["offs"][w]) % R if case["tables"] else k
                out.append((R - e) % R if neg else e)
    return out


def test_the_constants_and_rules_the_model_restates_are_the_sources():
    assert (HM, HS, C2, H.SEG_INLINE, H.CNT_BINS, H.STRIDE) == tuple(
        V.K[k] for k in ("HEAVY_MIN", "HEAVY_SLICE", "C2_CAP", "SEG_INLINE", "CNT_BINS", "HEAVY_CHUNK_STRIDE"))
    assert H.CNT_BINS - 1 < HM <= HS and HS <= C2 and C2 % HS == 0
    src, host = V._src("msm.hip.h"), V._src("msm_host.hip.h")
    # the threshold's two places, the slice count's two places, the slice range, the mode rule
    assert has(src, "if (c >= HEAVY_MIN)") and has(src, "bool msm_bucket_is_heavy(u32 cnt) { return cnt >= HEAVY_MIN; }")
    assert len(re.findall(r"nsl\s*=\s*\((?:c|counts\[t\])\s*\+\s*HEAVY_SLICE\s*-\s*1\)\s*/\s*HEAVY_SLICE;", src)) == 2
    assert has(src, "lo = (sid - hv_first[slot]) * HEAVY_SLICE, hi = min(cnt, lo + HEAVY_SLICE);")
    assert has(src, "h[c < CNT_BINS - 1 ? c : CNT_BINS - 1]")
    assert has(src, "__launch_bounds__(256) k_msm_heavy(") and H.STRIDE == 256, "one chunk of the bin per lane and trip"
    assert has(host, H.HV_MODE_RULE)
    assert has(host, "c.lazy_state = K > 1 && c.u29 && std::is_same<F, Fq>::value;")
    assert has(host, "if (st29 == KEAKI_ERR_OOM) { c.lazy_state = false; c.u29 = false;")
    for n, k in ((3 * 23 * 4096, 3), (2 * 11 * 4096, 2), (70001, 3), (1 << 20, 4)):
        b = H.pipe_bounds(n, k)
        assert b[0] == 0 and b[-1] == n and len(b) == k + 1 and all(x < y for x, y in zip(b, b[1:]))


def test_family_1_counts():
    full = [HM - 1, HM, HM + 1, HS - 1, HS, HS + 1, 2 * HS, C2 + 1, 3 * HS + 1]
    assert [n for n, _ in H.COUNTS_FULL] == [1022, 1023, 1024] + full
    assert [n for n, _ in H.COUNTS_G2] == [HM - 1, HM, HS, HS + 1, C2 + 1]
    cases = H.count_cases()
    assert [(c["group"], V.tile_sort_name(V.plan(c["c"])["W"]), c["tables"]) for c in cases] == [
        ("g1", "k_tile_sort<16>", False), ("g1", "k_tile_sort<0>", False), ("g1", "k_tile_sort<16>", True), ("g2", "k_tile_sort<0>", False)]
    for case in cases:
        show(case)
        a = H.analyse(case)[0]
        targets = H.COUNTS_G2 if case["group"] == "g2" else H.COUNTS_FULL
        p = V.plan(case["c"])
        win = H.windows(p)
        seen, signs_of = set(), {}
        for s in set(case["scalars"]):
            for w, b, neg in digits(s, case["c"]):
                signs_of.setdefault(H.gid(p, case["tables"], w, b), set()).add(neg)
        for n, kind in targets:
            d = a["buckets"]["%d/%s" % (n, kind)]
            assert d["count"] == n and d["heavy"] == (n >= HM) and d["size_bin"] == min(n, 1023)
            assert d["slices"] == (0 if n < HM else 1 if n <= HS else 2 if n <= 2 * HS else 3 if n <= 3 * HS else 4)
            assert d["last"] == (0 if n < HM else n if n <= HS else 1 if n % HS == 1 else HS)
            # signs and windows of the bucket's pairs, from the digits of the scalars
            w0, b0 = case["designed"]["%d/%s" % (n, kind)]
            assert signs_of[d["gid"]] == {"w0+": {False}, "w0-": {True}, "w0+-": {False, True}, "mid": {False}, "top": {False}}[kind]
            assert w0 == win[kind[:2] if kind[0] == "w" else kind]
            if d["heavy"]:
                seen.add(kind)
        assert seen == {"w0+", "w0-", "w0+-", "mid", "top"} if case["group"] == "g1" else seen == {"w0-", "w0+-", "mid", "top"}
        carry = a["buckets"]["carry"]
        assert carry["count"] == sum(n if k == "w0-" else n // 2 if k == "w0+-" else 0 for n, k in targets) and carry["heavy"]
        light = [n for g, n in a["counts"].items() if n < HM]
        assert len(light) > 10000, "the ordinary bucket kernel has work in the same launch"
        assert len(a["heavy"]) == sum(n >= HM for n, _ in targets) + 1
        assert len(case["scalars"]) <= 1 << 20
    # a bin of more chunks than the bucket-major table holds, with heavy buckets in it (seg_word's chunk-major rows)
    assert any(d["heavy"] and d["bin_chunks"] > H.SEG_INLINE for case in cases for d in H.analyse(case)[0]["buckets"].values())
    for case in H.all_exact_cases():
        show(case)
        a = H.analyse(case)[0]
        assert set(a["counts"].values()) == {HM} and len(a["counts"]) == 3 == len(a["heavy"])
    assert len(H.all_exact_case("g2", H.C_WALK, False)["scalars"]) <= 1 << 15, "the G2 case that is also compared with the oracle's MSM"


def test_family_2_a_slice_straddles_a_chunk_end_under_every_order():
    for case in H.straddle_cases():
        show(case)
        a = H.analyse(case)[0]
        alone, mixed = a["buckets"]["alone"], a["buckets"]["mixed"]
        assert alone["count"] == alone["bin_pairs"] == H.STRADDLE_ALONE and 1 < alone["bin_chunks"] <= H.SEG_INLINE and alone["slices"] == 4
        assert [b for b in H.straddle_bounds(case, "alone")] == [(C2, C2, C2)], "alone in its bin: chunk ends are slice ends"
        comps = [d for label, d in a["buckets"].items() if label.startswith("companion")]
        assert len(comps) == H.STRADDLE_COMPANIONS and all(d["bin"] == mixed["bin"] and 0 < d["count"] < HM for d in comps)
        assert mixed["count"] == H.STRADDLE_B and mixed["bin_chunks"] > H.SEG_INLINE and mixed["bin"] != alone["bin"]
        assert mixed["bin_pairs"] == mixed["count"] + sum(d["count"] for d in comps)
        assert H.STRADDLE_RATIO[0] != H.STRADDLE_RATIO[1] and sum(d["count"] for d in comps) * H.STRADDLE_RATIO[0] == mixed["count"] * H.STRADDLE_RATIO[1]
        bounds = H.straddle_bounds(case, "mixed")
        assert len(bounds) == mixed["bin_chunks"] - 1
        cut = H.straddled(bounds, mixed["count"])
        for e, lo, hi in bounds:
            print("    chunk end %6d: between %5d and %5d pairs of the bucket before it%s" % (
                e, lo, hi, " -- inside slice %d under every order" % (lo // HS) if (e, lo, hi) in cut else ""))
            assert 0 <= lo <= hi <= mixed["count"]
        assert cut, "no chunk end provably inside a slice"
        for e, lo, hi in cut:
            assert 0 < lo and hi < mixed["count"] and not any(lo <= k * HS <= hi for k in range(mixed["slices"] + 1))


def test_family_3_exceptional_additions():
    for case in H.exceptional_cases():
        show(case)
        a = H.analyse(case)[0]
        cancel_only = "cancel_only" in case["name"]
        assert len(case["scalars"]) <= 1 << 17
        for label, d in a["buckets"].items():
            logs = bucket_logs(case, label)
            assert d["heavy"] and len(logs) == d["count"]
            if label.startswith("same"):
                assert len(set(logs)) == 1 and logs[0] and d["count"] == {"same/S+1": HS + 1, "same/2S": 2 * HS}[label]
                # what the docstring calls guaranteed: alone in its bin, so every full slice is one run of HEAVY_SLICE pairs inside
                # one segment and each of the 256 lanes gets HEAVY_SLICE / 256 >= 2 copies -- equal sums at every level of the tree
                assert d["bin_pairs"] == d["count"] and d["bin_chunks"] == 1
                whole = H.single_segment_slices(case, label)
                print("    %s: chunk-end bounds %s, full slices inside one segment %s, %d copies per lane" % (
                    label, H.straddle_bounds(case, label), whole, HS // H.STRIDE))
                assert whole == list(range(d["count"] // HS)) and whole, (label, whole)
                assert HS % H.STRIDE == 0 and HS // H.STRIDE >= 2
                assert has(V._src("msm.hip.h"), "for (u32 q = threadIdx.x; q < nn; q += 256)")
            elif label.startswith("cancel"):
                k = max(logs, key=logs.count)
                assert set(logs) == {k, R - k} and sum(logs) % R == (k if label == "cancel+1" else 0)
            else:
                assert logs.count(0) == 64 and len(set(logs)) == HM + 1
        if cancel_only:
            assert H.expected_dlog(case) == 0 and len(a["counts"]) == 2
        else:
            assert H.expected_dlog(case) != 0 and len(a["counts"]) > 10000
    doc = H.exceptional_case.__doc__
    assert "GUARANTEED" in doc and "ORDER-DEPENDENT" in doc
    assert HS // 256 >= 2, "a full slice gives every lane at least two copies: the lane's second addition doubles"


def test_family_4_pass_matrix_and_reach_table():
    cases = H.matrix_cases()
    assert [(c["group"], c["passes"], c["tables"], c["acc_u29"], c["refuse_state"]) for c in cases] == [
        ("g1", 3, False, 1, False), ("g1", 3, True, 1, False), ("g1", 3, False, 0, False), ("g1", 3, False, 1, True), ("g2", 2, False, 1, False)]
    modes = {"g1": set(), "g2": set()}
    for case in cases:
        show(case)
        an = H.analyse(case)
        seqs = H.sequences(case["passes"])
        assert len(seqs) == 3 ** case["passes"] == len(set(seqs))
        for j, a in enumerate(an):
            for q in seqs:
                d = a["buckets"][q]
                assert (d["count"] == 0) == (q[j] == "E") and (d["count"] == H.LIGHT) == (q[j] == "L") and d["heavy"] == (q[j] == "H"), (q, j, d)
            designed = {d["gid"] for d in a["buckets"].values()}
            assert {g for g, _ in a["heavy"]} <= designed and len(a["counts"]) > 10000
        # the stored state: one point in pass 0 that equals (is opposite to) the heavy sum of pass 1
        for label, sign in (("dbl", 1), ("neg", -1)):
            q0, heavy = bucket_logs(case, label, 0), bucket_logs(case, label, 1)
            assert len(q0) == 1 and len(heavy) == HM and len(set(heavy)) == 1 and (q0[0] - sign * sum(heavy)) % R == 0
            assert an[1]["buckets"][label]["heavy"]
        if case["passes"] == 3:
            assert an[2]["buckets"]["neg"]["count"] == H.LIGHT, "a further pass adds into the emptied bucket"
        print("  reach table (group, mode, pass, bucket, pairs, slices):")
        for row in H.reach(case):
            print("    %s %-8s pass %d %-4s %6d pairs %d slices" % row)
            assert row[5] >= 1
            modes[row[0]].add(row[1])
        assert len(case["scalars"]) <= 1 << 20
    assert modes == H.REQUIRED_MODES, modes
    lazy = {(row[1], row[2]) for row in H.reach(cases[0])}
    assert lazy == {("HV_SET29", 0), ("HV_ADD29", 1), ("HV_ADD", 2)}
    assert {row[1] for row in H.reach(cases[3])} == {"HV_SET", "HV_ADD"}, "without the parked-state workspace the passes keep the canonical bucket"


def test_family_5_more_chunks_in_one_bin_than_one_trip_covers():
    m = H.many_chunks_model()
    print(m)
    assert m["n"] == 256 * C2 + C2 + 1 and m["bucket"]["count"] == m["n"] == m["bucket"]["bin_pairs"]
    assert m["bucket"]["bin_chunks"] == H.STRIDE + 2 and m["trips"] == 2 and m["bucket"]["last"] == 1
    assert m["bucket"]["slices"] == 2 * (H.STRIDE + 1) + 1
    assert V.part_make_shape(m["n"], V.plan(m["c"])["W"], V.plan(m["c"])["nb"]) is not None
    assert H.many_chunks_dlog([1, 2, 3]) == (m["n"] // 3 * 6 + sum([1, 2, 3][:m["n"] % 3])) % R
