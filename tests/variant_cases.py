"""Which kernel instantiation a call reaches, and the cases that reach them all -- TEST INFRASTRUCTURE (a plain module, imported by
tests/test_variant_cases_model.py and tests/test_gpu_variants.py; tests/heavy_cases.py builds on its plan and sort model; no GPU import).

The library ships several instantiations of its MSM, FK23 and fixed-base kernels; host code picks one from the input size and the tuning
switches of keaki_hip_ctx_set_option (also settable through KEAKI_* at context creation). This module restates those host-side choices
(keaki_amd/csrc/msm_host.hip.h: choose_window, choose_window_shared, msm_plan_call, msm_launch_accumulate; msm.hip.h: msm_make_plan, part_make_shape; fft_g1.hip:
stage_map, run_stages; ec_batch_g2.hip: encap_g2_fixed_run; pairing.hip: gt_encap_exp_run; api.hip: a_table), builds scalars that drive
every window of a plan through each branch of the digit walk, and lists the GPU cases of tests/test_gpu_variants.py and
tests/test_gpu_fb_digit_edges.py with the instantiations each one reaches. The CPU test checks the list against the launches it parses out
of the sources, so a variant added without a case fails there.
"""
import os
import re

import structured_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "keaki_amd", "csrc")
R = S.R


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header_consts():
    """the sort's limits as the headers define them (read, not copied)"""
    t = _src("msm.hip.h")
    out = {}
    for name in ("T1_THREADS", "T1_PER", "T1_CAP", "PART_MAX_BINS", "C2_CAP", "PART_MAX_FINE_SHIFT", "SEG_INLINE", "CNT_BINS", "HEAVY_MIN",
                 "HEAVY_SLICE"):
        m = re.search(r"constexpr u32 (?:\w+ = \d+, )*%s = (\d+)" % name, t)
        out[name] = int(m.group(1))
    # the chunks of a bin that one trip of k_msm_heavy's segment search covers (one per lane of the workgroup)
    m = re.search(r"for \(u32 cb = 0; cb < bm\.nch && vbase < hi; cb \+= (\d+)\)", t)
    out["HEAVY_CHUNK_STRIDE"] = int(m.group(1))
    m = re.search(r"constexpr int MSM_C_MAX = (\d+), MSM_C_SHARED_MAX = (\d+);", _src("internal.h"))
    out["MSM_C_MAX"], out["MSM_C_SHARED_MAX"] = int(m.group(1)), int(m.group(2))
    return out


K = header_consts()


# ---- the tuning options: Tuning (internal.h) and its table TUNE_OPTIONS (api.hip) ------------------------------------------------------
def _diag_lines(body):
    """(line, under #ifdef KEAKI_DIAG) for each line of a source excerpt"""
    diag = False
    for line in body.splitlines():
        if line.strip().startswith("#ifdef KEAKI_DIAG"):
            diag = True
        elif line.strip().startswith("#endif"):
            diag = False
        else:
            yield line, diag


def _c_value(expr):
    expr = expr.strip()
    if expr in ("true", "false"):
        return int(expr == "true")
    m = re.fullmatch(r"(-?\d+) << (\d+)", expr)
    return int(m.group(1)) << int(m.group(2)) if m else int(expr)


def tuning_members():
    """the members of struct Tuning as internal.h declares them: name -> (default as an int, diagnostic build only)"""
    body = re.search(r"struct Tuning \{\n(.*?)\n\};", _src("internal.h"), re.S).group(1)
    out = {}
    for line, diag in _diag_lines(body):
        m = re.match(r"\s+(?:int|bool|long long|unsigned|size_t) (\w+) = ([^;]+);", line)
        if m:
            out[m.group(1)] = (_c_value(m.group(2)), diag)
    return out


def table_options():
    """the entries of TUNE_OPTIONS (api.hip) in table order: [(name, diagnostic build only)]"""
    body = re.search(r"const TuneOption TUNE_OPTIONS\[\] = \{\n(.*?)\n\};", _src("api.hip"), re.S).group(1)
    return [(name, diag) for line, diag in _diag_lines(body) for name in re.findall(r"TUNE_OPTION\((\w+)", line)]


def shipped_options():
    """option name -> default for the options of the shipped library (what keaki_hip_ctx_set_option accepts outside KEAKI_DIAG)"""
    members = tuning_members()
    return {name: members[name][0] for name, diag in table_options() if not diag}


# ---- MSM: plan, window choice, bucket sort shape, reduction, kernels ---------------------------------------------------------------------
def plan(c_target):
    """msm_make_plan -> dict(c, W, k, offs, widths, nb, max_b)"""
    c, W, k, offs, widths = S.msm_plan(c_target)
    nbs = [(1 << widths[w]) if w == W - 1 else (1 << (widths[w] - 1)) for w in range(W)]
    return {"c": c, "W": W, "k": k, "offs": offs, "widths": widths, "nb": sum(nbs), "max_b": max(nbs), "nbs": nbs}


def choose_window(n, forced=0):
    if 3 <= forced <= K["MSM_C_MAX"]:
        return forced
    if n < 32:
        return 3
    best, bc = 1e300, 3
    for c in range(3, 23):
        p = plan(c)
        if p["nb"] > K["PART_MAX_BINS"] << K["PART_MAX_FINE_SHIFT"]:
            continue
        cost = float(n) * p["W"] + 2.8 * p["nb"]
        if p["nb"] < 131072.0:
            cost *= 131072.0 / p["nb"]
        if cost < best:
            best, bc = cost, c
    return bc


def choose_window_shared(n, forced=0):
    if 3 <= forced <= K["MSM_C_SHARED_MAX"]:
        return forced
    best, bc = 1e300, 8
    for c in range(8, 24):
        p = plan(c)
        if p["max_b"] > K["PART_MAX_BINS"] << K["PART_MAX_FINE_SHIFT"]:
            continue
        cost = float(n) * p["W"] + 2.8 * p["max_b"]
        if p["max_b"] < 131072.0:
            cost *= 131072.0 / p["max_b"]
        if cost < best:
            best, bc = cost, c
    return bc


def width_refused(c, shared):
    """set_option refuses the widths whose plan the bucket sort cannot address (the values between the limit and 24)"""
    return (K["MSM_C_SHARED_MAX"] if shared else K["MSM_C_MAX"]) < c <= 24


def part_make_shape(n, W, nb, lb_override=-1):
    """-> dict(lb, geom, tile, te, lg, shift, hb) or None (refused: 'window too large'). shift / hb: the low / high fine bits around the
    bin bits of a global bucket id (part_bin)"""
    lg = 0
    while (1 << lg) < nb:
        lg += 1
    pairs = n * W
    lb_max = 11 if pairs > (K["C2_CAP"] << 13) else 10
    lb = 0
    while lb < lb_max and (K["C2_CAP"] << lb) < pairs:
        lb += 1
    if 0 <= lb_override <= 11:
        lb = lb_override
    lb = min(lb, lg)
    if lg - lb > K["PART_MAX_FINE_SHIFT"]:
        lb = lg - K["PART_MAX_FINE_SHIFT"]
    if lb > 11:
        return None
    tile = min(K["T1_CAP"] // W, K["T1_THREADS"] * K["T1_PER"])
    te = tile * W
    mean = te >> lb
    geom = 0 if mean <= 24 else 1 if mean <= 48 else 2 if mean <= 100 else 3
    hb = min(lg - lb, 3)
    return {"lb": lb, "geom": geom, "tile": tile, "te": te, "lg": lg, "shift": lg - lb - hb, "hb": hb}


def part_bin(shape, g):
    """the bin of global bucket id g (msm.hip.h: part_bin): the lb bits above the `shift` low fine bits"""
    return (g >> shape["shift"]) & ((1 << shape["lb"]) - 1)


def bucket_base(p, w):
    """first global bucket id of window w on the generic path (msm.hip.h: msm_bucket_base; over window tables every window starts at 0)"""
    c, k = p["c"], p["k"]
    return w * (1 << (c - 1)) if w <= k else k * (1 << (c - 1)) + (w - k) * (1 << (c - 2))


def reduce_len(max_b, g2=False, reduce_l=0):
    """the chunk length L of k_msm_reduce (msm_plan_call)"""
    if g2:
        L = 8 if max_b >= 64 else max_b
    else:
        L = 32 if max_b >= 1 << 21 else 16 if max_b >= 1 << 20 else 8 if max_b >= 64 else max_b
    if 1 <= reduce_l <= 4096 and reduce_l <= max_b:
        L = reduce_l
    return L


CHUNK_GEOMS = {0: (8, 1, 16), 1: (16, 1, 16), 2: (16, 2, 8), 3: (16, 4, 4)}
TILE_STATIC = range(11, 17)


def tile_sort_name(W):
    return "k_tile_sort<%d>" % (W if W in TILE_STATIC else 0)


def chunk_sort_name(geom, masked):
    return "k_chunk_sort<%d,%d,%d,%s>" % (CHUNK_GEOMS[geom] + ("true" if masked else "false",))


ACC_MODES = {"WHOLE": "ACC_WHOLE", "FIRST": "ACC_FIRST", "MIDDLE": "ACC_MIDDLE", "LAST": "ACC_LAST"}


def acc_g1_name(nt, mode, pf=2):
    return "k_msm_accumulate_g1_u29<%d,%s,%d>" % (nt, mode, pf)


def accumulate_names(opts, passes):
    """the G1 bucket kernel of each pass (msm_launch_accumulate). opts: the switches; passes: K (1 = a whole MSM)"""
    if not opts.get("acc_u29", 1):
        return ["k_msm_accumulate<Fq>"] * passes
    if passes == 1:
        if opts.get("acc_nt", 0):
            return [acc_g1_name(1, "ACC_WHOLE")]
        if not opts.get("acc_prefetch", 1):
            return [acc_g1_name(0, "ACC_WHOLE", 0)]
        if not opts.get("acc_idxq", 1):
            return [acc_g1_name(0, "ACC_WHOLE", 1)]
        return [acc_g1_name(0, "ACC_WHOLE")]
    return [acc_g1_name(0, "ACC_FIRST")] + [acc_g1_name(0, "ACC_MIDDLE")] * (passes - 2) + [acc_g1_name(0, "ACC_LAST")]


def msm(n, opts=None, srs_len=None, table_c=None, g2=False, chunk_sizes=None):
    """One MSM as msm_plan_call plans it and msm_dev runs it. table_c: the window target the SRS tables were built with (None: no tables). chunk_sizes: the pass
    lengths of a chunked call. -> dict(shared, plan, c, L, shapes, refused, kernels)"""
    opts = opts or {}
    srs_len = n if srs_len is None else srs_len
    shared = table_c is not None and (2 * n > srs_len or opts.get("msm_short_tables", -1) != 0)
    p = plan(table_c if shared else choose_window(n, opts.get("msm_c", 0)))
    nb = p["max_b"] if shared else p["nb"]
    L = reduce_len(p["max_b"], g2, opts.get("reduce_l", 0))
    chunks = chunk_sizes or [n]
    shapes = [part_make_shape(m, p["W"], nb, opts.get("part_shift", -1)) for m in chunks]
    out = {"shared": shared, "plan": p, "c": p["c"], "L": L, "shapes": shapes, "refused": any(s is None for s in shapes), "kernels": set()}
    if out["refused"] or n == 0:
        return out
    ks = out["kernels"]
    masked = bool(opts.get("cs_masked", 1))
    for s in shapes:
        ks.add(tile_sort_name(p["W"]))
        ks.add(chunk_sort_name(s["geom"], masked))
    if not g2:
        ks.update(accumulate_names(opts, len(chunks)))
    ks.add("k_msm_reduce<%s>" % ("Fq2" if g2 else "Fq"))
    return out


# ---- the digit-edge scalars ---------------------------------------------------------------------------------------------------------
# the coefficient (digit + incoming carry) a non-top window is driven to, in an order where each target's predecessor leaves the carry it
# needs: 0 follows a window without carry, full one with (coef == full: zero digit, carry on -- the `coef != full` branch)
EDGE_TARGETS = ("one", "zero", "half", "half+1", "full", "full-1")


def _target(name, wd):
    full = 1 << wd
    return {"zero": 0, "one": 1, "half": full >> 1, "half+1": (full >> 1) + 1, "full-1": full - 1, "full": full}[name]


def digit_edge_scalars(c_target):
    """Scalars < r that put every non-top window of the plan through each branch of msm_for_each_digit_canon / msm_digits_static: coef
    0, 1, half, half + 1, full - 1, and full through an incoming carry (window 0 has no carry in: there `full` becomes full - 1). Scalar j
    drives window w to EDGE_TARGETS[(w + j) % 6]. The top window of these scalars is lowered to the largest value that keeps the scalar
    below r. Then r - 1 and r - 2 (the largest top-window values) and 2^offset(w) for every window."""
    p = plan(c_target)
    W, offs, widths = p["W"], p["offs"], p["widths"]
    out = []
    for j in range(len(EDGE_TARGETS)):
        low, carry = 0, 0
        for w in range(W - 1):
            coef = _target(EDGE_TARGETS[(w + j) % len(EDGE_TARGETS)], widths[w])
            d = min(max(coef - carry, 0), (1 << widths[w]) - 1)
            low |= d << offs[w]
            carry = 1 if d + carry > (1 << (widths[w] - 1)) else 0
        top = (R - 1 - low) >> offs[W - 1]              # lowered where needed: low + top * 2^offset < r
        out.append(low + (top << offs[W - 1]))
    out += [R - 1, R - 2]
    out += [1 << offs[w] for w in range(W)]
    return out


def digit_branches(s, c_target):
    """{(window, branch)} the digit walk takes for canonical scalar s (branch: zero / pos / half / neg / full, or top)"""
    p = plan(c_target)
    W, offs, widths = p["W"], p["offs"], p["widths"]
    seen, carry = set(), 0
    for w in range(W):
        wd = widths[w]
        full, half = 1 << wd, 1 << (wd - 1)
        coef = ((s >> offs[w]) & (full - 1)) + carry
        if w == W - 1:
            seen.add((w, "top_max" if coef == ((R - 1) >> offs[w]) + carry and s >= R - 2 else "top"))
            continue
        if coef > half:
            carry = 1
            seen.add((w, "full" if coef == full else "neg_first" if coef == half + 1 else "neg"))
        else:
            carry = 0
            seen.add((w, "zero" if coef == 0 else "one" if coef == 1 else "half" if coef == half else "pos"))
    return seen


# ---- FK23 stages ----------------------------------------------------------------------------------------------------------------------
def _stage_map_name(dit, uni, gt, as29):
    return "k_g1_fft_stage_map<%s,%s,%s,%s>" % tuple("true" if x else "false" for x in (dit, uni, gt, as29))


def _stage4_name(dit, as29):
    return "k_g1_fft_stage4<%s,%s>" % ("true" if dit else "false", "true" if as29 else "false")


def fk_stage_kernels(log2d, opts=None):
    """the butterfly kernels of open_fk_poly on a fresh SRS handle (hat_s: DIF over 2d points; then DIT_d, DIF_d of the odd half), as
    run_stages / stage_map pick them. The table workspace (fk_gtab) is assumed to fit (the cases stay far below FK_TAB_LANES)."""
    opts = opts or {}
    uni_on, gtab, r4_on, as29 = (bool(opts.get(k, 1)) for k in ("fk_uniform", "fk_gtab", "fk_radix4", "fk_addsub29"))
    r4 = r4_on and uni_on
    out = set()
    d = 1 << log2d

    def stage(m, half, dit):
        if uni_on and m // (2 * half) >= 64:
            out.add(_stage_map_name(dit, True, False, as29))
        else:
            out.add(_stage_map_name(dit, False, gtab, as29))

    def pairable(m, h):
        return r4 and h >= 8 and m // (4 * h) >= 64 and (m // 4) % 64 == 0

    def run(m, first, last, dit):
        if dit:
            half = first
            while half <= last:
                if 2 * half <= last and pairable(m, half):
                    out.add(_stage4_name(True, as29))
                    half <<= 2
                else:
                    stage(m, half, True)
                    half <<= 1
        else:
            half = first
            while half >= last and half >= 1:
                h = half // 2
                if h >= last and h >= 1 and pairable(m, h):
                    out.add(_stage4_name(False, as29))
                    half >>= 2
                else:
                    stage(m, half, False)
                    half >>= 1
    run(2 * d, d, 1, False)
    if d > 1:
        run(d, 1, d // 2, True)
        run(d, d // 2, 1, False)
    return out


# ---- G2 fixed-base kernel of encapsulate -----------------------------------------------------------------------------------------------
def encap_g2_fixed_name(n, share_simds, fb_occ1, wide_max=2048):
    if n <= wide_max:
        return "k_encap_fixed_g2_wide"
    return "k_encap_fixed<Fq2,%d>" % (1 if (n <= 65536 and not share_simds) or fb_occ1 else 2)


# ---- GT fixed-base exponentiation of encapsulate ---------------------------------------------------------------------------------------
GT_EXP_WIDE_AUTO, GT_SPLIT_ABOVE, FB_TABLES_MIN = 2048, 4096, 256


def gt_encap_exp_name(n, wide_max=GT_EXP_WIDE_AUTO, split=False):
    """the launches of GT_i = A^(r_i) B^(-(r_i v_i)) (pairing.hip: gt_encap_exp_run; api.hip: a_table, encap_items). split: the call
    builds the table of a new commitment; above 4096 items it then runs B's factor first (tab_a null, acc_out) and A's factor behind it
    (tab_b null, acc_in), and a launch with an accumulator or a single table is never the twelve-lane one. -> the set of launches"""
    if split and n > GT_SPLIT_ABOVE:
        return {"k_gt_encap_exp[acc_out]", "k_gt_encap_exp[acc_in]"}
    return {"pw::k_gt_encap_exp_wide" if n <= wide_max else "k_gt_encap_exp"}


# the cases of tests/test_gpu_fb_digit_edges.py: (id, items, pair_wide_max, the commitment is new to the context, GT path). The small
# batches are the unique items of S.fb_edge_batch plus the item r = 0; the larger ones tile them.
FB_EDGE_R_WIDTHS, FB_EDGE_B2_WIDTHS, FB_EDGE_B1_WIDTHS = (8, 13, 16), (8, 16), (16,)
FB_EDGE_B_WIDTHS = [8, 11, 13, 16, 20]
FB_EDGE_WIDE16_N, FB_EDGE_SPLIT_N = 261, GT_SPLIT_ABOVE + 3


def fb_edge_small_n(b1_widths=FB_EDGE_B1_WIDTHS):
    return len(S.fb_edge_batch(FB_EDGE_R_WIDTHS, FB_EDGE_B2_WIDTHS, b1_widths)) + 1


def fb_edge_runs():
    ns = fb_edge_small_n()
    out = [("small", ns, -1, True, True), ("repeat", ns, -1, False, True), ("wide16", FB_EDGE_WIDE16_N, -1, True, True),
           ("lane", FB_EDGE_WIDE16_N, 0, True, True), ("lane_repeat", FB_EDGE_WIDE16_N, 0, False, True),
           ("split", FB_EDGE_SPLIT_N, -1, True, True), ("split_repeat", FB_EDGE_SPLIT_N, -1, False, True),
           ("pairing", FB_EDGE_WIDE16_N, -1, True, False)]
    for wb in FB_EDGE_B_WIDTHS:
        out += [("b_width[%d,wide]" % wb, fb_edge_small_n((wb,)), -1, True, True), ("b_width[%d,lane]" % wb, fb_edge_small_n((wb,)), 0, False, True)]
    return out


def fb_edge_kernels(n, pair_wide_max, new, gt):
    """the per-item kernels of one encap_batch call on a context whose [tau]_2 tables hold the call's setup"""
    wide_max = GT_EXP_WIDE_AUTO if pair_wide_max < 0 else pair_wide_max
    ks = {encap_g2_fixed_name(n, n >= FB_TABLES_MIN and new and gt, 0, wide_max)}
    return ks | (gt_encap_exp_name(n, wide_max, new) if gt else {"k_encap_fixed<Fq,1>"})


# ---- the case table of tests/test_gpu_variants.py ----------------------------------------------------------------------------------------
N_SMALL, N_LARGE = 500, 1 << 14
G1_WINDOW_C = list(range(3, 25))
G1_SHARED_C = list(range(3, 25))
G2_WINDOW_C = [3, 8] + [c for c in range(9, 25) if 11 <= plan(c)["W"] <= 16] + [17, 19]
G2_WINDOW_C = sorted(set(G2_WINDOW_C))
G2_N = 600
SWITCHES = [{}, {"acc_nt": 1}, {"acc_prefetch": 0}, {"acc_idxq": 0}, {"cs_masked": 0}, {"acc_u29": 0}]
REDUCE_L = [1, 2, 3, 7, 8, 31, 64, 1000, 4096]
SCALAR_SETS = ("random", "edge", "collide", "heavy")
FK_LOG2D = [2, 3, 6, 9, 12]
FK_OPTS = [{"fk_uniform": u, "fk_gtab": g, "fk_addsub29": a} for u, g in ((0, 0), (0, 1), (1, 0)) for a in (1, 0)]
ENCAP_N = 100000
ENCAP_RUNS = [(occ, new) for occ in (0, 1) for new in (True, False)]
PIPE_CHUNKS = 3


def switch_lbs(n=N_LARGE):
    """the part_shift values whose bin count the sort keeps for the switch matrix's automatic plan (every other one is clamped)"""
    p = plan(choose_window(n))
    return [lb for lb in range(12) if part_make_shape(n, p["W"], p["nb"], lb)["lb"] == lb]


def switch_runs(n=N_LARGE):
    """(opts, scalar set) of the switch matrix: every switch setting x every scalar set, one MSM per accepted part_shift, reduce_l
    cycling alongside; then the chunked call under the same setting"""
    out = []
    lbs = switch_lbs(n)
    for sw in SWITCHES:
        for ss in SCALAR_SETS:
            for i in range(max(len(lbs), len(REDUCE_L))):
                out.append((dict(sw, part_shift=lbs[i % len(lbs)], reduce_l=REDUCE_L[i % len(REDUCE_L)]), ss, None))
            out.append((dict(sw), ss, PIPE_CHUNKS))
    return out


def pipe_chunk_sizes(n, k, growth=100):
    """msm_pipe_chunks = k, msm_pipe_growth = 100: equal chunks (the host entry's split, api.hip; the model needs their count only)"""
    base = n // k
    return [base + (1 if i < n % k else 0) for i in range(k)]


def cases():
    """[(case id, model result or kernel set)]: every GPU case of tests/test_gpu_variants.py and tests/test_gpu_fb_digit_edges.py with
    what it reaches"""
    out = []
    for n in (N_SMALL, N_LARGE):
        for c in G1_WINDOW_C:
            if not width_refused(c, False):
                out.append(("g1_window[c=%d,n=%d]" % (c, n), msm(n, {"msm_c": c})["kernels"]))
        for c in G1_SHARED_C:
            if not width_refused(c, True):
                m = N_LARGE if n == N_SMALL else n
                out.append(("g1_shared[c=%d,n=%d]" % (c, n), msm(n, {"msm_short_tables": 1}, srs_len=m, table_c=choose_window_shared(m, c))["kernels"]))
    for c in G2_WINDOW_C:
        if not width_refused(c, False):
            out.append(("g2_window[c=%d]" % c, msm(G2_N, {"msm_c": c}, g2=True)["kernels"]))
        if not width_refused(c, True):
            out.append(("g2_shared[c=%d]" % c, msm(G2_N, {}, table_c=c, g2=True)["kernels"]))
    for opts, ss, chunks in switch_runs():
        sizes = pipe_chunk_sizes(N_LARGE, chunks) if chunks else None
        out.append(("switch[%s,%s,%s]" % (sorted(opts.items()), ss, chunks), msm(N_LARGE, opts, chunk_sizes=sizes)["kernels"]))
    for log2d in FK_LOG2D:
        for o in FK_OPTS:
            out.append(("fk[%d,%s]" % (log2d, sorted(o.items())), fk_stage_kernels(log2d, o)))
    for occ, new in ENCAP_RUNS:
        out.append(("encap[fb_occ1=%d,new=%s]" % (occ, new), {encap_g2_fixed_name(ENCAP_N, new, occ)}))
    for name, n, wide, new, gt in fb_edge_runs():          # tests/test_gpu_fb_digit_edges.py
        out.append(("fb_edge[%s]" % name, fb_edge_kernels(n, wide, new, gt)))
    return out


# ---- automatic shapes at large n: the existing tests that reach them ------------------------------------------------------------------
# (test, n, SRS with window tables, passes): generic MSMs and MSMs over window tables at the sizes whose automatic plan and bin count
# no small case of the variant module reaches
AUTO_LARGE = [
    ("tests/test_gpu_baseline_sizes.py::test_config4_chunk_2p23_of_2p26_identity", 1 << 23, False, 1),
    ("tests/test_gpu_baseline_sizes.py::test_config4_chunk_2p23_of_2p26_identity", 1 << 23, True, 1),
    ("tests/test_gpu_baseline_sizes.py::test_headline_msm_2p24_with_tables", 1 << 24, True, 1),
    ("tests/test_gpu_baseline_sizes.py::test_config2_msm_2p20_bit_exact_vs_oracle", 1 << 20, False, 1),
    ("tests/test_gpu_baseline_sizes.py::test_config2_msm_2p20_bit_exact_vs_oracle", 1 << 20, True, 1),
    ("tests/test_gpu_baseline_sizes.py::test_msm_skewed_digits_exercise_the_sort_slow_paths", 1 << 21, False, 1),
    ("tests/test_gpu_group.py::test_two_contexts_share_one_table_allocation", 1 << 22, True, 1),
    # no existing test runs an unchunked MSM over window tables of 2^25 points (c = 22, 2048 bins, geometry 0): the one large case
    ("tests/test_gpu_variants.py::test_g1_automatic_shape_2p25_with_tables", 1 << 25, True, 1),
]


def auto_shape(n, tables, passes=1):
    """(shared, c, lb, geom) of the automatic choice for an MSM of n points (tables: over window tables built for n points)"""
    r = msm(n, {}, table_c=choose_window_shared(n) if tables else None,
            chunk_sizes=pipe_chunk_sizes(n, passes) if passes > 1 else None)
    s = r["shapes"][0]
    return (r["shared"], r["c"], s["lb"], s["geom"])


# Instantiations the host code launches but no input can reach, with the model's reason
UNREACHABLE = {
    "k_tile_sort<11>": "W = 11 windows is the plan of c = 24 only; generic widths above %d and shared widths above %d are refused" % (
        K["MSM_C_MAX"], K["MSM_C_SHARED_MAX"]),
}
