"""The heavy-bucket path of the variable-base MSM at its count, slice and pass edges -- TEST INFRASTRUCTURE (a plain module, imported by
tests/test_heavy_cases_model.py and tests/test_gpu_msm_heavy.py; no GPU import).

A bucket with >= HEAVY_MIN pairs leaves the one-lane-per-bucket kernels: k_cnt_hist gives it a slot and ceil(count / HEAVY_SLICE) slice
ids, k_msm_heavy sums each slice with 256 lanes and an LDS tree, k_msm_heavy_combine folds the slices into the bucket or into the parked
lazy-limb state (keaki_amd/csrc/msm.hip.h; the mode per pass: msm_host.hip.h, msm_bucket_pass). This module builds MSM inputs whose
buckets hold EXACTLY the counts at which that path changes, and says for every case and pass what each designed bucket holds.

A case is (bases as discrete logs, scalars, forced window width, window tables or not, passes). Bases are k_i G with k_i known, so the
expected point is (sum s_i k_i mod r) G. Designed buckets are driven by scalars with one non-zero digit: v << offset(w) puts point i into
bucket v - 1 of window w; 2^width(0) - v is the digit -v in window 0 and, through its carry, the digit 1 in window 1 (bucket 0 there: the
model counts it like any other). Random full-width fillers are drawn until they miss every designed bucket, so a designed count is the
number of designed scalars; the analysis nevertheless counts the digits of ALL scalars of a pass.

The limits HEAVY_MIN, HEAVY_SLICE, C2_CAP, SEG_INLINE, CNT_BINS and the 256-chunk stride of the heavy kernel's segment search are read
from msm.hip.h (variant_cases.header_consts): a changed constant moves the cases or fails the CPU test.
"""
import functools
import random

import structured_inputs as S
import variant_cases as V

R = S.R
K = V.K
HM, HS, C2, SEG_INLINE, CNT_BINS, STRIDE = (K[k] for k in ("HEAVY_MIN", "HEAVY_SLICE", "C2_CAP", "SEG_INLINE", "CNT_BINS", "HEAVY_CHUNK_STRIDE"))
HV_MODE_RULE = "const u32 hv_mode = c.lazy_state && !last ? (first ? HV_SET29 : HV_ADD29) : (first ? HV_SET : HV_ADD);"     # msm_bucket_pass
C_STATIC, C_WALK = 16, 12          # forced widths: 16 windows (a static tile sort, W in 11..16) and 22 windows (the run-time digit walk)
PIPE_PAGE = 4096                   # the host entry cuts chunks at whole pages of scalars from 65536 scalars on (host_plan.h)


# ---- digits and global bucket ids ---------------------------------------------------------------------------------------------------
def gid(p, tables, w, b):
    """global bucket id of bucket b of window w (over window tables every window shares one range)"""
    return b if tables else V.bucket_base(p, w) + b


@functools.lru_cache(maxsize=1 << 16)
def _gids(s, c, tables):
    p = V.plan(c)
    return tuple(gid(p, tables, w, b) for w, b, _ in S.msm_digits(s, c))


def single(p, w, v, neg=False):
    """the scalar whose one digit is v in window w (bucket v - 1); neg: the digit -v in window 0, which carries the digit 1 into window 1"""
    if neg:
        assert w == 0 and 0 < v < (1 << (p["widths"][0] - 1))
        return (1 << p["widths"][0]) - v
    s = v << p["offs"][w]
    assert 0 < v and s < R and (w == p["W"] - 1 or v <= (1 << (p["widths"][w] - 1)))
    return s


def windows(p):
    return {"w0": 0, "mid": p["W"] // 2, "top": p["W"] - 1}


def fillers(n, c, tables, avoid, rng, shape=None, avoid_bins=()):
    """n random full-width scalars none of whose digits falls into a bucket of `avoid` (global ids) or into a bin of `avoid_bins` of the
    sort shape `shape`"""
    out = []
    while len(out) < n:
        s = rng.getrandbits(253)
        gs = _gids(s, c, tables)
        if not (set(gs) & avoid) and not (avoid_bins and any(V.part_bin(shape, g) in avoid_bins for g in gs)):
            out.append(s)
    return out


def rand_dlogs(n, rng):
    return [rng.getrandbits(253) | 1 for _ in range(n)]


def make_case(name, group, c, tables, passes, dlogs, scalars, designed, **extra):
    assert len(dlogs) == len(scalars)
    case = {"name": name, "group": group, "c": c, "tables": tables, "passes": passes, "dlogs": dlogs, "scalars": scalars,
            "designed": designed, "acc_u29": 1, "refuse_state": False}
    case.update(extra)
    return case


def expected_dlog(case):
    return S.msm_dlog(case["dlogs"], case["scalars"])


def window_bits(case):
    """what last_msm_stats()['window_bits'] reports: the width of the plan's wide windows"""
    return V.plan(case["c"])["c"]


def pipe_bounds(n, k):
    """msm_pipe_bounds (host_plan.h) for msm_pipe_chunks = k >= 2 and msm_pipe_growth = 100"""
    k = min(k, 64, n)
    b = [0]
    for j in range(k - 1):
        e = int(float(n) * float(j + 1) / float(k))
        if n >= 65536:
            e &= ~(PIPE_PAGE - 1)
        if b[-1] < e < n:
            b.append(e)
    return b + [n]


def pass_sizes(case):
    """the scalars of each pass: variant_cases.pipe_chunk_sizes, which is what the host entry cuts when the chunks are whole pages"""
    n, k = len(case["scalars"]), case["passes"]
    if k == 1:
        return [n]
    sizes = V.pipe_chunk_sizes(n, k)
    b = pipe_bounds(n, k)
    assert n % (k * PIPE_PAGE) == 0 and [b[i + 1] - b[i] for i in range(len(b) - 1)] == sizes
    return sizes


# ---- the analysis: what every pass puts where ----------------------------------------------------------------------------------------
_ANALYSED = {}


def analyse(case):
    """per pass: dict(shape, buckets: {label: dict(gid, count, heavy, slices, last, bin, bin_pairs, bin_chunks)}, heavy: every bucket
    with >= HEAVY_MIN pairs as (gid, count), designed or not). Counts are taken over all scalars of the pass."""
    if case["name"] in _ANALYSED:
        return _ANALYSED[case["name"]]
    p = V.plan(case["c"])
    nb = p["max_b"] if case["tables"] else p["nb"]
    out, lo = [], 0
    for m in pass_sizes(case):
        shape = V.part_make_shape(m, p["W"], nb)
        counts = {}
        for s in case["scalars"][lo:lo + m]:
            for g in _gids(s, case["c"], case["tables"]):
                counts[g] = counts.get(g, 0) + 1
        lo += m
        bins = {}
        for g, n in counts.items():
            b = V.part_bin(shape, g)
            bins[b] = bins.get(b, 0) + n
        buckets = {}
        for label, (w, b) in case["designed"].items():
            g = gid(p, case["tables"], w, b)
            buckets[label] = describe(shape, g, counts.get(g, 0), bins)
        out.append({"shape": shape, "buckets": buckets, "heavy": sorted((g, n) for g, n in counts.items() if n >= HM), "counts": counts,
                    "bins": bins})
    _ANALYSED[case["name"]] = out
    return out


def describe(shape, g, n, bins):
    heavy = n >= HM
    nsl = -(-n // HS) if heavy else 0
    b = V.part_bin(shape, g)
    return {"gid": g, "count": n, "heavy": heavy, "slices": nsl, "last": n - (nsl - 1) * HS if heavy else 0, "bin": b,
            "bin_pairs": bins.get(b, 0), "bin_chunks": -(-bins.get(b, 0) // C2), "size_bin": min(n, CNT_BINS - 1)}


def straddle_bounds(case, label, pas=0):
    """Bounds on the number of pairs of designed bucket `label` that lie before each chunk end of its bin, valid for EVERY arrival order:
    the bin's pairs are ordered tile after tile (k_cell_prefix), only the order inside a tile's cell is open (LDS atomics), and a chunk
    is C2_CAP consecutive pairs of the bin (k_chunk_sort). Tiles wholly before the end contribute their full count; the tile the end
    falls into contributes between max(0, x - others) and min(own, x) of its pairs, x = the pairs of its cell before the end.
    -> [(chunk end, lo, hi)] for the chunk ends inside the bin."""
    p = V.plan(case["c"])
    a = analyse(case)[pas]
    shape, d = a["shape"], a["buckets"][label]
    sizes = pass_sizes(case)
    first = sum(sizes[:pas])
    sc = case["scalars"][first:first + sizes[pas]]
    cells = []                                             # per tile: (pairs of the bin, pairs of the bucket)
    for t0 in range(0, len(sc), shape["tile"]):
        cell = own = 0
        for s in sc[t0:t0 + shape["tile"]]:
            for g in _gids(s, case["c"], case["tables"]):
                if V.part_bin(shape, g) == d["bin"]:
                    cell += 1
                    own += g == d["gid"]
        cells.append((cell, own))
    assert sum(c for c, _ in cells) == d["bin_pairs"] and sum(o for _, o in cells) == d["count"] and p["W"] * shape["tile"] <= K["T1_CAP"]
    out = []
    for k in range(1, d["bin_chunks"]):
        end, start, before = k * C2, 0, 0
        for cell, own in cells:
            if start + cell <= end:
                start, before = start + cell, before + own
                continue
            x = end - start
            out.append((end, before + max(0, x - (cell - own)), before + min(own, x)))
            break
    return out


def straddled(bounds, count):
    """the chunk ends that cut a slice in two under every arrival order: no slice end in [lo, hi], and pairs of the bucket on both sides"""
    return [(e, lo, hi) for e, lo, hi in bounds if 0 < lo and hi < count and (lo - 1) // HS == hi // HS]


# ---- family 1: counts -----------------------------------------------------------------------------------------------------------------
COUNTS_FULL = [(1022, "w0+"), (1023, "mid"), (1024, "top"), (HM - 1, "w0-"), (HM, "w0-"), (HM + 1, "mid"), (HS - 1, "top"), (HS, "w0+-"),
               (HS + 1, "w0-"), (2 * HS, "mid"), (C2 + 1, "w0+"), (3 * HS + 1, "top")]
COUNTS_G2 = [(HM - 1, "w0+"), (HM, "w0-"), (HS, "mid"), (HS + 1, "top"), (C2 + 1, "w0+-")]


@functools.lru_cache(maxsize=None)
def counts_case(group, c, tables, n_fill=12000):
    """Designed buckets of exactly the listed counts among random fillers (the ordinary kernel runs in the same launch). kind: window 0
    with positive / negative / both signs, a middle window, the unsigned top window. Bucket values are 3, 5, 7, ...: bucket 0 (value 1)
    of window 1 takes the carries of the negative digits and is reported as 'carry'."""
    targets = COUNTS_G2 if group == "g2" else COUNTS_FULL
    p = V.plan(c)
    win = windows(p)
    rng = random.Random(1000 * c + 2 * tables + (group == "g2"))
    designed, sc = {}, []
    for j, (n, kind) in enumerate(targets):
        v, w = 3 + 2 * j, win[kind[:2] if kind.startswith("w0") else kind]
        designed["%d/%s" % (n, kind)] = (w, v - 1)
        neg = n if kind == "w0-" else n // 2 if kind == "w0+-" else 0
        sc += [single(p, 0, v, True)] * neg + [single(p, w, v)] * (n - neg)
    designed["carry"] = (1, 0)
    avoid = {gid(p, tables, w, b) for w, b in designed.values()}
    sc += fillers(n_fill, c, tables, avoid, rng)
    rng.shuffle(sc)
    return make_case("counts[%s,c=%d,%s]" % (group, c, "tables" if tables else "generic"), group, c, tables, 1, rand_dlogs(len(sc), rng), sc,
                     designed)


@functools.lru_cache(maxsize=None)
def all_exact_case(group, c, tables):
    """every pair of the call in a bucket of exactly HEAVY_MIN pairs (windows 0, middle, top): no light bucket at all"""
    p = V.plan(c)
    rng = random.Random(1100 + c + tables)
    designed = {"%d/%s" % (HM, kind): (w, 2 + 2 * j) for j, (kind, w) in enumerate(windows(p).items())}
    sc = [single(p, w, b + 1) for w, b in designed.values() for _ in range(HM)]
    rng.shuffle(sc)
    return make_case("all_exact[%s,c=%d,%s]" % (group, c, "tables" if tables else "generic"), group, c, tables, 1, rand_dlogs(len(sc), rng), sc,
                     designed)


# ---- family 2: slices against chunks --------------------------------------------------------------------------------------------------
STRADDLE_ALONE, STRADDLE_B, STRADDLE_COMPANIONS, STRADDLE_RATIO = 3 * HS + 1, 3 * HS + HS // 2, 15, (2, 3)


@functools.lru_cache(maxsize=None)
def straddle_case(group, c):
    """'alone': 3 HEAVY_SLICE + 1 pairs, the only bucket of its bin (two chunks <= SEG_INLINE: chunk ends fall on slice ends). 'mixed':
    3.5 slices in a bin of more than SEG_INLINE chunks that it shares with fifteen light companions, two of its pairs to three of
    theirs in scalar order, so that the bin's chunk ends fall inside its slices (straddle_bounds). Window 0, no tables, no fillers."""
    p = V.plan(c)
    rep = STRADDLE_B // STRADDLE_RATIO[0]
    n = STRADDLE_ALONE + rep * sum(STRADDLE_RATIO)
    shape = V.part_make_shape(n, p["W"], p["nb"])
    half = 1 << (p["widths"][0] - 1)
    bin_b = V.part_bin(shape, 1)
    comp = [v for v in range(3, half) if V.part_bin(shape, v - 1) == bin_b][:STRADDLE_COMPANIONS]
    alone = next(v for v in range(3, half) if V.part_bin(shape, v - 1) != bin_b)
    assert len(comp) == STRADDLE_COMPANIONS
    sc = [single(p, 0, alone)] * STRADDLE_ALONE
    j = 0
    for _ in range(rep):
        sc += [single(p, 0, 2)] * STRADDLE_RATIO[0]
        for _ in range(STRADDLE_RATIO[1]):
            sc.append(single(p, 0, comp[j % len(comp)]))
            j += 1
    designed = {"alone": (0, alone - 1), "mixed": (0, 1)}
    designed.update({"companion%d" % i: (0, v - 1) for i, v in enumerate(comp)})
    return make_case("straddle[%s,c=%d]" % (group, c), group, c, False, 1, rand_dlogs(n, random.Random(1200 + c)), sc, designed)


# ---- family 3: exceptional additions ----------------------------------------------------------------------------------------------------
EXCEPTIONAL_FILL = 2000


def single_segment_slices(case, label, pas=0):
    """the full slices of designed bucket `label` that lie inside ONE segment under every arrival order: no chunk end of the bin can
    fall strictly inside [k HEAVY_SLICE, (k + 1) HEAVY_SLICE) (straddle_bounds). k_msm_heavy then walks the slice as one run of
    HEAVY_SLICE pairs, lane q taking pairs q, q + 256, ...: HEAVY_SLICE / 256 pairs per lane."""
    d = analyse(case)[pas]["buckets"][label]
    bounds = straddle_bounds(case, label, pas)
    return [k for k in range(d["count"] // HS) if all(hi <= k * HS or lo >= (k + 1) * HS for _, lo, hi in bounds)]


@functools.lru_cache(maxsize=None)
def exceptional_case(group, c, acc_u29=1, cancel_only=False):
    """Heavy buckets whose additions take the exceptional branches of xyzz_add_mixed / xyzz_add.
    GUARANTEED, whatever the arrival order, for 'same/S+1' (HEAVY_SLICE + 1 copies of one base P) and 'same/2S' (2 HEAVY_SLICE
    copies of another): each is the ONLY bucket of its bin (no filler enters the bin either), so the bin's chunks hold its pairs
    alone, every full slice lies inside one segment (single_segment_slices; a chunk is two slices long) and the workgroup's lanes walk
    its HEAVY_SLICE pairs with stride 256 -- 64 copies per lane. The lane's second addition is P + P (the doubling of
    xyzz_add_mixed), every level of the LDS tree adds two equal sums (64 P + 64 P, 128 P + 128 P, ...: the doubling of xyzz_add), and
    for 'same/2S' the combine kernel adds two equal slice sums. The second slice of 'same/S+1' is one pair.
    ORDER-DEPENDENT (only the result is asserted): which lane meets P after -P in 'cancel' (HEAVY_MIN / 2 each of P and -P as bases:
    the bucket is the identity), 'cancel+1' (one more P: the bucket is P) and 'identity' (HEAVY_MIN random bases and 64 identity bases,
    which the kernels skip); these share their bins with each other and the fillers. cancel_only: two cancelling buckets and nothing
    else -- the MSM itself is the identity."""
    p = V.plan(c)
    win = windows(p)
    rng = random.Random(1300 + c + (group == "g2"))
    kp = rand_dlogs(6, rng)
    designed, sc, dl = {}, [], []

    def bucket(label, w, v, logs):
        designed[label] = (w, v - 1)
        sc.extend([single(p, w, v)] * len(logs))
        dl.extend(logs)
    if cancel_only:
        bucket("cancel", 0, 7, [kp[2], R - kp[2]] * (HM // 2))
        bucket("cancel/S+2", win["mid"], 9, [kp[3], R - kp[3]] * (HS // 2 + 1))
    else:
        bucket("cancel", 0, 7, [kp[2], R - kp[2]] * (HM // 2))
        bucket("cancel+1", win["top"], 9, [kp[3], R - kp[3]] * (HM // 2) + [kp[3]])
        bucket("identity", 0, 11, rand_dlogs(HM, rng) + [0] * 64)
        # the same-point buckets: the first bucket of their window whose bin no other designed bucket uses
        shape = V.part_make_shape(len(sc) + 3 * HS + 1 + EXCEPTIONAL_FILL, p["W"], p["nb"])
        taken = {V.part_bin(shape, gid(p, False, w, b)) for w, b in designed.values()}
        own = set()
        for label, w, k, m in (("same/S+1", 0, kp[0], HS + 1), ("same/2S", win["mid"], kp[1], 2 * HS)):
            v = next(v for v in range(3, 1 << (p["widths"][w] - 1)) if V.part_bin(shape, gid(p, False, w, v - 1)) not in taken | own)
            own.add(V.part_bin(shape, gid(p, False, w, v - 1)))
            bucket(label, w, v, [k] * m)
        avoid = {gid(p, False, w, b) for w, b in designed.values()}
        fl = fillers(EXCEPTIONAL_FILL, c, False, avoid, rng, shape, own)
        sc += fl
        dl += rand_dlogs(len(fl), rng)
        assert V.part_make_shape(len(sc), p["W"], p["nb"]) == shape, "the bins were chosen for the call's own sort shape"
    order = list(range(len(sc)))
    rng.shuffle(order)
    return make_case("exceptional[%s,c=%d,u29=%d%s]" % (group, c, acc_u29, ",cancel_only" if cancel_only else ""), group, c, False, 1,
                     [dl[i] for i in order], [sc[i] for i in order], designed, acc_u29=acc_u29)


# ---- family 4: the pass matrix ---------------------------------------------------------------------------------------------------------
LIGHT = 3


def sequences(passes):
    out = [""]
    for _ in range(passes):
        out = [s + x for s in out for x in "ELH"]
    return out


@functools.lru_cache(maxsize=None)
def matrix_case(group, c, tables, passes, acc_u29=1, refuse_state=False):
    """One designed bucket per sequence of {E empty, L light (3 pairs), H heavy (HEAVY_MIN + j pairs)} over the passes of a chunked call
    (3^passes buckets, windows 0 / middle / top in turn), and two buckets for the stored state: 'dbl' holds one point Q = HEAVY_MIN P
    after pass 0 and receives HEAVY_MIN copies of P in pass 1 (the combine kernel adds two equal points: the doubling in HV_ADD /
    HV_ADD29); 'neg' holds Q = -HEAVY_MIN P, is emptied by pass 1, and (three passes) receives three points in pass 2. Every pass is
    padded with zero scalars to a whole number of pages, 1500 fillers per pass."""
    p = V.plan(c)
    win = list(windows(p).values())
    rng = random.Random(1400 + 7 * c + 3 * tables + passes)
    seqs = sequences(passes)
    designed = {q: (win[j % 3], 2 + 2 * j) for j, q in enumerate(seqs)}
    designed["dbl"] = (0, 2 + 2 * len(seqs))
    designed["neg"] = (win[1], 4 + 2 * len(seqs))
    avoid = {gid(p, tables, w, b) for w, b in designed.values()}
    kd, kn = rand_dlogs(2, rng)
    per_pass = []
    for j in range(passes):
        sc, dl = [], []
        for i, q in enumerate(seqs):
            n = {"E": 0, "L": LIGHT, "H": HM + i}[q[j]]
            sc += [single(p, designed[q][0], designed[q][1] + 1)] * n
            dl += rand_dlogs(n, rng)
        for label, k, q0 in (("dbl", kd, HM * kd % R), ("neg", kn, (R - HM * kn) % R)):
            s = single(p, designed[label][0], designed[label][1] + 1)
            logs = [q0] if j == 0 else [k] * HM if j == 1 else rand_dlogs(LIGHT if label == "neg" else 1, rng)
            sc += [s] * len(logs)
            dl += logs
        fl = fillers(1500, c, tables, avoid, rng)
        sc += fl
        dl += rand_dlogs(len(fl), rng)
        per_pass.append((sc, dl))
    m = -(-max(len(sc) for sc, _ in per_pass) // PIPE_PAGE) * PIPE_PAGE
    scalars, dlogs = [], []
    for sc, dl in per_pass:
        pad = m - len(sc)
        sc, dl = sc + [0] * pad, dl + rand_dlogs(pad, rng)
        order = list(range(m))
        rng.shuffle(order)
        scalars += [sc[i] for i in order]
        dlogs += [dl[i] for i in order]
    what = "refused" if refuse_state else "lazy" if acc_u29 and group == "g1" else "saturated" if group == "g1" else "g2"
    return make_case("matrix[%s,%s,%d passes,%s]" % (group, what, passes, "tables" if tables else "generic"), group, c, tables, passes, dlogs,
                     scalars, designed, acc_u29=acc_u29, refuse_state=refuse_state)


def hv_mode(case, j):
    """the mode k_msm_heavy_combine runs in for pass j (msm_plan_call: lazy_state; msm_reserve: the fallback; msm_bucket_pass)"""
    first, last = j == 0, j == case["passes"] - 1
    lazy = case["passes"] > 1 and case["acc_u29"] and case["group"] == "g1" and not case["refuse_state"]
    if lazy and not last:
        return "HV_SET29" if first else "HV_ADD29"
    return "HV_SET" if first else "HV_ADD"


def reach(case):
    """[(group, hv_mode, pass, label or global bucket id, count, slices)] for every heavy bucket of every pass"""
    out = []
    for j, a in enumerate(analyse(case)):
        labels = {d["gid"]: label for label, d in a["buckets"].items()}
        for g, n in a["heavy"]:
            out.append((case["group"], hv_mode(case, j), j, labels.get(g, g), n, -(-n // HS)))
    return out


# ---- family 5: more than 256 chunks in one bin --------------------------------------------------------------------------------------------
MANY_N, MANY_BLOCK = STRIDE * C2 + C2 + 1, 1 << 16


def many_chunks_model():
    """(STRIDE + 1) C2_CAP + 1 scalars equal to 1: one pair each, all in bucket 0 of window 0, whose bin holds nothing else. Both numbers
    are compile-time constants, so no smaller input gives a bin of STRIDE + 2 chunks: the second trip of the heavy kernel's segment search
    finds a full chunk and one of a single pair, which is also the bucket's last slice."""
    c = V.choose_window(MANY_N)
    p = V.plan(c)
    shape = V.part_make_shape(MANY_N, p["W"], p["nb"])
    assert S.msm_digits(1, c) == [(0, 0, False)]
    d = describe(shape, 0, MANY_N, {V.part_bin(shape, 0): MANY_N})
    return {"n": MANY_N, "c": c, "window_bits": p["c"], "bucket": d, "trips": -(-d["bin_chunks"] // STRIDE)}


def many_chunks_dlog(block_dlogs):
    full, rest = divmod(MANY_N, len(block_dlogs))
    return (full * sum(block_dlogs) + sum(block_dlogs[:rest])) % R


# ---- the case lists of tests/test_gpu_msm_heavy.py ---------------------------------------------------------------------------------------
def count_cases():
    return [counts_case("g1", C_STATIC, False), counts_case("g1", C_WALK, False), counts_case("g1", C_STATIC, True), counts_case("g2", C_WALK, False)]


def all_exact_cases():
    return [all_exact_case("g1", C_STATIC, False), all_exact_case("g1", C_WALK, False), all_exact_case("g1", C_STATIC, True),
            all_exact_case("g2", C_WALK, False)]


def straddle_cases():
    return [straddle_case("g1", C_STATIC), straddle_case("g2", C_WALK)]


def exceptional_cases():
    return [exceptional_case("g1", C_STATIC, 1), exceptional_case("g1", C_STATIC, 0), exceptional_case("g2", C_WALK),
            exceptional_case("g1", C_STATIC, 1, True), exceptional_case("g1", C_STATIC, 0, True), exceptional_case("g2", C_WALK, 1, True)]


def matrix_cases():
    return [matrix_case("g1", C_STATIC, False, 3), matrix_case("g1", C_STATIC, True, 3), matrix_case("g1", C_STATIC, False, 3, 0),
            matrix_case("g1", C_STATIC, False, 3, 1, True), matrix_case("g2", C_WALK, False, 2)]


REQUIRED_MODES = {"g1": {"HV_SET", "HV_ADD", "HV_SET29", "HV_ADD29"}, "g2": {"HV_SET", "HV_ADD"}}


def report(case):
    """the lines the CPU test prints for a case: designed counts, slices, bins and chunk counts per pass"""
    lines = ["%s: n = %d, c = %d (window_bits %d), %d windows" % (case["name"], len(case["scalars"]), case["c"], window_bits(case),
                                                                  V.plan(case["c"])["W"])]
    for j, a in enumerate(analyse(case)):
        s = a["shape"]
        lines.append("  pass %d: %d bins, shift %d, tile %d" % (j, 1 << s["lb"], s["shift"], s["tile"]))
        for label, d in a["buckets"].items():
            if d["count"]:
                lines.append("    %-12s bucket %6d count %6d slices %d last %5d | bin %4d: %6d pairs, %d chunks" % (
                    label, d["gid"], d["count"], d["slices"], d["last"], d["bin"], d["bin_pairs"], d["bin_chunks"]))
    return lines
