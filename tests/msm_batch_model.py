"""Scalar model of the batched small MSM (keaki_amd/csrc/msm_batch.hip) -- TEST INFRASTRUCTURE, imported by tests/test_msm_batch_model.py,
tests/test_gpu_msm_batch.py and tests/test_gpu_msm_batch_paths.py.

Every base is k * G with k known (tests/structured_inputs.py), so a point is its scalar mod r and the model follows the kernels' documented
order of operations on scalars: window choice from n, the biased signed digits, the (window, bucket) slot, the bucket loop, the weighted
tree inside a workgroup and the Horner close. It counts the additions that meet equal operands, opposite operands or an identity
accumulator, which is how the GPU test's adversarial rows are known to reach those branches. The route model says which calls take the batch
kernels and which the row-by-row fallback; its constants are parsed out of the sources so that a changed limit fails the CPU test.
GPU_CASES lists the shapes tests/test_gpu_msm_batch_paths.py runs with what the model says each one reaches (window plan, passes, route,
exceptional additions); the CPU test holds the list against the plans, boundaries and pass splits the sources have."""
import functools
import os
import re

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "keaki_amd", "csrc")

# the model's own statement of the constants; test_msm_batch_model.py holds them against the sources
N_BATCH_MAX = 16384
C_MIN, C_MAX = 4, 9
THREADS = 256
PER_BUCKET = 16
CANON_BYTES = 1 << 28
ROWS_MAX = 16384


def parse_sources():
    """the same constants as the sources state them"""
    hip = open(os.path.join(CSRC, "msm_batch.hip")).read()
    hdr = open(os.path.join(CSRC, "internal.h")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()

    def num(text, pat):
        m = re.search(pat, text)
        assert m, "msm_batch_model: pattern %r no longer matches the source" % pat
        return m.group(1)

    shift = num(hdr, r"MSM_BATCH_CANON_BYTES = \(size_t\)1 << (\d+)")
    return {
        "N_BATCH_MAX": int(num(hdr, r"constexpr size_t N_BATCH_MAX = (\d+)")),
        "MB_N_MAX": int(num(hip, r"MB_N_MAX = (\d+)")),
        "C_MIN": int(num(hip, r"MB_C_MIN = (\d+)")),
        "C_MAX": int(num(hip, r"MB_C_MAX = (\d+)")),
        "THREADS": int(num(hip, r"MB_THREADS = (\d+)")),
        "PAIRS_MAX": int(num(hip, r"MB_PAIRS_MAX = (\d+)")),
        "PER_BUCKET": int(num(hip, r"\(n >> \(c - 1\)\) > (\d+)\) c\+\+")),
        "CANON_BYTES": 1 << int(shift),
        "ROWS_MAX": int(num(hdr, r"MSM_BATCH_ROWS_MAX = (\d+)")),
        "route_test": num(hip, r"bool batch = (n <= N_BATCH_MAX);"),
        "oom_falls_back": num(hip, r"if \(ws == KEAKI_ERR_OOM\) \{ (batch = false);"),
        "fallback_call": num(hip, r"ST_TRY\((msm_g1_run)\(ctx, d_points, srs_len, \(const Fr\*\)d_scalars \+ j \* stride, n, out \+ 3 \* j, d_table, c_table, nullptr\)\);"),
        # open_batch_core: the rows the quotient workspace starts with, the halving step and its exit; reserve's request
        "open_rows_start": num(api, r"size_t rows = (std::min\(m, std::max<size_t>\(1, MSM_BATCH_CANON_BYTES / \(nq \* 32\)\)\));"),
        "open_reserve": num(api, r"const keaki_status st = (reserve\(ctx, ctx->mb_q, rows \* nq \* 32\));"),
        "open_exit": num(api, r"if \((st != KEAKI_ERR_OOM \|\| rows == 1)\) return st;"),
        "open_halve": num(api, r"rows = (\(rows \+ 1\) / 2);"),
        "open_pass": num(api, r"for \(size_t r0 = 0; r0 < m; r0 \+= rows\) \{\s+const size_t k = (std::min\(rows, m - r0\));"),
        "reserve_request": num(api, r"size_t want = (bytes \+ bytes / 8 \+ 256);"),
    }


# ---- plan -----------------------------------------------------------------------------------------------------------------------------
def window_bits(n):
    """msm_batch_window: the smallest c in C_MIN .. C_MAX with floor(n / 2^(c-1)) <= PER_BUCKET"""
    c = C_MIN
    while c < C_MAX and (n >> (c - 1)) > PER_BUCKET:
        c += 1
    return c


def plan(c_target):
    """msm_make_plan: W windows, the first k of c bits, the rest of c - 1 -> (c, W, k, widths, offsets)"""
    W = (254 + c_target - 1) // c_target
    base, rem = divmod(254, W)
    c, k = (base, W) if rem == 0 else (base + 1, rem)
    widths = [c if w < k else c - 1 for w in range(W)]
    offsets = [sum(widths[:w]) for w in range(W)]
    return c, W, k, widths, offsets


def bias(c_target):
    _, W, _, widths, offsets = plan(c_target)
    return sum(1 << (offsets[w] + widths[w] - 1) for w in range(W - 1))


def digits(v, c_target):
    """signed digits of the canonical scalar v, lowest window first: u_w - half below the top window, u_(W-1) unsigned on top. The carries of
    the classical recoding (the one into the top window included) are the carries of the addition v + bias."""
    _, W, _, widths, offsets = plan(c_target)
    vb = v + bias(c_target)
    assert vb < 1 << 256
    out = []
    for w in range(W):
        u = (vb >> offsets[w]) & ((1 << widths[w]) - 1)
        out.append(u if w == W - 1 else u - (1 << (widths[w] - 1)))
    assert vb >> (offsets[-1] + widths[-1]) == 0, "the top digit holds every remaining bit"
    return out


def reconstruct(ds, c_target):
    _, _, _, _, offsets = plan(c_target)
    return sum(d << o for d, o in zip(ds, offsets))


def carries(v, c_target):
    """carry out of every signed window: bit offset(w + 1) of (v mod 2^offset(w+1)) + (bias mod 2^offset(w+1)); the last one enters the top window"""
    _, W, _, _, offsets = plan(c_target)
    bs = bias(c_target)
    return [((v % (1 << offsets[w + 1])) + (bs % (1 << offsets[w + 1]))) >> offsets[w + 1] for w in range(W - 1)]


def slot(w, d, c_target):
    """(workgroup, lane, negated) of a non-zero digit: lane = (w mod G) * B + |d| - 1"""
    c = plan(c_target)[0]
    B = 1 << (c - 1)
    G = THREADS // B
    assert d != 0 and abs(d) <= B
    return w // G, (w % G) * B + abs(d) - 1, d < 0


# ---- the kernels on scalars (a point is its discrete log; None is the identity) ------------------------------------------------------------
class Events(dict):
    def hit(self, k):
        self[k] = self.get(k, 0) + 1


def _add(a, b, ev, where):
    if a is None or b is None:
        return b if a is None else a
    if a == b:
        ev.hit(where + "_equal")
        return 2 * a % R
    if (a + b) % R == 0:
        ev.hit(where + "_opposite")
        return None
    return (a + b) % R


def msm_row(dlogs, scalars, ev=None):
    """out = sum scalars[i] * dlogs[i] in the order of k_mb_windows / k_mb_close; returns (result scalar or None, events)"""
    ev = Events() if ev is None else ev
    n = len(scalars)
    ct = window_bits(n)
    c, W, _, widths, _ = plan(ct)
    B = 1 << (c - 1)
    logB = c - 1
    buckets = [[None] * B for _ in range(W)]
    for i, v in enumerate(scalars):                      # bucket loop: entries in index order (the kernel's order is arbitrary; the sum is not)
        for w, d in enumerate(digits(v % R, ct)):
            if d == 0 or dlogs[i] % R == 0:
                continue
            p = dlogs[i] % R if d > 0 else (R - dlogs[i]) % R
            b = abs(d) - 1
            if buckets[w][b] is None:
                ev.hit("bucket_first" if not ev.get(("seen", w, b)) else "bucket_identity_acc")
                ev[("seen", w, b)] = 1
                buckets[w][b] = p
            else:
                buckets[w][b] = _add(buckets[w][b], p, ev, "bucket")
    wsum = []
    for w in range(W):                                   # weighted tree: node (A, Wt) over 2^k buckets
        nodes = [(s, None) for s in buckets[w]]
        for k in range(logB):
            nxt = []
            for j in range(0, len(nodes), 2):
                (al, wl), (ar, wr) = nodes[j], nodes[j + 1]
                sh = None if ar is None else ar * (1 << k) % R
                if sh == 0:
                    sh = None
                wt = sh if k == 0 else _add(_add(wl, wr, ev, "tree"), sh, ev, "tree")
                if k == logB - 1 and al is not None and ar is not None and (al == ar or (al + ar) % R == 0):
                    ev.hit("tree_top_equal" if al == ar else "tree_top_opposite")        # the last merge A_l + A_r, counted again by _add
                nxt.append((_add(al, ar, ev, "tree"), wt))
            nodes = nxt
        wsum.append(_add(nodes[0][0], nodes[0][1], ev, "tree"))
    acc = None
    for w in range(W - 1, -1, -1):                       # Horner close
        if acc is not None:
            acc = acc * (1 << widths[w]) % R
            if acc == 0:
                acc = None
        acc = _add(acc, wsum[w], ev, "close")
    for key in [k for k in ev if isinstance(k, tuple)]:
        del ev[key]
    return acc, ev


# ---- route --------------------------------------------------------------------------------------------------------------------------------
def rows_per_pass(n, m):
    return min(m, max(1, CANON_BYTES // (n * 32)), ROWS_MAX)


def request(nbytes):
    """what `reserve` asks the allocator for when a workspace has to grow"""
    return nbytes + nbytes // 8 + 256


def _reserve(need, have, alloc_limit):
    """reserve(ctx, buf, need) on a buffer of capacity `have` -> (granted, capacity afterwards). A buffer that has to grow is freed first, so
    a refused request leaves it empty."""
    if need <= have:
        return True, have
    if alloc_limit and request(need) > alloc_limit:
        return False, 0
    return True, request(need)


def workspace_requests(n, m):
    """the two reservations of the batch path in bytes, as `reserve` asks the allocator for them (bytes + bytes / 8 + 256)"""
    W = plan(window_bits(n))[1]
    rows = rows_per_pass(n, m)
    return [request(b) for b in (rows * n * 32, rows * W * 128)]


def route_held(n, m, alloc_limit=0, held=(0, 0)):
    """route of one msm_g1_batch_run and the capacities (mb_canon, mb_wsums) it leaves behind"""
    if m == 0:
        return "none", tuple(held)
    if n == 0:
        return "identity", tuple(held)
    if n > N_BATCH_MAX:
        return "fallback", tuple(held)
    W = plan(window_bits(n))[1]
    rows = rows_per_pass(n, m)
    ok, canon = _reserve(rows * n * 32, held[0], alloc_limit)
    if not ok:
        return "fallback", (canon, held[1])
    ok, wsums = _reserve(rows * W * 128, held[1], alloc_limit)
    return ("batch" if ok else "fallback"), (canon, wsums)


def route(n, m, tables=False, alloc_limit=0, held=(0, 0)):
    """'none' | 'identity' | 'batch' | 'fallback'. tables: the handle has window tables (no influence: the batch kernels read the points only);
    alloc_limit: keaki_hip_debug_set_alloc_limit; held: capacities of the two workspaces the context already holds (grow-only)"""
    return route_held(n, m, alloc_limit, held)[0]


def inner_passes(n, m):
    """launch rounds of msm_g1_batch_run on the batch route: [rows of each pass]"""
    rows = rows_per_pass(n, m)
    return [min(rows, m - r0) for r0 in range(0, m, rows)]


def open_rows(nq, m, alloc_limit=0, held=(0, 0, 0)):
    """open_batch_core for quotients of nq >= 1 coefficients: the rows of the quotient workspace start at min(m, max(1, CANON_BYTES / (nq * 32)))
    and halve ((rows + 1) / 2) while `reserve` is refused; one row refused is KEAKI_ERR_OOM (None). held: capacities of (mb_q, mb_canon,
    mb_wsums). -> {"rows": rows of each outer pass, "routes": route of the MSM of each outer pass, "held": capacities afterwards}"""
    rows = min(m, max(1, CANON_BYTES // (nq * 32)))
    q = held[0]
    while True:
        ok, q = _reserve(rows * nq * 32, q, alloc_limit)
        if ok:
            break
        if rows == 1:
            return None
        rows = (rows + 1) // 2
    inner = tuple(held[1:])
    passes, routes = [], []
    for r0 in range(0, m, rows):
        k = min(rows, m - r0)
        r, inner = route_held(nq, k, alloc_limit, inner)
        passes.append(k)
        routes.append(r)
    return {"rows": passes, "routes": routes, "held": (q,) + inner}


# ---- inputs that reach the exceptional branches ---------------------------------------------------------------------------------------------
def adversarial_rows(n, seed_row):
    """[zero row, n equal scalars, r - 1 everywhere, the caller's random row]"""
    return [[0] * n, [0x1234567 % R] * n, [R - 1] * n, list(seed_row)]


def _every_window_carries(ct):
    _, _, _, _, offsets = plan(ct)
    return (1 << offsets[-1]) - 1 + (1 << offsets[-1])          # all ones below the top window, one on top


def edge_scalars(n):
    """0, 1, r - 1, 2^(c-1) (window 0 goes negative with a carry) and the value whose every signed window carries, for the width of n"""
    ct = window_bits(n)
    return [0, 1, R - 1, 1 << (plan(ct)[0] - 1), _every_window_carries(ct)]


def branch_rows(n, seed_row):
    """adversarial_rows plus rows of two non-zero scalars that put chosen points into chosen buckets of window 0, so that on an SRS of equal
    points (tau = 1) the tree meets equal and opposite operands whatever the width: at its first level (1 and 2: G in buckets 0 and 1; 1 and
    2^c - 2: G and -G) and at its last level, the merge of the two halves of a window (1 and B / 2 + 1; 1 and 2^c - (B / 2 + 1)).
    test_msm_batch_model.py proves the events for every width."""
    c = plan(window_bits(n))[0]
    far = (1 << (c - 2)) + 1                                      # bucket B / 2: the first of the upper half
    pad = [0] * (n - 2)
    return adversarial_rows(n, seed_row) + [[1, 2] + pad, [1, (1 << c) - 2] + pad, [1, far] + pad, [1, (1 << c) - far] + pad]


# ---- the case table of tests/test_gpu_msm_batch_paths.py ------------------------------------------------------------------------------------
def width_boundaries():
    """[(n, n + 1)] where window_bits steps, found by walking n (not copied from the source)"""
    return [(n, n + 1) for n in range(1, N_BATCH_MAX) if window_bits(n) != window_bits(n + 1)]


BOUNDARY_N = [135, 136, 271, 272, 543, 544, 1087, 1088, 2175, 2176]
BRANCH_N = [65, 257, 400, 1000, 1500, 2500]                      # one n per width 4 .. 9
IDENTITY_N = [65, 1500]
QUOTIENT_N = [255, 256, 512, 513]
# allocation limits of the two limited open cases (bytes), chosen from open_rows: (a) admits 17 quotient rows of 256 coefficients but not 33,
# (b) admits the quotient and canonical rows of 65 x 33 but not their 65 x 64 window sums
OPEN_HALVING = {"n": 257, "m": 65, "limit": request(17 * 256 * 32) + 1000}
OPEN_FALLBACK = {"n": 34, "m": 65, "limit": request(65 * 33 * 32) + 1000}


def _cases():
    """(id, entry, n, m, stride, srs kind, scalar set, alloc limit). entry 'commit': keaki_hip_msm_g1_batch*, n scalars a row; 'open':
    keaki_hip_kzg_open_batch*, n coefficients a row (the MSM has n - 1). srs kinds: 'known' unrelated points of known discrete logs, 'one' /
    'minus_one' / 'random' / 'zero' tau^i G, 'holes' known logs with identity points."""
    out = []
    for n in BOUNDARY_N:
        out.append(("plan[n=%d]" % n, "commit", n, 3, n + 3, "known", "edge", 0))
    for n in BRANCH_N:
        for srs in ("one", "minus_one"):
            out.append(("branches[n=%d,%s]" % (n, srs), "commit", n, 8, n, srs, "branch", 0))
    for n in IDENTITY_N:
        out.append(("identity_points[n=%d]" % n, "commit", n, 4, n, "holes", "holes", 0))
        out.append(("identity_points[n=%d,zero]" % n, "commit", n, 4, n, "zero", "holes", 0))
    for n in (1, 3):
        out.append(("rows_max[n=%d]" % n, "commit", n, ROWS_MAX + 1, n, "random", "random", 0))
        out.append(("rows_max[n=%d,stride]" % n, "commit", n, ROWS_MAX + 1, n + 1, "random", "random", 0))
    out.append(("canon_bytes", "commit", N_BATCH_MAX, CANON_BYTES // (N_BATCH_MAX * 32) + 1, N_BATCH_MAX, "random", "numpy", 0))
    out.append(("open_halving", "open", OPEN_HALVING["n"], OPEN_HALVING["m"], OPEN_HALVING["n"], "known", "random", OPEN_HALVING["limit"]))
    out.append(("open_fallback", "open", OPEN_FALLBACK["n"], OPEN_FALLBACK["m"], OPEN_FALLBACK["n"], "known", "random", OPEN_FALLBACK["limit"]))
    out.append(("open_dev[stride]", "open", 257, 3, 262, "known", "random", 0))
    for n in (N_BATCH_MAX + 1, N_BATCH_MAX + 2):
        out.append(("open_route[n=%d]" % n, "open", n, 2, n, "random", "random", 0))
    for n in QUOTIENT_N:
        out.append(("quotient[n=%d]" % n, "open", n, 3, n, "random", "z01", 0))
    return out


@functools.lru_cache(maxsize=None)
def branch_events(n, srs):
    """events of branch_rows(n, a fixed pseudo-random row) on tau = 1 / -1, as sorted names"""
    from conftest_helpers import rand_fr_ints
    tau = {"one": 1, "minus_one": R - 1}[srs]
    dl, x = [], 1
    for _ in range(n):
        dl.append(x)
        x = x * tau % R
    ev = Events()
    for row in branch_rows(n, rand_fr_ints(n, 5 + n)):
        msm_row(dl, row, ev)
    return tuple(sorted(k for k in ev if ev[k]))


def reach(case):
    """what the model says a case reaches"""
    cid, entry, n, m, stride, srs, scalars, limit = case
    nq = n - 1 if entry == "open" else n
    c = plan(window_bits(nq))[0]
    out = {"c": c, "G": THREADS >> (c - 1), "depth": c - 1}
    if entry == "open":
        o = open_rows(nq, m, limit)
        out.update(outer=o["rows"], routes=o["routes"], held=o["held"],
                   inner=[len(inner_passes(nq, k)) if r == "batch" else 0 for k, r in zip(o["rows"], o["routes"])])
    else:
        r, held = route_held(nq, m, limit)
        out.update(outer=[m], routes=[r], held=(0,) + held, inner=[len(inner_passes(nq, m)) if r == "batch" else 0])
    out["events"] = branch_events(n, srs) if scalars == "branch" else ()
    return out


GPU_CASES = _cases()


def case(cid):
    hit = [k for k in GPU_CASES if k[0] == cid]
    assert len(hit) == 1, "msm_batch_model: no GPU case %r" % cid
    return hit[0]


def cases_of(prefix):
    return [k for k in GPU_CASES if k[0].split("[")[0] == prefix]
