"""Scalar model of the batched small MSM (keaki_amd/csrc/msm_batch.hip) -- TEST INFRASTRUCTURE, imported by tests/test_msm_batch_model.py
and tests/test_gpu_msm_batch.py.

Every base is k * G with k known (tests/structured_inputs.py), so a point is its scalar mod r and the model follows the kernels' documented
order of operations on scalars: window choice from n, the biased signed digits, the (window, bucket) slot, the bucket loop, the weighted
tree inside a workgroup and the Horner close. It counts the additions that meet equal operands, opposite operands or an identity
accumulator, which is how the GPU test's adversarial rows are known to reach those branches. The route model says which calls take the batch
kernels and which the row-by-row fallback; its constants are parsed out of the sources so that a changed limit fails the CPU test."""
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


def workspace_requests(n, m):
    """the two reservations of the batch path in bytes, as `reserve` asks the allocator for them (bytes + bytes / 8 + 256)"""
    W = plan(window_bits(n))[1]
    rows = rows_per_pass(n, m)
    return [b + b // 8 + 256 for b in (rows * n * 32, rows * W * 128)]


def route(n, m, tables=False, alloc_limit=0, held=(0, 0)):
    """'none' | 'identity' | 'batch' | 'fallback'. tables: the handle has window tables (no influence: the batch kernels read the points only);
    alloc_limit: keaki_hip_debug_set_alloc_limit; held: capacities of the two workspaces the context already holds (grow-only)"""
    if m == 0:
        return "none"
    if n == 0:
        return "identity"
    if n > N_BATCH_MAX:
        return "fallback"
    W = plan(window_bits(n))[1]
    rows = rows_per_pass(n, m)
    for need, req, have in zip((rows * n * 32, rows * W * 128), workspace_requests(n, m), held):
        if need > have and alloc_limit and req > alloc_limit:
            return "fallback"
    return "batch"


# ---- inputs that reach the exceptional branches ---------------------------------------------------------------------------------------------
def adversarial_rows(n, seed_row):
    """[zero row, n equal scalars, r - 1 everywhere, the caller's random row]"""
    return [[0] * n, [0x1234567 % R] * n, [R - 1] * n, list(seed_row)]
