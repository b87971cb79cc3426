"""Index-exact model of the batched FK23 pipeline (keaki_amd/csrc/fk_batch.hip, driven by api.hip: fkb_core) -- TEST INFRASTRUCTURE, imported
by tests/test_fk_batch_model.py and tests/test_gpu_fk_batch.py.

As in tests/fk_shard_model.py the group is the additive group of Z_q (a "scalar multiplication" is a product mod q); what the model keeps
from the device code is where every element lies and which lane touches it: the position-major point workspace work[pos * M + row] with the
rows of a pass padded to M (a multiple of 64), lane t of a launch = (position or butterfly t // M, row t % M), the twiddle of a butterfly, the
bit reversal at the finish, the split of m rows into passes and the route of a call (batch kernels, halved passes, row by row). The
constants are parsed out of the sources so that a changed limit fails the CPU test. GPU_CASES lists the calls tests/test_gpu_fk_batch.py runs
for the routes, with what the model says each one reaches."""
import os
import re

from fk_shard_model import Q, bitrev, dft, root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "keaki_amd", "csrc")

# the model's own statement of the constants; test_fk_batch_model.py holds them against the sources
LOG2D_MAX = 12
PASS_BYTES = 1 << 28
ROW_BYTES = 288              # per coefficient of a row: two Jacobian points (E, O) and three Fr (hat_a: 2, coefficients: 1)
ROWS_MAX = 16384
WAVE = 64
JAC, FR, AFF = 96, 32, 64


def parse_sources():
    hip = open(os.path.join(CSRC, "fk_batch.hip")).read()
    hdr = open(os.path.join(CSRC, "internal.h")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()

    def num(text, pat):
        m = re.search(pat, text)
        assert m, "fk_batch_model: pattern %r no longer matches the source" % pat
        return m.group(1)

    return {
        "LOG2D_MAX": int(num(hdr, r"FKB_LOG2D_MAX = (\d+)")),
        "PASS_BYTES": 1 << int(num(hdr, r"FKB_PASS_BYTES = \(size_t\)1 << (\d+)")),
        "ROW_BYTES": int(num(hdr, r"FKB_ROW_BYTES = (\d+)")),
        "ROWS_MAX": int(num(hdr, r"FKB_ROWS_MAX = (\d+)")),
        "rows_by_bytes": num(hip, r"const size_t by_bytes = (std::max<size_t>\(64, FKB_PASS_BYTES / \(FKB_ROW_BYTES << log2d\) / 64 \* 64\));"),
        "rows_per_pass": num(hip, r"return (std::min\(m, std::min\(by_bytes, FKB_ROWS_MAX\)\));"),
        "pts_bytes": num(hip, r"fkb_pts_bytes\(u32 log2d, size_t rows\) \{ return (.*?); \}"),
        "fr_bytes": num(hip, r"fkb_fr_bytes\(u32 log2d, size_t rows\) \{ return (.*?); \}"),
        "batch_domains": num(api, r"if \((log2d >= 1 && log2d <= FKB_LOG2D_MAX)\) \{\s+rows = fkb_rows_per_pass\(log2d, m\);"),
        "halve": num(api, r"if \(rows == 1\) \{ rows = 0; break; \}\s+rows = (\(rows \+ 1\) / 2);"),
        "fallback": num(api, r"if \((rows == 0)\) \{\s+for \(size_t j = 0; j < m; j\+\+\)\s+ST_TRY\(fkb_row_single\("),
        "pass": num(api, r"for \(size_t r0 = 0; r0 < m; r0 \+= rows\) \{\s+const size_t cnt = (std::min\(rows, m - r0\));"),
        "reserve_request": num(api, r"size_t want = (bytes \+ bytes / 8 \+ 256);"),
    }


def launch_sites():
    """the kernels fk_batch.hip launches, with their template arguments: {'k_fkb_stage<true>', ...}"""
    hip = open(os.path.join(CSRC, "fk_batch.hip")).read()
    return set(re.findall(r"hipLaunchKernelGGL\(\(?(k_\w+(?:<\w+>)?)\)?,", hip))


# ---- route and passes ---------------------------------------------------------------------------------------------------------------------
def pad64(rows):
    return (rows + WAVE - 1) // WAVE * WAVE


def request(b):
    """what `reserve` asks of the allocator for b bytes"""
    return b + b // 8 + 256


def pts_bytes(log2d, rows):
    return (2 << log2d) * pad64(rows) * JAC


def fr_bytes(log2d, rows):
    return (rows * (3 << log2d) + (3 << log2d)) * FR


def rows_per_pass(log2d, m):
    by_bytes = max(64, PASS_BYTES // (ROW_BYTES << log2d) // 64 * 64)
    return min(m, by_bytes, ROWS_MAX)


def plan(log2d, m, alloc_limit=0, held=(0, 0)):
    """fkb_core: {'route': 'none' | 'batch' | 'rows', 'passes': rows of every pass, 'halvings': n, 'held': the two workspaces afterwards}.
    alloc_limit: keaki_hip_debug_set_alloc_limit (0: none); held: capacities of (fkb_pts, fkb_fr) the context already has. A refused
    reservation frees the buffer it was to replace, as `reserve` does."""
    if m == 0:
        return {"route": "none", "passes": [], "halvings": 0, "held": held}
    if not 1 <= log2d <= LOG2D_MAX:
        return {"route": "rows", "passes": [1] * m, "halvings": 0, "held": held}
    held = list(held)

    def reserve(i, b):
        if b <= held[i]:
            return True
        held[i] = 0
        if alloc_limit and request(b) > alloc_limit:
            return False
        held[i] = request(b)
        return True

    rows, halvings = rows_per_pass(log2d, m), 0
    while not (reserve(0, pts_bytes(log2d, rows)) and reserve(1, fr_bytes(log2d, rows))):
        if rows == 1:
            return {"route": "rows", "passes": [1] * m, "halvings": halvings, "held": tuple(held)}
        rows = (rows + 1) // 2
        halvings += 1
    return {"route": "batch", "passes": [min(rows, m - r0) for r0 in range(0, m, rows)], "halvings": halvings, "held": tuple(held)}


def launches(log2d, vec):
    """the kernels of ONE pass in launch order (fkb_pass_run)"""
    d = 1 << log2d
    out = []
    if vec:
        out += ["k_fkb_fr_load"] + ["k_fkb_fr_stage"] * log2d + ["k_fkb_fr_scale"]
    out += ["k_fkb_fr_load"] + ["k_fkb_fr_stage"] * (log2d + 1) + ["k_fkb_fr_scale"]
    out += ["k_fkb_pointwise"] + ["k_fkb_stage<true>"] * log2d + ["k_fkb_twist"] + ["k_fkb_stage<false>"] * log2d + ["k_fkb_finish"]
    assert d >= 2
    return out


# ---- the pipeline over Z_q ------------------------------------------------------------------------------------------------------------------
def hat_s(srs, log2d):
    """the handle's cached transform (fft_g1.hip: fk_hat_s_run): position q < d holds hat_s[2 brev(q)], position d + q holds hat_s[2 brev(q) + 1]"""
    d = 1 << log2d
    full = dft([srs[d - 1 - i] for i in range(d)] + [0] * d, root(2 * d))
    return [full[2 * bitrev(q, log2d)] for q in range(d)] + [full[2 * bitrev(q, log2d) + 1] for q in range(d)]


def fr_transform(rows_in, n_rows, sstride, lo, hi, log2n, w, scale):
    """k_fkb_fr_load + the stages + the scaling: dst[row][brev(i)] = src[row * sstride + i - lo] (lo <= i < hi), then the in-place DIT"""
    n = 1 << log2n
    dst = [0] * (n_rows * n)
    for row in range(n_rows):
        for i in range(n):
            dst[row * n + bitrev(i, log2n)] = rows_in[row * sstride + i - lo] if lo <= i < hi else 0
    tw = [pow(w, k, Q) for k in range(max(1, n // 2))]
    length = 2
    while length <= n:
        half = length // 2
        for row in range(n_rows):
            for b in range(n // 2):
                j, i0 = b % half, (b // half) * length + b % half
                u, v = dst[row * n + i0], dst[row * n + i0 + half] * tw[j * (n // length)] % Q
                dst[row * n + i0], dst[row * n + i0 + half] = (u + v) % Q, (u - v) % Q
        length *= 2
    return [x * scale % Q for x in dst]


GARBAGE = Q - 1      # what the model's padding rows and row gaps hold: a result that depends on them is wrong


def pass_run(hs, log2d, data, n, rows, stride, vec):
    """fkb_pass_run: `rows` rows at data[j * stride ...] -> (proofs rows x d, natural order; coefficient rows or None)"""
    d, M = 1 << log2d, pad64(rows)
    w2 = root(2 * d)
    w2i = pow(w2, Q - 2, Q)
    tw, twi = [pow(w2, k, Q) for k in range(d)], [pow(w2i, k, Q) for k in range(d)]
    coef, p, pstride = None, data, stride
    if vec:
        wd_inv = pow(w2i, 2, Q)
        coef = fr_transform(data, rows, stride, 0, n, log2d, wd_inv, pow(d, Q - 2, Q))
        p, pstride = coef, d
    a = fr_transform(p, rows, pstride, d, 2 * d, log2d + 1, w2, pow(2 * d, Q - 2, Q))
    work = [GARBAGE] * (2 * d * M)
    for t in range(2 * d * M):                                 # k_fkb_pointwise
        pos, row = t // M, t % M
        if row >= rows:
            continue
        part, q = (1, pos - d) if pos >= d else (0, pos)
        sc = a[row * 2 * d + 2 * bitrev(q, log2d) + part]
        work[pos * M + row] = (sc * d if not part else sc) % Q * hs[pos] % Q
    base = d * M                                               # O = work + d M

    def stage(half, table, dit):
        stride_tw = 2 * (d // (2 * half))
        for t in range(d // 2 * M):
            b, row = t // M, t % M
            if row >= rows:
                continue
            j, blk = b % half, b // half
            i0 = base + (blk * 2 * half + j) * M + row
            i1 = i0 + half * M
            w = table[j * stride_tw]
            u, v = work[i0], work[i1]
            if dit:
                v = v * w % Q
                work[i0], work[i1] = (u + v) % Q, (u - v) % Q
            else:
                work[i0], work[i1] = (u + v) % Q, (u - v) * w % Q

    half = 1
    while half <= d // 2:
        stage(half, twi, True)
        half *= 2
    for t in range(d * M):                                     # k_fkb_twist
        i, row = t // M, t % M
        if row < rows and i:
            work[base + i * M + row] = work[base + i * M + row] * twi[i] % Q
    half = d // 2
    while half >= 1:
        stage(half, tw, False)
        half //= 2
    out = [GARBAGE] * (rows * d)
    for t in range(d * M):                                     # k_fkb_finish
        q, row = t // M, t % M
        if row < rows:
            out[row * d + bitrev(q, log2d)] = (work[q * M + row] + work[base + q * M + row]) % Q
    return out, coef


def open_direct(srs, p, log2d):
    """the d openings of p at the d-th roots of unity, point by point: proof_i = (p(tau) - p(w^i)) / (tau - w^i) in the exponent, written as
    sum_k q_k srs[k] with q the quotient's coefficients (srs[k] stands for tau^k G)"""
    d = 1 << log2d
    wd = pow(root(2 * d), 2, Q)
    out = []
    for i in range(d):
        z = pow(wd, i, Q)
        acc, quot = 0, [0] * d
        for k in range(d - 1, 0, -1):                          # synthetic division: Q_k = p_k + z Q_(k+1), q_(k-1) = Q_k
            acc = (acc * z + p[k]) % Q
            quot[k - 1] = acc
        out.append(sum(qk * s for qk, s in zip(quot, srs)) % Q)
    return out


def batch(srs, data, n, m, stride, log2d, vec, alloc_limit=0):
    """the whole call over Z_q -> (proofs m x d, commitments or None); rows of the 'rows' route go through the per-point reference"""
    d = 1 << log2d
    pl = plan(log2d, m, alloc_limit)
    proofs, coms = [], []

    def coeffs_of(j):
        row = list(data[j * stride:j * stride + n])
        if not vec:
            return row
        ev = row + [0] * (d - n)
        wd_inv = pow(pow(root(2 * d), 2, Q), Q - 2, Q) if d > 1 else 1
        return [x * pow(d, Q - 2, Q) % Q for x in dft(ev, wd_inv)]

    if pl["route"] == "rows":
        for j in range(m):
            c = coeffs_of(j)
            proofs += open_direct(srs, c, log2d)
            coms.append(sum(x * s for x, s in zip(c, srs)) % Q)
    else:
        hs = hat_s(srs, log2d)
        r0 = 0
        for cnt in pl["passes"]:
            pr, coef = pass_run(hs, log2d, data[r0 * stride:], n, cnt, stride, vec)
            proofs += pr
            if vec:
                coms += [sum(coef[j * d + k] * srs[k] for k in range(d)) % Q for j in range(cnt)]
            r0 += cnt
    return proofs, (coms if vec else None)


# ---- the route cases of tests/test_gpu_fk_batch.py: (id, log2d, m, stride, limit) ----------------------------------------------------------------
# limit: None, or ("pts", rows[, -1]): the request for the point workspace of a pass of `rows` rows (minus one byte)
GPU_CASES = [
    ("batch", 6, 130, 64, None),
    ("rows_cap", 1, ROWS_MAX + 66, 2, None),                  # two passes by FKB_ROWS_MAX, the second one ragged
    ("rows_cap_stride", 1, ROWS_MAX + 1, 3, None),            # ... its rows found through stride > d
    ("halved", 6, 130, 64, ("pts", 33)),                      # 130 -> 65 -> 33 rows: four passes
    ("row_by_row", 6, 130, 64, ("pts", 1, -1)),               # not even one row's workspace: the single pipeline
    ("d1", 0, 3, 1, None),                                    # d = 1 is not a batch domain
]


def case(name):
    return next(k for k in GPU_CASES if k[0] == name)


def case_limit(k):
    lim = k[4]
    if lim is None:
        return 0
    return request(pts_bytes(k[1], lim[1])) + (lim[2] if len(lim) > 2 else 0)


def reach(k):
    """what the case reaches, from a context that holds no batch workspace: the plan, and the kernels it launches"""
    pl = plan(k[1], k[2], case_limit(k))
    pl["kernels"] = set(launches(k[1], True) + launches(k[1], False)) if pl["route"] == "batch" else set()
    return pl
