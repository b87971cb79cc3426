"""Bases with known discrete logs, their references, and models of where the group kernels meet exceptional additions -- TEST
INFRASTRUCTURE (a plain module, imported by tests/test_structured_inputs_model.py, tests/test_gpu_structured_srs.py and
tests/test_gpu_fb_digit_edges.py).

Every base is k * G with k known, so an expected result is scalar arithmetic mod r and only its last step needs a point. The models follow
the kernels' documented order of operations on those scalars and count the additions that take an exceptional branch: equal or opposite
operands, or an identity produced from two non-identity inputs. With random bases each of these has probability ~2^-254; the structured
secrets below make them common. A model that stops matching a kernel's order must fail its CPU test rather than silently lose coverage.
"""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd      # GLV eigenvalue of Fr: lambda^2 + lambda + 1 = 0


def root_of_unity(n):
    """ark-poly Radix2EvaluationDomain generator of order n (n a power of two)"""
    return pow(pow(5, (R - 1) >> 28, R), (1 << 28) // n, R)


def secrets(c=8, log2d=3):
    """the catalogue of secrets tau: name -> value. c: the MSM window width of the call; log2d: the FK domain (d = 2^log2d)"""
    d = 1 << log2d
    w2d = root_of_unity(2 * d)
    return {
        "zero": 0,                      # SRS [G, O, O, ...], [tau]_2 = O
        "one": 1,                       # every point is G
        "minus_one": R - 1,             # points alternate +-G
        "two": 2,
        "half": (R + 1) // 2,
        "two_pow_c": 1 << c,            # P_(i+1) = the next window's table entry of P_i
        "lambda": LAMBDA,               # P_(i+1) = phi(P_i): same y, another x (R = 0 while H != 0 in the addition formulas)
        "omega_2d": w2d,                # the group FFT of a geometric sequence concentrates in a few bins
        "omega_d": w2d * w2d % R,
        "minus_omega_2d": R - w2d,
        "random": 0x1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80 % R,
    }


def powers(tau, n):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * tau % R
    return out


def poly_eval(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def poly_deriv_eval(p, x):
    acc = 0
    for i in range(len(p) - 1, 0, -1):
        acc = (acc * x + i * p[i]) % R
    return acc


# ---- references: the scalar of the expected point -----------------------------------------------------------------------------------
def msm_dlog(dlogs, scalars):
    return sum(k * s for k, s in zip(dlogs, scalars)) % R


def open_dlog(tau, p, z):
    """q(tau) for q = (p - p(z)) / (x - z): (p(tau) - p(z)) / (tau - z), or p'(z) when tau = z"""
    if tau % R == z % R:
        return poly_deriv_eval(p, z)
    return (poly_eval(p, tau) - poly_eval(p, z)) * pow(tau - z, -1, R) % R


def ntt(x, w):
    """DFT over Fr by the root w of order len(x) (a power of two), natural order in and out"""
    n = len(x)
    if n == 1:
        return list(x)
    ev, od = ntt(x[0::2], w * w % R), ntt(x[1::2], w * w % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        v = od[k] * t % R
        out[k], out[k + n // 2] = (ev[k] + v) % R, (ev[k] - v) % R
        t = t * w % R
    return out


def fk_dlogs(tau, p, evals):
    """the d FK23 proofs as scalars: proof i opens p at omega_d^i; evals[i] = p(omega_d^i) (a scalar-field DFT of p)"""
    d = len(evals)
    wd = root_of_unity(d) if d > 1 else 1
    pt = poly_eval(p, tau)
    out, x = [], 1
    for i in range(d):
        out.append(poly_deriv_eval(p, x) if x == tau % R else (pt - evals[i]) * pow(tau - x, -1, R) % R)
        x = x * wd % R
    return out


# ---- FK23 group FFTs (keaki_amd/csrc/fft_g1.hip: open_fk_poly_scalars_run, fk_hat_s_run, open_fk_run, run_stages) --------------------------------------------
def _bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def _pairable(m, h, radix4):
    """run_stages: two wave-uniform stages fused into one radix-4 pass (fk_radix4 with fk_uniform)"""
    return radix4 and h >= 8 and m // (4 * h) >= 64 and (m // 4) % 64 == 0


def _stage(a, half, tw, stride, dit, ev, key):
    """one radix-2 stage (k_g1_fft_stage_map). DIT (u, v) -> (u + w v, u - w v); DIF (u, v) -> (u + v, w (u - v)). The butterfly's
    add + subtract (addsub) leaves the lazy-limb formulas for the generic additions when an operand is the identity or u = +-(w) v; the
    latter is the exceptional case counted here -- it is also what makes an identity out of two non-identity inputs."""
    m = len(a)
    for blk in range(m // (2 * half)):
        for j in range(half):
            i0 = blk * 2 * half + j
            i1 = i0 + half
            w = tw[j * stride]
            u, v = a[i0], a[i1]
            if dit:
                v = v * w % R
            if u and v and (u == v or u + v == R):
                ev[key + "addsub_special"] += 1
            if dit:
                a[i0], a[i1] = (u + v) % R, (u - v) % R
            else:
                a[i0], a[i1] = (u + v) % R, (u - v) * w % R


def _pair_events(a, h, tw, s_h, s_2h, dit, ev, key):
    """lane events of a radix-4 pass (k_g1_fft_stage4) over the values it starts from. A lane with offset 0 or an identity among its four
    points takes the radix-2 sequence from the start. DIF: an identity among S02, D02, S13, D13 sends the lane to the radix-2 finish
    ('r4_fallback'); a two-term sum c2 / c3 of non-identities that cancels is 'mul2_identity'. DIT: L1 = w2 (e2 + w1 e3), L2 = w2' (e2 - w1 e3)."""
    m = len(a)
    for blk in range(m // (4 * h)):
        for j in range(h):
            p0 = blk * 4 * h + j
            e0, e1, e2, e3 = a[p0], a[p0 + h], a[p0 + 2 * h], a[p0 + 3 * h]
            if j == 0 or not (e0 and e1 and e2 and e3):
                continue
            ta, tb, tc = tw[j * s_h], tw[j * s_2h], tw[(j + h) * s_2h]
            if dit:
                if (e2 + ta * e3) % R == 0 or (e2 - ta * e3) % R == 0:
                    ev[key + "mul2_identity"] += 1
            else:
                s02, d02, s13, d13 = (e0 + e2) % R, (e0 - e2) % R, (e1 + e3) % R, (e1 - e3) % R
                if not (s02 and d02 and s13 and d13):
                    ev[key + "r4_fallback"] += 1
                elif (tb * d02 + tc * d13) % R == 0 or ta * (tb * d02 - tc * d13) % R == 0:
                    ev[key + "mul2_identity"] += 1


def _run_stages(a, tw, first, last, dit, stride_of, radix4, ev, key):
    m = len(a)
    if dit:
        half = first
        while half <= last:
            if 2 * half <= last and _pairable(m, half, radix4):
                _pair_events(a, half, tw, stride_of(half), stride_of(2 * half), True, ev, key)
                _stage(a, half, tw, stride_of(half), True, ev, key)
                _stage(a, 2 * half, tw, stride_of(2 * half), True, ev, key)
                half <<= 2
            else:
                _stage(a, half, tw, stride_of(half), True, ev, key)
                half <<= 1
    else:
        half = first
        while half >= last and half >= 1:
            h = half // 2
            if h >= last and h >= 1 and _pairable(m, h, radix4):
                _pair_events(a, h, tw, stride_of(h), stride_of(half), False, ev, key)
                _stage(a, half, tw, stride_of(half), False, ev, key)
                _stage(a, h, tw, stride_of(h), False, ev, key)
                half >>= 2
            else:
                _stage(a, half, tw, stride_of(half), False, ev, key)
                half >>= 1


FK_EVENTS = ("addsub_special", "r4_fallback", "mul2_identity")
FK_TRANSFORMS = ("hat_s", "inv", "fwd")


def fk_model(tau, p, log2d, radix4=True):
    """the FK23 pipeline from the coefficients (api.hip: open_fk_from_poly) over Fr: hat_s = DIF_2d(reversed powers of tau, padded with zeros); the pointwise products; DIT_d of the odd
    half, the twist, DIF_d; proofs[brev(q)] = E[q] + O[q]. Returns (proof scalars, {transform_event: count})."""
    d = 1 << log2d
    N = 2 * d
    w = root_of_unity(N)
    wi = pow(w, -1, R)
    tw = [pow(w, k, R) for k in range(d)]
    twi = [pow(wi, k, R) for k in range(d)]
    ev = {t + "_" + e: 0 for t in FK_TRANSFORMS for e in FK_EVENTS}
    pw = powers(tau, d)
    hs = [pw[d - 1 - i] for i in range(d)] + [0] * d
    _run_stages(hs, tw, d, 1, False, lambda half: N // (2 * half), radix4, ev, "hat_s_")
    # hat_a = DFT_2d(0..0, p) / 2d in natural order (a scalar-field transform: no group additions)
    inv_n = pow(N, -1, R)
    a = [x * inv_n % R for x in ntt([0] * d + [c % R for c in p], w)]
    e = [a[2 * _bitrev(q, log2d)] * d % R * hs[q] % R for q in range(d)]
    o = [a[2 * _bitrev(q, log2d) + 1] * hs[d + q] % R for q in range(d)]
    if d > 1:
        _run_stages(o, twi, 1, d // 2, True, lambda half: 2 * (d // (2 * half)), radix4, ev, "inv_")
    o = [o[i] * twi[i] % R for i in range(d)]
    if d > 1:
        _run_stages(o, tw, d // 2, 1, False, lambda half: 2 * (d // (2 * half)), radix4, ev, "fwd_")
    out = [0] * d
    for q in range(d):
        out[_bitrev(q, log2d)] = (e[q] + o[q]) % R
    return out, ev


# ---- MSM buckets (keaki_amd/csrc/msm.hip.h: msm_make_plan, msm_for_each_digit_canon, the bucket kernels) -----------------------------
def msm_plan(c_target):
    """-> (c, W, k, offsets, widths)"""
    W = (254 + c_target - 1) // c_target
    base, rem = 254 // W, 254 % W
    c, k = (base + 1, rem) if rem else (base, W)
    widths = [c if w < k else c - 1 for w in range(W)]
    offs = [sum(widths[:w]) for w in range(W)]
    return c, W, k, offs, widths


def msm_digits(s, c_target):
    """signed digits of a canonical scalar: [(window, bucket, negative)] for every non-zero digit"""
    _, W, _, offs, widths = msm_plan(c_target)
    out, carry = [], 0
    for w in range(W):
        wd = widths[w]
        full, half = 1 << wd, 1 << (wd - 1)
        coef = ((s >> offs[w]) & (full - 1)) + carry
        if w == W - 1:
            if coef:
                out.append((w, coef - 1, False))
        elif coef > half:
            carry = 1
            if coef != full:
                out.append((w, full - coef - 1, True))
        else:
            carry = 0
            if coef:
                out.append((w, coef - 1, False))
    return out


def msm_buckets(dlogs, scalars, c_target, tables):
    """bucket -> list of the dlogs of the points added to it. tables: the shared-bucket mode over window tables (window w of point i
    reads 2^offset(w) P_i, every window shares one bucket range); else the generic mode (a bucket range per window, point P_i)."""
    _, _, _, offs, _ = msm_plan(c_target)
    out = {}
    for k, s in zip(dlogs, scalars):
        for w, b, neg in msm_digits(s % R, c_target):
            e = (k << offs[w]) % R if tables else k % R
            if neg:
                e = (R - e) % R
            out.setdefault(b if tables else (w, b), []).append(e)
    return out


def bucket_events(buckets):
    """buckets whose two non-identity points meet whatever the order of arrival: 'same' (the doubling branch) and 'opposite' (the bucket
    empties). Identity points are skipped by the kernels."""
    ev = {"same": 0, "opposite": 0}
    for pts in buckets.values():
        pts = [e for e in pts if e]
        if len(pts) == 2:
            if pts[0] == pts[1]:
                ev["same"] += 1
            elif (pts[0] + pts[1]) % R == 0:
                ev["opposite"] += 1
    return ev


def collision_scalars(dlogs, c_target, tables, search=256):
    """Scalars (mostly zero) that put two equal points into one bucket and a point with its negation into another. Entries (i, w) with
    equal (or opposite) dlogs get one digit each in the same bucket; when only equal entries exist, the second pair takes the digit with a
    minus sign (the scalar 2^offset(w + 1) - m 2^offset(w)). Returns None when the SRS has no two equal or opposite entries."""
    _, W, _, offs, _ = msm_plan(c_target)
    n = min(len(dlogs), search)
    seen, same, opp = {}, [], []
    for w in range(W - 2):
        for i in range(n):
            e = (dlogs[i] << offs[w]) % R if tables else dlogs[i] % R
            if not e:
                continue
            key = e if tables else (w, e)
            nkey = (R - e) if tables else (w, R - e)
            paired = False
            for lst, out in ((seen.get(key), same), (seen.get(nkey), opp)):
                if not paired and lst and lst[-1][0] != i:
                    out.append((lst.pop(), (i, w)))           # an entry takes part in one pair at most
                    paired = True
            if not paired:
                seen.setdefault(key, []).append((i, w))
        if len(same) >= 2 and opp:
            break
    pairs = [(p, True) for p in same] + [(p, False) for p in opp]
    if not pairs:
        return None
    s = [0] * len(dlogs)
    used = set()
    # bucket 2 (digit 3) receives P and P, bucket 4 (digit 5) P and -P; a pair of the other kind flips the sign of its second digit
    for m, want_same in ((3, True), (5, False)):
        for ((a, wa), (b, wb)), is_same in pairs:
            if a in used or b in used:
                continue
            s[a] += m << offs[wa]
            s[b] += (m << offs[wb]) if is_same == want_same else (1 << offs[wb + 1]) - (m << offs[wb])
            used.update((a, b))
            break
    return [x % R for x in s]


# ---- fixed-base sums of encapsulation (keaki_amd/csrc/ec_batch.hip.h: fb_accumulate, k_encap_fixed_g2_wide, k_verify_points) ----------
def fb_windows(wb):
    return (254 + wb - 1) // wb + (1 if 254 % wb == 0 else 0)


def fb_digits(k, wb):
    """signed wb-bit digits in (-2^(wb-1), 2^(wb-1)] of a canonical scalar, one per window (0: nothing added)"""
    half = 1 << (wb - 1)
    out, carry = [], 0
    for _ in range(fb_windows(wb)):
        d = (k & (2 * half - 1)) + carry
        k >>= wb
        carry = 1 if d > half else 0
        out.append(d - 2 * half if d > half else d)
    return out


def _meet(acc, e, ev):
    if acc and e:
        if acc == e:
            ev["equal"] += 1
        elif (acc + e) % R == 0:
            ev["opposite"] += 1


def encap_ct_events(tau, r, z, wb, wide):
    """The ciphertext sum r [tau]_2 + (-(r z)) g2 over the window tables of [tau]_2 (table A) and g2 (table B). One lane adds the
    entries window by window, table A first (k_encap_fixed); the wide kernel gives window w of the concatenated list to lane w & 15,
    then adds the sixteen partial sums in a tree (lane l meets lane l ^ step). -> (ct dlog, {'equal', 'opposite'}) over the additions
    whose result reaches the output."""
    return fb_sum_events(tau, r % R, wb, 1, -(r * z) % R, wb, wide)


def fb_sum_events(base_a, ka, wb_a, base_b, kb, wb_b, wide):
    """encap_ct_events for any two tables: the sum ka (base_a G) + kb (base_b G) over a wb_a-bit table of base_a G and a wb_b-bit
    table of base_b G (also the G1 sum r C + (-(r v)) g1 of k_encap_fixed<Fq,1>: wide = False, 13 and 16 bits)"""
    ents = []
    for j, dg in enumerate(fb_digits(ka, wb_a)):
        ents.append(dg * (base_a << (wb_a * j)) % R)
    for j, dg in enumerate(fb_digits(kb, wb_b)):
        ents.append(dg * (base_b << (wb_b * j)) % R)
    ev = {"equal": 0, "opposite": 0}
    if not wide:
        acc = 0
        for e in ents:
            _meet(acc, e, ev)
            acc = (acc + e) % R
        return acc, ev
    lanes = [0] * 16
    for w, e in enumerate(ents):
        _meet(lanes[w & 15], e, ev)
        lanes[w & 15] = (lanes[w & 15] + e) % R
    step = 1
    while step < 16:
        for l in range(0, 16, 2 * step):
            _meet(lanes[l], lanes[l + step], ev)
        lanes = [(lanes[l] + lanes[l ^ step]) % R for l in range(16)]
        step <<= 1
    return lanes[0], ev


# ---- digit-edge scalars of the fixed-base walks (fb_accumulate, fb_accumulate_g2_u29, fb_pick_digits, gt_table_exp, w_gt_table_exp) ----
# Every walk forms coef = (the window's bits) + (carry in) and branches on it: coef <= half adds slot coef; coef > half adds the negated
# slot 2^wb - coef and carries; coef == 2^wb adds nothing and carries; coef == 0 adds nothing. The classes name coef values whose branch or
# table slot is special: slot `half` (the scatter of powers in the GT table, the doublings-only ladder in the EC table), slot half - 1 (the
# last entry of the top fill level wb - 2, reached with either sign), slots 2^L and 2^L + 1 (a level boundary of the fill), +-1, the two
# zeros. The order is the one a scalar walks through, window by window: each class leaves the carry its successor is meant to receive
# (`full` needs one; `zero` must not get one and sits between two non-zero digits; `pow+1` and `one` are formed by a carry).
FB_EDGE_CLASSES = ("one", "zero", "half", "half-1", "pow", "neg_first", "full", "pow+1", "minus_one")


def fb_edge_level(wb):
    """the interior fill level L whose boundary slots 2^L and 2^L + 1 the classes `pow` and `pow+1` read"""
    return wb // 2


def _fb_edge_coef(name, wb):
    full, half, p = 1 << wb, 1 << (wb - 1), 1 << fb_edge_level(wb)
    return {"one": 1, "zero": 0, "half": half, "half-1": half - 1, "pow": p, "pow+1": p + 1, "neg_first": half + 1, "full": full,
            "minus_one": full - 1}[name]


def fb_digit_classes(k, wb):
    """{(window, class)} of the walk over canonical k, the top window included. `zero` is a zero window without a carry in whose
    neighbours (the left one where there is one) have non-zero digits; any other zero window is `zero_run`, any other coef `other`."""
    W, full, half = fb_windows(wb), 1 << wb, 1 << (wb - 1)
    digs = fb_digits(k, wb)
    names = {_fb_edge_coef(c, wb): c for c in FB_EDGE_CLASSES}
    out, carry = set(), 0
    for j in range(W):
        coef = ((k >> (wb * j)) & (full - 1)) + carry
        carry = 1 if coef > half else 0
        name = names.get(coef, "other")
        if coef == 0 and not ((j == 0 or digs[j - 1]) and j + 1 < W and digs[j + 1]):
            name = "zero_run"
        out.add((j, name))
    return out


def fb_edge_required(wb):
    """the (window, class) pairs a set of edge scalars must reach: every class in every non-top window. No carry enters window 0, so
    coef = 2^wb cannot occur there: (0, 'full') is the one pair that does not exist."""
    return {(j, c) for j in range(fb_windows(wb) - 1) for c in FB_EDGE_CLASSES} - {(0, "full")}


def fb_edge_covered(scalars, wb):
    """the pairs of fb_edge_required(wb) that the scalars reach"""
    seen = set()
    for k in scalars:
        seen |= fb_digit_classes(k, wb)
    return seen & fb_edge_required(wb)


def fb_edge_scalars(wb):
    """Canonical scalars < r, all non-zero, that put every non-top window of the wb-bit walk through every class of FB_EDGE_CLASSES
    (fb_edge_required). Scalar s drives window j to class (j + s) mod 9; the bits are coef minus the carry that actually arrives. The
    top window follows the same schedule as far as a scalar below r allows, else it is lowered to the largest value that fits. Then
    r - 1, r - 2 and 1; the largest top-window digit that still takes a carry in; and a carry chain through every non-top window
    (half + 1 in window 0, all ones above it)."""
    W, full, half = fb_windows(wb), 1 << wb, 1 << (wb - 1)
    top_off = wb * (W - 1)
    nc = len(FB_EDGE_CLASSES)
    out = []
    for s in range(nc):
        low, carry = 0, 0
        for j in range(W - 1):
            raw = min(max(_fb_edge_coef(FB_EDGE_CLASSES[(j + s) % nc], wb) - carry, 0), full - 1)
            low |= raw << (wb * j)
            carry = 1 if raw + carry > half else 0
        fits = (R - 1 - low) >> top_off
        top = min(max(_fb_edge_coef(FB_EDGE_CLASSES[(W - 1 + s) % nc], wb) - carry, 0), fits)
        out.append(low + (top << top_off))
    out += [R - 1, R - 2, 1]
    # the top window of r - 1 is T; a carry enters it from window W - 2 when that one holds more than half. Where r - 1 itself has at
    # least half + 1 there, T + 1 is reached; else T - 1 under an all-ones window gives T
    T, off2 = (R - 1) >> top_off, wb * (W - 2)
    if ((R - 1) >> off2) & (full - 1) >= half + 1:
        out.append((T << top_off) | ((half + 1) << off2))
    else:
        out.append(((T - 1) << top_off) | ((full - 1) << off2))
    chain = (half + 1) + sum((full - 1) << (wb * j) for j in range(1, W - 1))
    out.append(chain + (((R - 1 - chain) >> top_off) << top_off))
    seen = set()
    return [k for k in out if not (k in seen or seen.add(k))]


def fb_edge_report(wb):
    """what fb_edge_scalars(wb) reaches: the number of (non-top window, class) pairs, the classes of the top window (which holds only
    what a scalar below r allows) and its largest digit"""
    sc = fb_edge_scalars(wb)
    W = fb_windows(wb)
    top = set()
    for k in sc:
        top |= {c for j, c in fb_digit_classes(k, wb) if j == W - 1}
    return {"scalars": len(sc), "pairs": len(fb_edge_covered(sc, wb)), "required": len(fb_edge_required(wb)),
            "top_classes": sorted(top), "top_max_digit": max(fb_digits(k, wb)[-1] for k in sc), "top_limit": (R - 1) >> (wb * (W - 1))}


def fb_edge_union(widths):
    seen = set()
    return [k for wb in widths for k in fb_edge_scalars(wb) if not (k in seen or seen.add(k))]


def fb_edge_batch(r_widths, b2_widths, b1_widths):
    """Encapsulation items (r, point, value) that carry three edge scalars each: r itself walks the tables of [tau]_2 and of the
    commitment (or A = e(C, g2)); the device's -(r point) and -(r value) are the chosen scalars for the tables of g2 and of g1 (or
    B = e(g1, g2)). Each side is the union of fb_edge_scalars over its widths; the three lists are crossed cyclically (one step apart,
    so that an item never carries the same scalar twice in a row of equal lists) until the longest is used up."""
    ta, tb2, tb1 = fb_edge_union(r_widths), fb_edge_union(b2_widths), fb_edge_union(b1_widths)
    items = []
    for i in range(max(len(ta), len(tb2), len(tb1))):
        r = ta[i % len(ta)]
        inv = pow(r, -1, R)
        items.append((r, -tb2[(i + 1) % len(tb2)] * inv % R, -tb1[(i + 2) % len(tb1)] * inv % R))
    return items


def fb_edge_sides(items):
    """the three scalars the device walks for each item: (r, -(r point), -(r value))"""
    return [it[0] % R for it in items], [-(it[0] * it[1]) % R for it in items], [-(it[0] * it[2]) % R for it in items]
