"""Model of the per-item side of the KZG set check over arbitrary point sets (keaki_hip_kzg_set_pairs, keaki_hip_kzg_verify_sets_each) on inputs with
KNOWN discrete logs, in plain big-int arithmetic -- TEST INFRASTRUCTURE, on top of tests/verify_sets_model.py (Case: com, z, y, q as integers mod r)
and tests/kzg_set_model.py (Z and I by schoolbook arithmetic).

    A_i = C_i - [I_i(tau)]_1      Z2_i = [Z_i(tau)]_2      status_i = 0  <=>  dl(A_i) == q_i dl(Z2_i)

with the identity rule: R = (q_i == 0 or dl(Z2_i) == 0); if dl(A_i) == 0 or R, the item is valid iff both hold (which is what the equation says
too: the rule only states that no pairing arithmetic is needed).

Also here: the rows the Fr kernel leaves (-I padded to kp, Z without its monic top coefficient), the host plan of csrc/set_rows_plan.h restated (table
width, bytes, slices, chunks; tests/test_set_rows_plan_cpu.py holds it against the header compiled into a program), and a scalar model of the G2 row
kernel's signed-digit walk in the documented order of operations (k_sp_rows_g2: bases in order, windows from the low digit, carry into the next digit;
[tau^k]_2 last). Nothing here touches the library under test."""
import kzg_set_model as KM
import verify_sets_model as M

R = M.R

# ---- the plan (csrc/set_rows_plan.h) -----------------------------------------------------------------------------------------------------
SR_TABLE_BYTES_MAX = 512 << 20
SR_WB_CANDIDATES = (13, 10, 8)
SR_MIN_LANES = 65536
SR_CHUNK_VALUES = 1 << 20
SE_CHUNK_MIN = 32


def sr_windows(wb):
    return (254 + wb - 1) // wb + (1 if 254 % wb == 0 else 0)


def sr_entries(wb):
    return (1 << (wb - 1)) + 1


def sr_table_bytes(kb, wb):
    return sr_windows(wb) * sr_entries(wb) * kb * 128


def sr_wb(kb):
    for wb in SR_WB_CANDIDATES:
        if sr_table_bytes(kb, wb) <= SR_TABLE_BYTES_MAX:
            return wb
    return 8


def sr_wb_narrower(wb):
    return 10 if wb > 10 else 8 if wb > 8 else 0


def sr_log2kp(k):
    b = 0
    while (1 << b) < k:
        b += 1
    return b


def sr_slices(n, log2kp, min_lanes=0):
    min_lanes = min_lanes or SR_MIN_LANES
    s_max = min(1 << log2kp, 64)
    S = 1
    while n * S < min_lanes and S < s_max:
        S *= 2
    return S


def sr_chunk_items(n, log2kp):
    return min(n, SR_CHUNK_VALUES >> log2kp)


def sr_item_bytes(k, log2kp, point_mode, msm_route):
    return ((1 << log2kp) + (3 if point_mode else 2) * k) * 32 + 128 + 256 + (96 if msm_route else 0)


def se_route(route_opt, n=0):
    return 1 if route_opt == 1 else 2


def se_chunk_items(n, launch_items):
    return min(n, launch_items // 2)


def se_chunk_halve(ch):
    return max(SE_CHUNK_MIN, ((ch + 1) // 2 + 31) & ~31)


# ---- the per-item equation ---------------------------------------------------------------------------------------------------------------
def com_of(c, i):
    return c.com[0 if len(c.com) == 1 else i]


def pair_dl(c, i):
    """(dl(A_i), dl(Z2_i)): the second over the G2 points the call reads (c.g2_powers: tau^t unless the case says otherwise)"""
    a = (com_of(c, i) - M.poly_eval(c.I(i), c.tau)) % R
    z2 = sum(zc * p for zc, p in zip(c.Z(i), c.g2_powers)) % R
    return a, z2


def status(c, i):
    a, z2 = pair_dl(c, i)
    r_inf = c.q[i] % R == 0 or z2 == 0
    if a == 0 or r_inf:
        return 0 if (a == 0 and r_inf) else 1
    return 0 if (a - c.q[i] * z2) % R == 0 else 1


def statuses(c):
    return [status(c, i) for i in range(c.n)]


def rows(c, i):
    """(-I padded with zeros to kp, Z without the top coefficient) of item i: what k_vs_polys<1> stores, as canonical integers"""
    kp = M.kp_of(c.k)
    ic = [(-v) % R for v in c.I(i)]
    return ic + [0] * (kp - c.k), c.Z(i)[:c.k]


def corrupt(c, kind, i, j=0, delta=1):
    """a copy of the case with item i broken: 'proof', 'value' (value j), 'point' (point j), 'com' (needs one commitment per item)"""
    d = c.copy()
    if kind == "proof":
        d.q[i] = (d.q[i] + delta) % R
    elif kind == "value":
        d.y[i][j] = (d.y[i][j] + delta) % R
    elif kind == "point":
        d.z[i][j] = (d.z[i][j] + delta) % R
        assert len(set(d.z[i])) == c.k
    elif kind == "com":
        assert len(d.com) == c.n
        d.com[i] = (d.com[i] + delta) % R
    else:
        raise ValueError(kind)
    return d


# ---- the signed-digit walk of the G2 row kernel ----------------------------------------------------------------------------------------------
def digits(v, wb):
    """the signed wb-bit digits of the canonical integer v < r as fb_accumulate_g2_u29 / k_sp_rows_g2 walk them: digit in (-2^(wb-1), 2^(wb-1)], a digit
    above half becomes digit - 2^wb with a carry into the next one (2^wb itself: 0 and a carry)"""
    half, out, carry = 1 << (wb - 1), [], 0
    for _ in range(sr_windows(wb)):
        d = (v & ((1 << wb) - 1)) + carry
        v >>= wb
        carry = 1 if d > half else 0
        out.append(d - (1 << wb) if d > half else d)
    assert v == 0 and carry == 0, "the top window absorbs the last carry"
    return out


def from_digits(ds, wb):
    return sum(d << (wb * w) for w, d in enumerate(ds))


def walk(zc, g2_powers, wb, S=1):
    """one item of k_sp_rows_g2: zc = the k stored coefficients of Z, g2_powers the k + 1 discrete logs of the bases. -> (events, dl of the sum): events
    are (dl of the accumulator before, dl of the entry added) for every table addition of every slice, then the joins of the slices (a tree over
    neighbours), then the addition of the top base"""
    k = len(zc)
    kp = M.kp_of(k)
    per = kp // S
    ev, parts = [], []
    for s in range(S):
        acc = None
        for j in range(s * per, min((s + 1) * per, k)):
            for w, d in enumerate(digits(zc[j] % R, wb)):
                e = d * (1 << (wb * w)) % R * g2_powers[j] % R
                if d and g2_powers[j] % R:
                    ev.append((acc, e))
                    acc = e if acc is None else (acc + e) % R
                    if acc == 0:
                        acc = None                     # opposite operands: the identity, and the walk goes on
        parts.append(acc)
    step = 1
    while step < S:
        for s in range(0, S, 2 * step):
            a, b = parts[s], parts[s + step]
            ev.append((a, b))
            t = ((a or 0) + (b or 0)) % R
            parts[s] = t if (a is not None or b is not None) and t else None
        step *= 2
    ev.append((parts[0], g2_powers[k] % R))
    return ev, ((parts[0] or 0) + g2_powers[k]) % R


def event_kinds(ev):
    """how many additions met an equal operand (a doubling), an opposite one (the identity) or an empty accumulator"""
    out = {"equal": 0, "opposite": 0, "empty": 0}
    for acc, e in ev:
        if acc is None or e is None:
            out["empty"] += 1
        elif acc == e % R:
            out["equal"] += 1
        elif (acc + e) % R == 0:
            out["opposite"] += 1
    return out


def branch_coeffs(wb):
    """k = 4 coefficients for an SRS of tau = 1 (all bases equal g2): 3 then 3 again (equal operands: a doubling), then 2^wb - 6 = digits (-6, +1) (the
    -6 meets the accumulator 6: opposite operands, the identity, and the walk goes on), then 5"""
    return [3, 3, (1 << wb) - 6, 5]


def point_for_coeff(v):
    """k = 1: Z_0 = -z, so z = -Z_0. k = 2 with z_1 = 0: Z_1 = -z_0, Z_0 = 0. -> the point that puts the chosen canonical integer v into the row"""
    return (-v) % R


def sqrt_mod_r(a):
    """a square root of a mod r, or None (Tonelli-Shanks: r - 1 = 2^28 x odd)"""
    a %= R
    if a == 0:
        return 0
    if pow(a, (R - 1) // 2, R) != 1:
        return None
    s, q = 0, R - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = 2
    while pow(z, (R - 1) // 2, R) == 1:
        z += 1
    m, c, t, x = s, pow(z, q, R), pow(a, q, R), pow(a, (q + 1) // 2, R)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % R, i + 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c, t, x = i, b * b % R, t * b * b % R, x * b % R
    return x


def points_for_pair(z0c, z1c):
    """k = 2: the two points with Z = X^2 + z1c X + z0c, or None when the polynomial does not split over Fr (or has a double root)"""
    s = sqrt_mod_r(z1c * z1c - 4 * z0c)
    if not s:
        return None
    h = M.inv(2)
    return [(-z1c + s) * h % R, (-z1c - s) * h % R]


def opposite_pair(wb):
    """k = 2 on an SRS of tau = 1: the smallest d for which Z_0 = d, Z_1 = 2^wb - d (digits -d, +1) splits: the walk holds d g2 and meets -d g2"""
    for d in range(1, 200):
        pts = points_for_pair(d, (1 << wb) - d)
        if pts and 1 not in pts:
            return d, pts
    raise AssertionError("no splitting pair")


def edge_scalars(wb):
    """canonical integers whose digits sit at the edges of the recoding: the half (stays positive), half + 1 (the first negative digit, with a carry),
    2^wb - 1 (digit -1 and a carry), a carry chain into the top window, and zero (the all-zero row)"""
    half, top = 1 << (wb - 1), sr_windows(wb) - 1
    out = [0, 1, half, half + 1, (1 << wb) - 1, 1 << wb, (half + 1) << wb, R - 1, R - half, R - half - 1]
    lim = min(R - 1, (1 << (wb * top)) - 1)
    out.append(lim)                                                          # all ones below the top window: the carry runs the whole way up
    return [v % R for v in out]
