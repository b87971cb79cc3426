"""Model of the per-item side of the KZG coset check (keaki_hip_kzg_coset_pairs, keaki_hip_kzg_verify_cosets_each) on inputs with KNOWN discrete
logs, in plain big-int arithmetic -- TEST INFRASTRUCTURE, on top of tests/coset_verify_model.py (Case: com, h, y, q as integers mod r).

    A_k = C_k - [I_k(tau)]_1      c_k = h_k^l      L_k = A_k + c_k proof_k      status_k = 0  <=>  dl(L_k) == tau_l q_k

Also here: the inverse map "chosen coefficients a -> values y", the host plan of csrc/coset_rows_plan.h restated (table width, bytes, slices, chunks;
tests/test_coset_rows_plan_cpu.py holds it against the header compiled into a program), and a scalar model of the row kernel's signed-digit walk in
the documented order of operations (k_cp_rows: bases in order, windows from the low digit, carry into the next digit), which the structured GPU
families are built from. Nothing here touches the library under test."""
import coset_verify_model as M
import fk_coset_model as FM

R = M.R

# ---- the plan (csrc/coset_rows_plan.h) ---------------------------------------------------------------------------------------------------
CR_TABLE_BYTES_MAX = 512 << 20
CR_WB_CANDIDATES = (13, 10, 8)
CR_MIN_LANES = 131072
CR_CHUNK_VALUES = 1 << 20


def cr_windows(wb):
    return (254 + wb - 1) // wb + (1 if 254 % wb == 0 else 0)


def cr_entries(wb):
    return (1 << (wb - 1)) + 1


def cr_table_bytes(log2l, wb):
    return (cr_windows(wb) * cr_entries(wb) << log2l) * 64


def cr_wb(log2l):
    for wb in CR_WB_CANDIDATES:
        if cr_table_bytes(log2l, wb) <= CR_TABLE_BYTES_MAX:
            return wb
    return 8


def cr_slices(n, log2l, min_lanes=0):
    min_lanes = min_lanes or CR_MIN_LANES
    s_max = min(1 << log2l, 64)
    S = 1
    while n * S < min_lanes and S < s_max:
        S *= 2
    return S


def cr_chunk_items(n, log2l):
    return min(n, CR_CHUNK_VALUES >> log2l)


# ---- the per-item equation ---------------------------------------------------------------------------------------------------------------
def com_of(c, k):
    return c.com[0 if len(c.com) == 1 else k]


def pair_dl(c, k):
    """(dl(A_k), c_k)"""
    return (com_of(c, k) - FM.poly_eval(c.a(k), c.tau)) % R, pow(c.h[k], c.l, R)


def lhs_dl(c, k):
    """dl(L_k) = dl(A_k) + c_k q_k"""
    a, ck = pair_dl(c, k)
    return (a + ck * c.q[k]) % R


def status(c, k):
    """0 valid / 1 invalid, with verify_each's treatment of identities: L and the proof both the identity is valid, exactly one of them is not;
    [tau^l]_2 = identity: valid <=> L is the identity"""
    return 0 if (lhs_dl(c, k) - c.tau_l * c.q[k]) % R == 0 else 1


def statuses(c):
    return [status(c, k) for k in range(c.n)]


def corrupt(c, kind, k, k2=None):
    """the corruptions of the GPU tests on a copy of the case: one changed value / proof / shift of item k, or the proofs of k and k2 swapped"""
    b = c.copy()
    if kind == "value":
        b.y[k][c.l - 1] = (b.y[k][c.l - 1] + 1) % R
    elif kind == "proof":
        b.q[k] = (b.q[k] + 1) % R
    elif kind == "shift":
        b.h[k] = b.h[k] * 3 % R
    elif kind == "swap":
        b.q[k], b.q[k2] = b.q[k2], b.q[k]
    return b


def values_from_coeffs(h, a):
    """y_t = I(h omega_l^t) for I(X) = sum_j a_j X^j, l = len(a): the inverse of coset_verify_model.interpolant_coset"""
    return [FM.poly_eval(list(a), z) for z in M.coset_points(h, len(a))]


# ---- the signed-digit walk of the row kernel -------------------------------------------------------------------------------------------------
def digits(v, wb):
    """the signed wb-bit digits of the canonical integer v < r as fb_accumulate / k_cp_rows walk them: digit in (-2^(wb-1), 2^(wb-1)], a digit above
    half becomes digit - 2^wb with a carry into the next one (2^wb itself: 0 and a carry)"""
    half, out, carry = 1 << (wb - 1), [], 0
    for _ in range(cr_windows(wb)):
        d = (v & ((1 << wb) - 1)) + carry
        v >>= wb
        carry = 1 if d > half else 0
        out.append(d - (1 << wb) if d > half else d)
    assert v == 0 and carry == 0, "the top window absorbs the last carry"
    return out


def from_digits(ds, wb):
    return sum(d << (wb * w) for w, d in enumerate(ds))


def walk(vs, tau, wb, first_base=0):
    """the discrete logs of the accumulator after every table addition of one lane that owns the bases first_base .. first_base + len(vs) - 1 with the
    canonical scalars vs: [(acc before, dl of the entry added)]"""
    out, acc = [], 0
    for i, v in enumerate(vs):
        tj = pow(tau, first_base + i, R)
        for w, d in enumerate(digits(v, wb)):
            if d:
                e = d * (1 << (wb * w)) % R * tj % R
                out.append((acc, e))
                acc = (acc + e) % R
    return out, acc


def neg_rows_to_coeffs(vs):
    """the kernel walks v_j = -a_j mod r: the coefficients a_j that put the chosen canonical integers vs into the rows"""
    return [(-v) % R for v in vs]


def case_from_rows(tau, com, h, rows, q=0, tau_l=None):
    """ONE item whose row of scalars -a_j is `rows` (canonical integers < r): its values follow from the coefficients"""
    a = neg_rows_to_coeffs(rows)
    return M.Case(tau, len(rows), [com], [h], [values_from_coeffs(h, a)], [q], [1], tau_l)


# ---- structured rows: the digit families and the branch families of the GPU tests ----------------------------------------------------------
def digit_rows(wb):
    """name -> one canonical scalar v < r whose walk at width wb meets the named digit case"""
    half, W = 1 << (wb - 1), cr_windows(wb)
    full = 253 // wb                                   # windows that lie wholly below bit 253: any digits there keep v < 2^253 < r
    top = (W - 1) * wb                                 # bit offset of the top window
    return {
        "zero": 0,
        "half": sum(half << (wb * w) for w in range(full)),                      # every digit exactly 2^(wb-1): the largest positive digit, no carry
        "half_plus_1": sum((half + 1) << (wb * w) for w in range(full)),         # every raw digit 2^(wb-1) + 1: negative digits, a carry out of each
        "carry_to_top": (1 << top) - 1,                                            # -1, then 2^wb (digit 0, carry 1) all the way into the top window
        "r_minus_1": R - 1,
    }


def digit_family(name, wb, l, seed_v=None):
    """the l scalars of one item: the named v at every base; 'one_base': zero but for the last base"""
    if name == "one_base":
        return [0] * (l - 1) + [seed_v % R]
    return [digit_rows(wb)[name]] * l


def branch_family(name, tau, wb):
    """rows of l = 2 scalars (bases 1 and tau) that drive the complete addition through its special cases: with ONE slice the lane adds base 0's
    entries, then base 1's; with TWO slices each lane sums one base and the exchange adds the two partial sums"""
    d = 5
    tail = 3 << wb                                     # a second digit of base 1: the walk goes on after the special case
    return {
        "double_mid_walk": [d * tau % R, d + tail],              # one slice: acc = 5 tau G meets the entry 5 [tau]_1
        "identity_mid_walk": [(-d * tau) % R, d + tail],         # one slice: acc = -5 tau G meets 5 [tau]_1, the sum is the identity, then 3 2^wb [tau]_1
        "slices_equal": [(d + tail) * tau % R, d + tail],        # two slices: both partial sums are (5 + 3 2^wb) tau G
        "slices_opposite": [(-(d + tail) * tau) % R, d + tail],  # two slices: opposite partial sums, the item's sum is the identity
    }[name]
