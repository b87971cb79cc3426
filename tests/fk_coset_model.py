"""FK23 coset openings in Python integers: the reference of keaki_amd/csrc/fk_coset.hip and of the C ABI built on it -- TEST INFRASTRUCTURE.

p has d = 2^log2d coefficients, l = 2^log2l <= d, r = d / l. Coset i < r is the index set {i + t r : t < l} of the size-d domain, the l solutions of
x^l = c_i, c_i = omega_r^i. Its proof commits to floor(p / (x^l - c_i)).
  quotient_coset(p, l, c)            that quotient by the recurrence q_m = f_(m+l) + c q_(m+l) (test_fk_coset_model.py checks it against schoolbook
                                     long division, kzg_set_model.long_division)
  proofs_direct(p, log2d, log2l, tau)  (a) the r discrete logs sum_m q_m tau^m, BY DEFINITION
  proofs_toeplitz(srs, p, ...)       (b) the device pipeline index for index, in discrete-log space: the group is Z_q under addition, a "scalar
                                     multiple" is a product mod q, srs[k] stands for tau^k
  split_plan(n2, l, ...)             (c) the host's split of a position's l terms over lanes and groups (csrc/fk_coset_plan.h: fkc_plan)
Everything takes the field as `F` (modulus, two-adic root and its log2 order): BN254's scalar field by default, and the small field of
tests/fk_shard_model.py where the two models are compared. Polynomials are coefficient lists, low degree first."""
from collections import namedtuple

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Field = namedtuple("Field", "q root two_adicity")
FR = Field(R, pow(5, (R - 1) >> 28, R), 28)          # ark-bn254's TWO_ADIC_ROOT_OF_UNITY
F_SMALL = Field(998244353, pow(3, (998244353 - 1) >> 23, 998244353), 23)   # the field of fk_shard_model.py (its root(n) = 3^((q-1)/n))

# csrc/fk_coset_plan.h (test_fk_coset_model.py compares these two with the header's text)
FKC_G = 4
FKC_SPLIT_MIN_LANES = 131072


def omega(n, F=FR):
    """the generator of the size-n Radix2EvaluationDomain"""
    log2n = n.bit_length() - 1
    assert n == 1 << log2n and log2n <= F.two_adicity
    return pow(F.root, 1 << (F.two_adicity - log2n), F.q)


def inv(a, F=FR):
    return pow(a % F.q, F.q - 2, F.q)


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def coset_indices(d, l, i):
    r = d // l
    return [i + t * r for t in range(l)]


def poly_eval(p, x, F=FR):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % F.q
    return acc


def quotient_coset(p, l, c, F=FR):
    """floor(p / (x^l - c)): len(p) - l coefficients (none when len(p) <= l)"""
    n = len(p)
    q = [0] * max(n - l, 0)
    for m in range(n - l - 1, -1, -1):
        q[m] = (p[m + l] + c * (q[m + l] if m + l < n - l else 0)) % F.q
    return q


def proofs_direct(p, log2d, log2l, tau, F=FR):
    d, l = 1 << log2d, 1 << log2l
    assert len(p) == d
    r = d // l
    wr = omega(r, F) if r > 1 else 1
    return [poly_eval(quotient_coset(p, l, pow(wr, i, F.q), F), tau, F) for i in range(r)]


def split_plan(n2, l, g_opt=0, min_lanes_opt=0):
    """(G, S, groups): terms per Straus group, lanes per position, groups per lane"""
    G = min(g_opt or FKC_G, l)
    min_lanes = min_lanes_opt or FKC_SPLIT_MIN_LANES
    S = 1
    while n2 * S < min_lanes and l // (2 * S) >= G:
        S *= 2
    return G, S, l // (S * G)


def dft(x, w, F=FR):
    n = len(x)
    pw = [1] * n
    for k in range(1, n):
        pw[k] = pw[k - 1] * w % F.q
    return [sum(x[i] * pw[i * k % n] for i in range(n)) % F.q for k in range(n)]


def dif(a, w, F=FR):
    """g1_dif_run: in place, natural order in, position q out holds X[brev(q)]; w: the root of order len(a)"""
    n = len(a)
    half = n // 2
    while half >= 1:
        stride = n // (2 * half)
        for blk in range(n // (2 * half)):
            for j in range(half):
                i0 = blk * 2 * half + j
                i1 = i0 + half
                u, v = a[i0], a[i1]
                a[i0], a[i1] = (u + v) % F.q, (u - v) * pow(w, j * stride, F.q) % F.q
        half //= 2
    return a


def hat_s_rows(srs, log2d, log2l, F=FR):
    """the handle's cache: row j, position q holds DFT_2r(S(j) reversed, then r identities)[brev(q)], S(j)_v = srs[v l + j]"""
    l, r = 1 << log2l, 1 << (log2d - log2l)
    w = omega(2 * r, F)
    return [dif([srs[(r - 1 - k) * l + j] for k in range(r)] + [0] * r, w, F) for j in range(l)]


def hat_a_rows(p, log2d, log2l, F=FR):
    """what keaki_hip_open_fk_cosets takes: row j = DFT_2r(r zeros, then f_(u l + j)) / 2r, natural order (k_fkc_pad + k_fkc_fr_stage)"""
    l, r = 1 << log2l, 1 << (log2d - log2l)
    w, s = omega(2 * r, F), inv(2 * r, F)
    return [[x * s % F.q for x in dft([0] * r + [p[u * l + j] for u in range(r)], w, F)] for j in range(l)]


def proofs_from_hat(hs, ha, log2d, log2l, F=FR, plan=None):
    """k_fkc_pointwise .. k_fkc_finish: lane (s, q) sums its slice of terms in groups, lane q of the gather adds the S partial sums"""
    l, r = 1 << log2l, 1 << (log2d - log2l)
    if r == 1:
        return [0]
    n2, L2 = 2 * r, log2d - log2l + 1
    G, S, groups = plan or split_plan(n2, l)
    assert S * G * groups == l
    partial = [0] * (S * n2)
    for t in range(S * n2):
        s, q = t // n2, t % n2
        total = 0
        for grp in range(groups):
            j0 = s * (l // S) + grp * G
            total += sum(ha[j][bitrev(q, L2)] * hs[j][q] for j in range(j0, j0 + G))
        partial[t] = total % F.q
    hh = [0] * n2
    for q in range(n2):                                        # k_fkc_gather
        hh[bitrev(q, L2)] = sum(partial[s * n2 + q] for s in range(S)) % F.q
    w2 = omega(n2, F)
    dif(hh, inv(w2, F), F)                                     # the (2r)^-1 is already in hat_a
    h = [hh[bitrev(k, L2)] for k in range(r)]                  # k_fkc_take
    dif(h, w2 * w2 % F.q, F)
    out = [0] * r
    for q in range(r):                                         # k_fkc_finish
        out[bitrev(q, L2 - 1)] = h[q]
    return out


def proofs_toeplitz(srs, p, log2d, log2l, F=FR, plan=None):
    return proofs_from_hat(hat_s_rows(srs, log2d, log2l, F), hat_a_rows(p, log2d, log2l, F), log2d, log2l, F, plan)
