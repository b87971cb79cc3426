"""KZG set openings over Z_r in Python integers: the reference of keaki_amd/csrc/kzg_multi.hip and of the C ABI built on it.

For DISTINCT points z_0 .. z_(k-1):  Z(x) = prod (x - z_j),  c_j = 1 / Z'(z_j) = 1 / prod_(t != j) (z_j - z_t),  I = the interpolant of (z_j, y_j).
  quotient_long_division(p, zs)      (p - I) / Z by schoolbook long division: what the proof commits to, BY DEFINITION
  quotient_partial_fractions(p, zs)  sum_j c_j (p - p(z_j)) / (x - z_j): what the kernel computes
Polynomials are coefficient lists, low degree first."""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FR_MONT_R = (1 << 256) % R


def inv(a):
    return pow(a % R, R - 2, R)


def poly_eval(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def poly_mul_linear(p, z):
    """p * (x - z)"""
    out = [0] * (len(p) + 1)
    for i, c in enumerate(p):
        out[i + 1] = (out[i + 1] + c) % R
        out[i] = (out[i] - z * c) % R
    return out


def vanishing(zs):
    """the k + 1 coefficients of Z, monic"""
    p = [1]
    for z in zs:
        p = poly_mul_linear(p, z)
    return p


def weights(zs):
    out = []
    for j, zj in enumerate(zs):
        d = 1
        for t, zt in enumerate(zs):
            if t != j:
                d = d * (zj - zt) % R
        out.append(inv(d))
    return out


def divide_linear(p, z):
    """(quotient of p by (x - z), remainder = p(z)): Q_i = p_i + z Q_(i+1), quotient coefficient i - 1 = Q_i"""
    q = [0] * max(len(p) - 1, 0)
    carry = 0
    for i in range(len(p) - 1, -1, -1):
        carry = (p[i] + z * carry) % R
        if i >= 1:
            q[i - 1] = carry
    return q, carry


def interpolant(zs, ys):
    """the k coefficients of I (deg < k), Lagrange: sum_j y_j c_j Z / (x - z_j)"""
    k = len(zs)
    zc, cs = vanishing(zs), weights(zs)
    out = [0] * k
    for zj, yj, cj in zip(zs, ys, cs):
        q, rem = divide_linear(zc, zj)
        assert rem == 0
        s = yj * cj % R
        for i in range(k):
            out[i] = (out[i] + s * q[i]) % R
    return out


def long_division(num, den):
    """schoolbook: num = quot * den + rem, den monic -> (quot, rem)"""
    assert den[-1] == 1
    rem = list(num)
    dq = len(num) - len(den)
    quot = [0] * max(dq + 1, 0)
    for i in range(dq, -1, -1):
        c = rem[i + len(den) - 1]
        quot[i] = c
        if c:
            for t, d in enumerate(den):
                rem[i + t] = (rem[i + t] - c * d) % R
    return quot, rem[:len(den) - 1]


def quotient_long_division(p, zs):
    """(the n - 1 coefficients of (p - I) / Z, zero-padded at the top as the MSM sees them; the values p(z_j)); asserts that the division is exact"""
    n, k = len(p), len(zs)
    ys = [poly_eval(p, z) for z in zs]
    ic = interpolant(zs, ys)
    num = [(c - (ic[i] if i < k else 0)) % R for i, c in enumerate(p)] + [(-ic[i]) % R for i in range(n, k)]
    quot, rem = long_division(num, vanishing(zs))
    assert not any(rem), "Z does not divide p - I"
    quot = quot + [0] * (max(n - 1, 0) - len(quot))
    assert not any(quot[max(n - 1, 0):])
    return quot[:max(n - 1, 0)], ys


def quotient_partial_fractions(p, zs):
    n = len(p)
    out = [0] * max(n - 1, 0)
    for z, c in zip(zs, weights(zs)):
        q, _ = divide_linear(p, z)
        for i in range(len(q)):
            out[i] = (out[i] + c * q[i]) % R
    return out


def set_proof_dl(p, zs, tau):
    """discrete log of the set proof for the SRS of secret tau"""
    q, _ = quotient_long_division(p, zs)
    return poly_eval(q, tau)
