"""Model of KZG batch verification (keaki_hip_kzg_verify_batch) on inputs with KNOWN discrete logs, in plain big-int arithmetic.

With a known secret tau and polynomial p: C = p(tau) g1, y_i = p(z_i), proof_i = q_i g1 with q_i = (p(tau) - y_i) / (tau - z_i). For
coefficients gamma_i the call forms

    L = sum gamma_i C_i - (sum gamma_i y_i) g1 + sum (gamma_i z_i) proof_i        R = sum gamma_i proof_i

so, with c_i the discrete log of C_i,  R = (sum gamma_i q_i) g1  and  L = (sum gamma_i c_i - sum gamma_i y_i + sum gamma_i z_i q_i) g1,
and e(L, g2) == e(R, [tau]_2)  <=>  L == tau R. Nothing here touches the library under test: the expected sums cost O(n) products
and two scalar multiplications. `combine` is the same thing on points (bn254_py), for small n."""
import bn254_py as py

R = py.R


def batch_inverse(xs):
    """Montgomery's trick: one modular inversion for the whole list (every entry non-zero)"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


class Case:
    """n openings as discrete logs: com[i] (one entry: shared by all items), z, y, q (proofs), gamma -- all integers mod r"""

    def __init__(self, tau, com, z, y, q, gamma):
        self.tau, self.com, self.z, self.y, self.q, self.gamma = tau % R, list(com), list(z), list(y), list(q), list(gamma)
        self.n = len(self.y)
        assert len(self.z) == self.n and len(self.q) == self.n and len(self.gamma) == self.n and len(self.com) in (1, self.n)

    def copy(self):
        return Case(self.tau, self.com, self.z, self.y, self.q, self.gamma)

    def com_of(self, i):
        return self.com[0] if len(self.com) == 1 else self.com[i]

    def sums(self):
        """(l, r): discrete logs of L and R"""
        r = sum(g * q for g, q in zip(self.gamma, self.q)) % R
        k = sum(self.gamma) * self.com[0] % R if len(self.com) == 1 else sum(g * c for g, c in zip(self.gamma, self.com)) % R
        t = sum(g * y for g, y in zip(self.gamma, self.y)) % R
        m = sum(g * z % R * q for g, z, q in zip(self.gamma, self.z, self.q)) % R
        return (k - t + m) % R, r

    def verdict(self):
        l, r = self.sums()
        return (self.tau * r - l) % R == 0

    def points(self):
        """(L, R) as bn254_py affine points (None = identity)"""
        l, r = self.sums()
        return py.g1_mul(py.G1_GEN, l), py.g1_mul(py.G1_GEN, r)


def valid_case(tau, coeffs, zs, gammas, shifts=None):
    """valid openings of p (coefficients low degree first) at zs (none equal to tau). shifts: item i opens p + shifts[i] instead -- n
    different polynomials with commitments C_i = (p(tau) + shifts[i]) g1 and the SAME quotients."""
    ptau = poly_eval(coeffs, tau)
    ys = [poly_eval(coeffs, z) for z in zs]
    inv = batch_inverse([(tau - z) % R for z in zs])
    qs = [(ptau - y) * i % R for y, i in zip(ys, inv)]
    if shifts is None:
        return Case(tau, [ptau], zs, ys, qs, gammas)
    return Case(tau, [(ptau + s) % R for s in shifts], zs, [(y + s) % R for y, s in zip(ys, shifts)], qs, gammas)


def combine(coms, zs, ys, proofs, gammas):
    """the same sums on POINTS (bn254_py affine tuples, None = identity): -> (L, R)"""
    n = len(ys)
    L, Rp, t = None, None, 0
    for i in range(n):
        g = gammas[i] % R
        L = py.g1_add(L, py.g1_mul(coms[0] if len(coms) == 1 else coms[i], g))
        L = py.g1_add(L, py.g1_mul(proofs[i], g * zs[i] % R))
        Rp = py.g1_add(Rp, py.g1_mul(proofs[i], g))
        t = (t + g * ys[i]) % R
    L = py.g1_add(L, py.g1_neg(py.g1_mul(py.G1_GEN, t)))
    return L, Rp


def powers(w, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * w % R
    return out


def barycentric_at(evals, w, d, x):
    """p(x) for the polynomial of degree < d with p(w^i) = evals[i] (i < len(evals), zero beyond), x not a d-th root of unity; also returns
    the inverses 1 / (x - w^i) it used: p(x) = (x^d - 1) / d * sum evals[i] w^i / (x - w^i)"""
    ws = powers(w, len(evals))
    inv = batch_inverse([(x - wi) % R for wi in ws])
    s = sum(e * wi % R * iv for e, wi, iv in zip(evals, ws, inv)) % R
    return (pow(x, d, R) - 1) * pow(d, -1, R) % R * s % R, inv
