"""Model of KZG coset batch verification (keaki_hip_kzg_verify_cosets) on inputs with KNOWN discrete logs, in plain big-int arithmetic -- TEST
INFRASTRUCTURE.

l = 2^log2l, omega_l the generator of the size-l Radix2EvaluationDomain. Item k: a commitment c_k = p_k(tau), a shift h_k != 0, the l values
y_(k,t) = p_k(h_k omega_l^t), a proof q_k = floor(p_k / (x^l - h_k^l))(tau), a coefficient gamma_k -- all as integers mod r. The call forms

    a_(k,j) = h_k^-j l^-1 sum_t y_(k,t) omega_l^(-j t)        J_j = sum_k gamma_k a_(k,j)        s_k = gamma_k h_k^l
    L = sum gamma_k C_k - sum_j J_j [tau^j]_1 + sum s_k proof_k        R = sum gamma_k proof_k

so dl(R) = sum gamma_k q_k, dl(L) = sum gamma_k c_k - sum_j J_j tau^j + sum s_k q_k, and e(L, g2) == e(R, [tau^l]_2) <=> dl(L) == tau^l dl(R).
`tau_l` is what the caller passes as the discrete log of the G2 point (tau^l unless a test passes another power). Nothing here touches the
library under test. The inverse transform is a recursive decimation in TIME (the kernel runs an iterative decimation in frequency);
tests/test_coset_verify_model.py checks it against Lagrange interpolation (kzg_set_model.interpolant)."""
import fk_coset_model as FM

R = FM.R
omega, inv = FM.omega, FM.inv
VC_TILE_ELEMS = 1024          # csrc/internal.h: values of one LDS tile of the transform kernel; a tile holds VC_TILE_ELEMS / l items
VC_INV = 16                   # csrc/kzg_cosets.hip: items that share one Fermat inversion


def tile_items(l):
    return VC_TILE_ELEMS // l


def _dft(x, w):
    """X[j] = sum_t x[t] w^(j t), len(x) a power of two, w of that order"""
    n = len(x)
    if n == 1:
        return list(x)
    w2 = w * w % R
    ev, od = _dft(x[0::2], w2), _dft(x[1::2], w2)
    out, tw = [0] * n, 1
    for j in range(n // 2):
        t = tw * od[j] % R
        out[j], out[j + n // 2] = (ev[j] + t) % R, (ev[j] - t) % R
        tw = tw * w % R
    return out


def interpolant_coset(h, ys):
    """the l coefficients a_j of the polynomial of degree < l with I(h omega_l^t) = ys[t]"""
    l = len(ys)
    b = _dft(ys, inv(omega(l)))
    li, hi = inv(l), inv(h)
    out, pw = [], li
    for j in range(l):
        out.append(b[j] * pw % R)
        pw = pw * hi % R
    return out


def coset_points(h, l):
    w, out, acc = omega(l), [], h % R
    for _ in range(l):
        out.append(acc)
        acc = acc * w % R
    return out


class Case:
    """n items as discrete logs: com (one entry: shared by all items), h, y (n rows of l), q (proofs), gamma; tau_l: the G2 point's discrete log"""

    def __init__(self, tau, l, com, h, y, q, gamma, tau_l=None):
        self.tau, self.l = tau % R, l
        self.com, self.h, self.y, self.q, self.gamma = list(com), list(h), [list(r) for r in y], list(q), list(gamma)
        self.tau_l = pow(self.tau, l, R) if tau_l is None else tau_l
        self.n = len(self.h)
        assert len(self.y) == self.n and len(self.q) == self.n and len(self.gamma) == self.n and len(self.com) in (1, self.n)
        assert all(len(r) == l for r in self.y)

    def copy(self):
        return Case(self.tau, self.l, self.com, self.h, self.y, self.q, self.gamma, self.tau_l)

    def a(self, k):
        return interpolant_coset(self.h[k], self.y[k])

    def J(self):
        out = [0] * self.l
        for k in range(self.n):
            g = self.gamma[k]
            for j, aj in enumerate(self.a(k)):
                out[j] = (out[j] + g * aj) % R
        return out

    def s(self):
        return [g * pow(h, self.l, R) % R for g, h in zip(self.gamma, self.h)]

    def sums(self):
        """(dl(L), dl(R))"""
        r = sum(g * q for g, q in zip(self.gamma, self.q)) % R
        k = sum(self.gamma) * self.com[0] % R if len(self.com) == 1 else sum(g * c for g, c in zip(self.gamma, self.com)) % R
        t = FM.poly_eval(self.J(), self.tau)
        m = sum(s * q for s, q in zip(self.s(), self.q)) % R
        return (k - t + m) % R, r

    def verdict(self):
        l, r = self.sums()
        return (self.tau_l * r - l) % R == 0

    def single(self, k):
        """verify_multi's verdict on item k alone: c_k - I_k(tau) == q_k (tau_l - h_k^l)"""
        lhs = (self.com[0 if len(self.com) == 1 else k] - FM.poly_eval(self.a(k), self.tau)) % R
        return (lhs - self.q[k] * (self.tau_l - pow(self.h[k], self.l, R))) % R == 0


def valid_case(tau, polys, hs, l, gammas):
    """valid items: item k opens polys[k] (polys of ONE entry: every item opens it, one shared commitment) on the coset hs[k] <omega_l>"""
    n = len(hs)
    shared = len(polys) == 1
    com, y, q = [], [], []
    for k in range(n):
        p = polys[0 if shared else k]
        y.append([FM.poly_eval(p, z) for z in coset_points(hs[k], l)])
        q.append(FM.poly_eval(FM.quotient_coset(p, l, pow(hs[k], l, R)), tau))
        if not shared or k == 0:
            com.append(FM.poly_eval(p, tau))
    return Case(tau, l, com, hs, y, q, gammas)


def vector_case(tau, p, log2d, log2l, gammas):
    """all r = d / l cosets {i + t r} of the size-d domain for the polynomial p (d coefficients): h_i = omega_d^i, proofs from
    fk_coset_model.proofs_direct. Also returns the d evaluations in domain order (value (i, t) is entry i + t r)."""
    d, l = 1 << log2d, 1 << log2l
    r = d // l
    wd = omega(d)
    hs = [pow(wd, i, R) for i in range(r)]
    evals = _dft(list(p), wd)
    y = [[evals[i + t * r] for t in range(l)] for i in range(r)]
    return Case(tau, l, [FM.poly_eval(p, tau)], hs, y, FM.proofs_direct(p, log2d, log2l, tau), gammas), evals
