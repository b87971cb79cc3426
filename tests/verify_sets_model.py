"""Model of KZG set batch verification (keaki_hip_kzg_verify_sets) on inputs with KNOWN discrete logs, in plain big-int arithmetic -- TEST
INFRASTRUCTURE.

Item i: a commitment c_i = p_i(tau), k DISTINCT points z_(i,0) .. z_(i,k-1), the k values y_(i,j) = p_i(z_(i,j)), a proof q_i = ((p_i - I_i) /
Z_i)(tau), a coefficient gamma_i -- all as integers mod r. With Z_i = sum_(t <= k) Z_(i,t) X^t (monic) and I_i = sum_(t < k) I_(i,t) X^t the call forms

    J_t = sum_i gamma_i I_(i,t)  (t < k)        rows: S[0][i] = -gamma_i Z_(i,0),  S[t][i] = gamma_i Z_(i,t) (1 <= t < k),  S[k][i] = gamma_i
    L   = sum gamma_i C_i - sum_t J_t [tau^t]_1 + sum_i S[0][i] proof_i        R_t = sum_i S[t][i] proof_i  (1 <= t <= k)

and accepts iff e(-L, g2) prod_(t = 1 .. k) e(R_t, [tau^t]_2) == 1, i.e. -dl(L) + sum_t tau^t dl(R_t) == 0. `g2_powers` are the discrete logs of
the G2 points the call reads (tau^t unless a test passes others). Z, the weights and I come from kzg_set_model (schoolbook); what is restated
here is the COMBINATION. Nothing here touches the library under test."""
import kzg_set_model as KM

R = KM.R
inv, poly_eval = KM.inv, KM.poly_eval
K_MAX = 64                    # include/keaki_hip.h: KEAKI_VERIFY_SETS_K_MAX
VS_THREADS = 256              # csrc/kzg_sets.hip: lanes of a workgroup of the polynomial kernel
VS_INV = 16                   # (item, j) pairs that share one Fermat inversion


def kp_of(k):
    """the power of two >= k: lanes of an item slot"""
    p = 1
    while p < k:
        p *= 2
    return p


def tile_items(k):
    return VS_THREADS // kp_of(k)


class Case:
    """n items of k points as discrete logs: com (one entry: shared by all items), z and y (n rows of k), q (proofs), gamma"""

    def __init__(self, tau, k, com, z, y, q, gamma, g2_powers=None):
        self.tau, self.k = tau % R, k
        self.com, self.z, self.y, self.q, self.gamma = list(com), [list(r) for r in z], [list(r) for r in y], list(q), list(gamma)
        self.g2_powers = [pow(self.tau, t, R) for t in range(k + 1)] if g2_powers is None else list(g2_powers)
        self.n = len(self.z)
        assert len(self.y) == self.n and len(self.q) == self.n and len(self.gamma) == self.n and (len(self.com) in (1, self.n) or self.n == 0)
        assert all(len(r) == k for r in self.z) and all(len(r) == k for r in self.y) and len(self.g2_powers) == k + 1

    def copy(self):
        return Case(self.tau, self.k, self.com, self.z, self.y, self.q, self.gamma, self.g2_powers)

    def Z(self, i):
        return KM.vanishing(self.z[i])

    def I(self, i):
        return KM.interpolant(self.z[i], self.y[i])

    def rows(self):
        """the k + 1 scalar rows of the batched MSM over the proofs: rows()[t][i], row t of stride n"""
        out = [[0] * self.n for _ in range(self.k + 1)]
        for i in range(self.n):
            zc, g = self.Z(i), self.gamma[i]
            out[0][i] = (-g * zc[0]) % R
            for t in range(1, self.k + 1):
                out[t][i] = g * zc[t] % R
        return out

    def rows_flat(self):
        """row t at offset t n + i: the layout in device memory"""
        return [v for row in self.rows() for v in row]

    def J(self):
        out = [0] * self.k
        for i in range(self.n):
            g = self.gamma[i]
            for t, c in enumerate(self.I(i)):
                out[t] = (out[t] + g * c) % R
        return out

    def com_dl(self):
        """dl(sum gamma_i C_i)"""
        if self.n == 0:
            return 0
        return sum(self.gamma) * self.com[0] % R if len(self.com) == 1 else sum(g * c for g, c in zip(self.gamma, self.com)) % R

    def sums(self):
        """[dl(L), dl(R_1), .. dl(R_k)]"""
        rows = self.rows()
        dots = [sum(s * q for s, q in zip(row, self.q)) % R for row in rows]
        l = (self.com_dl() - poly_eval(self.J(), self.tau) + dots[0]) % R
        return [l] + dots[1:]

    def verdict(self):
        s = self.sums()
        return (-s[0] * self.g2_powers[0] + sum(self.g2_powers[t] * s[t] for t in range(1, self.k + 1))) % R == 0

    def single(self, i):
        """verify_multi's verdict on item i alone: c_i - I_i(tau) == q_i Z_i(tau)"""
        lhs = (self.com[0 if len(self.com) == 1 else i] - poly_eval(self.I(i), self.tau)) % R
        zt = sum(c * p for c, p in zip(self.Z(i), self.g2_powers)) % R
        return (lhs * self.g2_powers[0] - self.q[i] * zt) % R == 0


def valid_case(tau, polys, zs, gammas):
    """valid items: item i opens polys[i] (polys of ONE entry: every item opens it, one shared commitment) at the k points zs[i]"""
    n = len(zs)
    k = len(zs[0]) if n else 1
    shared = len(polys) == 1
    com, y, q = [], [], []
    for i in range(n):
        p = polys[0 if shared else i]
        y.append([poly_eval(p, z) for z in zs[i]])
        q.append(KM.set_proof_dl(p, zs[i], tau))
        if not shared or i == 0:
            com.append(poly_eval(p, tau))
    if n == 0:
        com = [poly_eval(polys[0], tau)]
    return Case(tau, k, com, zs, y, q, gammas)


def batch_sums(com, z, y, q, gamma):
    """(dl(L), dl(R)) of keaki_hip_kzg_verify_batch on n single openings: L = sum gamma C - (sum gamma y) g1 + sum (gamma z) proof, R = sum gamma proof"""
    n = len(z)
    k = sum(gamma) * com[0] % R if len(com) == 1 else sum(g * c for g, c in zip(gamma, com)) % R
    t = sum(g * v for g, v in zip(gamma, y)) % R
    m = sum(g * zz % R * qq for g, zz, qq in zip(gamma, z, q)) % R
    assert len(y) == n and len(q) == n
    return (k - t + m) % R, sum(g * qq for g, qq in zip(gamma, q)) % R
