"""Model of keaki_hip_kzg_verify_each on inputs with KNOWN discrete logs, in plain big-int arithmetic.

With C_i = c_i g1, proof_i = p_i g1 and [tau]_2 = s g2 the call forms L_i = C_i - y_i g1 + z_i proof_i = (c_i - y_i + z_i p_i) g1 and decides
e(L_i, g2) e(-proof_i, [tau]_2) == 1, i.e.

    valid_i  <=>  c_i - y_i + (z_i - s) p_i == 0  (mod r)

The identity rules of the header are this equation and nothing else: L_i and proof_i both the identity (c_i = y_i, p_i = 0) is valid; proof_i
alone (p_i = 0, c_i != y_i) leaves c_i - y_i != 0; L_i alone (c_i - y_i + z_i p_i = 0, p_i != 0) leaves -s p_i != 0 unless s = 0, and with
s = 0 ([tau]_2 the identity) the equation IS "L_i is the identity". Valid items: choose p_i, z_i freely, y_i = c_i - p_i (s - z_i).
Nothing here touches the library under test."""
import bn254_py as py

R = py.R


class Case:
    """n openings as discrete logs: s ([tau]_2), com (one entry: shared by all items, or n), z, y, p (proofs) -- integers mod r"""

    def __init__(self, s, com, z, y, p):
        self.s, self.com, self.z, self.y, self.p = s % R, [c % R for c in com], [v % R for v in z], [v % R for v in y], [v % R for v in p]
        self.n = len(self.y)
        assert len(self.z) == self.n and len(self.p) == self.n and len(self.com) in (1, self.n)

    def copy(self):
        return Case(self.s, self.com, self.z, self.y, self.p)

    def com_of(self, i):
        return self.com[0] if len(self.com) == 1 else self.com[i]

    def lhs(self):
        """discrete logs of the L_i"""
        return [(self.com_of(i) - self.y[i] + self.z[i] * self.p[i]) % R for i in range(self.n)]

    def status(self):
        """0 = valid, 1 = invalid, per item"""
        return [0 if (self.com_of(i) - self.y[i] + (self.z[i] - self.s) * self.p[i]) % R == 0 else 1 for i in range(self.n)]

    def counters(self):
        """(n_bad, first_bad or None)"""
        st = self.status()
        return sum(st), (st.index(1) if 1 in st else None)

    def head(self, n):
        return Case(self.s, self.com if len(self.com) == 1 else self.com[:n], self.z[:n], self.y[:n], self.p[:n])


def valid_case(s, com, z, p):
    """valid openings for freely chosen proofs and points: y_i = c_i - p_i (s - z_i)"""
    n = len(z)
    c = Case(s, com, z, [0] * n, p)
    c.y = [(c.com_of(i) - c.p[i] * (c.s - c.z[i])) % R for i in range(n)]
    return c


def powers(w, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * w % R
    return out
