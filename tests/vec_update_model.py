"""vec_update over Z_r: the tables, the update formulas and the pass split of keaki_amd/csrc/vec_update.hip on scalars in the exponent -- TEST
INFRASTRUCTURE (a plain module, imported by tests/test_vec_update_model.py and tests/test_gpu_vec_update.py).

A point k G is its scalar k. The tables are built from the SRS powers alone (two DFTs with root omega^-1, as the device builds them), the
reference openings by synthetic division of the coefficients, so both work for every tau: tau = 0 and tau on the domain included, where the
closed forms A(tau) / (tau - omega^i) divide by zero.
"""
import structured_inputs as S

R = S.R
UPD_K_PASS = 8                      # internal.h: UPD_K_PASS (tests/test_vec_update_model.py compares)


def omega(d):
    return S.root_of_unity(d) if d > 1 else 1


def tables(srs, d):
    """(a, u, pw, e) from srs[k] = the scalar of P_k: a_i = w^-i sum_k w^(-ik) P_k, u_i = (w^-i / d) sum_k (d-1-k) w^(-ik) P_k,
    pw_i = w^-i, e_t = 1 / (w^t - 1) (e_0 = 0, never read)"""
    wi = pow(omega(d), -1, R)
    pw = S.powers(wi, d)
    s = S.ntt([x % R for x in srs[:d]], wi)
    t = S.ntt([(d - 1 - k) * srs[k] % R for k in range(d)], wi)
    inv_d = pow(d, -1, R)
    a = [pw[i] * s[i] % R for i in range(d)]
    u = [pw[i] * inv_d % R * t[i] % R for i in range(d)]
    e = [0] + [pow(pow(omega(d), t_, R) - 1, -1, R) for t_ in range(1, d)]
    return a, u, pw, e


def passes(k, k_pass=0):
    """[(first, count)]: the pieces of a change list of k entries (vec_update.hip: upd_apply_run); k_pass = 0: the built-in size"""
    kp = k_pass if 1 <= k_pass <= UPD_K_PASS else UPD_K_PASS
    return [(lo, min(kp, k - lo)) for lo in range(0, k, kp)]


def pass_edge_ks(k_pass):
    """the list lengths at which the split changes shape: one short pass, a full pass less one, exactly one, one and a single entry, two and one"""
    return sorted({1, k_pass - 1, k_pass, k_pass + 1, 2 * k_pass + 1} - {0})


def update_pass(tab, d, com, proofs, changes):
    """one pass: every proof moves by sum_{i != j} s_tj a_i - (sum s_tj) a_j + (sum_{i = j} delta) u_j, the commitment by sum (delta c_i) a_i"""
    a, u, pw, e = tab
    inv_d = pow(d, -1, R)
    sc = [dl % R * pw[(d - i) % d] % R * inv_d % R for i, dl in changes]             # delta_t c_(i_t)
    com = (com + sum(s * a[i] for s, (i, _) in zip(sc, changes))) % R
    out = []
    for j in range(d):
        shared, ssum, dsum = 0, 0, 0
        for s, (i, dl) in zip(sc, changes):
            if i == j:
                dsum += dl
            else:
                stj = s * pw[j] % R * e[(i - j) % d] % R
                ssum += stj
                shared += stj * a[i]
        out.append((proofs[j] + shared - ssum % R * a[j] + dsum % R * u[j]) % R)
    return com, out


def update(srs, d, com, proofs, changes, k_pass=0):
    """(com', proofs') after evaluation i += delta for every (i, delta) of `changes`, pass by pass as the device runs them"""
    tab = tables(srs, d)
    for lo, cnt in passes(len(changes), k_pass):
        com, proofs = update_pass(tab, d, com, proofs, changes[lo:lo + cnt])
    return com, proofs


def coeffs_of(evals):
    d = len(evals)
    inv_d = pow(d, -1, R)
    return [c * inv_d % R for c in S.ntt([x % R for x in evals], pow(omega(d), -1, R))]


def commit_and_open(srs, evals):
    """(commitment, the d openings) of the polynomial with these evaluations, as scalars: MSMs over the SRS powers of the coefficients and of
    the quotients (p - p(w^j)) / (x - w^j) from synthetic division"""
    d = len(evals)
    p = coeffs_of(evals)
    com = sum(c * s for c, s in zip(p, srs)) % R
    out = []
    for j in range(d):
        z, acc, q = pow(omega(d), j, R), 0, 0
        for t in range(d - 1, 0, -1):
            acc = (acc * z + p[t]) % R
            q += acc * srs[t - 1]
        out.append(q % R)
    return com, out
