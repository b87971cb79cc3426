"""The fixed-base window tables of the KEM at their digit boundaries: encap_batch and kzg_verify on scalars that put every non-top window
of every table they walk through each branch of the signed-digit recoding (tests/structured_inputs.py: fb_edge_scalars -- +-1, +half,
+-(half - 1), a level boundary of the table fill, the zero of an all-ones window under a carry, a plain zero, and carry chains).

The bases have known discrete logs (com = c g1, [tau]_2 = tau g2), so one item carries three chosen scalars: r walks the tables of
[tau]_2 and of the commitment (or A = e(C, g2)); point = -t2 / r and value = -t1 / r make the device's -(r point) and -(r value) the
chosen scalars for the tables of g2 and of g1 (or B = e(g1, g2)). Expected values come from the oracle's scalar multiplications, pairing
and BLAKE3, never from the library; everything is bit for bit. tests/variant_cases.py lists the cases (fb_edge_runs) with the kernels
each one reaches. Every case runs on a private context: a new context holds no table, so every base is new to it, and the session
context's options and tables stay untouched."""
import os

import numpy as np
import pytest

import structured_inputs as S
import variant_cases as V
from test_gpu_parity import mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(32, os.cpu_count() or 1)
RUNS = {name: (n, wide, new, gt) for name, n, wide, new, gt in V.fb_edge_runs()}
# the widths each run walks: (r over the tables of [tau]_2 and of A or the commitment, -(r point) over g2's, -(r value) over B's or g1's)
WALKS = {
    "small": ((8, 13), (8,), (16,)), "repeat": ((8, 16), (8,), (16,)),
    "wide16": ((16, 13), (16,), (16,)),
    "lane": ((16, 13), (16,), (16,)), "lane_repeat": ((16, 16), (16,), (16,)),
    "split": ((16, 13), (16,), (16,)), "split_repeat": ((16, 16), (16,), (16,)),
    "pairing": ((16, 13), (16,), (16,)),
}
for _wb in V.FB_EDGE_B_WIDTHS:
    WALKS["b_width[%d,wide]" % _wb] = ((8, 13), (8,), (_wb,))
    WALKS["b_width[%d,lane]" % _wb] = ((8, 16), (8,), (_wb,))


def g1_of(oc, ks):
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, [k % R for k in ks]), threads=TH)


def g2_of(oc, ks):
    return oc.g2_mul_batch(oc.generators()[1], mont(oc, [k % R for k in ks]), threads=TH)


class Batch:
    """the unique items of one B-side width set, the item r = 0 behind them, and what the oracle expects of each"""

    def __init__(self, oc, b1_widths):
        from conftest import rand_fr_ints
        self.tau, self.c, z0, v0 = rand_fr_ints(4, 9400)
        tau, c = self.tau, self.c
        self.com, self.tg2 = g1_of(oc, [c])[0], g2_of(oc, [tau])[0]
        edge = S.fb_edge_batch(V.FB_EDGE_R_WIDTHS, V.FB_EDGE_B2_WIDTHS, b1_widths)
        self.sides = S.fb_edge_sides(edge)
        # a random tau and c meet nothing, in either order of the additions: a failure below points at the digits, not at the addition formulas
        for r, z, v in edge:
            for wb, wide in ((8, True), (8, False), (16, True), (16, False)):
                dlog, ev = S.encap_ct_events(tau, r, z, wb, wide)
                assert dlog == r * (tau - z) % R and ev == {"equal": 0, "opposite": 0}, (r, wb, wide, ev)
            dlog, ev = S.fb_sum_events(c, r, 13, 1, -(r * v) % R, 16, False)
            assert dlog == r * (c - v) % R and ev == {"equal": 0, "opposite": 0}, (r, ev)
        items = edge + [(0, z0, v0)]
        self.n = len(items)
        self.zs, self.vs, self.rs = (mont(oc, [it[k] for it in items]) for k in (1, 2, 0))
        self.ct = g2_of(oc, [r * (tau - z) for r, z, v in items])
        self.gt = oc.pairing_batch(g1_of(oc, [r * (c - v) for r, z, v in items]), oc.generators()[1], threads=TH)
        self.key = np.stack([np.frombuffer(oc.blake3_xof(self.gt[i].tobytes(), 32), np.uint8) for i in range(self.n)])
        ect, egt, ekey = oc.encap_batch(self.com, self.tg2, self.zs[-1:], self.vs[-1:], self.rs[-1:], 32, threads=TH)
        self.ct[-1], self.gt[-1], self.key[-1] = ect[0], egt[0], ekey[0]              # r = 0: the oracle's own encapsulation
        ect, egt, ekey = oc.encap_batch(self.com, self.tg2, self.zs[:8], self.vs[:8], self.rs[:8], 32, threads=TH)
        assert np.array_equal(self.ct[:8], ect) and np.array_equal(self.gt[:8], egt) and np.array_equal(self.key[:8], ekey)

    def covers(self, walks):
        """the condition of every case: each side reaches every (non-top window, class) pair of every width it walks"""
        for side, widths in zip(self.sides, walks):
            for wb in widths:
                missing = S.fb_edge_required(wb) - S.fb_edge_covered(side, wb)
                assert not missing, (wb, sorted(missing))


@pytest.fixture(scope="module")
def batches(oc):
    made = {}

    def get(b1_widths=V.FB_EDGE_B1_WIDTHS):
        if b1_widths not in made:
            made[b1_widths] = Batch(oc, b1_widths)
        return made[b1_widths]
    return get


@pytest.fixture()
def fresh():
    """contexts of the test's own, closed afterwards"""
    from keaki_amd.hip import KeakiHip
    made = []

    def new(**opts):
        h = KeakiHip(0)
        made.append(h)
        for k, v in opts.items():
            h.set_option(k, v)
        return h
    yield new
    for h in made:
        h.close()


def run(h, b, name):
    """one encap_batch of the case's size (the unique items, tiled where the case needs more) against every unique item's expectation"""
    n, wide, new, gt = RUNS[name]
    b.covers(WALKS[name])
    assert n >= b.n and (n == b.n or n >= V.FB_TABLES_MIN), (name, n, b.n)
    h.set_option("pair_wide_max", wide)
    idx = np.arange(n) % b.n
    ct, gtb, key = h.encap_batch(b.com, b.tg2, b.zs[idx], b.vs[idx], b.rs[idx], 32)
    for what, got, exp in (("ct", ct, b.ct), ("gt", gtb, b.gt), ("key", key, b.key)):
        bad = np.flatnonzero((got != exp[idx]).reshape(n, -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs in %d of %d items, first at item %d (unique item %d)" % (name, what, bad.size, n, bad[0], idx[bad[0]])


def test_small_batch_8_bit_tables_then_the_same_call_again(batches, fresh):
    """< 256 items on a new context: the 8-bit tables of [tau]_2 and g2 in k_encap_fixed_g2_wide, A at 13 and B at 16 bits in
    k_gt_encap_exp_wide; the same call again widens A to 16 bits from the powers of the first build"""
    h, b = fresh(), batches()
    assert RUNS["small"][0] == b.n < V.FB_TABLES_MIN
    run(h, b, "small")
    run(h, b, "repeat")


def test_wide_kernels_over_16_bit_tables(batches, fresh):
    """256 <= n <= 2048: the 16-bit tables of [tau]_2 and g2, sixteen lanes per ciphertext and twelve per GT value"""
    run(fresh(), batches(), "wide16")


def test_one_lane_per_item_over_16_bit_tables(batches, fresh):
    """pair_wide_max = 0: k_encap_fixed<Fq2,2> beside the build of A's table, then <Fq2,1>; k_gt_encap_exp with both tables in one
    launch, A at 13 and then at 16 bits"""
    h, b = fresh(), batches()
    run(h, b, "lane")
    run(h, b, "lane_repeat")


def test_new_commitment_above_4096_items_splits_the_exponentiation(batches, fresh):
    """B's factor first into the accumulator (acc_out), A's factor behind it (acc_in) once its table is built; then the same
    commitment again in one launch"""
    h, b = fresh(), batches()
    run(h, b, "split")
    run(h, b, "split_repeat")


def test_per_item_pairing_path_over_the_g1_tables(batches, fresh):
    """encap_gt = 2^40: r over the 13-bit table of the commitment and -(r value) over the 16-bit table of g1 in k_encap_fixed<Fq,1>"""
    run(fresh(encap_gt=1 << 40), batches(), "pairing")


@pytest.mark.parametrize("wb", V.FB_EDGE_B_WIDTHS)
def test_every_width_of_the_table_of_b(batches, fresh, wb):
    """gt_wb_b = wb on a new context (a forced width is never rebuilt wider), the B-side scalars drawn from fb_edge_scalars(wb): twelve
    lanes per item with A at 13 bits, then two lanes per item with A at 16"""
    h, b = fresh(gt_wb_b=wb), batches((wb,))
    run(h, b, "b_width[%d,wide]" % wb)
    run(h, b, "b_width[%d,lane]" % wb)


def test_kzg_verify_over_the_8_bit_tables(oc, py, fresh, batches):
    """k_verify_points, sixteen lanes per sum: honest openings of p(x) = c0 + c1 x whose -z and -value run through fb_edge_scalars(8)
    verify; value + 1 and z + 1 do not; the pure-Python verifier agrees on the same integers"""
    from conftest import rand_fr_ints
    h = fresh()
    tau, c1 = batches().tau, rand_fr_ints(1, 9401)[0]
    tg2 = batches().tg2
    tg2_i = py.g2_mul(py.G2_GEN, tau)
    edge = S.fb_edge_scalars(8)
    zs = [(R - e) % R for e in edge]
    vals = [(R - edge[(i + 1) % len(edge)]) % R for i in range(len(edge))]
    for side in ([-z % R for z in zs], [-v % R for v in vals]):
        assert S.fb_edge_covered(side, 8) == S.fb_edge_required(8)
    c0s = [(v - c1 * z) % R for z, v in zip(zs, vals)]
    coms = g1_of(oc, [c0 + c1 * tau for c0 in c0s])
    proof = g1_of(oc, [c1])[0]
    coms_i, proof_i = oc.g1_to_ints(coms), oc.g1_to_ints(proof[None])[0]
    for i, (z, v) in enumerate(zip(zs, vals)):
        for dz, dv, verdict in ((0, 0, True), (0, 1, False), (1, 0, False)):
            zz, vv = (z + dz) % R, (v + dv) % R
            assert h.kzg_verify(coms[i], tg2, mont(oc, [zz])[0], mont(oc, [vv])[0], proof) is verdict, (i, dz, dv)
            assert py.kzg_verify(tg2_i, coms_i[i], zz, vv, proof_i) is verdict, (i, dz, dv)
