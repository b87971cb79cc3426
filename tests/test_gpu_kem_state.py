"""The cached tables of encapsulate and kzg verify (KemState, keaki_amd/csrc/internal.h) through the orders of calls that decide which table is
built, reused, replaced or shared: the small tables that verify and encapsulate both use, the [tau]_2 tables as the point changes, a build that
fails for lack of memory and is retried, and the memory classes the tables are counted in. Every case runs on a context of its own (the cache is
per context) and every encapsulation is compared byte for byte with the oracle's; the oracle's results are computed once for the module."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 300            # the per-item data of every case is a prefix of these items: encapsulation is item by item


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs(ints))


@pytest.fixture(scope="module")
def kem(oc, py, hip, rand_fr):
    g1, g2 = oc.generators()
    tau1, tau2, c1, c2, c0p, c1p, z = rand_fr(7, 7301)
    case = {"tau": [hip.g2_mul_batch(g2, mont(oc, [t]))[0] for t in (tau1, tau2)],
            "com": [hip.g1_mul_batch(g1, mont(oc, [c]))[0] for c in (c1, c2)],
            "items": [mont(oc, rand_fr(N, 7310 + k)) for k in range(3)]}
    A, V, R = case["items"]
    # (commitment, tau) -> the oracle's (ct, gt, key) for the first n items
    case["exp"] = {(0, 0): oc.encap_batch(case["com"][0], case["tau"][0], A, V, R, 32, threads=8),
                   (0, 1): oc.encap_batch(case["com"][0], case["tau"][1], A[:3], V[:3], R[:3], 32, threads=8),
                   (1, 0): oc.encap_batch(case["com"][1], case["tau"][0], A[:64], V[:64], R[:64], 32, threads=8)}
    # an honest opening of p(x) = c0p + c1p x under tau1, and the same with a wrong value: (com, point, value, proof, the oracle's verdict)
    G = py.G1_GEN
    com_i, proof_i = py.g1_mul(G, (c0p + c1p * tau1) % py.R), py.g1_mul(G, c1p)
    com, proof = oc.g1_from_ints([com_i])[0], oc.g1_from_ints([proof_i])[0]
    tau1_i = py.g2_mul(py.G2_GEN, tau1)
    case["openings"] = []
    for val in ((c0p + c1p * z) % py.R, (c0p + c1p * z + 1) % py.R):
        case["openings"].append((com, mont(oc, [z])[0], mont(oc, [val])[0], proof, py.kzg_verify(tau1_i, com_i, z, val, proof_i)))
    assert [o[4] for o in case["openings"]] == [True, False]
    return case


def check_encap(h, kem, ci, ti, n, what):
    A, V, R = kem["items"]
    got = h.encap_batch(kem["com"][ci], kem["tau"][ti], A[:n], V[:n], R[:n], 32)
    for g, e, name in zip(got, kem["exp"][ci, ti], ("ct", "gt", "key")):
        assert np.array_equal(g, e[:n]), "%s: %s differs from the oracle's" % (what, name)


def check_verify(h, kem, what):
    for com, z, val, proof, verdict in kem["openings"]:
        assert h.kzg_verify(com, kem["tau"][0], z, val, proof) is verdict, "%s: opening the oracle judges %s" % (what, verdict)


@pytest.mark.parametrize("verify_first", [True, False])
def test_small_tables_shared_by_verify_and_encap(kem, verify_first):
    """The 8-bit table of g2 is built by whichever of kzg verify and a small encapsulation comes first and used by both; after trim() both build
    their tables again."""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        for rnd in ("fresh", "after trim"):
            if verify_first:
                check_verify(h, kem, rnd)
            check_encap(h, kem, 0, 0, 3, rnd)
            if not verify_first:
                check_verify(h, kem, rnd)
            h.trim()
    finally:
        h.close()


def test_tau_tables_follow_the_point(kem):
    """The table of [tau]_2 is keyed by the point. Three items use the small table: built for tau1, replaced for tau2, rebuilt for tau1. 256 items
    (the smallest batch that builds the 16-bit tables) put tau1 into the big table, which three items with tau1 then use, while three items with
    tau2 go back to the small one."""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        for step, (ti, n) in enumerate([(0, 3), (1, 3), (0, 3), (0, 256), (0, 3), (1, 3)]):
            check_encap(h, kem, 0, ti, n, "step %d (tau%d, n = %d)" % (step, ti + 1, n))
    finally:
        h.close()


def test_encap_recovers_after_a_failed_table_build(kem):
    """The 16-bit table of B (201 MB) is refused: the call fails with KEAKI_ERR_OOM and leaves no table marked ready. With the limit lifted the same
    call builds everything and is right, and so is a second commitment behind it."""
    from keaki_amd.hip import KeakiHip, KeakiHipError
    h = KeakiHip(0)
    try:
        h.set_option("encap_gt", 64)
        h.debug_set_alloc_limit(128 << 20)
        with pytest.raises(KeakiHipError) as e:
            check_encap(h, kem, 0, 0, 64, "under the limit")
        assert e.value.status == -3, e.value
        h.debug_set_alloc_limit(0)
        check_encap(h, kem, 0, 0, 64, "limit lifted")
        check_encap(h, kem, 1, 0, 64, "second commitment")
    finally:
        h.close()


def test_memory_classes_of_the_kem_tables(kem):
    """One encapsulation of 300 items and one verify leave tables in both classes of keaki_hip_ctx_memory (the line tables and verify's block count as
    workspaces, the fixed-base and GT tables as gt_tables); trim() releases all of them; `total` is the sum of the three classes."""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        check_encap(h, kem, 0, 0, N, "n = %d" % N)
        check_verify(h, kem, "after the batch")
        mem = h.memory()
        print("memory after encap(%d) + verify: %s" % (N, mem))
        assert mem["gt_tables"] > 0 and mem["workspaces"] > 0, mem
        assert mem["total"] == mem["tables"] + mem["workspaces"] + mem["gt_tables"], mem
        h.trim()
        mem = h.memory()
        assert mem["gt_tables"] == 0 and mem["workspaces"] == 0 and mem["total"] == mem["tables"], mem
    finally:
        h.close()
