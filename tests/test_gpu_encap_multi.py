"""encap_multi / encrypt_multi through the C ABI (keaki_hip_encap_multi*, keaki_hip_encrypt_multi*): a commitment per GROUP of items. For every
group the ct, gt, key and body bytes are those of encap_batch / encrypt_batch for (its commitment, its items) alone: against the CPU oracle
per group, against m separate calls, on both routes (fused per-item pairing | single-commitment GT tables), with small and long fixed-base
tables, on commitments with known discrete logs that drive the final addition of the G1 kernel into its identity, equal-point and
opposite-point cases, across the chunks of the host pipeline, device-resident, and end to end with the batched receiver side."""
import ctypes as C
import os

import numpy as np
import pytest

import structured_inputs as S
from conftest_helpers import rand_fr_ints
from test_gpu_parity import jac_to_aff, mont

pytestmark = pytest.mark.gpu
R = S.R
TH = min(16, os.cpu_count() or 1)
ERR_BAD_ARG = -1
GT_ONE = bytes([1] + [0] * 383)           # serialize_uncompressed(Fq12::one)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


@pytest.fixture(scope="module")
def setup(oc):
    """[tau]_2 of a random tau and 70 unrelated commitments (oracle arithmetic: inputs, not results)"""
    g1, g2 = oc.generators()
    tau = rand_fr_ints(1, 7001)[0]
    return {"tau": tau, "tau_g2": oc.g2_mul_batch(g2, mont(oc, [tau]), threads=TH)[0],
            "coms": oc.g1_mul_batch(g1, mont(oc, rand_fr_ints(70, 7002)), threads=TH)}


def items(oc, n, seed):
    """(points, values, r) of n items, Montgomery"""
    x = mont(oc, rand_fr_ints(3 * n, seed))
    return x[:n], x[n:2 * n], x[2 * n:]


@pytest.fixture()
def own_ctx():
    """a context of its own: no table exists yet, so calls below 256 items run on the SMALL fixed-base tables"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    try:
        yield h
    finally:
        h.close()


def oracle_groups(oc, coms, sizes, tau_g2, a, v, r, msg_len=32):
    off = offsets_of(sizes)
    parts = [oc.encap_batch(coms[j], tau_g2, a[int(off[j]):int(off[j + 1])], v[int(off[j]):int(off[j + 1])], r[int(off[j]):int(off[j + 1])], msg_len, threads=TH)
             for j in range(len(sizes)) if sizes[j]]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def separate_calls(h, coms, sizes, tau_g2, a, v, r, msg_len=32):
    off = offsets_of(sizes)
    parts = [h.encap_batch(coms[j], tau_g2, a[int(off[j]):int(off[j + 1])], v[int(off[j]):int(off[j + 1])], r[int(off[j]):int(off[j + 1])], msg_len)
             for j in range(len(sizes)) if sizes[j]]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def same(got, exp):
    return all(np.array_equal(g, e) for g, e in zip(got, exp))


def test_group_edges_on_small_tables(oc, own_ctx, setup):
    """n = 193 < 256: a group edge inside a wave (item 1, 63, 64), one exactly on a wave edge (128), empty groups first, last and in a row"""
    sizes = [0, 1, 0, 0, 62, 1, 64, 65, 0]
    n = sum(sizes)
    assert n == 193
    a, v, r = items(oc, n, 7100)
    coms = setup["coms"][:len(sizes)]
    got = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    assert same(got, oracle_groups(oc, coms, sizes, setup["tau_g2"], a, v, r)), "against the oracle, group by group"
    assert same(got, separate_calls(own_ctx, coms, sizes, setup["tau_g2"], a, v, r)), "against m calls of encap_batch"


def test_long_tables(oc, own_ctx, setup):
    sizes = [100, 0, 156, 47]
    n = sum(sizes)
    assert n == 303
    a, v, r = items(oc, n, 7200)
    coms = setup["coms"][10:14]
    got = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    assert same(got, oracle_groups(oc, coms, sizes, setup["tau_g2"], a, v, r))
    assert same(got, separate_calls(own_ctx, coms, sizes, setup["tau_g2"], a, v, r))
    ct, key = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32, want_gt=False)
    assert np.array_equal(ct, got[0]) and np.array_equal(key, got[2]), "key_out only (gt_out NULL)"


@pytest.mark.parametrize("tables", ["small", "long"])
def test_known_discrete_logs(oc, own_ctx, setup, tables):
    """C = c g1 against one value beta: c = 0 (the identity point), 1, beta (r C and -(r beta) g1 are opposite: GT one), r - beta (they are EQUAL:
    the addition must double), 2 beta; r_i = 0 (both terms the identity), 1, r - 1, random. gt = e((r_i (c - beta)) g1, g2) from the oracle."""
    g1, g2 = oc.generators()
    beta = rand_fr_ints(1, 7300)[0]
    cs = [0, 1, beta, R - beta, 2 * beta % R]
    rs = [0, 1, R - 1, rand_fr_ints(1, 7301)[0]]
    coms = oc.g1_mul_batch(g1, mont(oc, cs), threads=TH)
    assert not coms[0].any(), "c = 0 is the identity point (0, 0)"
    sizes = [len(rs)] * len(cs)
    n = sum(sizes)
    a = mont(oc, rand_fr_ints(n, 7302))
    v = mont(oc, [beta] * n)
    r = mont(oc, rs * len(cs))
    if tables == "long":
        own_ctx.encap_prepare(setup["tau_g2"], 256)
    ct, gt, key = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    logs = [ri * (c - beta) % R for c in cs for ri in rs]
    exp_gt = oc.pairing_batch(oc.g1_mul_batch(g1, mont(oc, logs), threads=TH), g2, threads=TH)
    assert logs.count(0) == len(cs) + len(rs) - 1
    for i, k in enumerate(logs):
        assert gt[i].tobytes() == exp_gt[i].tobytes(), (i, i // len(rs), i % len(rs))
        assert (gt[i].tobytes() == GT_ONE) == (k == 0), i
        assert key[i].tobytes() == oc.blake3_xof(exp_gt[i].tobytes(), 32), i
    assert np.array_equal(ct, oracle_groups(oc, coms, sizes, setup["tau_g2"], a, v, r)[0])


def test_same_commitment_in_several_groups(oc, own_ctx, setup):
    sizes = [5, 9, 0, 7]
    n = sum(sizes)
    a, v, r = items(oc, n, 7400)
    c = setup["coms"]
    two = np.stack([c[20], c[21], c[22], c[20]])                       # groups 0 and 3 hold the same point
    assert same(own_ctx.encap_multi(two, offsets_of(sizes), setup["tau_g2"], a, v, r, 32), oracle_groups(oc, two, sizes, setup["tau_g2"], a, v, r))
    allsame = np.stack([c[20]] * 4)
    got = own_ctx.encap_multi(allsame, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    assert same(got, own_ctx.encap_batch(c[20], setup["tau_g2"], a, v, r, 32)), "one encap_batch over all items"
    assert same(got, oc.encap_batch(c[20], setup["tau_g2"], a, v, r, 32, threads=TH))


def test_routes_give_the_same_bytes(oc, own_ctx, setup):
    """threshold 64: groups of 64, 65 and 200 items take the single-commitment path (GT tables), 63 and 1 the fused route; threshold 0: all fused"""
    sizes = [63, 64, 65, 1, 200]
    n = sum(sizes)
    a, v, r = items(oc, n, 7500)
    coms = setup["coms"][30:35]
    exp = oracle_groups(oc, coms, sizes, setup["tau_g2"], a, v, r)
    own_ctx.set_option("encap_multi_single_min", 64)
    mixed = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    own_ctx.set_option("encap_multi_single_min", 0)
    fused = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 32)
    assert same(mixed, fused) and same(mixed, exp)
    # the cache of the single-commitment path survives a mixed call: the first commitment again, then a fresh one
    for j in (30, 40):
        got = own_ctx.encap_batch(setup["coms"][j], setup["tau_g2"], a[:9], v[:9], r[:9], 32)
        assert same(got, oc.encap_batch(setup["coms"][j], setup["tau_g2"], a[:9], v[:9], r[:9], 32, threads=TH)), j


def test_end_to_end_with_the_batched_receiver_side(oc, hip, own_ctx):
    """six receivers commit to 7 bits each (vec_commit_batch, d = 8); the sender encrypts two messages per position, under value 0 and under
    value 1, in ONE encrypt_multi; every receiver's proofs decrypt the message of its bit and not the other one"""
    g1, g2 = oc.generators()
    log2d, d, m, k, ml = 3, 8, 6, 7, 33
    tau = rand_fr_ints(1, 7600)[0]
    srs = hip.srs_g1_upload(oc.g1_mul_batch(g1, mont(oc, S.powers(tau, 16)), threads=TH))
    try:
        tau_g2 = oc.g2_mul_batch(g2, mont(oc, [tau]), threads=TH)[0]
        w2 = S.root_of_unity(2 * d)
        w = w2 * w2 % R
        consts = [mont(oc, [x])[0] for x in (pow(w, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]
        bits = [[(j * 5 + i * 3 + (i * j) // 2) % 2 for i in range(k)] for j in range(m)]
        pad = rand_fr_ints(m, 7601)
        rows = mont(oc, sum([bits[j] + [pad[j]] for j in range(m)], [])).reshape(m, d, 4)
        com_jac, proofs = hip.vec_commit_batch(srs, rows, log2d, *consts)
        coms = np.stack([jac_to_aff(c) for c in com_jac])          # one normalised Jacobian point at a time
        assert all(oc.g1_on_curve(c) for c in coms)
    finally:
        srs.free()
    # item (j, i, b): position omega^i, value b
    n = m * k * 2
    points = mont(oc, [pow(w, i, R) for j in range(m) for i in range(k) for b in (0, 1)])
    values = mont(oc, [b for j in range(m) for i in range(k) for b in (0, 1)])
    r = mont(oc, rand_fr_ints(n, 7602))
    msgs = np.frombuffer(np.random.default_rng(7603).bytes(n * ml), np.uint8).reshape(n, ml)
    ct, body = own_ctx.encrypt_multi(coms, offsets_of([2 * k] * m), tau_g2, points, values, r, msgs)
    exp = oracle_groups(oc, coms, [2 * k] * m, tau_g2, points, values, r, ml)
    assert np.array_equal(ct, exp[0]) and np.array_equal(body, msgs ^ exp[2]), "bodies = message XOR the oracle's key"
    pr = np.repeat(proofs[:, :k].reshape(m * k, 8), 2, axis=0)           # the receiver's proof at its position, for both items of the position
    out = hip.decrypt_batch(pr, ct, body)
    chosen = np.array([b == bits[j][i] for j in range(m) for i in range(k) for b in (0, 1)])
    assert np.array_equal(out[chosen], msgs[chosen]), "the message of the receiver's bit"
    assert not (out[~chosen] == msgs[~chosen]).all(axis=1).any(), "never the other one"


def dev(a):
    import torch
    a = np.array(a)                      # a writable copy
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def encap_multi_on_device(h, coms, sizes, tau_g2, a, v, r, msg_len, msgs=None):
    """the _dev forms on torch buffers -> (ct, gt, key) or, with msgs, (ct, body) computed in place"""
    import torch
    n = a.shape[0]
    d_in = [dev(x) for x in (coms, tau_g2, a, v, r)]
    d_ct = torch.full((n, 16), -1, dtype=torch.int64, device="cuda:0")
    if msgs is None:
        d_gt = torch.full((n, 384), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_key = torch.full((n, msg_len), 0xEE, dtype=torch.uint8, device="cuda:0")
    else:
        d_body = dev(msgs)
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in d_in]
    if msgs is None:
        h.encap_multi_dev(p[0], offsets_of(sizes), p[1], p[2], p[3], p[4], n, d_ct.data_ptr(), d_gt.data_ptr(), d_key.data_ptr(), msg_len)
    else:
        h.encrypt_multi_dev(p[0], offsets_of(sizes), p[1], p[2], p[3], p[4], n, d_ct.data_ptr(), d_body.data_ptr(), msg_len)
    h.synchronize()
    ct = d_ct.cpu().numpy().view(np.uint64)
    return (ct, d_gt.cpu().numpy(), d_key.cpu().numpy()) if msgs is None else (ct, d_body.cpu().numpy())


def test_chunk_pipeline_of_the_host_form(oc, hip, setup):
    """n = 65,536 + 77 in groups of 1,000: the host form runs in chunks of 32,768 items, so groups 32 and 65 straddle a chunk boundary.
    Every item: host form == _dev form (one launch over all items). 64 items against the oracle, the first and last item of both
    straddling groups among them (the oracle takes milliseconds per item: 65,549 items go without it). Run alone, most of this test's time
    is PyTorch's first initialisation of the device for the resident buffers (about 10 s); inside the suite it takes under 5 s."""
    n = 65536 + 77
    sizes = [1000] * 65 + [613]
    assert sum(sizes) == n
    # Montgomery limbs straight from a generator: any value below r is one, and 2^252 is below r
    a, v, r = (np.random.default_rng(7700 + t).integers(0, 1 << 64, (n, 4), dtype=np.uint64) for t in range(3))
    for x in (a, v, r):
        x[:, 3] &= np.uint64((1 << 60) - 1)
    coms = setup["coms"][:len(sizes)]
    off = offsets_of(sizes)
    host = hip.encap_multi(coms, off, setup["tau_g2"], a, v, r, 32)
    devf = encap_multi_on_device(hip, coms, sizes, setup["tau_g2"], a, v, r, 32)
    for name, h_, d_ in zip(("ct", "gt", "key"), host, devf):
        assert np.array_equal(h_, d_), name
    sample = sorted({32000, 32767, 32768, 32999, 65000, 65535, 65536, n - 1, 0, 999, 1000} | {int(i) for i in np.random.default_rng(7701).integers(0, n, 53)})
    assert 60 <= len(sample) <= 64
    for i in sample:
        j = int(np.searchsorted(off, i, side="right")) - 1
        e = oc.encap_batch(coms[j], setup["tau_g2"], a[i:i + 1], v[i:i + 1], r[i:i + 1], 32)
        assert all(np.array_equal(h_[i:i + 1], e_) for h_, e_ in zip(host, e)), (i, j)


def test_dev_forms(oc, own_ctx, setup):
    sizes = [0, 1, 0, 0, 62, 1, 64, 65, 0]
    n = sum(sizes)
    a, v, r = items(oc, n, 7800)
    coms = setup["coms"][:len(sizes)]
    host = own_ctx.encap_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, 48)
    assert same(encap_multi_on_device(own_ctx, coms, sizes, setup["tau_g2"], a, v, r, 48), host)
    msgs = np.frombuffer(np.random.default_rng(7801).bytes(n * 48), np.uint8).reshape(n, 48)
    ct, body = encap_multi_on_device(own_ctx, coms, sizes, setup["tau_g2"], a, v, r, 48, msgs=msgs)
    assert np.array_equal(ct, host[0]) and np.array_equal(body, msgs ^ host[2]), "d_body_inout: messages in, bodies out"
    hct, hbody = own_ctx.encrypt_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, msgs)
    assert np.array_equal(hct, ct) and np.array_equal(hbody, body)
    both = msgs.copy()
    own_ctx.encrypt_multi(coms, offsets_of(sizes), setup["tau_g2"], a, v, r, both, in_place=True)
    assert np.array_equal(both, body), "the host form with the message array as its output"


def test_errors_and_empty_calls(oc, own_ctx, setup):
    h, lib = own_ctx, own_ctx.lib
    sizes = [3, 0, 5]
    n = 8
    a, v, r = items(oc, n, 7900)
    coms, tau = np.ascontiguousarray(setup["coms"][:3]), setup["tau_g2"]
    msgs = np.full((n, 16), 0x5A, np.uint8)
    ct, gt, key, body = np.full((n, 16), 7, np.uint64), np.full((n, 384), 7, np.uint8), np.full((n, 16), 7, np.uint8), np.full((n, 16), 7, np.uint8)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    err = lambda: lib.keaki_hip_last_error(h.ctx).decode()
    good = offsets_of(sizes)

    def encap(fn, c=coms, o=good, m=3, t=tau, pa=a, pv=v, pr=r, n_=n, ct_=ct, gt_=gt, key_=key, ml=16):
        return fn(h.ctx, p(c), p(o), m, p(t), p(pa), p(pv), p(pr), n_, p(ct_), p(gt_), p(key_), ml)

    def encrypt(fn, host, c=coms, o=good, m=3, t=tau, pa=a, pv=v, pr=r, ms=msgs, n_=n, ct_=ct, body_=body, ml=16):
        if host:
            return fn(h.ctx, p(c), p(o), m, p(t), p(pa), p(pv), p(pr), p(ms), n_, p(ct_), p(body_), ml)
        return fn(h.ctx, p(c), p(o), m, p(t), p(pa), p(pv), p(pr), n_, p(ct_), p(body_), ml)

    u = lambda *w: np.array(w, np.uint64)
    bad_offsets = [dict(o=None), dict(o=u(1, 3, 3, 8)), dict(o=u(0, 5, 3, 8)), dict(o=u(0, 3, 3, 7)), dict(o=u(0, 3, 3, 9)), dict(m=2), dict(o=u(0, 1 << 31), m=1, n_=1 << 31),
                   dict(o=u(0), m=0)]
    nulls = [dict(c=None), dict(t=None), dict(pa=None), dict(pv=None), dict(pr=None), dict(ct_=None)]
    # every pointer of the _dev forms is only checked, never followed, in a refused call: host arrays stand in for device memory
    for fn in (lib.keaki_hip_encap_multi, lib.keaki_hip_encap_multi_dev):
        for bad in bad_offsets + nulls + [dict(gt_=None, key_=None), dict(ml=65537)]:
            assert encap(fn, **bad) == ERR_BAD_ARG and "encap_multi" in err(), bad
        assert encap(fn, o=u(0), m=0, n_=0) == 0 and encap(fn, n_=0) == 0, "n = 0 writes nothing"
    for fn, host in ((lib.keaki_hip_encrypt_multi, True), (lib.keaki_hip_encrypt_multi_dev, False)):
        for bad in bad_offsets + nulls + [dict(body_=None), dict(ml=0), dict(ml=65537)] + ([dict(ms=None)] if host else []):
            assert encrypt(fn, host, **bad) == ERR_BAD_ARG and "encrypt_multi" in err(), bad
        assert encrypt(fn, host, o=u(0), m=0, n_=0) == 0
    assert (ct == 7).all() and (gt == 7).all() and (key == 7).all() and (body == 7).all(), "a refused call writes nothing"
    # the context works afterwards
    got = h.encap_multi(coms, good, tau, a, v, r, 16)
    assert same(got, oracle_groups(oc, coms, sizes, tau, a, v, r, 16))


def test_host_mirror_vec_encrypt_batch(oc):
    """keaki::vec::vec_encrypt_batch of the C++ mirror: one r per item in global index order, so an identically seeded Rng gives what five
    vec_encrypt calls give, in points and in bodies"""
    import keaki_amd.keaki as K
    g1, _ = oc.generators()
    counts = [3, 0, 8, 1, 4]
    n, ml = sum(counts), 21
    d = K.Device(0)
    st = K.KZGSetup.setup(mont(oc, [S.secrets()["random"]])[0], 8, device=d)
    try:
        coms = oc.g1_mul_batch(g1, mont(oc, rand_fr_ints(len(counts), 8000)), threads=TH)
        a, v, _ = items(oc, n, 8001)
        msgs = np.frombuffer(np.random.default_rng(8002).bytes(n * ml), np.uint8).reshape(n, ml)
        g2, body = K.vec_encrypt_batch(K.Rng(23), st, coms, counts, a, v, msgs)
        rng, lo = K.Rng(23), 0
        for j, c in enumerate(counts):
            e_g2, e_body = K.vec_encrypt_arrays(rng, st, coms[j], a[lo:lo + c], v[lo:lo + c], msgs[lo:lo + c]) if c else (g2[:0], body[:0])
            assert np.array_equal(g2[lo:lo + c], e_g2) and np.array_equal(body[lo:lo + c], e_body), j
            lo += c
    finally:
        st.close()
        d.close()
