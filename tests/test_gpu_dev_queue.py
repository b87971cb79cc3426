"""The *_dev entry points as QUEUED work (include/keaki_hip.h: "enqueue on the ctx stream without synchronising"), on the three kinds of
stream a context can run on. Every other GPU test queues one call, synchronises and compares; here several calls of changing size lie
on the stream at once, so the state BETWEEN calls is what is tested:

 - the grow-only workspaces (a larger call goes through `reserve`, which drains the stream and frees the buffer earlier calls were using;
   smaller calls then run in buffers larger than they need; G1 and G2 share `buckets` / `partials` with different element sizes),
 - the encapsulation policy through the _dev branch (commitment read back from the device, cached / promoted / rebuilt GT tables, the
   build of a new commitment's table on the aux stream under queued readers),
 - stream order of inputs and outputs (a producer kernel in front of a call, the input overwritten right behind it),
 - the instrumentation and keaki_hip_ctx_trim after a queue.

One host synchronisation at the end of a queue, then EVERY output against the oracle, bit for bit. Device buffers are torch tensors."""
import os

import numpy as np
import pytest

import variant_cases as V

pytestmark = pytest.mark.gpu
TH = min(16, os.cpu_count() or 1)            # threads of the oracle: a test run is given 16 CPUs, whatever the machine has
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

G1_SIZES = [33, 4096, 257, 70000, 1, 5000, 70000, 0]           # the jump to 70000 grows every MSM workspace behind queued work
G2_SIZES = [33, 1000, 1, 4096]
MIX = [("g1", 4096), ("g2", 1000), ("g1", 257), ("g2", 33)]
MUL_SIZES = [1, 65, 300, 64]
PAIR_SIZES = [1, 3, 130, 64]
DECAP_CALLS = [(134, 64, 65), (4, 130, 32), (1, 3, 65)]        # (first item, items, msg_len): grows tmp_b behind a queued reader, then a short call in it
ENCAP_STEPS = [(1, 255), (1, 256), (2, 300), (1, 1), (2, 4097), (2, 64)]      # (commitment, n): see test_encap_policy_queue
STREAM_FORMS = ["private", "legacy", "torch"]


def _mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([int(v) % R for v in ints]))


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _fill(shape, dtype):
    """an output tensor that holds no valid answer (all bits set): what a call does not write stays visible"""
    import torch
    return torch.full(shape, -1 if dtype == "i64" else 255, dtype=torch.int64 if dtype == "i64" else torch.uint8, device="cuda:0")


def _aff_rows(jac):
    from keaki_amd.hip import jac_to_affine_words
    return np.stack([jac_to_affine_words(row) for row in jac])


def _jac_identity(words):
    """(R, R, 0): the normalised Jacobian identity of the ABI"""
    from bench import mont_words
    one = mont_words(1)
    return np.array(one + one + [0] * 4 if words == 12 else (one + [0] * 4) * 2 + [0] * 8, np.uint64)


def _scalars(n, seed):
    """n Fr (any canonical residue is a valid Montgomery form) with a zero and r - 1 mixed in"""
    from bench import random_fr_limbs
    s = random_fr_limbs(n, seed)
    if n > 2:
        s[1] = 0
        s[n // 2] = np.frombuffer(int(R - 1).to_bytes(32, "little"), np.uint64)
    return s


def _new_ctx(stream=None):
    from keaki_amd.hip import KeakiHip
    return KeakiHip(0, stream=stream)


# ---- 1. queued calls of changing size ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def msm_case(oc):
    """the bases (the oracle's scalar multiples of the generators: nothing here comes from the library), one scalar vector per queued call
    and the oracle's result of every call"""
    from bench import random_fr_limbs
    g1, g2 = oc.generators()
    p1 = oc.g1_mul_batch(g1, random_fr_limbs(max(G1_SIZES), 0xD0E1), threads=TH)
    p2 = oc.g2_mul_batch(g2, random_fr_limbs(max(G2_SIZES), 0xD0E2), threads=TH)
    p1[3] = 0; p1[300] = 0; p2[3] = 0                        # identity bases
    p1[9] = p1[8]; p2[9] = p2[8]                             # a repeated base

    def expected(group, n, s):
        if n == 0:
            return np.zeros(8 if group == "g1" else 16, np.uint64)
        return oc.msm_g1(p1[:n], s, threads=TH) if group == "g1" else oc.msm_g2(p2[:n], s, threads=TH)

    case = {"p1": p1, "p2": p2}
    for name, calls in (("g1", [("g1", n) for n in G1_SIZES]), ("g2", [("g2", n) for n in G2_SIZES]), ("mix", MIX)):
        sc = [_scalars(n, 0xD100 + 16 * len(name) + 977 * j) for j, (_, n) in enumerate(calls)]
        case[name] = (calls, sc, [expected(g, n, s) for (g, n), s in zip(calls, sc)])
    case["g1_sum"] = oc.g1_sum(np.stack(case["g1"][2]))
    return case


def _queue_msm(h, srs, calls, scalars, words=24):
    """one msm_*_dev per entry of `calls`, each into its own slot of `words` u64, nothing between them -> the slot tensor (one spare slot
    at the end), not synchronised"""
    import torch
    d_s = [_dev(s) for s in scalars]
    d_out = _fill((len(calls) + 1, words), "i64")
    torch.cuda.synchronize()
    for j, (g, n) in enumerate(calls):
        (h.msm_g1_dev if g == "g1" else h.msm_g2_dev)(srs[g], d_s[j].data_ptr() if n else 0, n, d_out[j].data_ptr())
    return d_out, d_s


def _check_msm(out, calls, exp, what):
    """every slot against the oracle; the words of a slot behind the point must be untouched. (With 12-word slots -- the G1 queue whose packed
    outputs feed g1_sum_dev -- a G1 point fills its slot and that check is empty: the instrumentation test runs the same G1 queue in
    24-word slots.)"""
    for j, (g, n) in enumerate(calls):
        w = 12 if g == "g1" else 24
        assert np.array_equal(_aff_rows(out[j:j + 1, :w])[0], exp[j]), (what, "call %d" % j, g, n)
        assert np.all(out[j, w:] == np.uint64(2**64 - 1)), (what, "call %d wrote past its slot" % j)
        if n == 0:
            assert np.array_equal(out[j, :w], _jac_identity(w)), (what, "n = 0 in the queue must leave the identity")


@pytest.mark.parametrize("tables", [False, True], ids=["no_tables", "tables"])
def test_g1_msm_queue_of_changing_sizes(msm_case, tables):
    """eight G1 MSMs over one SRS, sizes 33 .. 70000 .. 1 .. 0, each with its own scalars and its own output slot, then g1_sum_dev over
    the eight partial outputs (96 bytes apart, as an all-gather leaves them) -- and only then the one synchronisation. On a fresh context
    every workspace starts empty: the first 70000 grows all of them (reserve: drain, free, allocate) while three calls are queued, and the
    calls behind it run in buffers sized for 70000. n = 0 in the queue leaves the identity."""
    calls, sc, exp = msm_case["g1"]
    h = _new_ctx()
    try:
        srs = h.srs_g1_upload(msm_case["p1"])
        if tables:
            assert h.srs_g1_precompute(srs) > 0
        d_out, _keep = _queue_msm(h, {"g1": srs}, calls, sc, words=12)
        k = len(calls)
        h.g1_sum_dev(d_out.data_ptr(), k, d_out[k].data_ptr())
        h.synchronize()
        out = _host(d_out)
        _check_msm(out[:k], calls, exp, "tables" if tables else "no tables")
        assert np.array_equal(_aff_rows(out[k:])[0], msm_case["g1_sum"]), "g1_sum_dev behind the queue"
        srs.free()
    finally:
        h.close()


@pytest.mark.parametrize("tables", [False, True], ids=["no_tables", "tables"])
def test_g2_msm_queue_of_changing_sizes(msm_case, tables):
    calls, sc, exp = msm_case["g2"]
    h = _new_ctx()
    try:
        srs = h.srs_g2_upload(msm_case["p2"])
        if tables:
            assert h.srs_g2_precompute(srs) > 0
        d_out, _keep = _queue_msm(h, {"g2": srs}, calls, sc)
        h.synchronize()
        _check_msm(_host(d_out), calls, exp, "tables" if tables else "no tables")
        srs.free()
    finally:
        h.close()


def test_g1_and_g2_msm_interleaved_on_one_context(msm_case):
    """G1 4096, G2 1000, G1 257, G2 33 on one context: `buckets` / `partials` / `heavy` hold 128-byte G1 and 256-byte G2 elements in turn"""
    calls, sc, exp = msm_case["mix"]
    h = _new_ctx()
    try:
        srs = {"g1": h.srs_g1_upload(msm_case["p1"][:4096]), "g2": h.srs_g2_upload(msm_case["p2"][:1000])}
        d_out, _keep = _queue_msm(h, srs, calls, sc)
        h.synchronize()
        _check_msm(_host(d_out), calls, exp, "interleaved")
        for s in srs.values():
            s.free()
    finally:
        h.close()


@pytest.fixture(scope="module")
def mul_case(oc, rand_fr):
    """Chains of batched scalar multiplications, the oracle's. Call j writes the first n_j points of slot j (a slot = 300 base points); the
    next call reads slot j: one point of it (point_stride 0: the LAST one call j wrote) or its first n_(j+1) points (point_stride 1: what
    call j wrote, then base points). So every result is (k_j ... k_1) G, and nothing may be written behind the n_j points."""
    out = {}
    for gi, group in enumerate(("g1", "g2")):
        gen = oc.generators()[gi]
        mul = oc.g1_mul_batch if group == "g1" else oc.g2_mul_batch
        base = mul(gen, _mont(oc, rand_fr(300, 0xB00 + gi)), threads=TH)
        ks = []
        for j, n in enumerate(MUL_SIZES):
            k = rand_fr(n, 0xB10 + 16 * gi + j)
            if n > 2:
                k[0] = 0                                     # -> the identity, which the next stride-1 call takes as a point
                k[1] = R - 1
                k[2] = 1
            ks.append(_mont(oc, k))
        for stride in (0, 1):
            slots = []
            for j, n in enumerate(MUL_SIZES):
                if j == 0:
                    src = gen
                elif stride == 0:
                    src = slots[j - 1][MUL_SIZES[j - 1] - 1]
                else:
                    src = slots[j - 1][:n]
                slot = base.copy()
                slot[:n] = mul(src, ks[j], threads=TH)
                slots.append(slot)
            out[group, stride] = np.stack(slots)
        out[group, "base"], out[group, "ks"], out[group, "gen"] = base, ks, gen
        out[group, "base_times_k2"] = mul(base, ks[2], threads=TH)           # one call outside the chains: point i times scalar i
    return out


@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_mul_batch_chain(mul_case, group, stride):
    import torch
    h = _new_ctx()
    try:
        base, ks, gen = mul_case[group, "base"], mul_case[group, "ks"], mul_case[group, "gen"]
        call = h.g1_mul_batch_dev if group == "g1" else h.g2_mul_batch_dev
        d_gen = _dev(gen)
        d_ks = [_dev(k) for k in ks]
        d_slots = _dev(np.stack([base] * len(MUL_SIZES)))
        torch.cuda.synchronize()
        for j, n in enumerate(MUL_SIZES):
            if j == 0:
                src = d_gen.data_ptr()
            elif stride == 0:
                src = d_slots[j - 1, MUL_SIZES[j - 1] - 1].data_ptr()
            else:
                src = d_slots[j - 1].data_ptr()
            call(src, stride, d_ks[j].data_ptr(), n, d_slots[j].data_ptr())
        h.synchronize()
        got = _host(d_slots)
        for j, n in enumerate(MUL_SIZES):
            assert np.array_equal(got[j], mul_case[group, stride][j]), (group, stride, "call %d" % j, n)
    finally:
        h.close()


@pytest.fixture(scope="module")
def pair_case(oc, rand_fr):
    """198 (P, Q) pairs with identities in either slot; call j of a queue takes its own stretch of them. exp[1]: e(P_i, Q_i); exp[0]: every
    call against the ONE point Q[first item of the call]"""
    g1, g2 = oc.generators()
    tot = sum(PAIR_SIZES)
    P = oc.g1_mul_batch(g1, _mont(oc, rand_fr(tot, 0xA1)), threads=TH)
    Q = oc.g2_mul_batch(g2, _mont(oc, rand_fr(tot, 0xA2)), threads=TH)
    P[2] = 0; P[70] = 0; Q[3] = 0; Q[133] = 0; Q[197] = 0
    offs = [sum(PAIR_SIZES[:j]) for j in range(len(PAIR_SIZES))]
    e1 = oc.pairing_batch(P, Q, threads=TH)
    e0 = np.concatenate([oc.pairing_batch(P[o:o + n], Q[o], threads=TH) for o, n in zip(offs, PAIR_SIZES)])
    keys = [np.stack([np.frombuffer(oc.blake3_xof(e1[i].tobytes(), ml), np.uint8) for i in range(lo, lo + n)]) for lo, n, ml in DECAP_CALLS]
    return {"P": P, "Q": Q, "offs": offs, 0: e0, 1: e1, "keys": keys}


@pytest.mark.parametrize("g2_stride", [0, 1])
@pytest.mark.parametrize("wide_max", [0, -1], ids=["k_pairing", "wide"])
def test_pairing_queue_then_decap(pair_case, wide_max, g2_stride):
    """pairing_batch_dev of 1, 3, 130, 64 items (pair_ws grows behind queued work in the k_pairing form), then three decap_batch_dev without
    a GT output: their GT bytes all go through the context's tmp_b, which the second call grows while the first one's KDF is queued"""
    import torch
    h = _new_ctx()
    try:
        h.set_option("pair_wide_max", wide_max)
        d_P, d_Q = _dev(pair_case["P"]), _dev(pair_case["Q"])
        tot = sum(PAIR_SIZES)
        d_gt = _fill((tot + 1, 384), "u8")
        d_keys = [_fill((n + 1, ml), "u8") for _, n, ml in DECAP_CALLS]
        torch.cuda.synchronize()
        for o, n in zip(pair_case["offs"], PAIR_SIZES):
            h.pairing_batch_dev(d_P[o].data_ptr(), d_Q[o].data_ptr(), g2_stride, n, d_gt[o].data_ptr())
        for (lo, n, ml), d_k in zip(DECAP_CALLS, d_keys):
            h.decap_batch_dev(d_P[lo].data_ptr(), d_Q[lo].data_ptr(), n, 0, d_k.data_ptr(), ml)
        h.synchronize()
        gt = _host(d_gt)
        for o, n in zip(pair_case["offs"], PAIR_SIZES):
            bad = np.flatnonzero((gt[o:o + n] != pair_case[g2_stride][o:o + n]).any(axis=1))
            assert bad.size == 0, ("pairing call of %d items: wrong GT at items %s" % (n, bad[:8]))
        assert np.all(gt[tot] == 255)
        for c, ((lo, n, ml), d_k) in enumerate(zip(DECAP_CALLS, d_keys)):
            k = _host(d_k)
            assert np.array_equal(k[:n], pair_case["keys"][c]), ("decap call %d" % c, n, ml)
            assert np.all(k[n] == 255)
    finally:
        h.close()


# ---- 2. inputs and outputs in stream order, on the three stream forms -----------------------------------------------------------------
@pytest.fixture(scope="module")
def order_case(oc, rand_fr, msm_case, mul_case):
    """per family: the fixed operand, two valid contents (a, b) of the buffer that is overwritten between the calls, and the oracle's two results"""
    g1, g2 = oc.generators()
    pts = msm_case["p1"][:4096]
    sa, sb = _scalars(4096, 0xC1), _scalars(4096, 0xC2)
    base = mul_case["g1", "base"]
    ka, kb = _mont(oc, rand_fr(300, 0xC3)), _mont(oc, rand_fr(300, 0xC4))
    Pa = oc.g1_mul_batch(g1, _mont(oc, rand_fr(64, 0xC5)), threads=TH)
    Pb = oc.g1_mul_batch(g1, _mont(oc, rand_fr(64, 0xC6)), threads=TH)
    Pb[5] = 0
    Q = oc.g2_mul_batch(g2, _mont(oc, rand_fr(64, 0xC7)), threads=TH)
    return {"msm": (pts, sa, sb, oc.msm_g1(pts, sa, threads=TH), oc.msm_g1(pts, sb, threads=TH)),
            "mul": (base, ka, kb, oc.g1_mul_batch(base, ka, threads=TH), oc.g1_mul_batch(base, kb, threads=TH)),
            "pairing": (Q, Pa, Pb, oc.pairing_batch(Pa, Q, threads=TH), oc.pairing_batch(Pb, Q, threads=TH))}


@pytest.mark.parametrize("family", ["msm", "mul", "pairing"])
@pytest.mark.parametrize("form", STREAM_FORMS)
def test_inputs_and_outputs_in_stream_order(order_case, form, family):
    """producer kernel -> *_dev call -> the input overwritten -> the output copied away -> second call, and ONE synchronisation: each call
    must have read what the buffer held at its place in the stream and its output must be complete where the copy stands.
    A caller-created stream and the legacy default stream (torch's default stream on ROCm) order the calls with torch's kernels by
    themselves. A private stream is unordered against the caller's by contract: there the caller synchronises torch in front of a call and
    the context behind it (keaki_hip_synchronize), and the same equalities hold."""
    import torch
    from keaki_amd.hip import KEAKI_HIP_STREAM_LEGACY
    fixed, a, b, exp_a, exp_b = order_case[family]
    if form == "torch":
        stream = torch.cuda.Stream()
        h = _new_ctx(stream.cuda_stream)
    elif form == "legacy":
        stream = torch.cuda.default_stream()
        assert stream.cuda_stream == 0                          # the null stream, which the context names as STREAM_LEGACY
        h = _new_ctx(KEAKI_HIP_STREAM_LEGACY)
    else:
        stream = torch.cuda.default_stream()
        h = _new_ctx()
    front = torch.cuda.synchronize if form == "private" else (lambda: None)
    behind = h.synchronize if form == "private" else (lambda: None)
    srs = None
    try:
        d_fixed, st_a, st_b = _dev(fixed), _dev(a), _dev(b)
        d_in = torch.zeros_like(st_a)
        if family == "msm":
            srs = h.srs_g1_wrap_dev(d_fixed.data_ptr(), 4096)
            d_out, d_keep = _fill((1, 12), "i64"), _fill((1, 12), "i64")
            call = lambda: h.msm_g1_dev(srs, d_in.data_ptr(), 4096, d_out.data_ptr())
        elif family == "mul":
            d_out, d_keep = _fill((300, 8), "i64"), _fill((300, 8), "i64")
            call = lambda: h.g1_mul_batch_dev(d_fixed.data_ptr(), 1, d_in.data_ptr(), 300, d_out.data_ptr())
        else:
            d_out, d_keep = _fill((64, 384), "u8"), _fill((64, 384), "u8")
            call = lambda: h.pairing_batch_dev(d_in.data_ptr(), d_fixed.data_ptr(), 1, 64, d_out.data_ptr())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_in.copy_(st_a)                                   # 1. the producer
            front()
            call()                                             # 2.
            behind()
            d_in.copy_(st_b)                                   # 3. the input overwritten right behind the call
            d_keep.copy_(d_out)                                # 4. the output copied away
            front()
            call()                                             # 5. on the overwritten input, into the same output
            behind()
        torch.cuda.synchronize()
        h.synchronize()
        first, second = _host(d_keep), _host(d_out)
        if family == "msm":
            first, second = _aff_rows(first)[0], _aff_rows(second)[0]
        assert np.array_equal(first, exp_a), (form, family, "the first call did not see the producer's data / its output was copied too early")
        assert np.array_equal(second, exp_b), (form, family, "the second call did not see the overwritten input")
    finally:
        if srs is not None:
            srs.free()
        h.close()


# ---- 3. the encapsulation policy through the _dev branch ---------------------------------------------------------------------------------
def _kem_inputs(oc, rand_fr, seed, n, c, tau, zero_r=()):
    """n items to the commitment c g1 under [tau]_2: points, values, r (Montgomery), and the opening proofs ((c - value) / (tau - point)) g1
    that decapsulate them -- e(proof, ct) = e(g1, g2)^(r (c - value)) -- from the oracle's scalar multiplication"""
    al, be, r = rand_fr(n, seed), rand_fr(n, seed + 1), rand_fr(n, seed + 2)
    for i in zero_r:
        r[i] = 0
    proofs = oc.g1_mul_batch(oc.generators()[0], _mont(oc, [(c - b) * pow(tau - a, -1, R) for a, b in zip(al, be)]), threads=TH)
    return _mont(oc, al), _mont(oc, be), _mont(oc, r), proofs


def _kem_expected(oc, st, tau_g2):
    """the oracle's ciphertexts, GT bytes, 33-byte keys (and the 32-byte ones, a KDF call of their own) of the step's checked items"""
    i = st["idx"]
    ct, gt, key33 = oc.encap_batch(st["com"], tau_g2, st["A"][i], st["V"][i], st["R"][i], 33, threads=TH)
    key32 = np.stack([np.frombuffer(oc.blake3_xof(g.tobytes(), 32), np.uint8) for g in gt])
    st.update(ct=ct, gt=gt, key33=key33, key32=key32)
    return st


@pytest.fixture(scope="module")
def kem_case(oc, rand_fr):
    g1, g2 = oc.generators()
    tau, c1, c2 = rand_fr(3, 0xE0)
    tau_g2 = oc.g2_mul_batch(g2, _mont(oc, [tau]))[0]
    coms = {1: oc.g1_mul_batch(g1, _mont(oc, [c1]))[0], 2: oc.g1_mul_batch(g1, _mont(oc, [c2]))[0], 0: np.zeros(8, np.uint64)}
    dlog = {1: c1, 2: c2, 0: 0}
    rng = np.random.default_rng(0xE1)

    def step(which, n, seed, zero_r=()):
        A, Vv, Rr, proofs = _kem_inputs(oc, rand_fr, seed, n, dlog[which], tau, zero_r)
        # every item, except in the 4097-item step: 64 of them, first and last included (the oracle pairs one item at a time)
        idx = np.arange(n) if n <= 300 else np.unique(np.concatenate([[0, n - 1], np.arange(1, n - 1, (n - 2) // 62 + 1)]))[:64]
        st = {"which": which, "com": coms[which], "n": n, "A": A, "V": Vv, "R": Rr, "proofs": proofs, "idx": idx,
              "msgs": rng.integers(0, 256, (n, 33), dtype=np.uint8)}
        return _kem_expected(oc, st, tau_g2)

    steps = [step(w, n, 0xE100 + 16 * k) for k, (w, n) in enumerate(ENCAP_STEPS)]
    assert len(steps[4]["idx"]) == 64 and steps[4]["idx"][0] == 0 and steps[4]["idx"][-1] == 4096
    # steps 3 and 4 again with the identity as the commitment and r = 0 items (ct = identity, GT = one) inside the batches
    degenerate = [steps[1], step(0, 300, 0xE200, zero_r=(0, 7, 255, 299)), steps[3], step(0, 64, 0xE210, zero_r=(63,)), step(1, 3, 0xE220, zero_r=(1,))]
    return {"tau_g2": tau_g2, "coms": coms, "steps": steps, "degenerate": degenerate}


def _kem_device(case, steps, body_len=0):
    d = {"tau": _dev(case["tau_g2"]), "com": {w: _dev(c) for w, c in case["coms"].items()}, "steps": []}
    for st in steps:
        n = st["n"]
        e = {"A": _dev(st["A"]), "V": _dev(st["V"]), "R": _dev(st["R"]), "ct": _fill((n + 1, 16), "i64")}
        if body_len:
            e.update(body=_dev(st["msgs"][:, :body_len]), snap=_fill((n, body_len), "u8"), proofs=_dev(st["proofs"]))
        else:
            e.update(gt=_fill((n + 1, 384), "u8"), key=_fill((n + 1, 32), "u8"))
        d["steps"].append(e)
    return d


def _wrong(got, exp):
    return np.flatnonzero((got != exp).reshape(exp.shape[0], -1).any(axis=1))


def _check_encap(steps, dev, what):
    for k, (st, e) in enumerate(zip(steps, dev["steps"])):
        n, i = st["n"], st["idx"]
        ct, gt, key = _host(e["ct"]), _host(e["gt"]), _host(e["key"])
        tag = "%s step %d (commitment %d, n = %d)" % (what, k + 1, st["which"], n)
        bad = _wrong(gt[i], st["gt"])
        assert bad.size == 0, "%s: wrong GT bytes at %d of %d checked items, first %s" % (tag, bad.size, len(i), i[bad[:4]])
        bad = _wrong(ct[i], st["ct"])
        assert bad.size == 0, "%s: wrong ciphertext at %d of %d checked items, first %s" % (tag, bad.size, len(i), i[bad[:4]])
        bad = _wrong(key[i], st["key32"])
        assert bad.size == 0, "%s: wrong key at %d of %d checked items, first %s" % (tag, bad.size, len(i), i[bad[:4]])
        assert np.all(ct[n] == np.uint64(2**64 - 1)) and np.all(gt[n] == 255) and np.all(key[n] == 255), tag + ": wrote past its slot"


def _queue_encap(h, dev, steps):
    for st, e in zip(steps, dev["steps"]):
        h.encap_batch_dev(dev["com"][st["which"]].data_ptr(), dev["tau"].data_ptr(), e["A"].data_ptr(), e["V"].data_ptr(), e["R"].data_ptr(),
                          st["n"], e["ct"].data_ptr(), e["gt"].data_ptr(), e["key"].data_ptr(), 32)


def test_encap_policy_queue(kem_case):
    """encap_batch_dev, options automatic, no synchronisation by the caller (the call's read-back of com / [tau]_2 is the library's):
       1  C1  255   below the fixed-base tables; a first commitment: its GT table built on the aux stream
       2  C1  256   fixed-base tables built; the same commitment again: its table promoted from 13-bit to 16-bit windows
       3  C2  300   a new table on the aux stream while C1's readers are queued
       4  C1    1   back again: rebuilt over gt_base
       5  C2 4097   n > 4096: the constant base's factor first on the main stream, the commitment's behind the aux build
       6  C2   64   the same commitment behind a large call
    every item of every step against the oracle (step 5: 64 items, item 0 and item 4096 among them)"""
    import torch
    steps = kem_case["steps"]
    h = _new_ctx()
    try:
        dev = _kem_device(kem_case, steps)
        torch.cuda.synchronize()
        _queue_encap(h, dev, steps)
        h.synchronize()
        _check_encap(steps, dev, "encap")
    finally:
        h.close()


def test_encap_policy_queue_with_degenerate_items(kem_case):
    """C1 x 256, then the IDENTITY as a new commitment (300 items, r = 0 at four of them), C1 x 1 again, the identity x 64, C1 x 3 with
    r = 0 in the middle: degenerate items inside a queue rather than inside a single call"""
    import torch
    steps = kem_case["degenerate"]
    h = _new_ctx()
    try:
        dev = _kem_device(kem_case, steps)
        torch.cuda.synchronize()
        _queue_encap(h, dev, steps)
        h.synchronize()
        _check_encap(steps, dev, "degenerate")
        one = np.zeros(384, np.uint8); one[0] = 1
        assert np.array_equal(_host(dev["steps"][1]["gt"])[7], one) and not _host(dev["steps"][1]["ct"])[7].any()
    finally:
        h.close()


def test_encrypt_then_decrypt_queue(kem_case):
    """the same six steps through encrypt_batch_dev (messages in d_body_inout, 33 bytes each), every step's bodies copied away by a torch kernel
    and decrypt_batch_dev of the step's own ciphertexts with the oracle's proofs right behind it -- all on the caller's stream, one
    synchronisation. Bodies = oracle key XOR message, and every message comes back byte for byte (all 4097 of step 5 too). encrypt keeps
    its GT bytes in tmp_b, decrypt as well: a step's pairing kernel is queued while the next step's table is built on the aux stream."""
    import torch
    steps = kem_case["steps"]
    stream = torch.cuda.Stream()
    h = _new_ctx(stream.cuda_stream)
    try:
        dev = _kem_device(kem_case, steps, body_len=33)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for st, e in zip(steps, dev["steps"]):
                h.encrypt_batch_dev(dev["com"][st["which"]].data_ptr(), dev["tau"].data_ptr(), e["A"].data_ptr(), e["V"].data_ptr(), e["R"].data_ptr(),
                                    st["n"], e["ct"].data_ptr(), e["body"].data_ptr(), 33)
                e["snap"].copy_(e["body"])
                h.decrypt_batch_dev(e["proofs"].data_ptr(), e["ct"].data_ptr(), st["n"], e["body"].data_ptr(), 33)
        stream.synchronize()
        h.synchronize()
        for k, (st, e) in enumerate(zip(steps, dev["steps"])):
            n, i = st["n"], st["idx"]
            tag = "step %d (commitment %d, n = %d)" % (k + 1, st["which"], n)
            ct, body, back = _host(e["ct"]), _host(e["snap"]), _host(e["body"])
            bad = _wrong(ct[i], st["ct"])
            assert bad.size == 0, "%s: wrong ciphertext at %d checked items, first %s" % (tag, bad.size, i[bad[:4]])
            bad = _wrong(body[i], st["key33"] ^ st["msgs"][i])
            assert bad.size == 0, "%s: body != key XOR message at %d checked items, first %s" % (tag, bad.size, i[bad[:4]])
            bad = _wrong(back, st["msgs"])
            assert bad.size == 0, "%s: %d of %d messages did not come back, first %s" % (tag, bad.size, n, bad[:4])
            assert np.all(ct[n] == np.uint64(2**64 - 1)), tag
    finally:
        h.close()


# ---- 4. instrumentation and trim under a queue -----------------------------------------------------------------------------------------------
def test_instrumentation_and_trim_after_a_queue(msm_case, mul_case, pair_case, kem_case):
    """set_timing(1), the G1 MSM queue (it ENDS with n = 0) and an encapsulation, one synchronisation: the figures are those of the last
    non-empty MSM. Then ctx_trim gives every workspace and table back, and one more call of each family, queued, is still right."""
    import torch
    calls, sc, exp = msm_case["g1"]
    g2calls, g2sc, g2exp = msm_case["g2"]
    ksteps = [kem_case["steps"][0]]
    h = _new_ctx()
    try:
        h.set_timing(True)
        srs = h.srs_g1_upload(msm_case["p1"])
        srs2 = h.srs_g2_upload(msm_case["p2"])
        kdev = _kem_device(kem_case, ksteps)
        d_out, _keep = _queue_msm(h, {"g1": srs}, calls, sc)
        _queue_encap(h, kdev, ksteps)
        h.synchronize()
        _check_msm(_host(d_out), calls, exp, "timed")
        _check_encap(ksteps, kdev, "timed")
        stats = h.last_msm_stats()
        last_n = [n for _, n in calls if n][-1]
        assert stats["total_ms"] > 0, stats
        assert 0 < stats["bucket_ms"] <= stats["total_ms"], stats
        assert stats["window_bits"] == V.msm(last_n)["c"], (stats, "the window of the last non-empty call (n = %d)" % last_n)

        # the same through a caller that runs the MSM driver itself: `open` of a constant polynomial has an EMPTY quotient. Behind a timed MSM
        # that is still queued, its proof is the identity, its value the constant, and the figures stay those of the queued MSM
        d_s3 = _dev(sc[3])
        d_o3 = _fill((1, 12), "i64")
        torch.cuda.synchronize()
        h.msm_g1_dev(srs, d_s3.data_ptr(), calls[3][1], d_o3.data_ptr())
        proof, val = h.kzg_open(srs, sc[1][:1], sc[1][7])
        h.synchronize()
        assert np.array_equal(proof, _jac_identity(12)) and np.array_equal(val, sc[1][0])
        assert np.array_equal(_aff_rows(_host(d_o3))[0], exp[3])
        stats = h.last_msm_stats()
        assert stats["total_ms"] > 0 and stats["window_bits"] == V.msm(calls[3][1])["c"], stats

        assert h.memory()["workspaces"] > 0 and h.memory()["gt_tables"] > 0
        h.trim()
        mem = h.memory()
        assert mem["workspaces"] == 0 and mem["gt_tables"] == 0, mem
        # one more call of each family, queued
        ksteps = [kem_case["steps"][3]]
        kdev = _kem_device(kem_case, ksteps)
        est = kem_case["steps"][5]                            # encrypt + decrypt in place: C2, 64 items
        edev = _kem_device(kem_case, [est], body_len=33)
        ee = edev["steps"][0]
        d_b1, d_k1g = _dev(mul_case["g1", "base"]), _dev(mul_case["g1", "ks"][2])
        d_mul1 = _fill((MUL_SIZES[2] + 1, 8), "i64")
        d_s1, d_s2 = _dev(sc[5]), _dev(g2sc[0])
        d_m = _fill((2, 24), "i64")
        o, n = pair_case["offs"][2], PAIR_SIZES[2]
        d_P, d_Q = _dev(pair_case["P"]), _dev(pair_case["Q"])
        d_gt = _fill((n, 384), "u8")
        lo, dn, ml = DECAP_CALLS[2]
        d_key = _fill((dn, ml), "u8")
        d_gen, d_k0, d_k1 = _dev(mul_case["g2", "gen"]), _dev(mul_case["g2", "ks"][0]), _dev(mul_case["g2", "ks"][1])
        d_mul = _fill((MUL_SIZES[0] + MUL_SIZES[1], 16), "i64")
        torch.cuda.synchronize()
        h.msm_g1_dev(srs, d_s1.data_ptr(), calls[5][1], d_m[0].data_ptr())
        h.msm_g2_dev(srs2, d_s2.data_ptr(), g2calls[0][1], d_m[1].data_ptr())
        h.g2_mul_batch_dev(d_gen.data_ptr(), 0, d_k0.data_ptr(), MUL_SIZES[0], d_mul[0].data_ptr())        # the first two calls of the stride-0 chain
        h.g2_mul_batch_dev(d_mul[0].data_ptr(), 0, d_k1.data_ptr(), MUL_SIZES[1], d_mul[1].data_ptr())
        h.g1_mul_batch_dev(d_b1.data_ptr(), 1, d_k1g.data_ptr(), MUL_SIZES[2], d_mul1.data_ptr())
        h.pairing_batch_dev(d_P[o].data_ptr(), d_Q[o].data_ptr(), 1, n, d_gt.data_ptr())
        _queue_encap(h, kdev, ksteps)
        h.decap_batch_dev(d_P[lo].data_ptr(), d_Q[lo].data_ptr(), dn, 0, d_key.data_ptr(), ml)
        h.encrypt_batch_dev(edev["com"][est["which"]].data_ptr(), edev["tau"].data_ptr(), ee["A"].data_ptr(), ee["V"].data_ptr(), ee["R"].data_ptr(),
                            est["n"], ee["ct"].data_ptr(), ee["body"].data_ptr(), 33)
        h.synchronize()                                       # the bodies are read here; the decryption is queued behind a second encryption
        body = _host(ee["body"]).copy()
        h.encrypt_batch_dev(edev["com"][est["which"]].data_ptr(), edev["tau"].data_ptr(), ee["A"].data_ptr(), ee["V"].data_ptr(), ee["R"].data_ptr(),
                            est["n"], ee["ct"].data_ptr(), ee["snap"].data_ptr(), 33)           # snap holds 0xff bytes: body = key XOR 0xff
        h.decrypt_batch_dev(ee["proofs"].data_ptr(), ee["ct"].data_ptr(), est["n"], ee["body"].data_ptr(), 33)
        h.synchronize()
        assert np.array_equal(body, est["key33"] ^ est["msgs"]) and np.array_equal(_host(ee["ct"])[:est["n"]], est["ct"])
        assert np.array_equal(_host(ee["snap"]), est["key33"] ^ np.uint8(255)) and np.array_equal(_host(ee["body"]), est["msgs"])
        m = _host(d_m)
        assert np.array_equal(_aff_rows(m[0:1, :12])[0], exp[5]) and np.array_equal(_aff_rows(m[1:2])[0], g2exp[0])
        assert np.array_equal(_host(d_mul)[1:], mul_case["g2", 0][1][:MUL_SIZES[1]])
        mul1 = _host(d_mul1)                                  # point i of the base times scalar i, and nothing behind the 300 outputs
        assert np.array_equal(mul1[:MUL_SIZES[2]], mul_case["g1", "base_times_k2"]) and np.all(mul1[MUL_SIZES[2]] == np.uint64(2**64 - 1))
        assert np.array_equal(_host(d_gt), pair_case[1][o:o + n])
        _check_encap(ksteps, kdev, "after trim")
        assert np.array_equal(_host(d_key), pair_case["keys"][2])
        assert h.last_msm_stats()["window_bits"] == V.msm(g2calls[0][1], g2=True)["c"]
        srs.free(); srs2.free()
    finally:
        h.close()
