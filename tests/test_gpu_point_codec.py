"""keaki_hip_g1/g2_compress, _decompress, keaki_hip_g2_subgroup_check (host and _dev forms) and the wire functions of the host mirror on the GPU
against the big-int model (tests/point_codec_model.py). The points are multiples of the generators from the C oracle (known discrete logs) and
twist points the model builds; every expected byte, status and counter comes from the model, never from the library under test."""
import os
import random

import numpy as np
import pytest

import point_codec_model as M

pytestmark = pytest.mark.gpu

NCPU = os.cpu_count() or 1
P, R = M.P, M.R
BAD_ARG = -1
SIZES = [1, 63, 64, 65, 4096, (1 << 16) + 3]
RINV = pow(1 << 256, -1, P)


@pytest.fixture(scope="module")
def K():
    from keaki_amd import keaki as K
    return K


# ---- the model on arrays ------------------------------------------------------------------------------------------------------------------------
def canon(words):
    """u64[n, 4k] Montgomery limbs -> n rows of k canonical integers"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    k = w.shape[1] // 4
    raw = w.tobytes()
    return [[int.from_bytes(raw[(i * k + j) * 32:(i * k + j + 1) * 32], "little") * RINV % P for j in range(k)] for i in range(w.shape[0])]


def model_g1_bytes(words):
    out = bytearray()
    for (x, y), w in zip(canon(words), np.asarray(words)):
        out += M.g1_compress(None if not w.any() else (x, y))
    return np.frombuffer(bytes(out), np.uint8).reshape(-1, 32)


def model_g2_bytes(words):
    out = bytearray()
    for (x0, x1, y0, y1), w in zip(canon(words), np.asarray(words)):
        out += M.g2_compress(None if not w.any() else ((x0, x1), (y0, y1)))
    return np.frombuffer(bytes(out), np.uint8).reshape(-1, 64)


def words_of(points, g2):
    return np.array([(M.g2_words if g2 else M.g1_words)(p) for p in points], np.uint64).reshape(-1, 16 if g2 else 8)


_PTS = {}


def points(oc, n, g2):
    """n points k_i * generator (k_i random, a few structured), with the identity among them"""
    if (n, g2) not in _PTS:
        from conftest import rand_fr_ints
        ks = rand_fr_ints(n, 4100 + n + (7 if g2 else 0))
        for i, k in enumerate([0, 1, R - 1, 2, R - 2][:n]):
            ks[(i * 13) % n] = k                                 # identity, +-G, +-2G
        if n == 1:
            ks[0] = 5
        sc = oc.fr_to_mont(oc.ints_to_limbs(ks))
        gen = oc.generators()[1 if g2 else 0]
        _PTS[(n, g2)] = (oc.g2_mul_batch if g2 else oc.g1_mul_batch)(gen, sc, threads=NCPU)
    return _PTS[(n, g2)]


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ---- compress / decompress ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_compress_and_round_trip(oc, hip, n, g2):
    pts = points(oc, n, g2)
    if n > 1:
        assert not pts[0].any() or any(not p.any() for p in pts[:64]), "the identity is among the inputs"
    want = model_g2_bytes(pts) if g2 else model_g1_bytes(pts)
    got = hip.g2_compress(pts) if g2 else hip.g1_compress(pts)
    assert np.array_equal(got, want), "device bytes differ from the model"
    back, status, n_bad, first = hip.g2_decompress(got, 1) if g2 else hip.g1_decompress(got)
    assert n_bad == 0 and first is None and not status.any()
    assert np.array_equal(back, pts), "decompress(compress(points)) is not the identity on the limbs"
    # the resident forms
    import torch
    d_pts, d_bytes = dev(pts), torch.zeros(n * (64 if g2 else 32), dtype=torch.uint8, device="cuda")
    d_back, d_st = torch.zeros(pts.size * 8, dtype=torch.uint8, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    name = "g2" if g2 else "g1"
    hip.point_codec_dev(name + "_compress", d_pts, n, d_bytes)
    assert hip.point_codec_dev(name + "_decompress", d_bytes, n, d_back, d_st, 1) == (0, None)
    assert np.array_equal(d_bytes.cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(d_back.cpu().numpy().view(np.uint64).reshape(pts.shape), pts) and not d_st.cpu().numpy().any()
    assert hip.point_codec_dev(name + "_decompress", d_bytes, n, d_back, None, 0 if g2 else 1) == (0, None)      # status is optional


def test_model_bytes_decode_to_model_points(py, hip):
    rnd = random.Random(11)
    g1 = [None, py.G1_GEN, py.g1_neg(py.G1_GEN)] + [py.g1_mul(py.G1_GEN, rnd.randrange(1, R)) for _ in range(29)]
    g2 = [None, py.G2_GEN, py.g2_neg(py.G2_GEN)] + [py.g2_mul(py.G2_GEN, rnd.randrange(1, R)) for _ in range(13)]
    b1 = np.frombuffer(b"".join(M.g1_compress(p) for p in g1), np.uint8)
    b2 = np.frombuffer(b"".join(M.g2_compress(p) for p in g2), np.uint8)
    out, st, bad, _ = hip.g1_decompress(b1)
    assert bad == 0 and np.array_equal(out, words_of(g1, False))
    out, st, bad, _ = hip.g2_decompress(b2, 1)
    assert bad == 0 and np.array_equal(out, words_of(g2, True))
    assert hip.g1_compress(words_of(g1, False)).tobytes() == b1.tobytes() and hip.g2_compress(words_of(g2, True)).tobytes() == b2.tobytes()
    assert hip.g1_compress(words_of([py.G1_GEN], False))[0].tolist() == [1] + [0] * 31
    assert hip.g1_compress(np.zeros((1, 8), np.uint64))[0, 31] == 0x40 and hip.g2_compress(np.zeros((1, 16), np.uint64))[0, 63] == 0x40


def test_points_whose_y_and_minus_y_differ_in_c0_only(py, hip):
    """y.c1 = 0 (x^3 + b in Fq): the sign flag comes from c0. These twist points lie outside G2, so they decode with the check off."""
    q = M.g2_points_with_real_y(12, 21)
    q += [py.g2_neg(p) for p in q]
    assert all(p[1][1] == 0 for p in q)
    w = words_of(q, True)
    want = np.frombuffer(b"".join(M.g2_compress(p) for p in q), np.uint8).reshape(-1, 64)
    got = hip.g2_compress(w)
    assert np.array_equal(got, want) and sorted((got[:12, 63] ^ got[12:, 63]).tolist()) == [0x80] * 12
    out, st, bad, _ = hip.g2_decompress(got, 0)
    assert bad == 0 and np.array_equal(out, w)                   # the a1 = 0 branch of the Fq2 square root, both signs


@pytest.mark.parametrize("g2", [False, True])
def test_compress_at_2_to_20_sampled(oc, hip, g2):
    base = points(oc, (1 << 16) + 3, g2)
    n = 1 << 20
    idx = (np.arange(n, dtype=np.int64) * 2654435761 % base.shape[0])
    pts = base[idx]
    got = hip.g2_compress(pts) if g2 else hip.g1_compress(pts)
    ref = (model_g2_bytes if g2 else model_g1_bytes)(base)
    sample = np.concatenate([np.arange(0, 300), np.arange(65536 - 50, 65536 + 50), np.random.default_rng(5).integers(0, n, 2000), np.arange(n - 300, n)])
    assert np.array_equal(got[sample], ref[idx[sample]])
    assert np.array_equal(got, ref[idx])                        # the expected bytes of all 2^20 items follow from the 2^16 + 3 modelled ones
    back, st, bad, first = hip.g2_decompress(got, 1) if g2 else hip.g1_decompress(got)
    assert bad == 0 and first is None and np.array_equal(back[sample], pts[sample]) and np.array_equal(back, pts)


# ---- the verdict matrix -------------------------------------------------------------------------------------------------------------------------
def enc32(v):
    return int(v).to_bytes(32, "little")


def check_against_model(hip, rows, g2, check):
    data = np.frombuffer(b"".join(rows), np.uint8)
    out, st, bad, first = hip.g2_decompress(data, check) if g2 else hip.g1_decompress(data)
    exp = [M.g2_decompress(r, bool(check)) if g2 else M.g1_decompress(r) for r in rows]
    est = [e[0] for e in exp]
    assert st.tolist() == est, "status[] differs from the model"
    assert bad == sum(1 for s in est if s) and first == next((i for i, s in enumerate(est) if s), None)
    assert np.array_equal(out, words_of([e[1] for e in exp], g2)), "points differ (a rejected item must be all zero)"
    return est


def test_verdict_matrix_g1(hip):
    rnd = random.Random(31)
    rows = [bytes(31) + bytes([0xC0]), enc32(P), enc32(P + 1), enc32((1 << 254) - 1), bytes([1]) + bytes(30) + bytes([0x40]),
            bytes([1]) + bytes(30) + bytes([0xC0]), enc32(4), bytes(31) + bytes([0x40]), enc32(1), bytearray(enc32(1))]
    rows[-1] = bytes(rows[-1][:31]) + bytes([0x80])
    for _ in range(500):                                         # random x: about half have no root, every one of them must be status 2
        b = bytearray(enc32(rnd.randrange(P)))
        b[31] |= rnd.choice([0, 0x80])
        rows.append(bytes(b))
    est = check_against_model(hip, rows, False, 0)
    assert est[:10] == [1, 1, 1, 1, 1, 1, 2, 0, 0, 0]
    assert 180 < est[10:].count(2) < 320 and est[10:].count(0) + est[10:].count(2) == 500


def test_verdict_matrix_g2(py, hip):
    rnd = random.Random(32)
    one = enc32(1)
    rows = [bytes(63) + bytes([0xC0]), enc32(P) + one, one + enc32(P), enc32(P + 1) + one, one + enc32((1 << 254) - 1), enc32(1 << 255) + one,
            one + bytes(31) + bytes([0x40]), bytes(63) + bytes([0x40]), M.g2_compress(py.G2_GEN), M.g2_compress(py.g2_neg(py.G2_GEN))]
    for _ in range(300):                                         # random x: no root (2) or a twist point outside G2 (3 with the check, 0 without)
        b = bytearray(enc32(rnd.randrange(P)) + enc32(rnd.randrange(P)))
        b[63] |= rnd.choice([0, 0x80])
        rows.append(bytes(b))
    rows += [M.g2_compress(py.g2_mul(py.G2_GEN, rnd.randrange(1, R))) for _ in range(20)]
    rows += [M.g2_compress(M.mul_unreduced(q, M.COFACTOR)) for q in M.random_twist_points(4, 33)]      # cofactor-cleared: members
    on = check_against_model(hip, rows, True, 1)
    off = check_against_model(hip, rows, True, 0)
    assert on[:10] == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0] and on[-24:] == [0] * 24
    assert 100 < on[10:310].count(2) < 200 and on[10:310].count(3) == 300 - on[10:310].count(2)
    assert [0 if s == 3 else s for s in on] == off               # the same bytes with the check off: status 3 becomes 0, nothing else moves


def test_single_bad_item_in_a_large_batch(oc, hip):
    n = (1 << 16) + 3
    for g2 in (False, True):
        good = (hip.g2_compress if g2 else hip.g1_compress)(points(oc, n, g2))
        outsider = np.frombuffer(M.g2_compress(M.random_twist_points(1, 41)[0]), np.uint8)
        for at in (0, n // 2, n - 1):
            for bad_row, want in ([(np.frombuffer(enc32(P) * (2 if g2 else 1), np.uint8), 1)] + ([(outsider, 3)] if g2 else [])):
                b = good.copy()
                b[at] = bad_row
                out, st, bad, first = hip.g2_decompress(b, 1) if g2 else hip.g1_decompress(b)
                assert (bad, first) == (1, at) and st[at] == want and st.sum() == want and not out[at].any()
                keep = np.ones(n, bool); keep[at] = False
                assert np.array_equal(out[keep], points(oc, n, g2)[keep])


# ---- g2_subgroup_check and structured inputs ----------------------------------------------------------------------------------------------------
def test_g2_subgroup_check(oc, py, hip):
    n = 4096
    pts = points(oc, n, True).copy()
    assert hip.g2_subgroup_check(pts) == (0, None)
    assert hip.g2_subgroup_check(np.zeros((3, 16), np.uint64)) == (0, None)          # identity only
    assert hip.g2_subgroup_check(np.zeros((0, 16), np.uint64)) == (0, None)
    outs = M.random_twist_points(3, 51)
    pts[1234] = M.g2_words(outs[0])
    assert hip.g2_subgroup_check(pts) == (1, 1234)
    pts[77], pts[4095] = M.g2_words(outs[1]), M.g2_words(outs[2])
    assert hip.g2_subgroup_check(pts) == (3, 77)
    assert hip.point_codec_dev("g2_subgroup_check", dev(pts), n) == (3, 77)
    assert hip.g2_check(pts) == (0, None)                        # all of them are on the twist: the curve check cannot tell
    big = points(oc, (1 << 16) + 3, True).copy()
    big[65536] = M.g2_words(outs[0])
    assert hip.g2_subgroup_check(big) == (1, 65536)              # second chunk of the host pipeline: the index is global


def test_structured_points_and_degenerate_ladder_branches(py, hip):
    """Known multiples k G (the ladder never meets a degenerate addition inside G2: M.ladder_events) and points of the small order 10069 | 2p - r,
    on which the accumulator becomes the identity and additions meet equal / opposite operands: every one is outside G2 and must be reported."""
    ks = [1, 2, 3, R - 1, R - 2, M.SIX_Z2 % R, (M.SIX_Z2 + 1) % R, (M.SIX_Z2 - 1) % R, pow(M.SIX_Z2, -1, R), (R + 1) // 2, 10069, 1 << 126, (1 << 127) - 1]
    inside = [py.g2_mul(py.G2_GEN, k) for k in ks]
    assert all(M.ladder_events(q) == (0, 0, 0) for q in inside[:6])
    assert hip.g2_subgroup_check(words_of(inside + [None], True)) == (0, None)
    order = R * M.COFACTOR
    small = []
    for q in M.random_twist_points(3, 61):
        s = M.mul_unreduced(q, order // 10069)
        if s is not None:
            assert M.mul_unreduced(s, 10069) is None
            small += [s, py.g2_neg(s), M.mul_unreduced(s, 2), M.mul_unreduced(s, 10068 // 2)]
    assert small
    events = [M.ladder_events(q) for q in small]
    assert all(not M.in_subgroup_def(q) and not M.in_subgroup_fast(q) for q in small)
    w = words_of(small, True)
    assert hip.g2_subgroup_check(w) == (len(small), 0), events
    out, st, bad, first = hip.g2_decompress(hip.g2_compress(w), 1)
    assert st.tolist() == [3] * len(small) and not out.any()
    out, st, bad, first = hip.g2_decompress(hip.g2_compress(w), 0)
    assert bad == 0 and np.array_equal(out, w)


def test_host_forms_across_the_staging_threshold(oc, hip):
    base1, base2 = points(oc, (1 << 16) + 3, False), points(oc, (1 << 16) + 3, True)
    ref1, ref2 = model_g1_bytes(base1), model_g2_bytes(base2)
    for n in (65535, 65536, 65537, 131072 + 5):
        idx = np.arange(n) % base1.shape[0]
        for g2, base, ref in ((False, base1, ref1), (True, base2, ref2)):
            pts = base[idx]
            got = (hip.g2_compress if g2 else hip.g1_compress)(pts)
            assert np.array_equal(got, ref[idx]), n
            b = got.copy()
            b[n - 1, -1] |= 0xC0                                 # malformed, last item of the last chunk
            out, st, bad, first = hip.g2_decompress(b, 1) if g2 else hip.g1_decompress(b)
            assert (bad, first) == (1, n - 1) and st[n - 1] == 1 and np.array_equal(out[:n - 1], pts[:n - 1]) and not out[n - 1].any()
    hip.set_option("pipe_chunks", 0)
    try:
        n = 131072 + 5
        pts = base2[np.arange(n) % base2.shape[0]]
        out, st, bad, first = hip.g2_decompress(hip.g2_compress(pts), 1)
        assert bad == 0 and np.array_equal(out, pts)
    finally:
        hip.set_option("pipe_chunks", 1)


def test_state_does_not_leak_between_calls_and_error_paths(oc, py, hip):
    import ctypes as C
    big = points(oc, (1 << 16) + 3, True)
    bb = hip.g2_compress(big)
    out, st, bad, first = hip.g2_decompress(bb, 1)
    assert bad == 0
    small = np.frombuffer(M.g2_compress(M.random_twist_points(1, 71)[0]) + M.g2_compress(py.G2_GEN), np.uint8)
    out, st, bad, first = hip.g2_decompress(small, 1)           # after the big call: fresh counters, no stale status
    assert (st.tolist(), bad, first) == ([3, 0], 1, 0) and not out[0].any() and np.array_equal(out[1], np.array(M.g2_words(py.G2_GEN), np.uint64))
    lib, ctx = hip.lib, hip.ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o, s8, nb, fb = np.zeros((2, 16), np.uint64), np.zeros(2, np.uint8), C.c_uint64(7), C.c_uint64(7)
    for chk in (2, -1):
        assert lib.keaki_hip_g2_decompress(ctx, p(small), 2, chk, p(o), p(s8), C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g2_decompress_dev(ctx, None, 2, 3, None, None, C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g2_decompress(ctx, None, 2, 1, p(o), p(s8), C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g2_decompress(ctx, p(small), 2, 1, None, p(s8), C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g2_decompress(ctx, p(small), 2, 1, p(o), p(s8), None, C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g1_decompress(ctx, None, 2, p(o), p(s8), C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g1_compress(ctx, None, 2, p(s8)) == BAD_ARG and lib.keaki_hip_g2_compress(ctx, p(o), 2, None) == BAD_ARG
    assert lib.keaki_hip_g1_compress_dev(ctx, None, 2, None) == BAD_ARG
    assert lib.keaki_hip_g2_subgroup_check(ctx, None, 2, C.byref(nb), C.byref(fb)) == BAD_ARG
    assert lib.keaki_hip_g2_subgroup_check(ctx, p(o), 2, None, C.byref(fb)) == BAD_ARG
    assert (nb.value, fb.value) == (7, 7)                        # a refused call writes nothing
    assert b"check_subgroup" in lib.keaki_hip_last_error(ctx) or b"null" in lib.keaki_hip_last_error(ctx)
    # n = 0 and a null status / first_bad are fine
    assert lib.keaki_hip_g2_decompress(ctx, None, 0, 1, None, None, C.byref(nb), None) == 0 and nb.value == 0
    assert lib.keaki_hip_g2_decompress(ctx, p(small), 2, 1, p(o), None, C.byref(nb), None) == 0 and nb.value == 1
    # and the context still works
    out, st, bad, first = hip.g2_decompress(small, 0)
    assert bad == 0 and st.tolist() == [0, 0]


# ---- end to end through the host mirror ---------------------------------------------------------------------------------------------------------
def test_ciphertexts_and_proofs_cross_the_wire(K, py):
    n, ml = 300, 32
    rng = K.Rng(91)
    s = K.KZGSetup.setup(rng.fr_rand(), 512)
    v = np.stack([K.fr(i % 2) for i in range(n)]).astype(np.uint64)
    com, proofs = K.vec_commit(rng, s, v)
    msgs = np.random.default_rng(3).integers(0, 256, size=(n, ml), dtype=np.uint8)
    g2, body = K.vec_encrypt_arrays(rng, s, com, K.domain_elements(n + K.PADDING_LEN), v, msgs)
    wire = K.ciphertexts_to_bytes(s, g2, body)
    assert len(wire) == n * (64 + ml)
    raw = np.frombuffer(wire, np.uint8).reshape(n, 64 + ml)
    assert np.array_equal(raw[:, :64], model_g2_bytes(g2)) and np.array_equal(raw[:, 64:], body)
    g2b, bodyb = K.ciphertexts_from_bytes(s, wire, ml)
    assert np.array_equal(g2b, g2) and np.array_equal(bodyb, body)
    pw = K.proofs_to_bytes(s, proofs[:n])
    assert len(pw) == n * 32 and np.array_equal(np.frombuffer(pw, np.uint8).reshape(n, 32), model_g1_bytes(proofs[:n]))
    pb = K.proofs_from_bytes(s, pw)
    assert np.array_equal(pb, proofs[:n])
    assert np.array_equal(K.vec_decrypt_arrays(s, pb, g2b, bodyb), msgs)          # the messages that went in
    # one ciphertext becomes a point of the twist outside G2: named by its index; a malformed one and a bad proof likewise
    bad = raw.copy()
    bad[123, :64] = np.frombuffer(M.g2_compress(M.random_twist_points(1, 92)[0]), np.uint8)
    with pytest.raises(K.WireFormatError) as e:
        K.ciphertexts_from_bytes(s, bad.tobytes(), ml)
    assert (e.value.index, e.value.reason) == (123, 3) and "123" in str(e.value)
    bad[7, 63] |= 0xC0
    with pytest.raises(K.WireFormatError) as e:
        K.ciphertexts_from_bytes(s, bad.tobytes(), ml)
    assert (e.value.index, e.value.reason) == (7, 1)
    pbad = np.frombuffer(pw, np.uint8).reshape(n, 32).copy()
    pbad[299] = np.frombuffer(enc32(4), np.uint8)               # 4^3 + 3 is a non-residue
    with pytest.raises(K.WireFormatError) as e:
        K.proofs_from_bytes(s, pbad.tobytes())
    assert (e.value.index, e.value.reason) == (299, 2)
    s.close()


def test_laconic_ot_flow_over_the_compressed_wire(K, oc):
    """Laconic OT at 2^8 bits with the sender's ciphertexts crossing the wire compressed. The ORACLE's flow on the same draws is the reference: its
    serial `encrypt` gives the ciphertext points that must come off the wire, its pairing the keys that open them, and the messages recovered
    are the known inputs. Then laconic_ot.py's own flow with --wire compressed: what it reports about the bytes is measured, not written down."""
    log2n, vb = 8, 32
    n = 1 << log2n
    rng = K.Rng(2024)
    secret = rng.fr_rand()
    s = K.KZGSetup.setup(secret, 2 * n)
    try:
        np_rng = np.random.default_rng(7)
        bits = np_rng.integers(0, 2, n)
        zero, one = K.fr(0), K.fr(1)
        choices = np.where(bits[:, None] == 0, zero[None, :], one[None, :]).astype(np.uint64)
        com, proofs = K.vec_commit(rng, s, choices)
        sets = [np_rng.integers(0, 256, size=(n, vb), dtype=np.uint8) for _ in range(2)]
        elements = K.domain_elements(n + K.PADDING_LEN)
        zeros, ones = np.repeat(zero[None, :], n, 0), np.repeat(one[None, :], n, 0)
        g2_0, body_0 = K.vec_encrypt_arrays(rng, s, com, elements, zeros, sets[0])
        g2_1, body_1 = K.vec_encrypt_arrays(rng, s, com, elements, ones, sets[1])
        sent = [K.ciphertexts_to_bytes(s, g2_0, body_0), K.ciphertexts_to_bytes(s, g2_1, body_1)]
        assert [len(b) for b in sent] == [n * (64 + vb)] * 2                        # 64 B per point on the wire, 128 in the limb layout
        (w_g2_0, w_body_0), (w_g2_1, w_body_1) = (K.ciphertexts_from_bytes(s, b, vb) for b in sent)
        # the oracle's sender: the same r (one Fr::rand per item in index order, after the secret and the padding draw), its own encapsulation
        replay = K.Rng(2024)
        assert np.array_equal(replay.fr_rand(), secret)
        replay.fr_rand()                                                             # the padding draw of vec_commit
        r0, r1 = replay.fr_rand_many(n), replay.fr_rand_many(n)
        idx = np.array(sorted(set([0, 1, n - 1] + np.random.default_rng(2).integers(0, n, 13).tolist())))
        tau_g2 = s.tau_g2()
        for g2, body, rs, vals, msgs in ((w_g2_0, w_body_0, r0, zeros, sets[0]), (w_g2_1, w_body_1, r1, ones, sets[1])):
            ect, _, ekey = oc.encap_batch(com, tau_g2, elements[idx], vals[idx], rs[idx], vb, threads=NCPU)
            assert np.array_equal(g2[idx], ect), "the points that came off the wire are not the oracle's ciphertext points"
            assert np.array_equal(body[idx], ekey ^ msgs[idx])
            assert np.array_equal(np.frombuffer(sent[0 if g2 is w_g2_0 else 1], np.uint8).reshape(n, 64 + vb)[idx, :64], model_g2_bytes(ect))
        # Receiver::receive on what came off the wire: the known inputs, and the oracle's pairing on sampled items
        pick0 = bits[:, None] == 0
        sel_g2, sel_body = np.where(pick0, w_g2_0, w_g2_1), np.where(pick0, w_body_0, w_body_1)
        chosen = np.where(pick0, sets[0], sets[1])
        assert np.array_equal(K.vec_decrypt_arrays(s, proofs[:n], sel_g2, sel_body), chosen)
        _, dkey = oc.decap_batch(proofs[idx], sel_g2[idx], vb, threads=NCPU)
        assert np.array_equal(dkey ^ sel_body[idx], chosen[idx])
    finally:
        s.close()
    import laconic_ot
    from keaki_amd.dist import Shard
    plain = laconic_ot.run_flow(K, Shard(0, 1, None), 0, log2n)
    rep = laconic_ot.run_flow(K, Shard(0, 1, None), 0, log2n, wire="compressed")
    assert plain["all_messages_recovered"] and "wire" not in plain
    assert rep["all_messages_recovered"] and rep["wire_round_trip_exact"]
    assert rep["wire_bytes"] == 2 * n * (64 + vb) and rep["wire_point_bytes"] == 2 * n * 64 and rep["uncompressed_point_bytes"] == 2 * n * 128
