"""The host layer of the KZG set openings (keaki_amd/host: kzg::open_set / verify_set / aggregate_proofs, kem::encapsulate_set, enc::encrypt_set,
vec::vec_open_subset / vec_verify_subset / vec_encrypt_subset_batch, KZGSetup with G2 powers) through keaki_amd/keaki.py. The setup comes from a
KNOWN tau (setup_with_g2), so expected proofs are (q(tau)) x G with q from the model's long division (tests/kzg_set_model.py) and expected keys are
the oracle's KDF of e(r (C - I(tau) G), g2); r is what Fr::rand draws from the same seed."""
import os

import numpy as np
import pytest

import kzg_set_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

R = M.R
TAU = rand_fr_ints(1, 777)[0]
MAX_D, MAX_SET = 128, 64
PTAU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppot_0080_01.ptau.test")


@pytest.fixture(scope="module")
def K():
    from keaki_amd import keaki as K
    return K


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def unmont(oc, a):
    return oc.limbs_to_ints(oc.fr_from_mont(np.ascontiguousarray(a, np.uint64).reshape(-1, 4)))


def g1_of(oc, dls):
    return oc.g1_mul_batch(oc.generators()[0], mont(oc, dls))


@pytest.fixture(scope="module")
def setups(K, oc):
    with_g2 = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET)
    without = K.KZGSetup.setup(mont(oc, [TAU])[0], MAX_D)
    yield with_g2, without
    with_g2.close(); without.close()


def case(n, k, seed):
    r = rand_fr_ints(n + k, seed)
    p, zs = r[:n], r[n:]
    q, ys = M.quotient_long_division(p, zs)
    return p, zs, ys, M.poly_eval(q, TAU)


def test_setup_with_g2_powers(K, oc, setups):
    s, without = setups
    g2 = s.g2_pow()
    assert g2.shape == (MAX_SET + 1, 16) and without.g2_pow().shape == (0, 16)
    want = oc.g2_mul_batch(oc.generators()[1], mont(oc, [pow(TAU, i, R) for i in range(MAX_SET + 1)]))
    assert np.array_equal(g2, want) and np.array_equal(g2[1], s.tau_g2()) and np.array_equal(without.tau_g2(), s.tau_g2())
    assert np.array_equal(s.g1_pow(), without.g1_pow())
    again = K.KZGSetup.from_powers_g2(s.g1_pow(), g2)
    assert np.array_equal(again.g2_pow(), g2) and np.array_equal(again.tau_g2(), s.tau_g2())
    again.close()


def test_ptau_loader_keeps_section_3(K, py):
    plain, kept = K.KZGSetup.new_from_file(PTAU), K.KZGSetup.new_from_file_g2(PTAU)
    info = K.ptau_parse(PTAU)
    assert plain.g2_pow().shape[0] == 0
    g2 = kept.g2_pow()
    assert g2.shape[0] == 1 << info["power"] and np.array_equal(g2, info["tau_g2"]) and np.array_equal(g2[1], plain.tau_g2()) and np.array_equal(kept.tau_g2(), plain.tau_g2())
    assert np.array_equal(kept.g1_pow(), plain.g1_pow())
    plain.close(); kept.close()


@pytest.mark.parametrize("n,k", [(1, 1), (9, 9), (10, 9), (33, 8), (100, 17), (128, 64)])
def test_open_set_verify_set_aggregate(K, oc, setups, n, k):
    s, _ = setups
    p, zs, ys, dl = case(n, k, 50 * n + k)
    pm, zm = mont(oc, p), mont(oc, zs)
    proof, vals = K.open_set(s, pm, zm)
    assert unmont(oc, vals) == ys and np.array_equal(proof, g1_of(oc, [dl])[0])
    com = K.commit(s, pm)
    assert K.verify_set(s, com, zm, vals, proof)
    bad = vals.copy(); bad[k // 2] = mont(oc, [ys[k // 2] + 1])[0]
    assert not K.verify_set(s, com, zm, bad, proof)
    singles = np.stack([K.open(s, pm, z) for z in zm])
    assert np.array_equal(K.aggregate_proofs(s, zm, singles), proof), "byte for byte"
    if k == 1:
        assert np.array_equal(proof, singles[0])


@pytest.mark.parametrize("msg_len", [1, 32, 100])
def test_encapsulate_set_and_encrypt_set(K, oc, setups, msg_len):
    s, _ = setups
    n, k = 100, 9
    p, zs, ys, dl = case(n, k, 900 + msg_len)
    pm, zm, ym = mont(oc, p), mont(oc, zs), mont(oc, ys)
    com = K.commit(s, pm)
    seed = 4000 + msg_len
    r = unmont(oc, K.Rng(seed).fr_rand())[0]                  # the ONE draw encapsulate_set makes
    rng = K.Rng(seed)
    ct, key = K.encapsulate_set(rng, s, com, zm, ym, msg_len)
    assert np.array_equal(rng.fr_rand(), K.Rng(seed).fr_rand_many(2)[1]), "exactly one draw"
    a_dl = (M.poly_eval(p, TAU) - M.poly_eval(M.interpolant(zs, ys), TAU)) % R
    g2 = oc.generators()[1]
    _, want_key = oc.decap_batch(g1_of(oc, [r * a_dl]), g2.reshape(1, 16), msg_len)
    assert key == want_key[0].tobytes(), "the oracle's KDF of e(r (C - I(tau) G), g2)"
    assert np.array_equal(ct, oc.g2_mul_batch(g2, mont(oc, [r * M.poly_eval(M.vanishing(zs), TAU)]))[0]), "ct = r [Z(tau)]_2"
    proof, _ = K.open_set(s, pm, zm)
    assert K.decapsulate(s, proof, ct, msg_len) == key, "the unchanged decapsulate with the set proof"
    bad_y = list(ys); bad_y[4] = (bad_y[4] + 1) % R           # the proof a vector with one other value would hold opens another key
    bad_dl = (M.poly_eval(p, TAU) - M.poly_eval(M.interpolant(zs, bad_y), TAU)) * M.inv(M.poly_eval(M.vanishing(zs), TAU)) % R
    assert K.decapsulate(s, g1_of(oc, [bad_dl])[0], ct, msg_len) != key
    msg = bytes((7 * i + msg_len) & 0xFF for i in range(msg_len))
    c2 = K.encrypt_set(K.Rng(seed), s, com, zm, ym, msg)
    assert np.array_equal(c2[0], ct) and c2[1] == bytes(a ^ b for a, b in zip(key, msg))
    assert K.decrypt(s, proof, c2) == msg


def test_vec_subset_open_and_verify_from_vec_commit(K, oc, setups):
    """d = 64: the set proof aggregated from vec_commit's proofs equals open_set on the vector's polynomial, byte for byte"""
    s, _ = setups
    v = rand_fr_ints(63, 63)
    vm = mont(oc, v)
    com, proofs = K.vec_commit(K.Rng(11), s, vm)
    assert proofs.shape[0] == 64
    pad = K.Rng(11).fr_rand()
    coeffs = K.ifft(np.concatenate([vm, pad.reshape(1, 4)]), 64)
    omega = unmont(oc, K.domain_elements(64))
    for idx in ([5], [0, 63], [3, 17, 40, 41, 62, 1, 2, 9, 33]):
        proof = K.vec_open_subset(s, 64, idx, proofs)
        want, vals = K.open_set(s, coeffs, mont(oc, [omega[i] for i in idx]))
        assert np.array_equal(proof, want), idx
        held = [(v + unmont(oc, pad))[i] for i in idx]
        assert unmont(oc, vals) == held
        assert K.vec_verify_subset(s, com, 64, idx, mont(oc, held), proof)
        other = list(held); other[-1] = (other[-1] + 1) % R
        assert not K.vec_verify_subset(s, com, 64, idx, mont(oc, other), proof)


def test_vec_encrypt_subset_batch_all_tuples(K, oc, setups):
    """k = 3, all 8 value tuples at d = 16: exactly the tuple the vector holds decrypts, and every item equals encrypt_set alone with the same r"""
    s, _ = setups
    bits = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0]
    com, proofs = K.vec_commit(K.Rng(5), s, mont(oc, bits))
    assert proofs.shape[0] == 16
    idx = [2, 7, 12]
    held = tuple(bits[i] for i in idx)
    tuples = [((t >> 2) & 1, (t >> 1) & 1, t & 1) for t in range(8)]
    values = np.stack([mont(oc, list(t)) for t in tuples])
    msgs = np.frombuffer(np.random.default_rng(3).bytes(8 * 32), np.uint8).reshape(8, 32)
    ct, body = K.vec_encrypt_subset_batch(K.Rng(99), s, com, 16, idx, values, msgs)
    proof = K.vec_open_subset(s, 16, idx, proofs)
    omega = K.domain_elements(16)
    opened = [K.decrypt(s, proof, (ct[i], body[i].tobytes())) == msgs[i].tobytes() for i in range(8)]
    assert opened == [t == held for t in tuples]
    for i in range(8):
        rng = K.Rng(99)
        if i:
            rng.fr_rand_many(i)                               # the batch draws one r per item in index order
        alone = K.encrypt_set(rng, s, com, omega[idx], values[i], msgs[i].tobytes())
        assert np.array_equal(alone[0], ct[i]) and alone[1] == body[i].tobytes(), i


def test_refusals(K, oc, setups):
    """a setup without G2 powers, a repeated point, a repeated index, bad sizes: SetError, no draw from the rng, and the setup works afterwards"""
    s, without = setups
    p, zs, ys, dl = case(40, 5, 1234)
    pm, zm, ym = mont(oc, p), mont(oc, zs), mont(oc, ys)
    com = K.commit(s, pm)
    proof, _ = K.open_set(without, pm, zm)                    # open_set and aggregate need no G2 powers
    assert np.array_equal(proof, g1_of(oc, [dl])[0])
    rng = K.Rng(1)
    for call in (lambda: K.verify_set(without, com, zm, ym, proof),
                 lambda: K.encapsulate_set(rng, without, com, zm, ym, 32),
                 lambda: K.encrypt_set(rng, without, com, zm, ym, b"abc"),
                 lambda: K.vec_verify_subset(without, com, 16, [1, 2], ym[:2], proof),
                 lambda: K.vec_encrypt_subset_batch(rng, without, com, 16, [1, 2], ym[:2].reshape(1, 2, 4), np.zeros((1, 8), np.uint8))):
        with pytest.raises(K.SetError, match="G2 powers"):
            call()
    dup = zm.copy(); dup[3] = dup[0]
    for call in (lambda: K.open_set(s, pm, dup), lambda: K.verify_set(s, com, dup, ym, proof), lambda: K.aggregate_proofs(s, dup, np.stack([proof] * 5)),
                 lambda: K.encapsulate_set(rng, s, com, dup, ym, 32), lambda: K.vec_open_subset(s, 16, [4, 9, 4], np.stack([proof] * 16)),
                 lambda: K.vec_encrypt_subset_batch(rng, s, com, 16, [1, 1], ym[:2].reshape(1, 2, 4), np.zeros((1, 8), np.uint8))):
        with pytest.raises(K.SetError, match="repeated"):
            call()
    with pytest.raises(K.SetError):
        K.open_set(s, pm, np.zeros((0, 4), np.uint64))
    with pytest.raises(K.SetError):
        K.verify_set(s, com, mont(oc, rand_fr_ints(MAX_SET + 2, 9))[:1025], ym, proof)
    with pytest.raises(K.SetError):
        K.vec_open_subset(s, 16, [16], np.stack([proof] * 16))
    assert np.array_equal(rng.fr_rand(), K.Rng(1).fr_rand()), "a refused call draws nothing"
    assert K.verify_set(s, com, zm, ym, proof)
    with pytest.raises(K.KZGError):
        K.open_set(s, mont(oc, rand_fr_ints(MAX_D + 2, 4)), zm)
