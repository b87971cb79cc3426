"""The host layer of the per-coset verdicts and of encryption to cosets (keaki_amd/host: vec::vec_verify_cosets_each, vec_verify_cosets_each_subset,
vec_encrypt_cosets) through keaki_amd/keaki.py: what vec_open_cosets produces is valid coset by coset, one changed evaluation marks exactly its
coset, a message encrypted to a coset's values opens with that coset's proof and no other, every item is encrypt_set alone with the same r, and the
ciphertext and key are what the oracle computes from the known tau. Refusals leave the Rng untouched."""
import numpy as np
import pytest

import coset_verify_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

R = M.R
TAU = rand_fr_ints(1, 779)[0]
MAX_D, MAX_SET = 64, 16


@pytest.fixture(scope="module")
def K():
    from keaki_amd import keaki as K
    return K


def mont(oc, ints):
    return oc.fr_to_mont(oc.ints_to_limbs([x % R for x in ints]))


def unmont(oc, a):
    return oc.limbs_to_ints(oc.fr_from_mont(np.ascontiguousarray(a, np.uint64).reshape(-1, 4)))


def g1_of(oc, dls):
    out = oc.g1_mul_batch(oc.generators()[0], mont(oc, dls)).copy()
    for i, x in enumerate(dls):
        if x % R == 0:
            out[i] = 0
    return out


@pytest.fixture(scope="module")
def setup(K, oc):
    s = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET)
    yield s
    s.close()


def committed_vector(K, oc, setup, d, seed):
    """(com, the d evaluations the commitment holds as Montgomery limbs, the same as integers)"""
    v = rand_fr_ints(d - 1, seed)
    vm = mont(oc, v)
    com, _ = K.vec_commit(K.Rng(21), setup, vm)
    pad = K.Rng(21).fr_rand()
    evals = np.concatenate([vm, pad.reshape(1, 4)])
    return com, evals, v + unmont(oc, pad)


@pytest.mark.parametrize("d,l", [(64, 4), (64, 16), (32, 1), (16, 16)])
def test_vec_open_cosets_then_verdicts(K, oc, setup, d, l):
    r = d // l
    com, evals, held = committed_vector(K, oc, setup, d, 640 + d + l)
    proofs = K.vec_open_cosets(setup, evals, l)
    st = K.vec_verify_cosets_each(setup, com, evals, l, proofs)
    assert st.shape == (r,) and not st.any()
    bad = evals.copy()
    bad[7] = mont(oc, [held[7] + 1])[0]                           # position 7 = 7 mod r + t r: coset 7 mod r
    st = K.vec_verify_cosets_each(setup, com, bad, l, proofs)
    assert list(np.nonzero(st)[0]) == [7 % r]
    if r > 1:
        swapped = proofs.copy()
        swapped[[0, r - 1]] = swapped[[r - 1, 0]]
        assert list(np.nonzero(K.vec_verify_cosets_each(setup, com, evals, l, swapped))[0]) == [0, r - 1]
    pick = [r - 1, 0] if r > 1 else [0]
    rows = np.stack([evals[K.vec_coset_indices(d, l, i).astype(np.int64)] for i in pick])
    assert not K.vec_verify_cosets_each_subset(setup, com, d, l, pick, rows, proofs[pick]).any()
    if r > 1:
        assert K.vec_verify_cosets_each_subset(setup, com, d, l, pick, rows[::-1], proofs[pick]).all()
        one = rows.copy()
        one[1, l - 1] = mont(oc, [5])[0]
        assert list(K.vec_verify_cosets_each_subset(setup, com, d, l, pick, one, proofs[pick])) == [0, 1]


@pytest.mark.parametrize("d,l", [(64, 4), (64, 16), (16, 16)])
def test_encrypt_to_all_cosets_and_decrypt(K, oc, setup, d, l):
    r = d // l
    com, evals, held = committed_vector(K, oc, setup, d, 900 + d + l)
    proofs = K.vec_open_cosets(setup, evals, l)
    cosets = list(range(r))
    rows = np.stack([evals[K.vec_coset_indices(d, l, i).astype(np.int64)] for i in cosets])
    msgs = np.frombuffer(np.random.default_rng(d + l).bytes(r * 32), np.uint8).reshape(r, 32)
    rng = K.Rng(77)
    ct, body = K.vec_encrypt_cosets(rng, setup, com, d, l, cosets, rows, msgs)
    assert ct.shape == (r, 16) and body.shape == (r, 32)
    assert np.array_equal(rng.fr_rand(), K.Rng(77).fr_rand_many(r + 1)[r]), "one draw per item"
    got = K.vec_decrypt(setup, proofs, [(ct[i], body[i].tobytes()) for i in range(r)])
    assert [bytes(g) for g in got] == [msgs[i].tobytes() for i in range(r)]
    if r > 1:
        assert K.decrypt(setup, proofs[1], (ct[0], body[0].tobytes())) != msgs[0].tobytes(), "a proof of another coset"
    # every item is encrypt_set alone on the coset's points with the same r
    omega = K.domain_elements(d)
    rs = unmont(oc, K.Rng(77).fr_rand_many(r))
    wd = M.omega(d)
    g2 = oc.generators()[1]
    for i in sorted({0, r - 1, r // 2}):
        one = K.Rng(77)
        if i:
            one.fr_rand_many(i)
        idx = K.vec_coset_indices(d, l, i).astype(np.int64)
        alone = K.encrypt_set(one, setup, com, omega[idx], rows[i], msgs[i].tobytes())
        assert np.array_equal(alone[0], ct[i]) and alone[1] == body[i].tobytes(), i
        # the oracle: ct = (r (tau^l - c)) G2, key = KDF(e((r dl(A)) G1, g2)), dl(A) = q_i (tau^l - c) for the valid item
        c_i = pow(wd, i * l, R)
        assert np.array_equal(ct[i], oc.g2_mul_batch(g2, mont(oc, [rs[i] * (pow(TAU, l, R) - c_i)]))[0]), i
        coeffs = unmont(oc, K.ifft(evals, d))
        a_dl = (M.FM.poly_eval(coeffs, TAU) - M.FM.poly_eval(M.interpolant_coset(pow(wd, i, R), [held[k] for k in idx]), TAU)) % R
        _, key = oc.decap_batch(g1_of(oc, [rs[i] * a_dl]), g2.reshape(1, 16), 32)
        assert body[i].tobytes() == bytes(a ^ b for a, b in zip(key[0].tobytes(), msgs[i].tobytes())), i


def test_a_subset_of_cosets_and_wrong_values(K, oc, setup):
    """two ciphertexts for coset 5 of (64, 4): one to the values the vector holds, one to values that differ in one entry; key-only form (msg_len 0)"""
    d, l = 64, 4
    com, evals, held = committed_vector(K, oc, setup, d, 64)
    proofs = K.vec_open_cosets(setup, evals, l)
    idx = K.vec_coset_indices(d, l, 5).astype(np.int64)
    right = [held[k] for k in idx]
    wrong = list(right); wrong[2] = (wrong[2] + 1) % R
    rows = np.stack([mont(oc, wrong), mont(oc, right)])
    msgs = np.frombuffer(np.random.default_rng(8).bytes(2 * 32), np.uint8).reshape(2, 32)
    ct, body = K.vec_encrypt_cosets(K.Rng(31), setup, com, d, l, [5, 5], rows, msgs)
    assert K.decrypt(setup, proofs[5], (ct[1], body[1].tobytes())) == msgs[1].tobytes()
    assert K.decrypt(setup, proofs[5], (ct[0], body[0].tobytes())) != msgs[0].tobytes()
    ct0, body0 = K.vec_encrypt_cosets(K.Rng(31), setup, com, d, l, [5, 5], rows, np.zeros((2, 0), np.uint8))
    assert np.array_equal(ct0, ct) and body0.shape == (2, 0)


def test_refusals_leave_the_rng_untouched(K, oc, setup):
    d, l = 16, 4
    com, evals, _ = committed_vector(K, oc, setup, d, 16)
    rows = np.stack([evals[K.vec_coset_indices(d, l, i).astype(np.int64)] for i in range(4)])
    msgs = np.zeros((4, 8), np.uint8)
    plain = K.KZGSetup.setup(mont(oc, [TAU])[0], MAX_D)
    group_dev = K.Device([0, 0])
    group = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET, device=group_dev)
    rng = K.Rng(3)
    try:
        for name, call in [
            ("no G2 powers", lambda: K.vec_encrypt_cosets(rng, plain, com, d, l, [0, 1, 2, 3], rows, msgs)),
            ("coset index", lambda: K.vec_encrypt_cosets(rng, setup, com, d, l, [0, 1, 2, 4], rows, msgs)),
            ("l = 3", lambda: K.vec_encrypt_cosets(rng, setup, com, d, 3, [0], rows[0, :3], msgs[:1])),
            ("a device group", lambda: K.vec_encrypt_cosets(rng, group, com, d, l, [0, 1, 2, 3], rows, msgs)),
            ("sizes", lambda: K.vec_encrypt_cosets(rng, setup, com, d, l, [0, 1], rows, msgs[:2])),
            ("each: a device group", lambda: K.vec_verify_cosets_each(group, com, evals, l, np.zeros((4, 8), np.uint64))),
            ("each: no G2 powers", lambda: K.vec_verify_cosets_each(plain, com, evals, l, np.zeros((4, 8), np.uint64))),
            ("each: l = 3", lambda: K.vec_verify_cosets_each(setup, com, evals, 3, np.zeros((4, 8), np.uint64))),
            ("each: proofs", lambda: K.vec_verify_cosets_each(setup, com, evals, l, np.zeros((3, 8), np.uint64))),
            ("each subset: coset index", lambda: K.vec_verify_cosets_each_subset(setup, com, d, l, [4], rows[:1], np.zeros((1, 8), np.uint64))),
        ]:
            with pytest.raises(K.SetError):
                call()
                pytest.fail(name)
        assert np.array_equal(rng.fr_rand(), K.Rng(3).fr_rand()), "a refusal drew from the rng"
    finally:
        group.close()
        group_dev.close()
        plain.close()
    ct, _ = K.vec_encrypt_cosets(K.Rng(3), setup, com, d, l, [0, 1, 2, 3], rows, msgs)
    assert ct.shape == (4, 16), "the setup is still usable"
