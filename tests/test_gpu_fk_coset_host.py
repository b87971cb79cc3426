"""The host layer of the FK23 coset openings (keaki_amd/host: kzg::open_fk_cosets, vec::vec_open_cosets, vec::vec_coset_indices) through
keaki_amd/keaki.py. The setup comes from a KNOWN tau, so expected proofs are (q_i(tau)) x G with q_i from the model's division by x^l - c_i
(tests/fk_coset_model.py); a coset proof is then used as the ordinary set proof it is: vec_verify_subset and the decryption of one
vec_encrypt_subset_batch ciphertext."""
import numpy as np
import pytest

import fk_coset_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

R = M.R
TAU = rand_fr_ints(1, 778)[0]
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


def test_coset_indices(K):
    assert K.vec_coset_indices(64, 8, 3).tolist() == [3 + 8 * t for t in range(8)]
    assert K.vec_coset_indices(60, 4, 15).tolist() == [15, 31, 47, 63], "the domain of 60 entries has 64"
    assert K.vec_coset_indices(16, 16, 0).tolist() == list(range(16)) and K.vec_coset_indices(16, 1, 9).tolist() == [9]
    for d, l, i in ((64, 8, 8), (64, 3, 0), (16, 32, 0)):
        with pytest.raises(K.SetError):
            K.vec_coset_indices(d, l, i)


@pytest.mark.parametrize("d,l,n", [(64, 4, 64), (64, 16, 50), (32, 1, 32), (16, 16, 16), (8, 2, 1)])
def test_open_fk_cosets_against_long_division(K, oc, setup, d, l, n):
    p = rand_fr_ints(n, 300 + d + l)
    log2d, log2l = d.bit_length() - 1, l.bit_length() - 1
    got = K.open_fk_cosets(setup, mont(oc, p), d, l)
    assert got.shape == (d // l, 8)
    assert np.array_equal(got, g1_of(oc, M.proofs_direct(p + [0] * (d - n), log2d, log2l, TAU)))
    if n == d:                                                 # proof i is open_set's proof for the coset's points
        omega = unmont(oc, K.domain_elements(d))
        for i in (0, d // l - 1):
            zs = [omega[k] for k in M.coset_indices(d, l, i)]
            assert np.array_equal(K.open_set(setup, mont(oc, p), mont(oc, zs))[0], got[i]), i


def test_vec_open_cosets_verify_and_decrypt(K, oc, setup):
    """the holder of a vector opens every block; each proof passes vec_verify_subset with the block's values, fails with the neighbour's, and opens
    the one ciphertext of vec_encrypt_subset_batch that was made for the block's values"""
    d, l = 64, 4
    r = d // l
    v = rand_fr_ints(d - 1, 64)
    vm = mont(oc, v)
    com, single = K.vec_commit(K.Rng(21), setup, vm)
    pad = K.Rng(21).fr_rand()
    evals = np.concatenate([vm, pad.reshape(1, 4)])
    held = v + unmont(oc, pad)
    proofs = K.vec_open_cosets(setup, evals, l)
    assert proofs.shape == (r, 8)
    coeffs = unmont(oc, K.ifft(evals, d))
    assert np.array_equal(proofs, g1_of(oc, M.proofs_direct(coeffs, 6, 2, TAU)))
    for i in range(r):
        idx = K.vec_coset_indices(d, l, i)
        assert K.vec_verify_subset(setup, com, d, idx, mont(oc, [held[k] for k in idx]), proofs[i]), i
        assert np.array_equal(K.vec_open_subset(setup, d, idx, single), proofs[i]), "the aggregate of vec_commit's single proofs: the same bytes"
    idx0, idx1 = K.vec_coset_indices(d, l, 0), K.vec_coset_indices(d, l, 1)
    assert not K.vec_verify_subset(setup, com, d, idx0, mont(oc, [held[k] for k in idx1]), proofs[0])
    assert not K.vec_verify_subset(setup, com, d, idx1, mont(oc, [held[k] for k in idx1]), proofs[0])
    # two value tuples for block 5: the one the vector holds and one that differs in a single entry
    idx = K.vec_coset_indices(d, l, 5)
    right = [held[k] for k in idx]
    wrong = list(right); wrong[2] = (wrong[2] + 1) % R
    values = np.stack([mont(oc, wrong), mont(oc, right)])
    msgs = np.frombuffer(np.random.default_rng(8).bytes(2 * 32), np.uint8).reshape(2, 32)
    ct, body = K.vec_encrypt_subset_batch(K.Rng(31), setup, com, d, idx, values, msgs)
    assert K.decrypt(setup, proofs[5], (ct[1], body[1].tobytes())) == msgs[1].tobytes()
    assert K.decrypt(setup, proofs[5], (ct[0], body[0].tobytes())) != msgs[0].tobytes()
    assert K.decrypt(setup, proofs[4], (ct[1], body[1].tobytes())) != msgs[1].tobytes(), "another block's proof"


def test_refusals(K, oc, setup):
    p = mont(oc, rand_fr_ints(16, 5))
    for call in (lambda: K.open_fk_cosets(setup, p, 16, 3), lambda: K.open_fk_cosets(setup, p, 12, 4), lambda: K.open_fk_cosets(setup, p, 8, 2),
                 lambda: K.open_fk_cosets(setup, p, 16, 32), lambda: K.open_fk_cosets(setup, p, 2 * MAX_D, 2), lambda: K.vec_open_cosets(setup, p, 3),
                 lambda: K.vec_open_cosets(setup, p[:0], 1)):
        with pytest.raises(K.SetError):
            call()
    assert K.open_fk_cosets(setup, p, 16, 4).shape == (4, 8)
