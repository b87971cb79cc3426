"""The host layer of the coset batch verification (keaki_amd/host: kzg::verify_cosets, vec::vec_verify_cosets, vec::vec_verify_cosets_subset)
through keaki_amd/keaki.py: what vec_open_cosets produces is accepted, one changed evaluation is not, and the layer refuses what the device
library leaves to its caller. The setup comes from a KNOWN tau; the model (tests/coset_verify_model.py) supplies proofs that do not come from
the library."""
import numpy as np
import pytest

import coset_verify_model as M
import fk_coset_model as FM
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


@pytest.mark.parametrize("d,l", [(64, 4), (64, 16), (32, 1), (16, 16)])
def test_vec_open_cosets_then_vec_verify_cosets(K, oc, setup, d, l):
    r = d // l
    v = rand_fr_ints(d - 1, 640 + d + l)
    vm = mont(oc, v)
    com, _ = K.vec_commit(K.Rng(21), setup, vm)
    evals = np.concatenate([vm, K.Rng(21).fr_rand().reshape(1, 4)])
    proofs = K.vec_open_cosets(setup, evals, l)
    assert K.vec_verify_cosets(K.Rng(5), setup, com, evals, l, proofs)
    bad = evals.copy()
    bad[7] = mont(oc, [v[7] + 1])[0]
    assert not K.vec_verify_cosets(K.Rng(5), setup, com, bad, l, proofs), "one changed evaluation"
    if r > 1:
        swapped = proofs.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        assert not K.vec_verify_cosets(K.Rng(5), setup, com, evals, l, swapped)
    # some of the cosets, listed in any order
    pick = [r - 1, 0] if r > 1 else [0]
    rows = np.stack([evals[K.vec_coset_indices(d, l, i).astype(np.int64)] for i in pick])
    assert K.vec_verify_cosets_subset(K.Rng(6), setup, com, d, l, pick, rows, proofs[pick])
    if r > 1:
        assert not K.vec_verify_cosets_subset(K.Rng(6), setup, com, d, l, pick, rows[::-1], proofs[pick])
    # the draws: one per coset in index order, whatever the verdict
    a, b = K.Rng(9), K.Rng(9)
    K.vec_verify_cosets(a, setup, com, evals, l, proofs)
    for _ in range(r):
        b.fr_rand()
    assert np.array_equal(a.fr_rand(), b.fr_rand())


def test_verify_cosets_on_the_models_items(K, oc, setup):
    """shifts that are no roots of unity, one commitment per item, proofs by long division (the model)"""
    n, l = 7, 8
    rnd = rand_fr_ints(n + n * 20, 91)
    c = M.valid_case(TAU, [rnd[n + 20 * k:n + 20 * (k + 1)] for k in range(n)], rnd[:n], l, [1] * n)
    coms, proofs = g1_of(oc, c.com), g1_of(oc, c.q)
    vals = mont(oc, [y for row in c.y for y in row])
    assert K.verify_cosets(K.Rng(1), setup, coms, mont(oc, c.h), l, vals, proofs)
    vals[3 * l + l - 1] = mont(oc, [c.y[3][l - 1] + 1])[0]
    assert not K.verify_cosets(K.Rng(1), setup, coms, mont(oc, c.h), l, vals, proofs)


def test_refusals(K, oc, setup):
    n, l = 3, 4
    rnd = rand_fr_ints(n + 12, 92)
    c = M.valid_case(TAU, [rnd[n:]], rnd[:n], l, [1] * n)
    com, proofs, h = g1_of(oc, c.com), g1_of(oc, c.q), mont(oc, c.h)
    vals = mont(oc, [y for row in c.y for y in row])
    assert K.verify_cosets(K.Rng(1), setup, com, h, l, vals, proofs)
    zero = h.copy()
    zero[1] = 0
    plain = K.KZGSetup.setup(mont(oc, [TAU])[0], MAX_D)
    group_dev = K.Device([0, 0])
    group = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET, device=group_dev)
    try:
        for name, call in [
            ("a zero shift", lambda: K.verify_cosets(K.Rng(1), setup, com, zero, l, vals, proofs)),
            ("l = 3", lambda: K.verify_cosets(K.Rng(1), setup, com, h, 3, vals[:9], proofs)),
            ("no G2 powers", lambda: K.verify_cosets(K.Rng(1), plain, com, h, l, vals, proofs)),
            ("[tau^l]_2 beyond the G2 powers", lambda: K.verify_cosets(K.Rng(1), setup, com, h[:1], 32, np.zeros((32, 4), np.uint64), proofs[:1])),
            ("a device group", lambda: K.verify_cosets(K.Rng(1), group, com, h, l, vals, proofs)),
            ("a device group, vector form", lambda: K.vec_verify_cosets(K.Rng(1), group, com[0], np.zeros((16, 4), np.uint64), 4, np.zeros((4, 8), np.uint64))),
            ("sizes", lambda: K.verify_cosets(K.Rng(1), setup, com, h, l, vals[:-1], proofs)),
            ("vector: l = 3", lambda: K.vec_verify_cosets(K.Rng(1), setup, com[0], np.zeros((16, 4), np.uint64), 3, np.zeros((4, 8), np.uint64))),
            ("vector: proofs", lambda: K.vec_verify_cosets(K.Rng(1), setup, com[0], np.zeros((16, 4), np.uint64), 4, np.zeros((3, 8), np.uint64))),
            ("subset: coset index", lambda: K.vec_verify_cosets_subset(K.Rng(1), setup, com[0], 16, 4, [4], np.zeros((4, 4), np.uint64), np.zeros((1, 8), np.uint64))),
        ]:
            with pytest.raises(K.SetError):
                call()
                pytest.fail(name)
    finally:
        group.close()
        group_dev.close()
        plain.close()
    assert K.verify_cosets(K.Rng(1), setup, com, h, l, vals, proofs), "the setup is still usable"
