"""The host layer of the set batch verification (keaki_amd/host: kzg::verify_sets, vec::vec_verify_subsets) through keaki_amd/keaki.py: what
open_set / vec_open_subset produce is accepted, the verdict is the AND of verify_set / vec_verify_subset per item, items of unequal size are
grouped, the rng is consumed one draw per item, and the layer refuses what the device library leaves to its caller. The setup comes from a KNOWN
tau; the model (tests/verify_sets_model.py) supplies proofs that do not come from the library."""
import numpy as np
import pytest

import verify_sets_model as M
from conftest import rand_fr_ints

pytestmark = pytest.mark.gpu

R = M.R
TAU = rand_fr_ints(1, 780)[0]
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


def draws_taken(K, call, n):
    """the call consumed exactly n draws of its rng"""
    a, b = K.Rng(9), K.Rng(9)
    call(a)
    for _ in range(n):
        b.fr_rand()
    return np.array_equal(a.fr_rand(), b.fr_rand())


def mixed_items(oc, seed):
    """seven valid items of 2, 4, 2, 1, 4, 16 and 2 points, each with a polynomial and a commitment of its own; proofs by long division (the model)"""
    ks = [2, 4, 2, 1, 4, 16, 2]
    items = []
    for i, k in enumerate(ks):
        r = rand_fr_ints(2 * k + 3, seed + i)
        c = M.valid_case(TAU, [r[k:]], [r[:k]], [1])
        items.append(c)
    coms, proofs = g1_of(oc, [c.com[0] for c in items]), g1_of(oc, [c.q[0] for c in items])
    return items, coms, proofs, [mont(oc, c.z[0]) for c in items], [mont(oc, c.y[0]) for c in items]


def test_mixed_sizes_are_grouped_and_agree_with_verify_set(K, oc, setup):
    items, coms, proofs, zs, ys = mixed_items(oc, 300)
    n = len(items)
    singles = [K.verify_set(setup, coms[i], zs[i], ys[i], proofs[i]) for i in range(n)]
    assert all(singles)
    assert K.verify_sets(K.Rng(1), setup, coms, zs, ys, proofs)
    assert draws_taken(K, lambda rng: K.verify_sets(rng, setup, coms, zs, ys, proofs), n)
    for bad_item in (1, 5, 6):                    # one item of a group of two, the group of one, the last of a group of three
        bad = [y.copy() for y in ys]
        bad[bad_item][0] = mont(oc, [items[bad_item].y[0][0] + 1])[0]
        singles = [K.verify_set(setup, coms[i], zs[i], bad[i], proofs[i]) for i in range(n)]
        assert singles == [i != bad_item for i in range(n)]
        assert not K.verify_sets(K.Rng(1), setup, coms, zs, bad, proofs)
        assert draws_taken(K, lambda rng: K.verify_sets(rng, setup, coms, zs, bad, proofs), n), "one draw per item, whatever the verdict"
    swapped = proofs.copy()
    swapped[[0, 2]] = swapped[[2, 0]]             # two items of ONE group: the grouping keeps each proof with its item
    assert not K.verify_sets(K.Rng(1), setup, coms, zs, ys, swapped)
    # a wrong point
    badz = [z.copy() for z in zs]
    badz[4][3] = mont(oc, [items[4].z[0][3] + 1])[0]
    assert not K.verify_sets(K.Rng(1), setup, coms, badz, ys, proofs)
    # no items: true, nothing drawn
    assert K.verify_sets(K.Rng(1), setup, coms[:1], [], [], np.zeros((0, 8), np.uint64))
    assert draws_taken(K, lambda rng: K.verify_sets(rng, setup, coms[:1], [], [], np.zeros((0, 8), np.uint64)), 0)


def test_proofs_of_open_set_with_one_commitment(K, oc, setup):
    p = mont(oc, rand_fr_ints(20, 41))
    com = K.commit(setup, p)
    rows = [mont(oc, rand_fr_ints(k, 50 + i)) for i, k in enumerate([3, 3, 7, 3])]
    opened = [K.open_set(setup, p, z) for z in rows]
    proofs, ys = np.stack([o[0] for o in opened]), [o[1] for o in opened]
    assert K.verify_sets(K.Rng(2), setup, com.reshape(1, 8), rows, ys, proofs)
    ys[2][6] = mont(oc, [12345])[0]
    assert not K.verify_sets(K.Rng(2), setup, com.reshape(1, 8), rows, ys, proofs)


def test_vec_open_subset_then_vec_verify_subsets(K, oc, setup):
    d = 64
    v = rand_fr_ints(d - 1, 640)
    vm = mont(oc, v)
    com, proofs = K.vec_commit(K.Rng(21), setup, vm)
    evals = np.concatenate([vm, K.Rng(21).fr_rand().reshape(1, 4)])
    rows = [[0, 63, 5], [1, 2, 3, 4, 62], [7, 9, 11], [33], [63, 0, 31, 32, 1], list(range(16))]
    n = len(rows)
    sub = np.stack([K.vec_open_subset(setup, d, r, proofs) for r in rows])
    vals = [evals[np.array(r)] for r in rows]
    assert all(K.vec_verify_subset(setup, com, d, rows[i], vals[i], sub[i]) for i in range(n))
    assert K.vec_verify_subsets(K.Rng(5), setup, com, d, rows, vals, sub)
    assert draws_taken(K, lambda rng: K.vec_verify_subsets(rng, setup, com, d, rows, vals, sub), n)
    bad = [x.copy() for x in vals]
    bad[4][2] = mont(oc, [v[31] + 1])[0]
    singles = [K.vec_verify_subset(setup, com, d, rows[i], bad[i], sub[i]) for i in range(n)]
    assert singles == [i != 4 for i in range(n)]
    assert not K.vec_verify_subsets(K.Rng(5), setup, com, d, rows, bad, sub)
    moved = [list(r) for r in rows]
    moved[2][1] = 10                              # another position with the old value
    assert not K.vec_verify_subsets(K.Rng(5), setup, com, d, moved, vals, sub)


def test_refusals(K, oc, setup):
    items, coms, proofs, zs, ys = mixed_items(oc, 400)
    assert K.verify_sets(K.Rng(1), setup, coms, zs, ys, proofs)
    rep = [z.copy() for z in zs]
    rep[1][3] = rep[1][0]
    big = mont(oc, rand_fr_ints(17, 401))
    plain = K.KZGSetup.setup(mont(oc, [TAU])[0], MAX_D)
    group_dev = K.Device([0, 0])
    group = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET, device=group_dev)
    z8 = np.zeros((1, 8), np.uint64)
    one = lambda k: [np.zeros((k, 4), np.uint64)]
    try:
        for name, call in [
            ("a repeated point", lambda: K.verify_sets(K.Rng(1), setup, coms, rep, ys, proofs)),
            ("an empty set", lambda: K.verify_sets(K.Rng(1), setup, z8, [np.zeros((0, 4), np.uint64)], [np.zeros((0, 4), np.uint64)], z8)),
            ("a value too few", lambda: K.verify_sets(K.Rng(1), setup, coms, zs, [y[:-1] if i == 1 else y for i, y in enumerate(ys)], proofs)),
            ("a proof too few", lambda: K.verify_sets(K.Rng(1), setup, coms, zs, ys, proofs[:-1])),
            ("two commitments for seven items", lambda: K.verify_sets(K.Rng(1), setup, coms[:2], zs, ys, proofs)),
            ("no G2 powers", lambda: K.verify_sets(K.Rng(1), plain, coms, zs, ys, proofs)),
            ("[tau^17]_2 beyond the G2 powers", lambda: K.verify_sets(K.Rng(1), setup, z8, [big], [big], z8)),
            ("65 points", lambda: K.verify_sets(K.Rng(1), setup, z8, [mont(oc, list(range(1, 66)))], one(65), z8)),
            ("a device group", lambda: K.verify_sets(K.Rng(1), group, coms, zs, ys, proofs)),
            ("subsets: a repeated index", lambda: K.vec_verify_subsets(K.Rng(1), setup, coms[0], 16, [[1, 2, 1]], one(3), z8)),
            ("subsets: an index outside the domain", lambda: K.vec_verify_subsets(K.Rng(1), setup, coms[0], 16, [[1, 16]], one(2), z8)),
            ("subsets: a value too few", lambda: K.vec_verify_subsets(K.Rng(1), setup, coms[0], 16, [[1, 2]], one(1), z8)),
            ("subsets: a proof too few", lambda: K.vec_verify_subsets(K.Rng(1), setup, coms[0], 16, [[1, 2], [3]], one(2) + one(1), z8)),
            ("subsets: no G2 powers", lambda: K.vec_verify_subsets(K.Rng(1), plain, coms[0], 16, [[1, 2]], one(2), z8)),
            ("subsets: a device group", lambda: K.vec_verify_subsets(K.Rng(1), group, coms[0], 16, [[1, 2]], one(2), z8)),
        ]:
            with pytest.raises(K.SetError):
                call()
                pytest.fail(name)
    finally:
        group.close()
        group_dev.close()
        plain.close()
    assert K.verify_sets(K.Rng(1), setup, coms, zs, ys, proofs), "the setup is still usable"
