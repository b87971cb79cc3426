"""The host layer of the per-item set calls (keaki_amd/host: kzg::set_pairs, kzg::verify_sets_each, vec::vec_verify_subsets_each, kem::encapsulate_sets,
enc::encrypt_sets, vec::vec_encrypt_subsets) through keaki_amd/keaki.py: items of unequal size are grouped by size and come back in item order, the
verdicts are verify_set's per item, every ciphertext equals encrypt_set alone with the same r byte for byte and opens under the unchanged decrypt with
the set proof, one r is drawn per item in index order, and every refusal comes before any draw. The setup comes from a KNOWN tau; the model
(tests/verify_sets_model.py) supplies proofs that do not come from the library. The device of these tests forces 8-bit tables (a few MB)."""
import numpy as np
import pytest

import set_pairs_model as P
import verify_sets_model as M
from conftest import rand_fr_ints
from test_gpu_verify_sets_host import K, MAX_D, MAX_SET, TAU, draws_taken, g1_of, mixed_items, mont  # noqa: F401

pytestmark = pytest.mark.gpu
R = M.R


@pytest.fixture(scope="module")
def setup(K, oc):
    dev = K.Device(0)
    dev.hip().set_option("set_rows_wb", 8)
    dev.hip().set_option("coset_rows_wb", 8)
    s = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET, device=dev)
    yield s
    s.close()
    dev.close()


def untouched(K, call):
    """the refused call left its rng alone"""
    a, b = K.Rng(9), K.Rng(9)
    with pytest.raises(K.SetError):
        call(a)
    return np.array_equal(a.fr_rand(), b.fr_rand())


def test_mixed_sizes_are_grouped_and_the_verdicts_are_verify_sets(K, oc, setup):
    items, coms, proofs, zs, ys = mixed_items(oc, 300)
    n = len(items)
    assert K.verify_sets_each(setup, coms, zs, ys, proofs).tolist() == [0] * n
    a, z2 = K.set_pairs(setup, coms, zs, ys)
    dl = [P.pair_dl(c, 0) for c in items]
    assert np.array_equal(a, g1_of(oc, [x for x, _ in dl]))                       # in item order, whatever the grouping
    assert np.array_equal(z2, oc.g2_mul_batch(oc.generators()[1], mont(oc, [z for _, z in dl])))
    for bad_item in (1, 5, 6):                    # one item of a group of two, the group of one, the last of a group of three
        bad = [y.copy() for y in ys]
        bad[bad_item][0] = mont(oc, [items[bad_item].y[0][0] + 1])[0]
        singles = [K.verify_set(setup, coms[i], zs[i], bad[i], proofs[i]) for i in range(n)]
        assert singles == [i != bad_item for i in range(n)]
        assert K.verify_sets_each(setup, coms, zs, bad, proofs).tolist() == [1 if i == bad_item else 0 for i in range(n)]
    swapped = proofs.copy()
    swapped[[0, 2]] = swapped[[2, 0]]             # two items of ONE group: the grouping keeps each proof with its item
    assert K.verify_sets_each(setup, coms, zs, ys, swapped).tolist() == [1, 0, 1, 0, 0, 0, 0]
    assert K.verify_sets_each(setup, coms[:1], [], [], np.zeros((0, 8), np.uint64)).tolist() == []


def test_encrypt_sets_equals_encrypt_set_item_by_item_and_decrypts(K, oc, setup):
    items, coms, proofs, zs, ys = mixed_items(oc, 500)
    n = len(items)
    msgs = np.frombuffer(bytes((37 * i + j) & 255 for i in range(n) for j in range(40)), np.uint8).reshape(n, 40)
    ct, body = K.encrypt_sets(K.Rng(77), setup, coms, zs, ys, msgs)
    one = K.Rng(77)
    for i in range(n):                              # the same stream: one r per item in index order
        c1, b1 = K.encrypt_set(one, setup, coms[i], zs[i], ys[i], msgs[i].tobytes())
        assert np.array_equal(ct[i], c1) and body[i].tobytes() == b1, i
        assert K.decrypt(setup, proofs[i], (ct[i], body[i].tobytes())) == msgs[i].tobytes()
    assert draws_taken(K, lambda rng: K.encrypt_sets(rng, setup, coms, zs, ys, msgs), n)
    # a wrong claimed value seals the message against the holder of the true proof
    bad = [y.copy() for y in ys]
    bad[3][0] = mont(oc, [items[3].y[0][0] + 1])[0]
    ct2, body2 = K.encrypt_sets(K.Rng(77), setup, coms, zs, bad, msgs)
    assert K.decrypt(setup, proofs[3], (ct2[3], body2[3].tobytes())) != msgs[3].tobytes()
    assert K.decrypt(setup, proofs[2], (ct2[2], body2[2].tobytes())) == msgs[2].tobytes()
    # the keys alone
    cte, keys = K.encapsulate_sets(K.Rng(77), setup, coms, zs, ys, 40)
    assert np.array_equal(cte, ct) and np.array_equal(keys ^ msgs, body)
    one = K.Rng(77)
    for i in range(n):
        c1, k1 = K.encapsulate_set(one, setup, coms[i], zs[i], ys[i], 40)
        assert np.array_equal(cte[i], c1) and keys[i].tobytes() == k1


def test_vec_encrypt_subsets_opens_with_vec_open_subset(K, oc, setup):
    d = 64
    v = rand_fr_ints(d - 1, 641)
    vm = mont(oc, v)
    com, proofs = K.vec_commit(K.Rng(21), setup, vm)
    evals = np.concatenate([vm, K.Rng(21).fr_rand().reshape(1, 4)])
    rows = [[0, 63, 5], [1, 2, 3, 4, 62], [7, 9, 11], [33], [63, 0, 31, 32, 1], list(range(16))]
    n = len(rows)
    sub = np.stack([K.vec_open_subset(setup, d, r, proofs) for r in rows])
    vals = [evals[np.array(r)] for r in rows]
    assert K.vec_verify_subsets_each(setup, com, d, rows, vals, sub).tolist() == [0] * n
    bad = [x.copy() for x in vals]
    bad[4][2] = mont(oc, [v[31] + 1])[0]
    assert K.vec_verify_subsets_each(setup, com, d, rows, bad, sub).tolist() == [0, 0, 0, 0, 1, 0]
    msgs = np.frombuffer(bytes((11 * i + 3 * j) & 255 for i in range(n) for j in range(24)), np.uint8).reshape(n, 24)
    ct, body = K.vec_encrypt_subsets(K.Rng(8), setup, com, d, rows, vals, msgs)
    w = pow(pow(5, (R - 1) >> 28, R), (1 << 28) // d, R)
    one = K.Rng(8)
    for i in range(n):
        assert K.decrypt(setup, sub[i], (ct[i], body[i].tobytes())) == msgs[i].tobytes(), i
        c1, b1 = K.encrypt_set(one, setup, com, mont(oc, [pow(w, e, R) for e in rows[i]]), vals[i], msgs[i].tobytes())
        assert np.array_equal(ct[i], c1) and body[i].tobytes() == b1, i
    assert draws_taken(K, lambda rng: K.vec_encrypt_subsets(rng, setup, com, d, rows, vals, msgs), n)
    ctb, bodyb = K.vec_encrypt_subsets(K.Rng(8), setup, com, d, rows, bad, msgs)
    assert K.decrypt(setup, sub[4], (ctb[4], bodyb[4].tobytes())) != msgs[4].tobytes()


def test_refusals_come_before_any_draw(K, oc, setup):
    items, coms, proofs, zs, ys = mixed_items(oc, 400)
    n = len(items)
    msgs = np.zeros((n, 8), np.uint8)
    rep = [z.copy() for z in zs]
    rep[1][3] = rep[1][0]
    big = mont(oc, rand_fr_ints(17, 401))
    plain = K.KZGSetup.setup(mont(oc, [TAU])[0], MAX_D)
    group_dev = K.Device([0, 0])
    group = K.KZGSetup.setup_with_g2(mont(oc, [TAU])[0], MAX_D, MAX_SET, device=group_dev)
    z8 = np.zeros((1, 8), np.uint64)
    m1 = np.zeros((1, 8), np.uint8)
    one = lambda k: [np.zeros((k, 4), np.uint64)]
    short = [y[:-1] if i == 1 else y for i, y in enumerate(ys)]
    try:
        for name, call in [
            ("a repeated point", lambda rng: K.encrypt_sets(rng, setup, coms, rep, ys, msgs)),
            ("a value too few", lambda rng: K.encrypt_sets(rng, setup, coms, zs, short, msgs)),
            ("two commitments for seven items", lambda rng: K.encrypt_sets(rng, setup, coms[:2], zs, ys, msgs)),
            ("no G2 powers", lambda rng: K.encrypt_sets(rng, plain, coms, zs, ys, msgs)),
            ("[tau^17]_2 beyond the G2 powers", lambda rng: K.encrypt_sets(rng, setup, z8, [big], [big], m1)),
            ("65 points", lambda rng: K.encapsulate_sets(rng, setup, z8, [mont(oc, list(range(1, 66)))], one(65), 8)),
            ("a device group", lambda rng: K.encrypt_sets(rng, group, coms, zs, ys, msgs)),
            ("subsets: a repeated index", lambda rng: K.vec_encrypt_subsets(rng, setup, coms[0], 16, [[1, 2, 1]], one(3), m1)),
            ("subsets: an index outside the domain", lambda rng: K.vec_encrypt_subsets(rng, setup, coms[0], 16, [[1, 16]], one(2), m1)),
            ("subsets: a device group", lambda rng: K.vec_encrypt_subsets(rng, group, coms[0], 16, [[1, 2]], one(2), m1)),
        ]:
            assert untouched(K, call), name
        for name, call in [
            ("each: a repeated point", lambda: K.verify_sets_each(setup, coms, rep, ys, proofs)),
            ("each: a proof too few", lambda: K.verify_sets_each(setup, coms, zs, ys, proofs[:-1])),
            ("each: a device group", lambda: K.verify_sets_each(group, coms, zs, ys, proofs)),
            ("each: no G2 powers", lambda: K.verify_sets_each(plain, coms, zs, ys, proofs)),
            ("subsets each: a repeated index", lambda: K.vec_verify_subsets_each(setup, coms[0], 16, [[1, 2, 1]], one(3), z8)),
            ("subsets each: a device group", lambda: K.vec_verify_subsets_each(group, coms[0], 16, [[1, 2]], one(2), z8)),
            ("pairs: an empty set", lambda: K.set_pairs(setup, z8, [np.zeros((0, 4), np.uint64)], [np.zeros((0, 4), np.uint64)])),
        ]:
            with pytest.raises(K.SetError):
                call()
                pytest.fail(name)
    finally:
        group.close()
        group_dev.close()
        plain.close()
    assert K.verify_sets_each(setup, coms, zs, ys, proofs).tolist() == [0] * n, "the setup is still usable"
