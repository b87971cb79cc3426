"""The three derived tables of a G1 SRS handle (keaki_amd/csrc/api_host.h: SrsCache fk / upd / fkc, all kept by srs_cache_ensure) under the rules that
one function now owns: a REPLACE that keaki_hip_debug_set_alloc_limit refuses leaves that cache empty, its bytes off the count, the caller's
array as it was and the handle's other two caches alone; the next call builds it; and a handle freed through another context gives every
cache's bytes back to the context that built them. fk is reached through open_fk_poly, upd through vec_update, fkc through open_fk_cosets_poly.
Every table here is 192 << log2d bytes; no log2d below 3 (at 2 a table is 768 B and passes the 1,024 B limit). Expected proofs: the same call on
a fresh handle, and the oracle's literal FK23 where d <= 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SRS = 16
OOM = -3
LIMIT = 1024
SENT = np.uint64(0xDEADBEEFDEADBEEF)
# (cache, key A, key B): A is built, B is the refused replacement. fkc's second pair keeps d and changes l: the second part of the key
REPLACE = [("fk", (3,), (4,)), ("upd", (3,), (4,)), ("fkc", (4, 1), (3, 1)), ("fkc", (4, 1), (4, 2))]
KEY_A = {"fk": (3,), "upd": (3,), "fkc": (4, 1)}


def table_bytes(key):
    return 192 << key[0]


def mont(oc, ints):
    return np.ascontiguousarray(oc.fr_to_mont(oc.ints_to_limbs(ints)), np.uint64)


@pytest.fixture(scope="module")
def srs_pts(oc, rand_fr):
    """any 16 points serve as an "SRS": every expectation is the same call on a fresh handle or the oracle's literal FK23 over these points"""
    g1, _ = oc.generators()
    return oc.g1_mul_batch(g1, mont(oc, rand_fr(N_SRS, 2600)))


@pytest.fixture()
def ctx_tables():
    """an own context (its accounting starts at a known value, its allocation limit is its own) and `tables()` relative to that start"""
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    base = h.memory()["tables"]
    try:
        yield h, (lambda: h.memory()["tables"] - base)
    finally:
        h.debug_set_alloc_limit(0)
        h.close()


class Op:
    """one call that needs cache `kind` at `key`: call(h, srs, out) -> status of the C entry, out = start() or a copy of it. `pristine` is what
    out must still be after a refused call: the sentinel for the two openings, the proofs to update for vec_update (updated in place)."""

    def __init__(self, oc, py, rand_fr, kind, key, start_proofs=None):
        self.kind, self.key = kind, key
        log2d = key[0]
        d = 1 << log2d
        self.p = rand_fr(d, 2610 + log2d)
        self.pm = mont(oc, self.p)
        n2 = 2 * d >> (key[1] if kind == "fkc" else 0)                    # the transform's size: 2d, or 2r for the cosets
        w = py.fr_root_of_unity(n2)
        self.roots = [mont(oc, [x])[0] for x in (w, pow(w, -1, py.R), pow(n2, -1, py.R))]
        if kind == "upd":
            wd = w * w % py.R
            self.roots = [mont(oc, [x])[0] for x in (wd, pow(wd, -1, py.R), pow(d, -1, py.R))]
            self.idx, self.deltas = np.array([1, d - 1], np.uint32), mont(oc, [5, py.R - 9])
            self.pristine = start_proofs
        else:
            self.pristine = np.full((n2 // 2, 8), SENT)

    def call(self, h, srs, out):
        from keaki_amd.hip import _ptr
        lib, r = h.lib, [_ptr(x) for x in self.roots]
        if self.kind == "fk":
            return lib.keaki_hip_open_fk_poly(h.ctx, srs.handle, self.key[0], _ptr(self.pm), *r, _ptr(out))
        if self.kind == "fkc":
            return lib.keaki_hip_open_fk_cosets_poly(h.ctx, srs.handle, self.key[0], self.key[1], _ptr(self.pm), *r, _ptr(out))
        return lib.keaki_hip_vec_update(h.ctx, srs.handle, self.key[0], *r, _ptr(self.idx), _ptr(self.deltas), 2, None, _ptr(out))

    def run(self, h, srs):
        out = self.pristine.copy()
        st = self.call(h, srs, out)
        assert st == 0, (self.kind, self.key, st, h.lib.keaki_hip_last_error(h.ctx))
        return out


@pytest.fixture(scope="module")
def ops(oc, py, hip, rand_fr, srs_pts):
    """(kind, key) -> Op, made once. The proofs that a vec_update op starts from are the FK23 proofs of its polynomial (session context, own handle)."""
    cache = {}

    def make(kind, key):
        if (kind, key) not in cache:
            start = None
            if kind == "upd":
                fk = make("fk", key)
                srs = hip.srs_g1_upload(srs_pts)
                try:
                    start = fk.run(hip, srs)
                finally:
                    srs.free()
            cache[kind, key] = Op(oc, py, rand_fr, kind, key, start)
        return cache[kind, key]
    return make


@pytest.mark.parametrize("kind,key_a,key_b", REPLACE)
def test_refused_replace(oc, py, ops, srs_pts, ctx_tables, kind, key_a, key_b):
    h, tables = ctx_tables
    a, b = ops(kind, key_a), ops(kind, key_b)
    others = [ops(k, KEY_A[k]) for k in ("fk", "upd", "fkc") if k != kind]
    warm, sut, fresh = (h.srs_g1_upload(srs_pts) for _ in range(3))
    try:
        first_a = a.run(h, warm)                           # a fresh handle's answer for A; with B, every workspace of both shapes is warm
        b.run(h, warm)
        got_a = a.run(h, sut)
        assert np.array_equal(got_a, first_a)
        if kind == "fk" and (1 << key_a[0]) <= 8:
            assert oc.g1_to_ints(got_a) == py.kzg_open_fk(oc.g1_to_ints(srs_pts)[:1 << key_a[0]], a.p)
        got_others = [o.run(h, sut) for o in others]       # the handle's other two caches, and their workspaces
        t0 = tables()
        assert t0 == table_bytes(key_b) + table_bytes(key_a) + sum(table_bytes(o.key) for o in others)

        h.debug_set_alloc_limit(LIMIT)
        out = b.pristine.copy()
        assert b.call(h, sut, out) == OOM and b"keaki_hip_debug_set_alloc_limit" in h.lib.keaki_hip_last_error(h.ctx)
        assert np.array_equal(out, b.pristine), "a refused call writes nothing"
        assert tables() == t0 - table_bytes(key_a), "A's table is gone and counts nothing, nothing else moved"
        for o, exp in zip(others, got_others):             # under the limit: a hit allocates nothing
            assert np.array_equal(o.run(h, sut), exp), (kind, o.kind)
        assert tables() == t0 - table_bytes(key_a)

        h.debug_set_alloc_limit(0)
        got_b = b.run(h, sut)
        assert tables() == t0 - table_bytes(key_a) + table_bytes(key_b)
        assert np.array_equal(got_b, b.run(h, fresh))
        assert np.array_equal(a.run(h, sut), first_a) and tables() == t0 + table_bytes(key_b), "A again (sut), B on the fresh handle"
        for o, exp in zip(others, got_others):
            assert np.array_equal(o.run(h, sut), exp), (kind, o.kind)
    finally:
        for s in (warm, sut, fresh):
            s.free()
    assert tables() == 0


@pytest.mark.parametrize("kind,key_a,key_b", REPLACE)
def test_free_through_another_context(ops, srs_pts, ctx_tables, kind, key_a, key_b):
    """all three caches on one handle, `kind`'s replaced once (A, then B); the handle is freed through another context of the device"""
    from keaki_amd.hip import KeakiHip
    h, tables = ctx_tables
    other = KeakiHip(0)
    srs = h.srs_g1_upload(srs_pts)
    try:
        for k in ("fk", "upd", "fkc"):
            ops(k, key_a if k == kind else KEY_A[k]).run(h, srs)
        ops(kind, key_b).run(h, srs)
        assert tables() == table_bytes(key_b) + sum(table_bytes(KEY_A[k]) for k in ("fk", "upd", "fkc") if k != kind)
        srs.owner = other                                  # whichever context frees the handle, the bytes leave the one that built the tables
        srs.free()
        assert tables() == 0
    finally:
        srs.free()
        other.close()
