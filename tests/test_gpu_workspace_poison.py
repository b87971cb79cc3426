"""No result may depend on what a workspace held before the call.

Every entry point runs in the grow-only workspaces of its context, which `reserve` never clears: a call that reads a word it has not written itself
sees zeros on a fresh context and its own earlier output in a test of one shape, and is right both times. keaki_hip_debug_poison_workspaces fills
every scratch workspace (and, with also_new, every later allocation) with a chosen byte. For every row and shape of tests/workspace_cases.py, on a
context of its own:

 1. baseline   the call on the fresh context, compared with the oracle or the Python model where the row has a direct reference
 2. poison     the same call after poisoning with 0x00, 0xFF and 0x5A, in that order: every output word, status byte, counter and verdict identical
 3. residue    a strictly larger call of the family on other inputs, then the small call again with nothing in between: identical again
 4. fresh      a second context that is under poison 0x5A before its first call and allocates everything itself: identical again
 5. footprint  (rows with a _dev form) inputs and outputs are slices in the middle of one device tensor filled with 0xC3: the outputs equal the
               baseline, the inputs are unchanged and every byte before, between and behind the slices is still 0xC3

The order of the bytes and of the rows puts the mildest poison first: run the file with -x."""
import numpy as np
import pytest

import workspace_cases as W

pytestmark = pytest.mark.gpu
CASES = W.case_ids()


@pytest.fixture(scope="module")
def E(oc, py):
    return W.Env(oc, py)


class Arena:
    """one device tensor filled with ARENA_FILL; inputs and outputs are 64-byte aligned slices of exactly their size with at least 64 bytes of fill
    around each, so a lane that reads past n reads the fill and a store past the documented size lands in it"""
    SIZE, GAP = 4 << 20, 64

    def __init__(self):
        import torch
        self.t = torch.full((self.SIZE,), W.ARENA_FILL, dtype=torch.uint8, device="cuda:0")
        self.base = self.t.data_ptr()
        assert self.base % 64 == 0
        self.off, self.inputs, self.outputs = 4096, [], []

    def _take(self, nbytes):
        off = self.off
        self.off = (off + nbytes + self.GAP + 63) & ~63
        assert self.off + 4096 <= self.SIZE, "arena too small"
        return off

    def put(self, arr, out=False):
        import torch
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()
        off = self._take(raw.size)
        self.t[off:off + raw.size].copy_(torch.from_numpy(raw))
        (self.outputs if out else self.inputs).append((off, raw.size) if out else (off, raw))
        return self.base + off

    def out(self, nbytes):
        off = self._take(nbytes)
        self.outputs.append((off, nbytes))
        return self.base + off

    def ready(self):
        import torch
        torch.cuda.synchronize()          # the context's stream is unordered against torch's

    def read(self, ptr, dtype, shape):
        import torch
        torch.cuda.synchronize()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        off = ptr - self.base
        return self.t[off:off + n].cpu().numpy().view(dtype).reshape(shape).copy()

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        host = self.t.cpu().numpy()
        free = np.ones(self.SIZE, bool)
        for off, raw in self.inputs:
            assert np.array_equal(host[off:off + raw.size], raw), (what, "an input slice was written")
            free[off:off + raw.size] = False
        for off, n in self.outputs:
            free[off:off + n] = False
        bad = np.flatnonzero(free & (host != W.ARENA_FILL))
        assert bad.size == 0, (what, "bytes outside the documented slices were written", [(int(b), self._where(int(b))) for b in bad[:4]])

    def _where(self, b):
        near = min(self.outputs + [(o, r.size) for o, r in self.inputs], key=lambda s: min(abs(b - s[0]), abs(b - s[0] - s[1])))
        return "slice at %d (%d bytes)" % near


def _same(a, b):
    """bit-identical tuples: arrays by dtype, shape and bytes, everything else by ==; None on either side (an output a form does not have) is skipped"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x is None or y is None:
            continue
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                return False
        elif type(x) is not type(y) or x != y:
            return False
    return True


def _ctx(options):
    from keaki_amd.hip import KeakiHip
    h = KeakiHip(0)
    for k, v in options.items():
        h.set_option(k, v)
    return h


def _tuple(out):
    return out if isinstance(out, tuple) else (out,)


@pytest.mark.parametrize("row,shape", CASES, ids=["%s-%s" % (r.family, s[0]) for r, s in CASES])
def test_results_do_not_depend_on_what_the_workspaces_held(E, row, shape):
    sid, small_p, large_p = shape
    small, large = row.build(E, small_p), row.build(E, large_p)
    what = "%s[%s]" % (row.family, sid)
    h = h2 = None
    handles = []
    try:
        h = _ctx(small.options)
        st = small.setup(h)
        handles += st["free"]
        base = _tuple(small.run(h, st))                                                  # 1. baseline
        if small.expect is not None:
            small.expect(base)
        for byte in W.POISON_BYTES:                                                      # 2. poison
            h.debug_poison_workspaces(byte, True)
            assert _same(_tuple(small.run(h, st)), base), (what, "differs from the baseline under poison 0x%02X" % byte)
        for k, v in large.options.items():                                               # 3. residue
            h.set_option(k, v)
        st_l = large.setup(h)
        handles += st_l["free"]
        large.run(h, st_l)
        for k, v in small.options.items():
            h.set_option(k, v)
        assert _same(_tuple(small.run(h, st)), base), (what, "differs from the baseline behind a larger call")
        if small.run_dev is not None:                                                    # 5. footprint of the _dev form (on the used context, poisoned once more)
            h.debug_poison_workspaces(0x5A, True)
            A = Arena()
            got = _tuple(small.run_dev(h, st, A))
            h.synchronize()
            A.check(what)
            assert _same(got, base), (what, "the _dev form differs from the baseline")
        h2 = _ctx(small.options)                                                         # 4. a fresh context under poison
        h2.debug_poison_workspaces(0x5A, True)
        st2 = small.setup(h2)
        handles += st2["free"]
        assert _same(_tuple(small.run(h2, st2)), base), (what, "differs from the baseline on a fresh context under poison 0x5A")
    finally:
        for s in handles:
            s.free()
        for c in (h, h2):
            if c is not None:
                c.close()


def test_the_hook_itself():
    """a null context is refused; capacities and the memory report do not change; also_new = 0 switches the fill of new allocations off"""
    import torch
    from keaki_amd.hip import KeakiHip, load_library
    assert load_library().keaki_hip_debug_poison_workspaces(None, 0x5A, 1) == -1
    h = KeakiHip(0)
    try:
        h.debug_poison_workspaces(0x5A, True)               # nothing allocated yet: legal
        assert h.memory()["workspaces"] == 0
        k = torch.arange(1, 33, dtype=torch.int64, device="cuda:0").reshape(8, 4)
        g = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        out = torch.zeros((8, 8), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        h.g1_mul_batch_dev(g.data_ptr(), 0, k.data_ptr(), 8, out.data_ptr())
        h.synchronize()
        before = h.memory()
        h.debug_poison_workspaces(0xFF, False)
        assert h.memory() == before
    finally:
        h.close()
