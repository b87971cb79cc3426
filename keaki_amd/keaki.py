"""ctypes binding of libkeaki_host.so: the C++ mirror of keaki's public API (kzg / kem / enc / vec,
reference src/kzg.rs, src/kem.rs, src/enc.rs, src/vec.rs) for E = Bn254. Used by the parity tests
and the Laconic-OT harness so they read like the reference's own tests.

Values: Fr = numpy uint64[4] (Montgomery limbs), G1 = uint64[8], G2 = uint64[16] (affine, identity = zeros).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PADDING_LEN = 1  # src/vec.rs:18


class KZGError(Exception):
    """KZGError::PolynomialTooLarge(degree, max_degree) -- src/kzg.rs:205-209"""

    def __init__(self, degree, max_degree):
        super().__init__(f"Can't commit to polynomial: polynomial has degree {degree} but max degree is {max_degree}")
        self.args_tuple = (degree, max_degree)

    def __eq__(self, other):
        return isinstance(other, KZGError) and self.args_tuple == other.args_tuple


class SetError(ValueError):
    """a set call refused by the host layer: a repeated point (or index), a setup without G2 powers, 0 or more than 1,024 points, mismatched lengths"""


class KeakiHostError(RuntimeError):
    pass


class WireFormatError(ValueError):
    """bytes that do not decode (proofs_from_bytes, ciphertexts_from_bytes): `index` of the first rejected item, `reason` 1 malformed encoding,
    2 no point of the curve has this x, 3 a G2 point outside the order-r subgroup"""

    def __init__(self, index: int, reason: int, text: str):
        super().__init__(text)
        self.index, self.reason = index, reason


class SetupFileError(Exception):
    """SetupFileError -- src/kzg/ptau.rs:360-376 (+ OffCurve, Truncated: what the reference does not detect / panics on)"""
    KINDS = ["ElementSizeMismatch", "EmptySection", "FileError", "InvalidFileType", "InvalidNumberOfSections", "ParseError",
             "UnknownSection", "OffCurve", "Truncated"]

    def __init__(self, kind: int, a: int, b: int, text: str):
        super().__init__(text)
        self.kind, self.a, self.b = self.KINDS[kind], a, b

    def __eq__(self, other):
        return isinstance(other, SetupFileError) and (self.kind, self.a, self.b) == (other.kind, other.a, other.b)


def _lib():
    global _LIB
    if _LIB is None:
        from . import hip
        hip.load_library()  # the host mirror links against libkeaki_hip.so; fail loudly if it is missing
        path = os.path.join(_HERE, "libkeaki_host.so")
        if not os.path.exists(path):
            raise KeakiHostError(f"{path} not built (make -C keaki_amd/host)")
        lib = C.CDLL(path)
        lib.keaki_host_last_error.restype = C.c_char_p
        lib.keaki_host_rng_splitmix.restype = C.c_void_p
        lib.keaki_host_rng_splitmix.argtypes = [C.c_uint64]
        lib.keaki_host_rng_free.argtypes = [C.c_void_p]
        lib.keaki_host_domain.restype = C.c_size_t
        lib.keaki_host_domain.argtypes = [C.c_size_t, C.c_void_p]
        lib.keaki_host_setup_len.restype = C.c_size_t
        lib.keaki_host_setup_len.argtypes = [C.c_void_p]
        lib.keaki_host_setup_g2_len.restype = C.c_size_t
        lib.keaki_host_setup_g2_len.argtypes = [C.c_void_p]
        _LIB = lib
    return _LIB


def _u64(a, width=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, width) if width else a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ck(st, err=None):
    if st == 0:
        return
    if st == 1 and err is not None:
        raise KZGError(int(err[0]), int(err[1]))
    if st == 3:
        raise SetError(_lib().keaki_host_last_error().decode())
    if st == 2 and err is not None:
        raise SetupFileError(int(err[0]), int(err[1]), int(err[2]), _lib().keaki_host_last_error().decode())
    raise KeakiHostError(f"status {st}: {_lib().keaki_host_last_error().decode()}")


class Rng:
    """Deterministic u64 stream standing in for rand::Rng (SplitMix64)."""

    def __init__(self, seed: int):
        self.h = C.c_void_p(_lib().keaki_host_rng_splitmix(seed))

    def fr_rand(self) -> np.ndarray:
        out = np.zeros(4, np.uint64)
        _lib().keaki_host_fr_rand(self.h, _p(out))
        return out

    def fr_rand_many(self, n: int) -> np.ndarray:
        """n consecutive Fr::rand draws, (n, 4)"""
        out = np.zeros((n, 4), np.uint64)
        _lib().keaki_host_fr_rand_many(self.h, C.c_size_t(n), _p(out))
        return out

    def __del__(self):
        try:
            _lib().keaki_host_rng_free(self.h)
        except Exception:
            pass


# ---- Fr helpers -------------------------------------------------------------------------------
def fr(v: int) -> np.ndarray:
    """Fr::from(i64)"""
    out = np.zeros(4, np.uint64)
    _lib().keaki_host_fr_from_i64(C.c_int64(v), _p(out))
    return out


def _binop(name, a, b):
    out = np.zeros(4, np.uint64)
    getattr(_lib(), name)(_p(_u64(a)), _p(_u64(b)), _p(out))
    return out


def fr_mul(a, b): return _binop("keaki_host_fr_mul", a, b)
def fr_add(a, b): return _binop("keaki_host_fr_add", a, b)
def fr_sub(a, b): return _binop("keaki_host_fr_sub", a, b)


def poly_evaluate(coeffs, x) -> np.ndarray:
    c = _u64(coeffs, 4); out = np.zeros(4, np.uint64)
    _lib().keaki_host_poly_eval(_p(c), C.c_size_t(c.shape[0]), _p(_u64(x)), _p(out))
    return out


def domain_elements(min_size: int) -> np.ndarray:
    """Radix2EvaluationDomain::new(min_size).elements()"""
    size = _lib().keaki_host_domain(min_size, None)
    out = np.zeros((size, 4), np.uint64)
    _lib().keaki_host_domain(min_size, _p(out))
    return out


def ifft(evals, domain_min) -> np.ndarray:
    e = _u64(evals, 4); size = _lib().keaki_host_domain(domain_min, None)
    out = np.zeros((size, 4), np.uint64)
    _lib().keaki_host_ifft(_p(e), C.c_size_t(e.shape[0]), C.c_size_t(domain_min), _p(out))
    return out


def fft(coeffs, domain_min) -> np.ndarray:
    c = _u64(coeffs, 4); size = _lib().keaki_host_domain(domain_min, None)
    out = np.zeros((size, 4), np.uint64)
    _lib().keaki_host_fft(_p(c), C.c_size_t(c.shape[0]), C.c_size_t(domain_min), _p(out))
    return out


# ---- kzg --------------------------------------------------------------------------------------
def ptau_parse(path: str) -> dict:
    """get_powers_from_file (src/kzg/ptau.rs:347-358) without a GPU: header, section table, and the limbs of sections 2 and 3."""
    lib = _lib()
    err = np.zeros(3, np.uint64)
    mod = np.zeros(64, np.uint8); mod_len = C.c_uint32(); power = C.c_uint32(); cer = C.c_uint32()
    secs = np.zeros((11, 3), np.uint64); flen = C.c_size_t(); n1 = C.c_size_t(); n2 = C.c_size_t()
    args = [os.fsencode(path), _p(mod), C.c_size_t(64), C.byref(mod_len), C.byref(power), C.byref(cer), _p(secs), C.byref(flen), C.byref(n1), C.byref(n2)]
    _ck(lib.keaki_host_ptau_parse(*args, None, None, _p(err)), err)
    g1 = np.zeros((n1.value, 8), np.uint64); g2 = np.zeros((n2.value, 16), np.uint64)
    _ck(lib.keaki_host_ptau_parse(*args, _p(g1), _p(g2), _p(err)), err)
    return {"file_len": flen.value, "field_modulus": bytes(mod[:mod_len.value]), "power": power.value, "ceremony_power": cer.value,
            "sections": [tuple(int(v) for v in r) for r in secs], "tau_g1": g1, "tau_g2": g2}


def ptau_section_info(header12: bytes, offset: int):
    """SectionInfo::new_from_data (src/kzg/ptau.rs:169-182) -> (id, size, position)"""
    out = np.zeros(3, np.uint64); err = np.zeros(3, np.uint64)
    buf = np.frombuffer(bytes(header12), np.uint8).copy()
    _ck(_lib().keaki_host_ptau_section_info(_p(buf), C.c_size_t(offset), _p(out), _p(err)), err)
    return tuple(int(v) for v in out)


def ptau_section_index(section_id: int) -> int:
    """SectionId::try_from + section_index (src/kzg/ptau.rs:54-90); -1 = UnknownSection"""
    return _lib().keaki_host_ptau_section_index(C.c_uint8(section_id))


class _CtxView:
    """a keaki_hip_ctx owned by someone else (a keaki::Device), with the option / debug / memory calls of the C ABI"""

    def __init__(self, ctx):
        from . import hip as H
        self.lib, self.ctx, self._H = H.load_library(), ctx, H

    def _ck(self, st):
        if st != 0:
            raise self._H.KeakiHipError(st, self.lib.keaki_hip_last_error(self.ctx).decode())

    def set_option(self, name: str, value: int):
        self._ck(self.lib.keaki_hip_ctx_set_option(self.ctx, name.encode(), int(value)))

    def debug_set_alloc_limit(self, nbytes: int):
        self._ck(self.lib.keaki_hip_debug_set_alloc_limit(self.ctx, int(nbytes)))

    def memory(self) -> dict:
        out = (C.c_size_t * 4)()
        self._ck(self.lib.keaki_hip_ctx_memory(self.ctx, out))
        return {"tables": int(out[0]), "workspaces": int(out[1]), "gt_tables": int(out[2]), "total": int(out[3])}


class Device:
    """keaki::Device: one GPU context shared by the setups created on it -- or, from a LIST of ordinals, several GPUs of this process
    behind one object (one context + one host thread per entry inside libkeaki_hip.so; an ordinal may repeat): commit / open then
    spread the MSM over the members by SRS range, vec_encrypt / vec_decrypt split their items."""

    def __init__(self, ordinals=0):
        lib = _lib()
        lib.keaki_host_device_ctx.restype = C.c_void_p
        lib.keaki_host_device_ctx.argtypes = [C.c_void_p, C.c_size_t]
        lib.keaki_host_device_members.restype = C.c_size_t
        lib.keaki_host_device_members.argtypes = [C.c_void_p]
        lib.keaki_host_device_free.argtypes = [C.c_void_p]
        ords = [int(ordinals)] if isinstance(ordinals, (int, np.integer)) else [int(o) for o in ordinals]
        arr = (C.c_int * len(ords))(*ords)
        h = C.c_void_p()
        _ck(lib.keaki_host_device_new(arr, C.c_size_t(len(ords)), C.byref(h)))
        self.h = h
        self.members = int(lib.keaki_host_device_members(h))

    def hip(self, member: int = 0):
        """the member's context as a non-owning view with set_option / debug_set_alloc_limit / memory (keaki_amd.hip.KeakiHip's methods)"""
        return _CtxView(C.c_void_p(_lib().keaki_host_device_ctx(self.h, member)))

    def close(self):
        if self.h:
            _lib().keaki_host_device_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KZGSetup:
    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def setup(secret, max_d: int, device=0) -> "KZGSetup":
        """device: a GPU ordinal (a context of its own is created) or a Device (shared context, or a group of GPUs)"""
        h = C.c_void_p()
        if isinstance(device, Device):
            _ck(_lib().keaki_host_setup_on(device.h, _p(_u64(secret)), C.c_size_t(max_d), C.byref(h)))
        else:
            _ck(_lib().keaki_host_setup(device, _p(_u64(secret)), C.c_size_t(max_d), C.byref(h)))
        return KZGSetup(h)

    @staticmethod
    def from_powers(g1_aff, tau_g2, device=0) -> "KZGSetup":
        pts = _u64(g1_aff, 8); h = C.c_void_p()
        if isinstance(device, Device):
            _ck(_lib().keaki_host_setup_from_powers_on(device.h, _p(pts), C.c_size_t(pts.shape[0]), _p(_u64(tau_g2)), C.byref(h)))
        else:
            _ck(_lib().keaki_host_setup_from_powers(device, _p(pts), C.c_size_t(pts.shape[0]), _p(_u64(tau_g2)), C.byref(h)))
        return KZGSetup(h)

    @staticmethod
    def new_from_file(path: str, device: int = 0) -> "KZGSetup":
        """KZGSetup::new_from_file (src/kzg.rs:33-52): sections 2 / 3 of a snarkjs .ptau uploaded verbatim, curve-checked on the GPU"""
        h = C.c_void_p(); err = np.zeros(3, np.uint64)
        _ck(_lib().keaki_host_setup_from_file(device, os.fsencode(path), C.byref(h), _p(err)), err)
        return KZGSetup(h)

    @staticmethod
    def setup_with_g2(secret, max_d: int, max_set: int, device=0) -> "KZGSetup":
        """`setup` plus the G2 powers [secret^i]_2, i <= max_set, which the set openings need (open_set .. vec_encrypt_subset_batch)"""
        h = C.c_void_p(); on = isinstance(device, Device)
        _ck(_lib().keaki_host_setup_with_g2(device.h if on else None, 0 if on else device, _p(_u64(secret)), C.c_size_t(max_d), C.c_size_t(max_set), C.byref(h)))
        return KZGSetup(h)

    @staticmethod
    def from_powers_g2(g1_aff, g2_pow, device=0) -> "KZGSetup":
        """g2_pow[i] = [tau^i]_2 (g2_pow[0] = g2, g2_pow[1] = tau_g2): a set of k points needs k + 1 of them"""
        pts = _u64(g1_aff, 8); g2s = _u64(g2_pow, 16); h = C.c_void_p(); on = isinstance(device, Device)
        _ck(_lib().keaki_host_setup_from_powers_g2(device.h if on else None, 0 if on else device, _p(pts), C.c_size_t(pts.shape[0]), _p(g2s),
                                                   C.c_size_t(g2s.shape[0]), C.byref(h)))
        return KZGSetup(h)

    @staticmethod
    def new_from_file_g2(path: str, device: int = 0) -> "KZGSetup":
        """new_from_file that keeps ALL of section 3 of the .ptau ([tau^i]_2) as the setup's G2 powers"""
        h = C.c_void_p(); err = np.zeros(3, np.uint64)
        _ck(_lib().keaki_host_setup_from_file_g2(device, os.fsencode(path), C.byref(h), _p(err)), err)
        return KZGSetup(h)

    def g2_pow(self) -> np.ndarray:
        """the G2 powers (n, 16); empty for a setup made by setup / from_powers / new_from_file"""
        n = _lib().keaki_host_setup_g2_len(self.h)
        out = np.zeros((n, 16), np.uint64)
        if n:
            _lib().keaki_host_setup_g2_all(self.h, _p(out))
        return out

    def g1_pow(self) -> np.ndarray:
        n = _lib().keaki_host_setup_len(self.h)
        out = np.zeros((n, 8), np.uint64)
        _lib().keaki_host_setup_g1_all(self.h, _p(out))
        return out

    g1_aff = g1_pow

    def tau_g2(self) -> np.ndarray:
        out = np.zeros(16, np.uint64)
        _lib().keaki_host_setup_tau_g2(self.h, _p(out))
        return out

    def has_window_tables(self) -> bool:
        """False when the optional SRS window tables did not fit in HBM (commit / open then take the generic MSM path)"""
        return bool(_lib().keaki_host_setup_has_tables(self.h))

    def close(self):
        if self.h:
            _lib().keaki_host_setup_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def commit(setup: KZGSetup, p) -> np.ndarray:
    c = _u64(p, 4); out = np.zeros(8, np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_commit(setup.h, _p(c), C.c_size_t(c.shape[0]), _p(out), _p(err)), err)
    return out


def open(setup: KZGSetup, p, point) -> np.ndarray:  # noqa: A001 (mirrors kzg::open)
    c = _u64(p, 4); out = np.zeros(8, np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_open(setup.h, _p(c), C.c_size_t(c.shape[0]), _p(_u64(point)), _p(out), _p(err)), err)
    return out


def commit_batch_min() -> int:
    """kzg::COMMIT_BATCH_MIN: from this many polynomials on commit_batch / open_batch make ONE device call; below it they loop over commit / open"""
    return int(_lib().keaki_host_commit_batch_min())


def commit_batch(setup: KZGSetup, polys) -> np.ndarray:
    """m commitments over one setup (kzg::commit_batch). polys: (m, n, 4) zero-padded rows, or a list of polynomials of any lengths -> (m, 8)"""
    rows = _rows(polys)
    m, n = rows.shape[0], rows.shape[1]
    out = np.zeros((m, 8), np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_commit_batch(setup.h, _p(rows), C.c_size_t(n), C.c_size_t(m), C.c_size_t(n), _p(out), _p(err)), err)
    return out


def open_batch(setup: KZGSetup, polys, points) -> np.ndarray:
    """m opening proofs (kzg::open_batch): polynomial j at points[j] -> (m, 8)"""
    rows = _rows(polys)
    m, n = rows.shape[0], rows.shape[1]
    z = _u64(points, 4)
    if z.shape[0] != m:
        raise ValueError("open_batch: one point per polynomial")
    out = np.zeros((m, 8), np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_open_batch(setup.h, _p(rows), C.c_size_t(n), C.c_size_t(m), C.c_size_t(n), _p(z), _p(out), _p(err)), err)
    return out


def _rows(polys) -> np.ndarray:
    """(m, n, 4) rows, zero-padded to the longest polynomial"""
    if isinstance(polys, np.ndarray) and polys.ndim == 3:
        return np.ascontiguousarray(polys, dtype=np.uint64)
    ps = [_u64(p, 4) for p in polys]
    n = max([p.shape[0] for p in ps], default=0)
    rows = np.zeros((len(ps), n, 4), np.uint64)
    for j, p in enumerate(ps):
        rows[j, :p.shape[0]] = p
    return rows


def verify(setup: KZGSetup, commitment, point, value, proof) -> bool:
    ok = C.c_int(0)
    _ck(_lib().keaki_host_verify(setup.h, _p(_u64(commitment)), _p(_u64(point)), _p(_u64(value)), _p(_u64(proof)), C.byref(ok)))
    return bool(ok.value)


# ---- set openings: ONE proof, one check, one ciphertext for k <= 1,024 DISTINCT points (this layer refuses repeats: SetError) ----
def open_set(setup: KZGSetup, p, points):
    """-> (proof u64[8], the k values p(z_j) (k, 4)) in one device call (kzg::open_set)"""
    c = _u64(p, 4); z = _u64(points, 4); k = z.shape[0]
    out = np.zeros(8, np.uint64); vals = np.zeros((max(k, 1), 4), np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_open_set(setup.h, _p(c), C.c_size_t(c.shape[0]), _p(z), C.c_size_t(k), _p(out), _p(vals), _p(err)), err)
    return out, vals[:k]


def verify_set(setup: KZGSetup, commitment, points, values, proof) -> bool:
    z = _u64(points, 4); y = _u64(values, 4); ok = C.c_int(0)
    if y.shape[0] != z.shape[0]:
        raise SetError("verify_set: one value per point")
    _ck(_lib().keaki_host_verify_set(setup.h, _p(_u64(commitment)), _p(z), _p(y), C.c_size_t(z.shape[0]), _p(_u64(proof)), C.byref(ok)))
    return bool(ok.value)


def aggregate_proofs(setup: KZGSetup, points, proofs) -> np.ndarray:
    """the set proof from the k single proofs at the k points, without the polynomial: byte for byte open_set's"""
    z = _u64(points, 4); pr = _u64(proofs, 8); out = np.zeros(8, np.uint64)
    if pr.shape[0] != z.shape[0]:
        raise SetError("aggregate_proofs: one proof per point")
    _ck(_lib().keaki_host_aggregate_proofs(setup.h, _p(z), _p(pr), C.c_size_t(z.shape[0]), _p(out)))
    return out


def encapsulate_set(rng: "Rng", setup: KZGSetup, commitment, points, values, msg_len: int):
    """(ct, key) readable by the holder of the set proof for (points, values); ONE draw from rng. Decapsulation: decapsulate(setup, set_proof, ct, msg_len)"""
    z = _u64(points, 4); y = _u64(values, 4); ct = np.zeros(16, np.uint64); key = np.zeros(max(msg_len, 1), np.uint8)
    if y.shape[0] != z.shape[0]:
        raise SetError("encapsulate_set: one value per point")
    _ck(_lib().keaki_host_encapsulate_set(rng.h, setup.h, _p(_u64(commitment)), _p(z), _p(y), C.c_size_t(z.shape[0]), C.c_size_t(msg_len), _p(ct), _p(key)))
    return ct, key[:msg_len].tobytes()


def encrypt_set(rng: "Rng", setup: KZGSetup, com, points, values, msg: bytes):
    """encapsulate_set plus the XOR; decryption: decrypt(setup, set_proof, ct)"""
    z = _u64(points, 4); y = _u64(values, 4)
    if y.shape[0] != z.shape[0]:
        raise SetError("encrypt_set: one value per point")
    m = np.frombuffer(msg or b"\0", np.uint8).copy(); ct = np.zeros(16, np.uint64); out = np.zeros(max(len(msg), 1), np.uint8)
    _ck(_lib().keaki_host_encrypt_set(rng.h, setup.h, _p(_u64(com)), _p(z), _p(y), C.c_size_t(z.shape[0]), _p(m), C.c_size_t(len(msg)), _p(ct), _p(out)))
    return ct, out[:len(msg)].tobytes()


def vec_open_subset(setup: KZGSetup, domain_size: int, idx, proofs) -> np.ndarray:
    """one set proof for the positions idx of a committed vector, from the d proofs of vec_commit (points omega^idx)"""
    ix = np.ascontiguousarray(idx, np.uint64); pr = _u64(proofs, 8); out = np.zeros(8, np.uint64)
    _ck(_lib().keaki_host_vec_open_subset(setup.h, C.c_size_t(domain_size), _p(ix), C.c_size_t(ix.shape[0]), _p(pr), C.c_size_t(pr.shape[0]), _p(out)))
    return out


def _next_pow2(n: int) -> int:
    return 1 << max(n - 1, 0).bit_length()


def open_fk_cosets(setup: KZGSetup, coeffs, domain_size: int, l: int) -> np.ndarray:
    """the r = domain_size / l set proofs of the l-point cosets {i + t r} of the size-domain_size domain, in one device call (kzg::open_fk_cosets)
    -> (r, 8) affine; proof i is open_set's proof for the coset's points. Bad shapes: SetError"""
    c = _u64(coeffs, 4)
    if domain_size < 1 or l < 1 or domain_size % l:
        raise SetError("open_fk_cosets: l divides the domain size")
    out = np.zeros((domain_size // l, 8), np.uint64)
    _ck(_lib().keaki_host_open_fk_cosets(setup.h, _p(c), C.c_size_t(c.shape[0]), C.c_size_t(domain_size), C.c_size_t(l), _p(out)))
    return out


def vec_open_cosets(setup: KZGSetup, evals, l: int) -> np.ndarray:
    """every block proof of a vector from its evaluations over the domain (vec::vec_open_cosets): the inverse transform, then open_fk_cosets;
    proof i belongs to the positions vec_coset_indices(size, l, i)"""
    e = _u64(evals, 4)
    size = _next_pow2(e.shape[0])
    if e.shape[0] < 1 or l < 1 or size % l:
        raise SetError("vec_open_cosets: l divides the domain size")
    out = np.zeros((size // l, 8), np.uint64)
    _ck(_lib().keaki_host_vec_open_cosets(setup.h, _p(e), C.c_size_t(e.shape[0]), C.c_size_t(l), _p(out)))
    return out


def vec_coset_indices(domain_size: int, l: int, i: int) -> np.ndarray:
    """{i + t r : t < l}, r = size / l: the index list vec_verify_subset and vec_encrypt_subset_batch take"""
    if l < 1 or i < 0 or domain_size < 1:
        raise SetError("vec_coset_indices: bad argument")
    out = np.zeros(l, np.uint64)
    _ck(_lib().keaki_host_vec_coset_indices(C.c_size_t(domain_size), C.c_size_t(l), C.c_size_t(i), _p(out)))
    return out


def vec_verify_subset(setup: KZGSetup, com, domain_size: int, idx, values, proof) -> bool:
    ix = np.ascontiguousarray(idx, np.uint64); y = _u64(values, 4); ok = C.c_int(0)
    if y.shape[0] != ix.shape[0]:
        raise SetError("vec_verify_subset: one value per index")
    _ck(_lib().keaki_host_vec_verify_subset(setup.h, _p(_u64(com)), C.c_size_t(domain_size), _p(ix), _p(y), C.c_size_t(ix.shape[0]), _p(_u64(proof)), C.byref(ok)))
    return bool(ok.value)


def verify_cosets(rng: "Rng", setup: KZGSetup, commitments, shifts, l: int, values, proofs) -> bool:
    """kzg::verify_cosets: n set proofs over cosets shifts[k] <omega_l> of ONE size l in one device call. values (n, l, 4): value t of item k belongs to
    shifts[k] omega_l^t. One gamma per item is drawn from `rng` in index order. commitments: one G1 (shared) or n. The setup needs G2 powers beyond l.
    A zero shift, an l that is not a power of two, a setup without [tau^l]_2, a device group: SetError"""
    h = np.ascontiguousarray(_u64(shifts, 4)); n = h.shape[0]
    coms = np.ascontiguousarray(_u64(commitments, 8)); pr = np.ascontiguousarray(_u64(proofs, 8)); y = np.ascontiguousarray(_u64(values, 4))
    if l < 1 or y.shape[0] != n * l or pr.shape[0] != n or coms.shape[0] not in (1, n):
        raise SetError("verify_cosets: l values and one proof per item, commitments one or n")
    ok = C.c_int(0)
    _ck(_lib().keaki_host_verify_cosets(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(h), C.c_size_t(l), _p(y), _p(pr), C.c_size_t(n), C.byref(ok)))
    return bool(ok.value)


def _ragged(rows, width):
    """rows of unequal length one behind the other -> (sizes u64[n], the flat array)"""
    rows = [np.ascontiguousarray(r, np.uint64).reshape(-1, width) if width else np.ascontiguousarray(r, np.uint64).reshape(-1) for r in rows]
    sizes = np.array([r.shape[0] for r in rows], np.uint64)
    flat = np.concatenate(rows) if rows else np.zeros((0, width) if width else 0, np.uint64)
    return sizes, np.ascontiguousarray(flat)


def verify_sets(rng: "Rng", setup: KZGSetup, commitments, points, values, proofs) -> bool:
    """kzg::verify_sets: n set proofs over ARBITRARY point sets in one device call per set size. points, values: n rows (row i: the k_i <= 64 distinct points
    of item i, and one value per point); the rows may differ in length (the host layer groups them by length). One gamma per item is drawn from `rng` in
    index order. commitments: one G1 (shared) or n. A repeated point within an item, sizes that disagree, a setup whose G2 powers do not reach the
    largest set, a device group: SetError"""
    coms = np.ascontiguousarray(_u64(commitments, 8)); pr = np.ascontiguousarray(_u64(proofs, 8)); n = pr.shape[0]
    zs, z = _ragged(points, 4)
    ys, y = _ragged(values, 4)
    if zs.shape[0] != n or ys.shape[0] != n or coms.shape[0] not in (1, n):
        raise SetError("verify_sets: points, values and proofs must have one entry per item, commitments one or n")
    if not np.array_equal(zs, ys):
        raise SetError("verify_sets: one value per point")
    ok = C.c_int(0)
    _ck(_lib().keaki_host_verify_sets(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(zs), _p(z), _p(y), _p(pr), C.c_size_t(n), C.byref(ok)))
    return bool(ok.value)


def vec_verify_subsets(rng: "Rng", setup: KZGSetup, com, domain_size: int, idx_rows, values, proofs) -> bool:
    """vec::vec_verify_subsets: n subset proofs (vec_open_subset) of ONE committed vector in one device call per subset size. idx_rows, values: n rows
    (positions < the domain, distinct within a row; one value per position). One gamma per item is drawn from `rng` in index order. A repeated index,
    an index outside the domain, sizes that disagree, a setup without enough G2 powers, a device group: SetError"""
    pr = np.ascontiguousarray(_u64(proofs, 8)); n = pr.shape[0]
    ks, ix = _ragged(idx_rows, 0)
    ys, y = _ragged(values, 4)
    if ks.shape[0] != n or ys.shape[0] != n:
        raise SetError("vec_verify_subsets: idx_rows, values and proofs must have one entry per item")
    if not np.array_equal(ks, ys):
        raise SetError("vec_verify_subsets: one value per position")
    ok = C.c_int(0)
    _ck(_lib().keaki_host_vec_verify_subsets(rng.h, setup.h, _p(_u64(com)), C.c_size_t(domain_size), _p(ks), _p(ix), _p(y), _p(pr), C.c_size_t(n), C.byref(ok)))
    return bool(ok.value)


def _set_rows(what, commitments, points, values, n, width):
    """the ragged rows of a per-item set call -> (coms, sizes, flat points or indices, flat values)"""
    coms = np.ascontiguousarray(_u64(commitments, 8))
    zs, z = _ragged(points, width)
    ys, y = _ragged(values, 4)
    if zs.shape[0] != n or ys.shape[0] != n or coms.shape[0] not in (1, n):
        raise SetError("%s: points, values and proofs must have one entry per item, commitments one or n" % what)
    if not np.array_equal(zs, ys):
        raise SetError("%s: one value per point" % what)
    pad = lambda arr, shape: arr if arr.shape[0] else np.zeros(shape, np.uint64)
    return coms, pad(zs, 1), pad(z, (1, 4) if width else 1), pad(y, (1, 4))


def set_pairs(setup: KZGSetup, commitments, points, values):
    """kzg::set_pairs: the two points of every item's set check, A_i = C_i - [I_i(tau)]_1 (n, 8) and Z2_i = [Z_i(tau)]_2 (n, 16); rows as verify_sets"""
    n = len(points)
    coms, zs, z, y = _set_rows("set_pairs", commitments, points, values, n, 4)
    a = np.zeros((max(n, 1), 8), np.uint64); z2 = np.zeros((max(n, 1), 16), np.uint64)
    _ck(_lib().keaki_host_set_pairs(setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(zs), _p(z), _p(y), C.c_size_t(n), _p(a), _p(z2)))
    return a[:n], z2[:n]


def verify_sets_each(setup: KZGSetup, commitments, points, values, proofs) -> np.ndarray:
    """kzg::verify_sets_each: WHICH of n set proofs over arbitrary point sets are wrong -> uint8[n], 0 = valid, 1 = invalid; one device call per set size,
    nothing is drawn. Arguments and refusals as verify_sets"""
    pr = np.ascontiguousarray(_u64(proofs, 8)); n = pr.shape[0]
    coms, zs, z, y = _set_rows("verify_sets_each", commitments, points, values, n, 4)
    status = np.zeros(max(n, 1), np.uint8)
    _ck(_lib().keaki_host_verify_sets_each(setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(zs), _p(z), _p(y), _p(pr if n else np.zeros((1, 8), np.uint64)),
                                           C.c_size_t(n), _p(status)))
    return status[:n]


def vec_verify_subsets_each(setup: KZGSetup, com, domain_size: int, idx_rows, values, proofs) -> np.ndarray:
    """vec::vec_verify_subsets_each: WHICH subset proofs of ONE committed vector are wrong -> uint8[n]; arguments and refusals as vec_verify_subsets"""
    pr = np.ascontiguousarray(_u64(proofs, 8)); n = pr.shape[0]
    coms, ks, ix, y = _set_rows("vec_verify_subsets_each", _u64(com), idx_rows, values, n, 0)
    status = np.zeros(max(n, 1), np.uint8)
    _ck(_lib().keaki_host_vec_verify_subsets_each(setup.h, _p(coms), C.c_size_t(domain_size), _p(ks), _p(ix), _p(y), _p(pr if n else np.zeros((1, 8), np.uint64)),
                                                  C.c_size_t(n), _p(status)))
    return status[:n]


def _msgs(messages, n):
    msgs = np.ascontiguousarray(messages, np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
    ml = msgs.shape[1]
    body = np.zeros((max(n, 1), max(ml, 1)), np.uint8)
    return (msgs if ml and n else body), ml, body


def encapsulate_sets(rng: "Rng", setup: KZGSetup, commitments, points, values, msg_len: int):
    """kem::encapsulate_sets: encapsulate_set for n items with their own point sets in one batch -> (ct_g2 (n, 16), keys (n, msg_len)). One r per item in
    index order, after every refusal; item i equals encapsulate_set alone with the same r"""
    n = len(points)
    coms, zs, z, y = _set_rows("encapsulate_sets", commitments, points, values, n, 4)
    ct = np.zeros((max(n, 1), 16), np.uint64); keys = np.zeros((max(n, 1), max(msg_len, 1)), np.uint8)
    _ck(_lib().keaki_host_encapsulate_sets(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(zs), _p(z), _p(y), C.c_size_t(n), C.c_size_t(msg_len), _p(ct), _p(keys)))
    return ct[:n], keys[:n, :msg_len]


def encrypt_sets(rng: "Rng", setup: KZGSetup, commitments, points, values, messages: np.ndarray):
    """enc::encrypt_sets: message i to the claimed values of item i's own point set; messages (n, msg_len) uint8 -> (ct_g2 (n, 16), bodies (n, msg_len)).
    Item i equals encrypt_set alone with the same r; decrypt(setup, set_proof_i, ct_i) opens it. Refusals (SetError) leave rng untouched"""
    n = len(points)
    coms, zs, z, y = _set_rows("encrypt_sets", commitments, points, values, n, 4)
    msgs, ml, body = _msgs(messages, n)
    ct = np.zeros((max(n, 1), 16), np.uint64)
    _ck(_lib().keaki_host_encrypt_sets(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(zs), _p(z), _p(y), C.c_size_t(n), _p(msgs), C.c_size_t(ml), _p(ct), _p(body)))
    return ct[:n], body[:n, :ml]


def vec_encrypt_subsets(rng: "Rng", setup: KZGSetup, com, domain_size: int, idx_rows, values, messages: np.ndarray):
    """vec::vec_encrypt_subsets: message i to the claimed values[i] at the positions idx_rows[i] of ONE committed vector, every item with its own index set
    -> (ct_g2 (n, 16), bodies (n, msg_len)). vec_open_subset's proof and the unchanged decrypt open item i. Refusals (SetError) leave rng untouched"""
    n = len(idx_rows)
    coms, ks, ix, y = _set_rows("vec_encrypt_subsets", _u64(com), idx_rows, values, n, 0)
    msgs, ml, body = _msgs(messages, n)
    ct = np.zeros((max(n, 1), 16), np.uint64)
    _ck(_lib().keaki_host_vec_encrypt_subsets(rng.h, setup.h, _p(coms), C.c_size_t(domain_size), _p(ks), _p(ix), _p(y), C.c_size_t(n), _p(msgs), C.c_size_t(ml), _p(ct),
                                              _p(body)))
    return ct[:n], body[:n, :ml]


def vec_verify_cosets(rng: "Rng", setup: KZGSetup, com, evals, l: int, proofs) -> bool:
    """vec::vec_verify_cosets: are the size / l proofs of vec_open_cosets(evals, l) the block proofs of `com`? One device call over the evaluations
    in domain order; one gamma per coset is drawn from `rng`"""
    e = np.ascontiguousarray(_u64(evals, 4)); pr = np.ascontiguousarray(_u64(proofs, 8)); ok = C.c_int(0)
    if e.shape[0] < 1 or l < 1:
        raise SetError("vec_verify_cosets: no evaluations")
    _ck(_lib().keaki_host_vec_verify_cosets(rng.h, setup.h, _p(_u64(com)), _p(e), C.c_size_t(e.shape[0]), C.c_size_t(l), _p(pr), C.c_size_t(pr.shape[0]), C.byref(ok)))
    return bool(ok.value)


def vec_verify_cosets_subset(rng: "Rng", setup: KZGSetup, com, domain_size: int, l: int, cosets, values, proofs) -> bool:
    """vec::vec_verify_cosets_subset: the listed cosets only. cosets[k] < size / l names the positions vec_coset_indices(size, l, cosets[k]); values
    (k, l, 4) in the order of those positions; proofs (k, 8)"""
    ix = np.ascontiguousarray(cosets, np.uint64); k = ix.shape[0]
    y = np.ascontiguousarray(_u64(values, 4)); pr = np.ascontiguousarray(_u64(proofs, 8)); ok = C.c_int(0)
    if l < 1 or y.shape[0] != k * l or pr.shape[0] != k:
        raise SetError("vec_verify_cosets_subset: l values and one proof per listed coset")
    _ck(_lib().keaki_host_vec_verify_cosets_subset(rng.h, setup.h, _p(_u64(com)), C.c_size_t(domain_size), C.c_size_t(l), _p(ix), C.c_size_t(k), _p(y), _p(pr),
                                                   C.byref(ok)))
    return bool(ok.value)


def vec_verify_cosets_each(setup: KZGSetup, com, evals, l: int, proofs) -> np.ndarray:
    """vec::vec_verify_cosets_each: WHICH of the size / l proofs of vec_open_cosets(evals, l) are wrong -> uint8[size / l], 0 = valid, 1 = invalid. One
    device call over the evaluations in domain order; exact, nothing is drawn"""
    e = np.ascontiguousarray(_u64(evals, 4)); pr = np.ascontiguousarray(_u64(proofs, 8))
    if e.shape[0] < 1 or l < 1:
        raise SetError("vec_verify_cosets_each: no evaluations")
    status = np.zeros(max(pr.shape[0], 1), np.uint8)
    _ck(_lib().keaki_host_vec_verify_cosets_each(setup.h, _p(_u64(com)), _p(e), C.c_size_t(e.shape[0]), C.c_size_t(l), _p(pr), C.c_size_t(pr.shape[0]), _p(status)))
    return status[:pr.shape[0]]


def vec_verify_cosets_each_subset(setup: KZGSetup, com, domain_size: int, l: int, cosets, values, proofs) -> np.ndarray:
    """vec::vec_verify_cosets_each_subset: the listed cosets only, arguments as vec_verify_cosets_subset -> uint8[k]"""
    ix = np.ascontiguousarray(cosets, np.uint64); k = ix.shape[0]
    y = np.ascontiguousarray(_u64(values, 4)); pr = np.ascontiguousarray(_u64(proofs, 8))
    if l < 1 or y.shape[0] != k * l or pr.shape[0] != k:
        raise SetError("vec_verify_cosets_each_subset: l values and one proof per listed coset")
    status = np.zeros(max(k, 1), np.uint8)
    _ck(_lib().keaki_host_vec_verify_cosets_each_subset(setup.h, _p(_u64(com)), C.c_size_t(domain_size), C.c_size_t(l), _p(ix), C.c_size_t(k), _p(y), _p(pr),
                                                        _p(status)))
    return status[:k]


def vec_encrypt_cosets(rng: "Rng", setup: KZGSetup, com, domain_size: int, l: int, cosets, values, messages: np.ndarray):
    """vec::vec_encrypt_cosets: message k to the l claimed values of coset cosets[k]: values (k, l, 4) in the order of vec_coset_indices, messages
    (k, msg_len) uint8 -> (ct_g2 (k, 16), bodies (k, msg_len)). One r per item in index order; item k equals encrypt_set on the coset's points with
    the same r, and vec_decrypt with the proofs of vec_open_cosets opens it. Refusals (SetError) leave rng untouched"""
    ix = np.ascontiguousarray(cosets, np.uint64); n = ix.shape[0]
    y = np.ascontiguousarray(_u64(values, 4))
    if l < 1 or y.shape[0] != n * l:
        raise SetError("vec_encrypt_cosets: l values per listed coset")
    msgs = np.ascontiguousarray(messages, np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
    ml = msgs.shape[1]
    ct = np.zeros((max(n, 1), 16), np.uint64); body = np.zeros((max(n, 1), max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt_cosets(rng.h, setup.h, _p(_u64(com)), C.c_size_t(domain_size), C.c_size_t(l), _p(ix if n else np.zeros(1, np.uint64)),
                                             C.c_size_t(n), _p(y if n else np.zeros((1, 4), np.uint64)), _p(msgs if ml and n else body), C.c_size_t(ml), _p(ct), _p(body)))
    return ct[:n], body[:n, :ml]


def vec_encrypt_subset_batch(rng: "Rng", setup: KZGSetup, com, domain_size: int, idx, values, messages: np.ndarray):
    """n items over ONE index set with different value tuples: values (n, k, 4), messages (n, msg_len) uint8 -> (ct_g2 (n, 16), bodies (n, msg_len)).
    Item i is readable by the holder of a vector with values[i, j] at idx[j] for every j; one r per item in index order."""
    ix = np.ascontiguousarray(idx, np.uint64); k = ix.shape[0]
    y = np.ascontiguousarray(values, np.uint64).reshape(-1, max(k, 1), 4); n = y.shape[0]
    msgs = np.ascontiguousarray(messages, np.uint8).reshape(n, -1); ml = msgs.shape[1]
    ct = np.zeros((n, 16), np.uint64); body = np.zeros((n, max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt_subset_batch(rng.h, setup.h, _p(_u64(com)), C.c_size_t(domain_size), _p(ix), C.c_size_t(k), _p(y), C.c_size_t(n),
                                                   _p(msgs if ml else body), C.c_size_t(ml), _p(ct), _p(body)))
    return ct, body[:, :ml]


def _opening_args(what, commitments, points, values, proofs, roots_of_unity):
    """n openings as contiguous arrays: commitments (1 or n), points (n, or the ONE omega with roots_of_unity), values, the first n proofs"""
    vals = np.ascontiguousarray(_u64(values, 4)); n = vals.shape[0]
    coms = np.ascontiguousarray(_u64(commitments, 8)); pts = np.ascontiguousarray(_u64(points, 4)); pr = np.ascontiguousarray(_u64(proofs, 8)[:n])
    if coms.shape[0] not in (1, n) or pts.shape[0] != (1 if roots_of_unity else n) or pr.shape[0] != n:
        raise ValueError("%s: array lengths disagree" % what)
    return coms, pts, vals, pr, n


def verify_batch(rng: "Rng", setup: "KZGSetup", commitments, points, values, proofs, roots_of_unity: bool = False) -> bool:
    """kzg::verify_batch: n openings in one device call. One gamma per item is drawn from `rng` in index order. commitments: one G1 (shared) or n;
    points: n Fr -- or, with roots_of_unity, the ONE Fr omega (item i is opened at omega^i)."""
    coms, pts, vals, pr, n = _opening_args("verify_batch", commitments, points, values, proofs, roots_of_unity)
    ok = C.c_int(0)
    _ck(_lib().keaki_host_verify_batch(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(pts), C.c_int(1 if roots_of_unity else 0), _p(vals), _p(pr),
                                       C.c_size_t(n), C.byref(ok)))
    return bool(ok.value)


def verify_each(setup: "KZGSetup", commitments, points, values, proofs, roots_of_unity: bool = False) -> np.ndarray:
    """kzg::verify_each: one verdict per opening in one device call -> uint8[n], 0 = valid, 1 = invalid. Exact: nothing is drawn. Arguments as
    verify_batch."""
    coms, pts, vals, pr, n = _opening_args("verify_each", commitments, points, values, proofs, roots_of_unity)
    status = np.zeros(n, np.uint8); bad = C.c_uint64(0)
    _ck(_lib().keaki_host_verify_each(setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(pts), C.c_int(1 if roots_of_unity else 0), _p(vals), _p(pr), C.c_size_t(n),
                                      _p(status), C.byref(bad)))
    return status


def locate_invalid(rng: "Rng", setup: "KZGSetup", commitments, points, values, proofs, roots_of_unity: bool = False) -> list:
    """kzg::locate_invalid: verify_batch (drawing from `rng` what verify_batch draws), and verify_each only if it rejects -> the indices of the
    invalid items, [] for a clean batch"""
    coms, pts, vals, pr, n = _opening_args("locate_invalid", commitments, points, values, proofs, roots_of_unity)
    idx = np.zeros(max(n, 1), np.uint64); count = C.c_uint64(0)
    _ck(_lib().keaki_host_locate_invalid(rng.h, setup.h, _p(coms), C.c_size_t(coms.shape[0]), _p(pts), C.c_int(1 if roots_of_unity else 0), _p(vals), _p(pr),
                                         C.c_size_t(n), _p(idx), C.byref(count)))
    return [int(i) for i in idx[:count.value]]


def vec_verify_each(setup: "KZGSetup", com, v, proofs) -> np.ndarray:
    """vec::vec_verify_each: uint8[len(v)], 0 where proof i opens `com` to v[i] over the domain of len(v) + PADDING_LEN evaluations"""
    vals = np.ascontiguousarray(_u64(v, 4)); n = vals.shape[0]
    pr = np.ascontiguousarray(_u64(proofs, 8)[:n])
    if pr.shape[0] != n:
        raise ValueError("vec_verify_each: fewer proofs than values")
    status = np.zeros(n, np.uint8); bad = C.c_uint64(0)
    _ck(_lib().keaki_host_vec_verify_each(setup.h, _p(_u64(com)), _p(vals), C.c_size_t(n), _p(pr), _p(status), C.byref(bad)))
    return status


def vec_verify(rng: "Rng", setup: "KZGSetup", com, v, proofs) -> bool:
    """vec::vec_verify: the first len(v) proofs of a vec_commit open `com` to v over the domain of len(v) + PADDING_LEN evaluations"""
    vals = np.ascontiguousarray(_u64(v, 4)); n = vals.shape[0]
    pr = np.ascontiguousarray(_u64(proofs, 8)[:n])
    if pr.shape[0] != n:
        raise ValueError("vec_verify: fewer proofs than values")
    ok = C.c_int(0)
    _ck(_lib().keaki_host_vec_verify(rng.h, setup.h, _p(_u64(com)), _p(vals), C.c_size_t(n), _p(pr), C.byref(ok)))
    return bool(ok.value)


def _ck_wire(st, bad):
    if st == 2:
        raise WireFormatError(int(bad[0]), int(bad[1]), _lib().keaki_host_last_error().decode())
    _ck(st)


def proofs_to_bytes(setup: "KZGSetup", proofs) -> bytes:
    """kzg::proofs_to_bytes: n G1 points -> n x 32 B (`serialize_compressed`), compressed on the device"""
    pr = np.ascontiguousarray(_u64(proofs, 8)); n = pr.shape[0]
    out = np.zeros(n * 32, np.uint8)
    _ck(_lib().keaki_host_proofs_to_bytes(setup.h, _p(pr), C.c_size_t(n), _p(out)))
    return out.tobytes()


def proofs_from_bytes(setup: "KZGSetup", data) -> np.ndarray:
    """kzg::proofs_from_bytes: n x 32 B -> u64[n, 8], validated (canonical, on the curve); raises WireFormatError naming the first bad index"""
    b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if b.size % 32:
        raise ValueError("proofs_from_bytes: the length is not a multiple of 32")
    n = b.size // 32
    out = np.zeros((n, 8), np.uint64); bad = np.zeros(2, np.uint64)
    _ck_wire(_lib().keaki_host_proofs_from_bytes(setup.h, _p(b), C.c_size_t(n), _p(out), _p(bad)), bad)
    return out


def ciphertexts_to_bytes(setup: "KZGSetup", ct_g2, ct_body) -> bytes:
    """enc::ciphertexts_to_bytes on arrays (ct G2 points (n, 16) u64, bodies (n, len) u8) -> n x (64 B compressed point + body)"""
    body = np.ascontiguousarray(ct_body, dtype=np.uint8); n, ml = body.shape
    g2 = np.ascontiguousarray(_u64(ct_g2, 16)[:n])
    if g2.shape[0] != n:
        raise ValueError("ciphertexts_to_bytes: fewer points than bodies")
    out = np.zeros(n * (64 + ml), np.uint8)
    _ck(_lib().keaki_host_ciphertexts_to_bytes(setup.h, _p(g2), _p(body), C.c_size_t(n), C.c_size_t(ml), _p(out)))
    return out.tobytes()


def ciphertexts_from_bytes(setup: "KZGSetup", data, msg_len: int):
    """enc::ciphertexts_from_bytes -> (ct G2 points (n, 16) u64, bodies (n, msg_len) u8). Every point is validated as arkworks'
    deserialize_compressed does (canonical, on the twist, in the order-r subgroup); raises WireFormatError naming the first bad index"""
    b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if b.size % (64 + msg_len):
        raise ValueError("ciphertexts_from_bytes: the length is not a multiple of 64 + msg_len")
    n = b.size // (64 + msg_len)
    g2 = np.zeros((n, 16), np.uint64); body = np.zeros((n, msg_len), np.uint8); bad = np.zeros(2, np.uint64)
    _ck_wire(_lib().keaki_host_ciphertexts_from_bytes(setup.h, _p(b), C.c_size_t(n), C.c_size_t(msg_len), _p(g2), _p(body), _p(bad)), bad)
    return g2, body


def precompute_open_fk(setup: "KZGSetup", domain_size: int) -> None:
    """setup-time: the SRS-only transform of FK23 (hat_s) for this domain size"""
    _ck(_lib().keaki_host_precompute_open_fk(setup.h, C.c_size_t(domain_size)))


def open_fk(setup: KZGSetup, p, domain_size: int) -> np.ndarray:
    c = _u64(p, 4); size = _lib().keaki_host_domain(domain_size, None)
    out = np.zeros((size, 8), np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_open_fk(setup.h, _p(c), C.c_size_t(c.shape[0]), C.c_size_t(domain_size), _p(out), _p(err)), err)
    return out


# ---- kem / enc ---------------------------------------------------------------------------------
def encapsulate(rng: Rng, setup: KZGSetup, commitment, point, value, msg_len: int):
    ct = np.zeros(16, np.uint64); key = np.zeros(max(msg_len, 1), np.uint8)
    _ck(_lib().keaki_host_encapsulate(rng.h, setup.h, _p(_u64(commitment)), _p(_u64(point)), _p(_u64(value)), C.c_size_t(msg_len), _p(ct), _p(key)))
    return ct, key[:msg_len].tobytes()


def kem_prepare(setup: KZGSetup, batch_hint: int) -> None:
    """setup-time: the tables of encapsulation that depend on the setup only, for batches of `batch_hint` items (keaki::kem::prepare)"""
    _ck(_lib().keaki_host_kem_prepare(setup.h, C.c_size_t(batch_hint)))


def decapsulate(setup: KZGSetup, proof, ciphertext, msg_len: int) -> bytes:
    key = np.zeros(max(msg_len, 1), np.uint8)
    _ck(_lib().keaki_host_decapsulate(setup.h, _p(_u64(proof)), _p(_u64(ciphertext)), C.c_size_t(msg_len), _p(key)))
    return key[:msg_len].tobytes()


def encrypt(rng: Rng, setup: KZGSetup, com, point, value, msg: bytes):
    m = np.frombuffer(msg or b"\0", np.uint8).copy(); ct = np.zeros(16, np.uint64); out = np.zeros(max(len(msg), 1), np.uint8)
    _ck(_lib().keaki_host_encrypt(rng.h, setup.h, _p(_u64(com)), _p(_u64(point)), _p(_u64(value)), _p(m), C.c_size_t(len(msg)), _p(ct), _p(out)))
    return ct, out[:len(msg)].tobytes()


def decrypt(setup: KZGSetup, proof, ct) -> bytes:
    g2, body = ct
    b = np.frombuffer(body or b"\0", np.uint8).copy(); out = np.zeros(max(len(body), 1), np.uint8)
    _ck(_lib().keaki_host_decrypt(setup.h, _p(_u64(proof)), _p(_u64(g2)), _p(b), C.c_size_t(len(body)), _p(out)))
    return out[:len(body)].tobytes()


# ---- vec ---------------------------------------------------------------------------------------
def vec_commit(rng: Rng, setup: KZGSetup, v):
    v = _u64(v, 4); n = v.shape[0]
    size = _lib().keaki_host_domain(n + PADDING_LEN, None)
    com = np.zeros(8, np.uint64); proofs = np.zeros((size, 8), np.uint64)
    _ck(_lib().keaki_host_vec_commit(rng.h, setup.h, _p(v), C.c_size_t(n), _p(com), _p(proofs)))
    return com, proofs


def vec_update(setup: KZGSetup, com, proofs, idx, old_values, new_values):
    """vec::vec_update: positions idx[t] of a committed vector go from old_values[t] to new_values[t] -> (com, proofs) of the changed vector with
    the same padding scalar, without the vector. The domain is len(proofs); index len(v) is the padding slot; duplicates add."""
    pr = np.array(_u64(proofs, 8)); c = np.array(_u64(com)).reshape(8)
    ix = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1); k = ix.shape[0]
    ov = np.ascontiguousarray(_u64(old_values, 4)); nv = np.ascontiguousarray(_u64(new_values, 4))
    if ov.shape[0] != k or nv.shape[0] != k:
        raise ValueError("vec_update: idx, old_values and new_values differ in length")
    _ck(_lib().keaki_host_vec_update(setup.h, _p(ix), _p(ov), _p(nv), C.c_size_t(k), C.c_size_t(pr.shape[0]), _p(c), _p(pr)))
    return c, pr


def vec_update_flat(setup: KZGSetup, domain_size: int, idx, deltas, com=None, proofs=None):
    """vec::vec_update_flat: the same from the differences, IN PLACE on `com` (u64[8]) and `proofs` (u64[domain_size, 8]); either may be None"""
    ix = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1); dl = np.ascontiguousarray(_u64(deltas, 4))
    if dl.shape[0] != ix.shape[0]:
        raise ValueError("vec_update_flat: idx and deltas differ in length")
    _ck(_lib().keaki_host_vec_update_flat(setup.h, C.c_size_t(domain_size), _p(ix), _p(dl), C.c_size_t(ix.shape[0]),
                                          _p(com) if com is not None else None, _p(proofs) if proofs is not None else None))
    return com, proofs


def precompute_vec_update(setup: KZGSetup, domain_size: int) -> None:
    """setup-time: the update tables of this domain size (192 bytes per evaluation)"""
    _ck(_lib().keaki_host_precompute_vec_update(setup.h, C.c_size_t(domain_size)))


def vec_commit_batch(rng: Rng, setup: KZGSetup, vecs):
    """m vectors over one domain (that of the longest + PADDING_LEN) in one device call -> (commitments (m, 8), proofs (m, size, 8)); one
    padding scalar per vector, drawn in index order; see keaki::vec::vec_commit_batch"""
    vecs = [_u64(v, 4) for v in vecs]
    m = len(vecs)
    lens = (C.c_size_t * max(m, 1))(*[v.shape[0] for v in vecs])
    size = _lib().keaki_host_domain(max([v.shape[0] for v in vecs], default=0) + PADDING_LEN, None)
    flat = np.ascontiguousarray(np.concatenate(vecs) if m and sum(v.shape[0] for v in vecs) else np.zeros((1, 4), np.uint64))
    com = np.zeros((m, 8), np.uint64); proofs = np.zeros((m, size, 8), np.uint64)
    _ck(_lib().keaki_host_vec_commit_batch(rng.h, setup.h, _p(flat), lens, C.c_size_t(m), _p(com), _p(proofs)))
    return com, proofs


def vec_encrypt(rng: Rng, setup: KZGSetup, com, points, values, messages):
    n = len(messages); ml = len(messages[0]) if n else 0
    assert all(len(m) == ml for m in messages)
    pts = _u64(points, 4)[:n]; vals = _u64(values, 4)[:n]
    msgs = np.frombuffer(b"".join(messages) or b"\0", np.uint8).copy()
    g2 = np.zeros((n, 16), np.uint64); body = np.zeros(max(n * ml, 1), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt(rng.h, setup.h, _p(_u64(com)), _p(np.ascontiguousarray(pts)), _p(np.ascontiguousarray(vals)), _p(msgs),
                                     C.c_size_t(n), C.c_size_t(ml), _p(g2), _p(body)))
    return [(g2[i].copy(), body[i * ml:(i + 1) * ml].tobytes()) for i in range(n)]


def vec_encrypt_batch(rng: Rng, setup: KZGSetup, coms, counts, points, values, messages: np.ndarray):
    """vec_encrypt to m commitments in one device call: group j = the next counts[j] items, encrypted under coms[j]; messages is an
    (n, len) uint8 array over all n = sum(counts) items -> (ct G2 points (n, 16) u64, ct bodies (n, len) u8). One r per item in global index
    order: the draws and bytes of m consecutive vec_encrypt calls; see keaki::vec::vec_encrypt_batch"""
    msgs = np.ascontiguousarray(messages, dtype=np.uint8)
    n, ml = msgs.shape
    cnt = [int(c) for c in counts]
    m = len(cnt)
    assert sum(cnt) == n, "counts must add up to the number of messages"
    cs = np.ascontiguousarray(_u64(coms, 8)[:m]) if m else np.zeros((1, 8), np.uint64)
    pts = np.ascontiguousarray(_u64(points, 4)[:n]); vals = np.ascontiguousarray(_u64(values, 4)[:n])
    g2 = np.zeros((n, 16), np.uint64); body = np.zeros((n, max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt_batch(rng.h, setup.h, _p(cs), (C.c_size_t * max(m, 1))(*cnt), C.c_size_t(m), _p(pts), _p(vals), _p(msgs), C.c_size_t(ml),
                                           _p(g2), _p(body)))
    return g2, body[:, :ml]


def vec_encrypt_arrays(rng: Rng, setup: KZGSetup, com, points, values, messages: np.ndarray):
    """vec_encrypt on contiguous arrays (n equal-length messages as an (n, len) uint8 array) -> (ct G2 points (n, 16) u64,
    ct bodies (n, len) u8): the same call without a Python object per item."""
    msgs = np.ascontiguousarray(messages, dtype=np.uint8)
    n, ml = msgs.shape
    pts = np.ascontiguousarray(_u64(points, 4)[:n]); vals = np.ascontiguousarray(_u64(values, 4)[:n])
    g2 = np.zeros((n, 16), np.uint64); body = np.zeros((n, max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt(rng.h, setup.h, _p(_u64(com)), _p(pts), _p(vals), _p(msgs), C.c_size_t(n), C.c_size_t(ml), _p(g2), _p(body)))
    return g2, body[:, :ml]


def vec_decrypt_arrays(setup: KZGSetup, proofs, ct_g2: np.ndarray, ct_body: np.ndarray) -> np.ndarray:
    body = np.ascontiguousarray(ct_body, dtype=np.uint8)
    n, ml = body.shape
    pr = np.ascontiguousarray(_u64(proofs, 8)[:n]); g2 = np.ascontiguousarray(_u64(ct_g2, 16)[:n])
    out = np.zeros((n, max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_decrypt(setup.h, _p(pr), _p(g2), _p(body), C.c_size_t(n), C.c_size_t(ml), _p(out)))
    return out[:, :ml]


def vec_decrypt(setup: KZGSetup, proofs, cts):
    n = len(cts); ml = len(cts[0][1]) if n else 0
    pr = np.ascontiguousarray(_u64(proofs, 8)[:n])
    g2 = np.ascontiguousarray(np.stack([_u64(c[0]) for c in cts])) if n else np.zeros((0, 16), np.uint64)
    body = np.frombuffer(b"".join(c[1] for c in cts) or b"\0", np.uint8).copy()
    out = np.zeros(max(n * ml, 1), np.uint8)
    _ck(_lib().keaki_host_vec_decrypt(setup.h, _p(pr), _p(g2), _p(body), C.c_size_t(n), C.c_size_t(ml), _p(out)))
    return [out[i * ml:(i + 1) * ml].tobytes() for i in range(n)]


# ---- keaki::dist (host/keaki.hpp): one process per GPU; the exchange of the 96-byte partials is the caller's (keaki_amd/dist.py) --------
def prepare_shard(setup: KZGSetup, rank: int, world: int) -> None:
    """setup-time: window tables of this rank's SRS chunk (commit_partial would build them on first use)"""
    _ck(_lib().keaki_host_prepare_shard(setup.h, C.c_size_t(rank), C.c_size_t(world)))


def commit_partial(setup: KZGSetup, p, rank: int, world: int) -> np.ndarray:
    """this rank's share of kzg::commit: the MSM over its contiguous range of the SRS -> normalised Jacobian u64[12]"""
    c = _u64(p, 4); out = np.zeros(12, np.uint64); err = np.zeros(2, np.uint64)
    _ck(_lib().keaki_host_commit_partial(setup.h, _p(c), C.c_size_t(c.shape[0]), C.c_size_t(rank), C.c_size_t(world), _p(out), _p(err)), err)
    return out


def vec_commit_partial(rng: Rng, setup: KZGSetup, v, rank: int, world: int):
    """vec_commit with the final commit left as this rank's partial -> (partial u64[12], proofs); see keaki::dist::vec_commit_partial"""
    v = _u64(v, 4); n = v.shape[0]
    size = _lib().keaki_host_domain(n + PADDING_LEN, None)
    part = np.zeros(12, np.uint64); proofs = np.zeros((size, 8), np.uint64)
    _ck(_lib().keaki_host_vec_commit_partial(rng.h, setup.h, _p(v), C.c_size_t(n), C.c_size_t(rank), C.c_size_t(world), _p(part), _p(proofs)))
    return part, proofs


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)    # (user, d_send, d_recv, bytes per peer / per rank) -> 0 = ok


class ShardedOpenFk:
    """keaki::dist::ShardedOpenFk: kzg::open_fk with the group FFTs sharded over the ranks. `all_to_all(d_send, d_recv, bytes_per_peer)` and
    `all_gather(d_send, d_recv, bytes_per_rank)` are the caller's collectives over device memory (they must have completed on return);
    d_send / d_recv: device pointers to buffer_bytes each (keaki_amd/dist.py::ShardedFk provides all of this over torch.distributed)."""

    def __init__(self, setup: KZGSetup, domain_size: int, rank: int, world: int, all_to_all, all_gather):
        lib = _lib()
        lib.keaki_host_fk_shard_buffer_bytes.restype = C.c_size_t
        lib.keaki_host_fk_shard_buffer_bytes.argtypes = [C.c_void_p]
        lib.keaki_host_fk_shard_free.argtypes = [C.c_void_p]
        h = C.c_void_p()
        _ck(lib.keaki_host_fk_shard_new(setup.h, C.c_size_t(domain_size), C.c_size_t(rank), C.c_size_t(world), C.byref(h)))
        self.h, self.setup, self.domain_size, self.rank, self.world = h, setup, domain_size, rank, world
        self.buffer_bytes = int(lib.keaki_host_fk_shard_buffer_bytes(h))
        self.callback_error = None

        def wrap(fn):
            def cb(user, s, r, n):
                try:                                   # an exception must not cross the C frames: report it as a status
                    fn(s, r, n)
                    return 0
                except BaseException as e:             # noqa: BLE001
                    self.callback_error = e
                    return 1
            return EXCHANGE_FN(cb)
        self._a2a, self._gather = wrap(all_to_all), wrap(all_gather)          # kept alive with the object

    @staticmethod
    def can_shard(setup: KZGSetup, domain_size: int, rank: int, world: int) -> bool:
        return bool(_lib().keaki_host_fk_shard_can(setup.h, C.c_size_t(domain_size), C.c_size_t(rank), C.c_size_t(world)))

    def _ck(self, st):
        if st != 0 and self.callback_error is not None:
            e, self.callback_error = self.callback_error, None
            raise KeakiHostError("the exchange callback failed: %r" % (e,)) from e
        _ck(st)

    def prepare(self, d_send: int, d_recv: int) -> None:
        self._ck(_lib().keaki_host_fk_shard_prepare(self.h, C.c_void_p(d_send), C.c_void_p(d_recv), self._a2a, self._gather, None))

    def open(self, p, d_send: int, d_recv: int) -> np.ndarray:
        c = _u64(p, 4); out = np.zeros((self.domain_size, 8), np.uint64)
        self._ck(_lib().keaki_host_fk_shard_open(self.h, _p(c), C.c_size_t(c.shape[0]), C.c_void_p(d_send), C.c_void_p(d_recv), self._a2a, self._gather,
                                           None, _p(out)))
        return out

    def vec_commit_partial(self, rng: Rng, v, d_send: int, d_recv: int):
        """keaki::dist::vec_commit_partial_fk -> (partial u64[12], proofs)"""
        v = _u64(v, 4); n = v.shape[0]
        part = np.zeros(12, np.uint64); proofs = np.zeros((self.domain_size, 8), np.uint64)
        self._ck(_lib().keaki_host_vec_commit_partial_fk(rng.h, self.setup.h, _p(v), C.c_size_t(n), C.c_size_t(self.rank), C.c_size_t(self.world), self.h,
                                                   C.c_void_p(d_send), C.c_void_p(d_recv), self._a2a, self._gather, None, _p(part), _p(proofs)))
        return part, proofs

    def close(self):
        if self.h:
            _lib().keaki_host_fk_shard_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def commit_combine(setup: KZGSetup, partials) -> np.ndarray:
    pr = _u64(partials, 12); out = np.zeros(8, np.uint64)
    _ck(_lib().keaki_host_commit_combine(setup.h, _p(pr), C.c_size_t(pr.shape[0]), _p(out)))
    return out


def vec_encrypt_arrays_shard(rng: Rng, setup: KZGSetup, com, points, values, messages: np.ndarray, rank: int, world: int):
    """vec_encrypt_arrays for the items of rank `rank` only: consumes the rng exactly as the full call does (one r per item of the WHOLE
    vector, in index order), returns the ciphertexts of this rank's contiguous item range"""
    from .dist import chunk_bounds
    msgs = np.ascontiguousarray(messages, dtype=np.uint8)
    n, ml = msgs.shape
    lo, hi = chunk_bounds(n, world, rank)
    pts = np.ascontiguousarray(_u64(points, 4)[:n]); vals = np.ascontiguousarray(_u64(values, 4)[:n])
    g2 = np.zeros((hi - lo, 16), np.uint64); body = np.zeros((hi - lo, max(ml, 1)), np.uint8)
    _ck(_lib().keaki_host_vec_encrypt_shard(rng.h, setup.h, _p(_u64(com)), _p(pts), _p(vals), _p(msgs), C.c_size_t(n), C.c_size_t(ml),
                                           C.c_size_t(rank), C.c_size_t(world), _p(g2), _p(body)))
    return g2, body[:, :ml]
