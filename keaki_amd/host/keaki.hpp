// keaki.hpp -- C++ mirror of keaki's public Rust API for E = Bn254, above the C ABI of
// libkeaki_hip.so. (The reference's own toolchain, Rust, is absent from this image; INTEGRATION.md
// shows the feature-gated Rust shim that binds the same C ABI.)
//
// Same module / function names, argument meaning and error behaviour as the reference:
//   keaki::kzg::KZGSetup, commit, open, verify, KZGError::PolynomialTooLarge   (src/kzg.rs:22-151,205-209)
//   keaki::kem::encapsulate, decapsulate                                        (src/kem.rs:13-72)
//   keaki::enc::Ciphertext, encrypt, decrypt                                    (src/enc.rs:13-55)
//   keaki::vec::PADDING_LEN, vec_commit, vec_encrypt, vec_decrypt               (src/vec.rs:18-81)
// All group / pairing arithmetic runs on the GPU through the C ABI; the host only does what keaki's
// own glue does on the host: O(n) scalar-field work (Horner, quotient, iFFT), RNG draws, XOR.
// There is no CPU fallback for the group arithmetic.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/keaki_hip.h"

namespace keaki {

// ---- scalar field Fr (ark-ff Fp<MontBackend<FrConfig,4>>): 4 x u64 Montgomery limbs ------------------
struct Fr {
  uint64_t l[4] = {0, 0, 0, 0};
  static Fr zero() { return Fr(); }
  static Fr one();
  static Fr from_u64(uint64_t v);
  static Fr from_i64(int64_t v);  // Fr::from(-24) in the reference tests
  bool operator==(const Fr& o) const { return l[0] == o.l[0] && l[1] == o.l[1] && l[2] == o.l[2] && l[3] == o.l[3]; }
  bool operator!=(const Fr& o) const { return !(*this == o); }
  bool is_zero() const { return (l[0] | l[1] | l[2] | l[3]) == 0; }
  Fr operator+(const Fr& o) const;
  Fr operator-(const Fr& o) const;
  Fr operator*(const Fr& o) const;
  Fr operator-() const;
  Fr pow(uint64_t e) const;
  Fr inverse() const;  // Fermat; zero -> zero
};

// rand::Rng: the only thing keaki needs from it is next_u64 (Fr::rand draws 4 per candidate)
struct Rng {
  virtual ~Rng() {}
  virtual uint64_t next_u64() = 0;
};
// ark-ff 0.4.2 `impl Distribution<Fp> for Standard`: 4 x next_u64, clear the top 2 bits, reject >= r;
// the accepted limbs ARE the Montgomery representation (src/kem.rs:26, src/vec.rs:32).
Fr fr_rand(Rng& rng);

// ---- group elements: affine, Montgomery limbs, identity = all zero (the C-ABI encodings) --------------
struct G1 {
  std::array<uint64_t, 8> w{};
  bool operator==(const G1& o) const { return w == o.w; }
  bool operator!=(const G1& o) const { return w != o.w; }
  bool is_zero() const { for (auto x : w) if (x) return false; return true; }
};
struct G2 {
  std::array<uint64_t, 16> w{};
  bool operator==(const G2& o) const { return w == o.w; }
  bool operator!=(const G2& o) const { return w != o.w; }
};

struct HipError : std::runtime_error {
  int status;
  HipError(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};
// What `*_from_bytes` throws for bytes that do not decode: the index of the first rejected item and why (1 malformed: flags or a coordinate
// >= p; 2 no point of the curve has this x; 3 a G2 point outside the order-r subgroup) -- arkworks' SerializationError::InvalidData with a place
struct WireError : std::runtime_error {
  size_t index;
  int reason;
  WireError(size_t i, int r, const std::string& m) : std::runtime_error(m), index(i), reason(r) {}
};

// One GPU context shared by the setup objects created from it -- or, built from a LIST of ordinals, several GPUs of this process behind
// one object (keaki_hip_group_*: one context and one host thread per entry inside the library; an ordinal may repeat). With a group,
// kzg::commit / open spread the MSM over all members by SRS range (each member keeps its chunk of the SRS and that chunk's window
// tables from setup on; the 96-byte partial sums come back through host memory) and the loops of vec_encrypt / vec_decrypt are
// split by item range. Everything else (verify, single encapsulate / decapsulate, open_fk) runs on member 0, whose context ctx() returns.
class Device {
 public:
  explicit Device(int ordinal = 0);
  explicit Device(const std::vector<int>& ordinals);
  ~Device();
  Device(const Device&) = delete;
  keaki_hip_ctx* ctx() const { return ctx_; }
  keaki_hip_group* group() const { return group_; }   // null for a single-GPU device
  size_t members() const;
  void check(int status) const;        // throws HipError
  void check_group(int status) const;  // the same for keaki_hip_group_* calls
 private:
  keaki_hip_ctx* ctx_ = nullptr;
  keaki_hip_group* group_ = nullptr;
};
// batches below this many items stay on member 0 of a group (a launch per member costs more than it saves)
constexpr size_t GROUP_MIN_ITEMS = 1024;

using DensePolynomial = std::vector<Fr>;  // coefficients, low degree first (ark-poly DensePolynomial::coeffs)

namespace kzg {

// src/kzg.rs:205-209
struct KZGError {
  enum Kind { PolynomialTooLarge } kind;
  size_t degree, max_degree;  // "{0}" and "{1}" of the thiserror message
  bool operator==(const KZGError& o) const { return kind == o.kind && degree == o.degree && max_degree == o.max_degree; }
  std::string to_string() const;
};
template <class T>
struct Result {  // Result<T, KZGError>
  bool ok;
  T value;
  KZGError error;
  static Result Ok(T v) { return Result{true, std::move(v), KZGError{KZGError::PolynomialTooLarge, 0, 0}}; }
  static Result Err(KZGError e) { return Result{false, T(), e}; }
  const T& unwrap() const { if (!ok) throw std::runtime_error("called unwrap() on Err: " + error.to_string()); return value; }
};

// src/kzg.rs:22-86. g1_pow and g1_aff hold the same affine values here (the reference keeps a
// projective and an affine copy; equality and serialisation only ever see the affine value).
class KZGSetup {
 public:
  // `setup(secret, max_d)`: [secret^i]_1 for i < max_d and [secret]_2.  "Don't use this." (src/kzg.rs:54)
  static KZGSetup setup(std::shared_ptr<Device> dev, const Fr& secret, size_t max_d);
  // from already-known powers (what new_from_file produces after parsing; the .ptau parser itself is out of scope)
  static KZGSetup from_powers(std::shared_ptr<Device> dev, std::vector<G1> g1_aff, const G2& tau_g2);
  // The same with the OPTIONAL G2 powers the set openings need (open_set .. vec_encrypt_subset_batch below): g2_pow[i] = [tau^i]_2, so
  // g2_pow[0] = g2, g2_pow[1] = tau_g2, and a set of k points needs k + 1 of them. setup_with_g2 produces [secret^i]_2 for i <= max_set on the
  // device (one g2_mul_batch); from_powers_g2 takes what a ceremony file holds (new_from_file_g2, ptau.hpp, keeps all of its section 3).
  // setup, from_powers and new_from_file are unchanged and carry no G2 powers: a set call on such a setup throws, it never falls back.
  static KZGSetup setup_with_g2(std::shared_ptr<Device> dev, const Fr& secret, size_t max_d, size_t max_set);
  static KZGSetup from_powers_g2(std::shared_ptr<Device> dev, std::vector<G1> g1_aff, std::vector<G2> g2_pow);
  bool has_g2_powers() const { return !g2_pow_.empty(); }
  const std::vector<G2>& g2_pow() const { return g2_pow_; }
  keaki_hip_srs_g2* srs_g2() const;          // device handle of g2_pow on (member 0 of) the device, uploaded on first use; throws without G2 powers
  ~KZGSetup();
  KZGSetup(KZGSetup&&) noexcept;
  KZGSetup(const KZGSetup&) = delete;
  const std::vector<G1>& g1_pow() const { return g1_aff_; }
  const std::vector<G1>& g1_aff() const { return g1_aff_; }
  const G2& tau_g2() const { return tau_g2_; }
  const std::shared_ptr<Device>& device() const { return dev_; }
  // device-resident copy of the whole SRS on (member 0 of) the device. With a group it is uploaded on first use: commit / open never
  // need it (they read the per-member chunks), open_fk and the keaki::dist calls do.
  keaki_hip_srs_g1* srs() const;
  keaki_hip_group_srs_g1* group_srs() const { return gsrs_; }
  // group devices: the FK23 handle of domain size d = 2^log2d (every member's copy of srs[0..d) and its part of the SRS-only transform),
  // built on first use and kept until another size is asked for
  keaki_hip_group_fk* group_fk(unsigned log2d) const;
  // false when the optional window tables of the SRS did not fit in HBM: commit / open then run the generic per-window MSM (same results)
  bool has_window_tables() const { return tables_; }
  // this rank's chunk [lo, hi) of the SRS as a handle of its own, with its own window tables (built on first use; see keaki::dist)
  keaki_hip_srs_g1* chunk_srs(size_t lo, size_t hi) const;
 private:
  KZGSetup() {}
  std::shared_ptr<Device> dev_;
  std::vector<G1> g1_aff_;
  G2 tau_g2_;
  mutable keaki_hip_srs_g1* srs_ = nullptr;  // device-resident copy of g1_aff, uploaded once
  keaki_hip_group_srs_g1* gsrs_ = nullptr;   // group devices: one chunk (+ its window tables) per member
  mutable keaki_hip_group_fk* gfk_ = nullptr;
  mutable unsigned gfk_log2d_ = 0;
  bool tables_ = false;
  std::vector<G2> g2_pow_;                      // empty: no set openings on this setup
  mutable keaki_hip_srs_g2* srs_g2_ = nullptr;
  mutable keaki_hip_srs_g1* chunk_ = nullptr;
  mutable size_t chunk_lo_ = 0, chunk_hi_ = 0;
};

Result<G1> commit(const KZGSetup& setup, const DensePolynomial& p);                          // src/kzg.rs:89-101
Result<G1> open(const KZGSetup& setup, const DensePolynomial& p, const Fr& point);           // src/kzg.rs:104-124
Result<bool> verify(const KZGSetup& setup, const G1& commitment, const Fr& point, const Fr& value, const G1& proof);  // :127-151
// m polynomials over one setup in ONE device call each (no counterpart in the reference; generalise commit, :89-101, and open, :104-124):
// keaki_hip_msm_g1_batch / keaki_hip_kzg_open_batch with the rows zero-padded to the longest polynomial (a zero coefficient contributes nothing,
// which is what DensePolynomial's trimming means). PolynomialTooLarge is raised first, for the first polynomial that is too long, as commit /
// open raise it. Results equal the loop over commit / open; below COMMIT_BATCH_MIN polynomials, and on a device group, that loop is what runs.
constexpr size_t COMMIT_BATCH_MIN = 5;      // a batch call costs 1.8-2.5 ms up to m = 16 (profiles/msm_batch.txt), a single commit through the window tables a setup builds 0.4-0.7 ms
Result<std::vector<G1>> commit_batch(const KZGSetup& setup, const std::vector<DensePolynomial>& polys);
Result<std::vector<G1>> open_batch(const KZGSetup& setup, const std::vector<DensePolynomial>& polys, const std::vector<Fr>& points);
// n openings at once (no counterpart in the reference; generalises :127-148): draws one gamma_i = Fr::rand per item from `rng` in index order
// and checks e(L, g2) == e(R, [tau]_2) for L = sum gamma_i C_i - (sum gamma_i y_i) g1 + sum (gamma_i z_i) proof_i, R = sum gamma_i proof_i
// in ONE device call (keaki_hip_kzg_verify_batch: two or three MSMs and two pairings whatever n is). All openings valid: always true. One
// invalid: false except with probability <= 1/r over the draws -- `rng` must be unpredictable to whoever produced the proofs.
// commitments: one (shared by all items) or one per item. Below VERIFY_BATCH_MIN items the draws still happen (the stream of `rng` does not
// depend on the path) and the items are checked one by one with `verify`, which is faster there. On a group device: member 0.
constexpr size_t VERIFY_BATCH_MIN = 5;      // measured: a batch call costs 6.9 ms at n <= 16, a single verify 1.68 ms (profiles/verify_batch.txt)
Result<bool> verify_batch(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points,
                          const std::vector<Fr>& values, const std::vector<G1>& proofs);
// the same on contiguous buffers. n_coms: 1 or n. roots_of_unity: `points` is ONE Fr omega and item i is opened at omega^i.
bool verify_batch_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values,
                       const uint64_t* proofs, size_t n);
// One verdict per opening (no counterpart in the reference): out[i] = 0 iff e(C_i - y_i g1 + z_i proof_i, g2) e(-proof_i, [tau]_2) == 1, the
// predicate of :135-148 with z_i proof_i moved across the pairing, in ONE device call (keaki_hip_kzg_verify_each: both G2 arguments are fixed,
// so both line sequences are tables, and the two Miller loops share one final exponentiation). Exact: no draws, no error probability; the
// verdict equals `verify` on the item. commitments: one (shared) or one per item. On a group device: member 0.
Result<std::vector<uint8_t>> verify_each(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points, const std::vector<Fr>& values,
                                         const std::vector<G1>& proofs);
// the same on contiguous buffers (arguments as verify_batch_flat); status_out: n bytes. Returns the number of invalid items.
size_t verify_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values, const uint64_t* proofs,
                        size_t n, uint8_t* status_out);
// Which openings are invalid? verify_batch first -- it draws from `rng` exactly what verify_batch draws -- and verify_each only if that rejects:
// the indices of the invalid items in ascending order, empty for a clean batch.
std::vector<size_t> locate_invalid(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points, const std::vector<Fr>& values,
                                   const std::vector<G1>& proofs);
std::vector<size_t> locate_invalid_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values,
                                        const uint64_t* proofs, size_t n);
// Proofs (any G1 points) on the wire: n x 32 B, `serialize_compressed`. `proofs_from_bytes` validates (canonical, on the curve; G1 has cofactor 1)
// and throws WireError naming the first bad index.
std::vector<uint8_t> proofs_to_bytes(const KZGSetup& setup, const std::vector<G1>& proofs);
std::vector<G1> proofs_from_bytes(const KZGSetup& setup, const std::vector<uint8_t>& bytes);
void proofs_to_bytes_flat(const KZGSetup& setup, const uint64_t* proofs, size_t n, uint8_t* wire_out);
void proofs_from_bytes_flat(const KZGSetup& setup, const uint8_t* wire, size_t n, uint64_t* proofs_out);
// ---- set openings (no counterpart in the reference: its open / verify take one point; the batch opening of the KZG paper) -----------------
// ONE proof pi_S = [((p - I) / Z)(tau)]_1 for the k <= KEAKI_SET_MAX points, Z = prod (x - z_j), I the interpolant of the values; checked by
// e(C - [I(tau)]_1, g2) == e(pi_S, [Z(tau)]_2). The device library does not look for repeated points (a repeat makes the weights meaningless):
// THIS layer refuses them -- every function below sorts a copy of the points and throws SetError when two are equal -- and it throws SetError
// on a setup without G2 powers (verify_set and everything that encrypts; open_set and aggregate_proofs need none). Single device or member 0.
struct SetError : std::invalid_argument { using std::invalid_argument::invalid_argument; };
// (proof, the k values p(z_j)) in one device call (keaki_hip_kzg_open_multi). PolynomialTooLarge as `open` raises it.
Result<std::pair<G1, std::vector<Fr>>> open_set(const KZGSetup& setup, const DensePolynomial& p, const std::vector<Fr>& points);
bool verify_set(const KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points, const std::vector<Fr>& values, const G1& proof);
// pi_S = sum_j c_j pi_j from the k single proofs, without the polynomial (keaki_hip_kzg_aggregate): byte for byte open_set's proof
G1 aggregate_proofs(const KZGSetup& setup, const std::vector<Fr>& points, const std::vector<G1>& proofs);
// what the set ciphertexts are made of: (C - [I(tau)]_1, [Z(tau)]_2) for the tuple (points, values); two small MSMs and one sum on the device
std::pair<G1, G2> set_pair(const KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points, const std::vector<Fr>& values);
// all openings at the roots of unity of a size-d domain (src/kzg.rs:157-203): FK23 -- three G1 FFTs + 2d scalar-mults on
// the GPU (keaki_hip_open_fk) when p.size() == domain_size is a power of two; per-point `open` otherwise.
Result<std::vector<G1>> open_fk(const KZGSetup& setup, const std::vector<Fr>& p, size_t domain_size);
// setup-time: tabulate the SRS-only part of open_fk (hat_s) for power-of-two domain size d, so the first open_fk does not pay for it
void precompute_open_fk(const KZGSetup& setup, size_t domain_size);
// The set-opening counterpart of open_fk (no counterpart in the reference): the r = domain_size / l set proofs of the l-point cosets
// {i + t r : t < l} of the size-domain_size domain, in one device call (keaki_hip_open_fk_cosets_poly). Proof i is byte for byte
// open_set(p, the coset's points).first and is checked by verify_set / vec_verify_subset. p.size() <= domain_size (zero-padded); domain_size and l
// powers of two, l <= min(domain_size, KEAKI_SET_MAX), domain_size <= the SRS: anything else throws SetError. Single device or member 0.
std::vector<G1> open_fk_cosets(const KZGSetup& setup, const std::vector<Fr>& p, size_t domain_size, size_t l);
// The verifier's counterpart (no counterpart in the reference): n set proofs over cosets of ONE size l in one device call
// (keaki_hip_kzg_verify_cosets: three or four MSMs and two pairings whatever n is, against n x verify_set). Item k: commitments[k] (or the one
// commitment of all items), the coset shifts[k] <omega_l> (omega_l: the generator of Radix2Domain::create(l)), its l values values[k * l + t] =
// p_k(shifts[k] omega_l^t), proofs[k]. Draws one Fr::rand per item in index order (the gammas of the combination, as verify_batch). All items
// valid: always true; one invalid: false except with probability <= 1 / r. Needs a setup whose G2 powers reach [tau^l]_2 (g2_pow().size() > l);
// refuses (SetError) a zero shift -- the device library does not look --, an l that is not a power of two or exceeds KEAKI_SET_MAX or the SRS,
// array sizes that disagree, and a device group (single device only). A rejected batch says nothing about WHICH item: verify_set per coset does.
bool verify_cosets(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& shifts, size_t l, const std::vector<Fr>& values,
                   const std::vector<G1>& proofs);
// the same on contiguous buffers, with the value addressing of the device call: value (k, t) is values[k * item_stride + t * t_stride]; roots_of_unity:
// `shifts` is ONE Fr omega and item k has the shift omega^k (nothing to refuse: a power of a root of unity is not zero)
bool verify_cosets_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values,
                        size_t item_stride, size_t t_stride, size_t l, const uint64_t* proofs, size_t n);
// The per-item points of the same check (keaki_hip_kzg_coset_pairs): lhs_out[8 k ..] = A_k = C_k - [I_k(tau)]_1 (affine words), c_out[k] = shifts[k]^l.
// Arguments and refusals as verify_cosets_flat, but nothing is drawn and no G2 power is needed.
void coset_pairs_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values, size_t item_stride,
                      size_t t_stride, size_t l, size_t n, uint64_t* lhs_out, Fr* c_out);
// WHICH items are invalid (keaki_hip_kzg_verify_cosets_each): one byte per item, 0 = the set proof holds, 1 = it does not. Exact -- nothing is
// drawn --, and equal to verify_set on the l points of the item. Arguments and refusals as verify_cosets_flat.
std::vector<uint8_t> verify_cosets_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values,
                                             size_t item_stride, size_t t_stride, size_t l, const uint64_t* proofs, size_t n);
// n set proofs over ARBITRARY point sets -- what open_set, aggregate_proofs and vec_open_subset hand out -- in one device call per set size
// (keaki_hip_kzg_verify_sets: a batched MSM over the proofs, two or three more MSMs, k + 1 Miller loops and ONE final exponentiation whatever n is,
// against n x verify_set). Item i: commitments[i] (or the one commitment of all items), its points[i] (1 .. KEAKI_VERIFY_SETS_K_MAX of them, distinct),
// values[i] (one per point), proofs[i]. Draws one Fr::rand per item in index order BEFORE anything else is looked at per group; items of unequal size
// are grouped by size into one call each (the device call takes one k), and the verdict is the AND of the groups'. All items valid: always true; one
// invalid: false except with probability <= 1 / r. Refuses (SetError): a repeated point within an item -- the device library does not look --, an empty
// or too large set, array sizes that disagree, a setup whose G2 powers do not reach the largest set (g2_pow().size() > k), a set larger than the SRS,
// and a device group (single device only). A rejected batch says nothing about WHICH item: verify_set per item does.
bool verify_sets(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                 const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);
// ONE group of the above on contiguous buffers: n items of k points, point (i, j) = points[i * k + j] -- or, with `omega`, the u32 domain index at that
// place (z = omega^index, derived on the device) --, value (i, j) = values[i * k + j], the gammas GIVEN (the grouping layers draw them). Refuses what
// can be told without looking at the points: k, n_coms, the G2 powers, the SRS, a device group.
bool verify_sets_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k,
                      const uint64_t* proofs, const Fr* gammas, size_t n);
// verify_sets for ONE commitment with the points given as indices into the powers of `omega` (an element of order `domain`): what vec::vec_verify_subsets
// is made of. Draws, grouping and refusals as verify_sets; also refuses an index >= domain and a repeated index within an item.
bool verify_sets_indexed(Rng& rng, const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                         const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);

// The per-item side of verify_sets (keaki_hip_kzg_set_pairs, keaki_hip_kzg_verify_sets_each). Nothing is drawn: the results are exact.
// set_pairs_flat: ONE group on contiguous buffers, addressed as verify_sets_flat: lhs_out[8 i ..] = A_i = C_i - [I_i(tau)]_1, z2_out[16 i ..] = Z2_i =
// [Z_i(tau)]_2 (affine words, zeros = the identity). verify_sets_each_flat: one byte per item, 0 = the set proof holds (= verify_set on the item).
// Both refuse what verify_sets_flat refuses.
void set_pairs_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k, size_t n,
                    uint64_t* lhs_out, uint64_t* z2_out);
std::vector<uint8_t> verify_sets_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k,
                                           const uint64_t* proofs, size_t n);
// Items of unequal size, grouped by size into one device call each as verify_sets does, the results back in item order. Refusals as verify_sets (a repeated
// point within an item, an empty or too large set, sizes that disagree, G2 powers that do not reach the largest set, a device group), all before any call.
// set_pairs: lhs_out n x 8 words, z2_out n x 16 words. The _indexed forms take ONE commitment and domain indices (z = omega^index, derived on the device)
// and also refuse an index >= domain and a repeated index.
void set_pairs(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points, const std::vector<std::vector<Fr>>& values,
               uint64_t* lhs_out, uint64_t* z2_out);
void set_pairs_indexed(const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                       const std::vector<std::vector<Fr>>& values, uint64_t* lhs_out, uint64_t* z2_out);
std::vector<uint8_t> verify_sets_each(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                                      const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);
std::vector<uint8_t> verify_sets_each_indexed(const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                                              const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);

}  // namespace kzg

namespace kem {
// What encapsulate_sets, enc::encrypt_sets and vec::vec_encrypt_subsets end in, on the n pairs of kzg::set_pairs: one r per item in index order, ONE
// keaki_hip_encrypt_multi / _encap_multi call with n groups of one item (coms := A, points = values = 0: key_i = KDF(e(r_i A_i, g2))), then ct_i = r_i Z2_i by ONE
// keaki_hip_g2_mul_batch. msgs (n x msg_len) given: bodies_out = msgs ^ keys; null: bodies_out = the keys. Every item equals encapsulate_set / encrypt_set
// alone with the same r, byte for byte.
void seal_pairs(Rng& rng, const kzg::KZGSetup& setup, const uint64_t* lhs, const uint64_t* z2, size_t n, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out,
                uint8_t* bodies_out);
// src/kem.rs:13-50 / :55-72
std::pair<G2, std::vector<uint8_t>> encapsulate(Rng& rng, const kzg::KZGSetup& setup, const G1& commitment, const Fr& point,
                                                const Fr& value, size_t msg_len);
std::vector<uint8_t> decapsulate(const kzg::KZGSetup& setup, const G1& proof, const G2& ciphertext, size_t msg_len);
// setup-time (optional): the tables of encapsulation that depend on the setup only (generators, [tau]_2, e(g1, g2)), for batches of
// `batch_hint` items per call -- on every member of a group device for its share. Like the SRS window tables: results never depend on it.
void prepare(const kzg::KZGSetup& setup, size_t batch_hint);
// Witness encryption to a SET claim: readable by whoever holds the set proof of `commitment` for (points, values). Draws ONE Fr::rand for r;
// ct = r [Z(tau)]_2 (g2_mul_batch), key = KDF(e(r (C - [I(tau)]_1), g2)) (g1_mul_batch, then decap_batch against g2). One G2 point whatever k is.
// Decapsulation is the UNCHANGED decapsulate(setup, pi_S, ct, msg_len) above: e(pi_S, r [Z]_2) is the same GT element; there is no second function.
std::pair<G2, std::vector<uint8_t>> encapsulate_set(Rng& rng, const kzg::KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points,
                                                    const std::vector<Fr>& values, size_t msg_len);
// encapsulate_set for n items, each with its own point set (and its own commitment, or the one of all), in one kzg::set_pairs and one seal_pairs. Every refusal
// (kzg::set_pairs's) comes before the first draw; then one r per item in index order.
std::vector<std::pair<G2, std::vector<uint8_t>>> encapsulate_sets(Rng& rng, const kzg::KZGSetup& setup, const std::vector<G1>& commitments,
                                                                  const std::vector<std::vector<Fr>>& points, const std::vector<std::vector<Fr>>& values, size_t msg_len);
}  // namespace kem

namespace enc {
using Ciphertext = std::pair<G2, std::vector<uint8_t>>;  // src/enc.rs:13
Ciphertext encrypt(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr& point, const Fr& value, const std::vector<uint8_t>& msg);
std::vector<uint8_t> decrypt(const kzg::KZGSetup& setup, const G1& proof, const Ciphertext& ct);
// encapsulate_set plus the XOR; decryption is the unchanged decrypt(setup, pi_S, ct)
Ciphertext encrypt_set(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& points, const std::vector<Fr>& values,
                       const std::vector<uint8_t>& msg);
// encrypt_set for n items with their own point sets (kem::encapsulate_sets plus the XOR); messages: one per item, all of one length. The unchanged decrypt
// with the set proof of item i opens ciphertext i.
std::vector<Ciphertext> encrypt_sets(Rng& rng, const kzg::KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                                     const std::vector<std::vector<Fr>>& values, const std::vector<std::vector<uint8_t>>& messages);
// Ciphertexts on the wire: n x (64 B compressed G2 point + body), the point as ark-serialize `serialize_compressed` writes it
// (include/keaki_hip.h: compressed point wire format), all bodies of one length. The points are compressed / decompressed on the device in one
// call. `ciphertexts_from_bytes` VALIDATES like `deserialize_compressed`: canonical encoding, on the twist, in the order-r subgroup (the points
// come from the other party and go into a pairing); bytes that fail throw WireError naming the first bad index. On a group device: member 0.
std::vector<uint8_t> ciphertexts_to_bytes(const kzg::KZGSetup& setup, const std::vector<Ciphertext>& cts);
std::vector<Ciphertext> ciphertexts_from_bytes(const kzg::KZGSetup& setup, const std::vector<uint8_t>& bytes, size_t msg_len);
// the same on contiguous arrays: ct_g2 n x u64[16], bodies n x msg_len, wire n x (64 + msg_len)
void ciphertexts_to_bytes_flat(const kzg::KZGSetup& setup, const uint64_t* ct_g2, const uint8_t* bodies, size_t n, size_t msg_len, uint8_t* wire_out);
void ciphertexts_from_bytes_flat(const kzg::KZGSetup& setup, const uint8_t* wire, size_t n, size_t msg_len, uint64_t* ct_g2_out, uint8_t* bodies_out);
}  // namespace enc

namespace vec {
constexpr size_t PADDING_LEN = 1;  // src/vec.rs:18
// Radix2EvaluationDomain over Fr (ark-poly): size = next power of two >= n, generator of that order
struct Radix2Domain {
  size_t size; Fr group_gen, group_gen_inv, size_inv;
  static Radix2Domain create(size_t min_size);
  std::vector<Fr> elements() const;
  std::vector<Fr> ifft(std::vector<Fr> evals) const;  // pads with zeros to `size`
  std::vector<Fr> fft(std::vector<Fr> coeffs) const;
};
// src/vec.rs:22-49
std::pair<G1, std::vector<G1>> vec_commit(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v);
// the same on contiguous buffers: proofs_out = domain_size affine points (8 words each). For domains of >= 2^12 evaluations on a single-GPU
// device everything behind the padding draw is ONE device call (keaki_hip_vec_commit: iFFT, FK23 openings, commit; the coefficients never
// return to the host); smaller domains and group devices take the steps one by one. Same values either way.
G1 vec_commit_flat(Rng& rng, const kzg::KZGSetup& setup, const Fr* v, size_t n, uint64_t* proofs_out);
// m vectors over ONE domain -- Radix2Domain::create(longest + PADDING_LEN), which is every vector's own domain when their lengths round to the
// same power of two -- in one device call (keaki_hip_vec_commit_batch; domains up to 2^12 run its batch kernels). One padding scalar per vector,
// drawn in index order, the rule vec_commit follows; (commitment, proofs) per vector as vec_commit returns them over that domain. Single device only.
std::vector<std::pair<G1, std::vector<G1>>> vec_commit_batch(Rng& rng, const kzg::KZGSetup& setup, const std::vector<std::vector<Fr>>& vecs);
// What src/vec.rs lacks and vector commitments are chosen for: the holder of (com, proofs) changes positions idx[t] from old_values[t] to
// new_values[t] WITHOUT the vector; afterwards com and proofs are what vec_commit returns for the changed vector with the same padding scalar. The
// domain is Radix2Domain::create(proofs.size()); indices address its evaluations (index v.size() is the padding slot), duplicates add. One device
// call (keaki_hip_vec_update): (k + 1) d scalar multiples against FK23's d (log2 d + 3). Measured (profiles/vec_update_times.txt): one entry costs a
// ninth of vec_commit at d = 2^16 and 2^20; the update wins up to k = 16 and loses at k = 64 at every measured d (break-even near k = 32, near 48
// at 2^16): above that commit afresh. Single device only.
void vec_update(const kzg::KZGSetup& setup, G1& com, std::vector<G1>& proofs, const std::vector<size_t>& idx, const std::vector<Fr>& old_values,
                const std::vector<Fr>& new_values);
// the same on contiguous buffers, taking the differences: com = 8 words (affine) in / out or null, proofs = domain_size x 8 words in / out or null
void vec_update_flat(const kzg::KZGSetup& setup, size_t domain_size, const uint32_t* idx, const Fr* deltas, size_t k, uint64_t* com_inout, uint64_t* proofs_inout);
// setup-time, optional: the update tables of (setup, domain_size) (192 bytes per evaluation; vec_update builds them on first use anyway)
void precompute_vec_update(const kzg::KZGSetup& setup, size_t domain_size);
// lines :27-37 of it (padding draw, iFFT): the coefficient vector over the whole domain, not trimmed
std::vector<Fr> vec_commit_coeffs(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v);
// lines :27-44 of it (padding draw, iFFT, open_fk): the dense coefficient vector and the proofs, without the final commit
std::pair<DensePolynomial, std::vector<G1>> vec_commit_openings(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v);
// The sibling src/vec.rs lacks: are the first v.size() proofs of a vec_commit openings of `com` to v? Item i is the opening at omega^i of the
// domain Radix2Domain::create(v.size() + PADDING_LEN) to the value v[i]; the padding slot is the committer's secret and is not checked.
// One kzg::verify_batch over the powers of the domain's generator (they are derived on the device): n draws from `rng`, one device call.
bool vec_verify(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& v, const std::vector<G1>& proofs);
bool vec_verify_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* v, size_t n, const uint64_t* proofs);
// kzg::verify_each over the same items: out[i] = 0 iff proof i opens `com` to v[i] at omega^i. No draws.
std::vector<uint8_t> vec_verify_each(const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& v, const std::vector<G1>& proofs);
size_t vec_verify_each_flat(const kzg::KZGSetup& setup, const G1& com, const Fr* v, size_t n, const uint64_t* proofs, uint8_t* status_out);
// ---- subsets of a committed vector: the set openings at the points omega^idx of Radix2Domain::create(domain_size) ---------------------------
// The holder of vec_commit's d proofs aggregates the k of them at idx (distinct, < domain_size) into one set proof, without the vector.
G1 vec_open_subset(const kzg::KZGSetup& setup, size_t domain_size, const std::vector<size_t>& idx, const std::vector<G1>& proofs);
bool vec_verify_subset(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<size_t>& idx, const std::vector<Fr>& values, const G1& proof);
// n subset proofs of ONE committed vector in one device call per subset size (kzg::verify_sets_flat with the indices as they are: the points omega^idx
// are derived on the device). Item i: the positions idx_rows[i] (distinct, < the domain), values[i] (one per position), proofs[i]. One draw per item in
// index order; subsets of unequal size are grouped by size. Refuses (kzg::SetError) a repeated index within an item, an index outside the domain,
// sizes that disagree, and what kzg::verify_sets refuses about the setup and the device.
bool vec_verify_subsets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                        const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);
// WHICH subset proofs are wrong: one byte per item (0 = valid) from kzg::verify_sets_each_indexed; nothing is drawn. Refusals as vec_verify_subsets.
std::vector<uint8_t> vec_verify_subsets_each(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                                             const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs);
// Message i to the claimed values[i] at the positions idx_rows[i] of ONE committed vector, every item with its OWN index set (vec_encrypt_subset_batch shares
// one): kzg::set_pairs_indexed, then kem::seal_pairs. msgs n x msg_len. Every refusal comes before the first draw; item i equals enc::encrypt_set on the points
// omega^idx with the same r, and the unchanged decrypt with vec_open_subset's proof opens it.
void vec_encrypt_subsets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                         const std::vector<std::vector<Fr>>& values, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
// For the holder of the vector who wants EVERY block proof: evals are the evaluations over Radix2Domain::create(evals.size()) (what vec_commit
// commits to: the vector, its padding scalar, zeros); the inverse transform, then kzg::open_fk_cosets: r = size / l proofs, proof i for the
// positions vec_coset_indices(size, l, i) = {i + t r : t < l} -- the index list vec_verify_subset and vec_encrypt_subset_batch take.
std::vector<G1> vec_open_cosets(const kzg::KZGSetup& setup, const std::vector<Fr>& evals, size_t l);
std::vector<size_t> vec_coset_indices(size_t domain_size, size_t l, size_t i);
// The counterpart of vec_open_cosets for whoever holds the evaluations: are the r = size / l proofs the block proofs of `com` for evals? ONE
// kzg::verify_cosets_flat over the vector in domain order (value (i, t) is evals[i + t r]; the shifts omega_d^i are derived on the device): r
// draws from `rng`, one device call. evals.size() <= the domain (zero-padded, as vec_open_cosets reads them), proofs.size() == r.
bool vec_verify_cosets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& evals, size_t l, const std::vector<G1>& proofs);
// evals: domain_size (a power of two) Fr; proofs: domain_size / l affine points
bool vec_verify_cosets_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* evals, size_t domain_size, size_t l, const uint64_t* proofs);
// some of the cosets: cosets[k] < size / l names the positions vec_coset_indices(domain_size, l, cosets[k]), values[k * l + t] is the value at position
// cosets[k] + t r, proofs[k] its block proof. One draw per listed coset in list order, one device call.
bool vec_verify_cosets_subset(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets,
                              const std::vector<Fr>& values, const std::vector<G1>& proofs);
// WHICH block proofs are wrong: one byte per coset (0 = valid, 1 = invalid) from ONE kzg::verify_cosets_each_flat call; nothing is drawn. The first form
// takes the vector as vec_verify_cosets does, the second the listed cosets as vec_verify_cosets_subset does; refusals as theirs.
std::vector<uint8_t> vec_verify_cosets_each(const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& evals, size_t l, const std::vector<G1>& proofs);
std::vector<uint8_t> vec_verify_cosets_each_subset(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets,
                                                   const std::vector<Fr>& values, const std::vector<G1>& proofs);
// Message k to the l claimed values of coset cosets[k], for all listed cosets in a few device calls: values[k * l + t] is the claimed value at position
// cosets[k] + t r, msgs n x msg_len. kzg::coset_pairs_flat gives A_k = C - [I_k(tau)]_1 and c_k; then one r per item in index order and ONE
// encrypt_multi (encap_multi at msg_len 0) with n groups of one item, coms := A, points := c, values := 0, tau_g2 := [tau^l]_2. Item k is byte for byte
// enc::encrypt_set on the points of coset k with the same r, and the UNCHANGED vec_decrypt with the proof of vec_open_cosets opens it. Every refusal
// (l not a power of two, a coset index out of range, a setup without [tau^l]_2, a device group) is a SetError thrown before anything is drawn from rng.
void vec_encrypt_cosets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets, const Fr* values,
                        const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
// n items over ONE index set with different value tuples (the 1-of-2^k string-OT shape): item i is readable by the holder of a vector with
// values[i * k + j] at idx[j] for all j. One r per item in index order. The rows -I_i come from ONE set_polys call and O(n k^2) host scalar
// work, [-I_i(tau)]_1 from ONE msm_g1_batch (n rows of k coefficients), C is added by one g1_sum per item, then ONE encrypt_multi call with n
// groups of one item, tau_g2 := [Z(tau)]_2, points = values = 0. Every item equals enc::encrypt_set alone with the same r. msgs: n x msg_len.
void vec_encrypt_subset_batch(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<size_t>& idx, const Fr* values,
                              size_t n, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
// src/vec.rs:52-69: one Fr::rand per item in index order, then ONE batched GPU call for all items
std::vector<enc::Ciphertext> vec_encrypt(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& points,
                                         const std::vector<Fr>& values, const std::vector<std::vector<uint8_t>>& messages);
// src/vec.rs:72-81
void vec_encrypt_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* points, const Fr* values, const uint8_t* msgs, size_t n,
                      size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
// vec_encrypt to m commitments in one device call (keaki_hip_encrypt_multi; flat like vec_encrypt_flat): group j = the next counts[j] items of the
// item-major arrays, encrypted under coms[j]; n = the sum of counts. One r per item in GLOBAL index order, which is the stream of m consecutive
// vec_encrypt calls, so ct_g2_out (n x 16 words) and ct_msg_out (n x msg_len) hold what that loop returns. Single device only.
void vec_encrypt_batch(Rng& rng, const kzg::KZGSetup& setup, const G1* coms, const size_t* counts, size_t m, const Fr* points, const Fr* values,
                       const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
void vec_decrypt_flat(const kzg::KZGSetup& setup, const uint64_t* proofs, const uint64_t* ct_g2, const uint8_t* ct_msgs, size_t n, size_t msg_len,
                      uint8_t* msgs_out);
std::vector<std::vector<uint8_t>> vec_decrypt(const kzg::KZGSetup& setup, const std::vector<G1>& proofs,
                                              const std::vector<const enc::Ciphertext*>& cts);
}  // namespace vec

// ---- one process per GPU: the same calls with the work split over `world` ranks ------------------------------------------------------
// commit's MSM (src/kzg.rs:98) shards by contiguous coefficient / point range: every rank runs a complete Pippenger on its range and
// emits one 96-byte normalised-Jacobian partial; the CALLER exchanges the partials (RCCL all-gather in the harness, any transport
// in an application: the library never opens a connection) and every rank adds them. EC addition is exact, so the affine result equals
// the single-GPU one bit for bit. The loops of vec_encrypt / vec_decrypt (src/vec.rs:63-66, :75-78) shard by item, no exchange at all.
namespace dist {
struct Shard {
  size_t rank = 0, world = 1;
  // contiguous range of rank `rank` out of n units; sizes differ by at most one
  std::pair<size_t, size_t> bounds(size_t n) const;
};
using Partial = std::array<uint64_t, 12>;   // normalised Jacobian (x, y, 1) or (1, 1, 0)
// setup-time: this rank's SRS chunk as a handle of its own with its window tables (commit_partial would build them on first use)
void prepare(const kzg::KZGSetup& setup, const Shard& sh);
// this rank's share of kzg::commit: sum over i in bounds(setup.len) and i < p.size() of p[i] [tau^i]_1. Same error as commit.
kzg::Result<Partial> commit_partial(const kzg::KZGSetup& setup, const DensePolynomial& p, const Shard& sh);
// vec_commit with the final commit (src/vec.rs:46) left as this rank's partial. Padding draw, iFFT and the FK23 openings are REPLICATED:
// every rank runs them with the same rng stream and gets the same proofs (vec_commit_partial_fk shards the openings too).
std::pair<Partial, std::vector<G1>> vec_commit_partial(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v, const Shard& sh);
// ---- kzg::open_fk (FK23, src/kzg.rs:157-203) sharded over the ranks: every rank does 1/world of the butterflies of the group FFTs (one
// inverse and one forward transform of size d: csrc/fft_g1.hip) and of the 2d scalar-mults (keaki_hip_fk_shard_*). Between the steps the
// ranks exchange 96-byte points: two all-to-alls of d / world^2 points per peer and one all-gather of the d / world affine proofs per
// rank and call, one all-to-all of 2d / world^2 points per peer at setup -- the one place of the whole path where xGMI bandwidth matters.
// The exchanges are the CALLER's (RCCL in an application: the library never opens a connection):
struct FkExchange {
  // d_send: `world` chunks of bytes_per_peer, chunk q for rank q; d_recv: the chunks received, in rank order. Device memory.
  // Must not return before d_recv is complete (the steps run on the Device's own stream). Returns 0, or non-zero to abort the call
  // (the function then throws std::runtime_error).
  int (*all_to_all)(void* user, void* d_send, void* d_recv, size_t bytes_per_peer);
  // d_send: bytes_per_rank of this rank; d_recv: every rank's, in rank order
  int (*all_gather)(void* user, void* d_send, void* d_recv, size_t bytes_per_rank);
  void* user;
};
class ShardedOpenFk {
 public:
  // domain_size: a power of two >= world^2 and <= the SRS; world a power of two >= 2 (can_shard). The setup must outlive every call of prepare / open.
  ShardedOpenFk(const kzg::KZGSetup& setup, size_t domain_size, const Shard& sh);
  ~ShardedOpenFk();
  ShardedOpenFk(const ShardedOpenFk&) = delete;
  static bool can_shard(const kzg::KZGSetup& setup, size_t domain_size, const Shard& sh);
  size_t buffer_bytes() const { return sizes_[0]; }       // of d_send and of d_recv (device memory, the caller's)
  size_t domain_size() const { return d_; }
  // setup time: this rank's part of hat_s = DFT_2d(reversed SRS); one all-to-all
  void prepare(void* d_send, void* d_recv, const FkExchange& ex);
  // == kzg::open_fk(setup, p, domain_size).unwrap() on every rank (p.size() == domain_size)
  std::vector<G1> open(const std::vector<Fr>& p, void* d_send, void* d_recv, const FkExchange& ex);
 private:
  const kzg::KZGSetup& setup_;
  std::shared_ptr<Device> dev_;           // keeps the context alive for the destructor even if the setup goes first
  keaki_hip_fk_shard* fk_ = nullptr;
  size_t d_ = 0, sizes_[4] = {0, 0, 0, 0};
  bool prepared_ = false;
};
// vec_commit_partial with the FK23 openings sharded as well: nothing but the padding draw and the scalar-field iFFT is replicated
std::pair<Partial, std::vector<G1>> vec_commit_partial_fk(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v, const Shard& sh,
                                                          ShardedOpenFk& fk, void* d_send, void* d_recv, const FkExchange& ex);
// the sum of all ranks' partials (in any order)
G1 commit_combine(const kzg::KZGSetup& setup, const Partial* partials, size_t world);
// vec_encrypt_flat for the items in bounds(n) only: draws ALL n values of r in index order (so every rank's stream, and therefore every
// ciphertext, equals the single-process call's) and writes (hi - lo) ciphertexts
void vec_encrypt_flat_shard(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* points, const Fr* values, const uint8_t* msgs, size_t n,
                            size_t msg_len, const Shard& sh, uint64_t* ct_g2_out, uint8_t* ct_msg_out);
}  // namespace dist

}  // namespace keaki
