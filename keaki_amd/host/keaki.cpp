// Host mirror of keaki's public API (see keaki.hpp). Group arithmetic = C-ABI calls into libkeaki_hip.so.
#include "keaki.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <sys/mman.h>

namespace keaki {

// ------------------------------------------------------------------------------------------------ Fr
namespace {
typedef unsigned __int128 u128;
const uint64_t FR_MOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
const uint64_t FR_INV = 0xc2e1f593efffffffULL;
const uint64_t FR_ONE[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
const uint64_t FR_R2[4] = {0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL};
// ark-bn254 FrConfig::TWO_ADIC_ROOT_OF_UNITY = 5^((r-1)/2^28), Montgomery form; TWO_ADICITY = 28
const uint64_t FR_TWO_ADIC_ROOT[4] = {0x636e735580d13d9cULL, 0xa22bf3742445ffd6ULL, 0x56452ac01eb203d8ULL, 0x1860ef942963f9e7ULL};
const unsigned FR_TWO_ADICITY = 28;

bool geq_mod(const uint64_t a[4]) {
  for (int i = 3; i >= 0; i--) { if (a[i] > FR_MOD[i]) return true; if (a[i] < FR_MOD[i]) return false; }
  return true;
}
void sub_mod_raw(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  u128 br = 0;
  for (int i = 0; i < 4; i++) { u128 t = (u128)a[i] - b[i] - (uint64_t)br; r[i] = (uint64_t)t; br = (t >> 64) & 1; }
}
void mont_mul(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) { c += (u128)a[j] * b[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
    uint64_t m = t[0] * FR_INV;
    c = (u128)m * FR_MOD[0] + t[0]; c >>= 64;
    for (int j = 1; j < 4; j++) { c += (u128)m * FR_MOD[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
  }
  if (t[4] || geq_mod(t)) sub_mod_raw(t, t, FR_MOD);
  memcpy(r, t, 32);
}
}  // namespace

Fr Fr::one() { Fr r; memcpy(r.l, FR_ONE, 32); return r; }
Fr Fr::from_u64(uint64_t v) { Fr a; a.l[0] = v; Fr r; mont_mul(r.l, a.l, FR_R2); return r; }
Fr Fr::from_i64(int64_t v) { return v >= 0 ? from_u64((uint64_t)v) : -from_u64((uint64_t)(-(v + 1)) + 1); }
Fr Fr::operator+(const Fr& o) const {
  Fr r; u128 c = 0;
  for (int i = 0; i < 4; i++) { c += (u128)l[i] + o.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
  if (c || geq_mod(r.l)) sub_mod_raw(r.l, r.l, FR_MOD);
  return r;
}
Fr Fr::operator-(const Fr& o) const {
  Fr r; u128 br = 0;
  for (int i = 0; i < 4; i++) { u128 t = (u128)l[i] - o.l[i] - (uint64_t)br; r.l[i] = (uint64_t)t; br = (t >> 64) & 1; }
  if (br) { u128 c = 0; for (int i = 0; i < 4; i++) { c += (u128)r.l[i] + FR_MOD[i]; r.l[i] = (uint64_t)c; c >>= 64; } }
  return r;
}
Fr Fr::operator*(const Fr& o) const { Fr r; mont_mul(r.l, l, o.l); return r; }
Fr Fr::operator-() const { return is_zero() ? *this : Fr::zero() - *this; }
Fr Fr::pow(uint64_t e) const {
  Fr acc = Fr::one(), b = *this;
  while (e) { if (e & 1) acc = acc * b; b = b * b; e >>= 1; }
  return acc;
}
Fr Fr::inverse() const {
  uint64_t e[4], two[4] = {2, 0, 0, 0};
  sub_mod_raw(e, FR_MOD, two);
  Fr acc = Fr::one();
  for (int i = 255; i >= 0; i--) { acc = acc * acc; if ((e[i >> 6] >> (i & 63)) & 1) acc = acc * *this; }
  return acc;
}
Fr fr_rand(Rng& rng) {
  for (;;) {
    Fr r;
    for (int i = 0; i < 4; i++) r.l[i] = rng.next_u64();
    r.l[3] &= 0xFFFFFFFFFFFFFFFFULL >> 2;
    if (!geq_mod(r.l)) return r;
  }
}

// ------------------------------------------------------------------------------------------------ Device
Device::Device(int ordinal) {
  int st = keaki_hip_ctx_create(ordinal, nullptr, &ctx_);
  if (st != KEAKI_OK) throw HipError(st, keaki_hip_last_error(nullptr));
}
Device::Device(const std::vector<int>& ordinals) {
  std::vector<int32_t> d(ordinals.begin(), ordinals.end());
  int st = keaki_hip_group_create(d.data(), d.size(), &group_);
  if (st != KEAKI_OK) throw HipError(st, keaki_hip_group_last_error(nullptr));
  ctx_ = keaki_hip_group_ctx(group_, 0);       // owned by the group
}
Device::~Device() {
  if (group_) keaki_hip_group_destroy(group_);
  else keaki_hip_ctx_destroy(ctx_);
}
size_t Device::members() const { return group_ ? keaki_hip_group_size(group_) : 1; }
void Device::check(int status) const {
  if (status != KEAKI_OK) throw HipError(status, keaki_hip_last_error(ctx_));
}
void Device::check_group(int status) const {
  if (status != KEAKI_OK) throw HipError(status, keaki_hip_group_last_error(group_));
}

namespace {
// Montgomery limbs of the BN254 generators (ark-bn254 g1.rs / g2.rs): G1 = (1, 2)
const uint64_t G1_GEN_W[8] = {0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL,
                              0xa6ba871b8b1e1b3aULL, 0x14f1d651eb8e167bULL, 0xccdd46def0f28c58ULL, 0x1c14ef83340fbe5eULL};
G1 g1_generator() { G1 g; memcpy(g.w.data(), G1_GEN_W, 64); return g; }
G2 g2_generator(const Device& dev) {
  // obtained from the device library so there is one source of truth for the G2 generator:
  // 1 * g2 via the fixed-generator path of encap (ct = r * (tau_g2 - 0 * g2) with tau_g2 = ... ) would be
  // roundabout; instead keep the constant here.
  static const uint64_t W[16] = {0x8e83b5d102bc2026ULL, 0xdceb1935497b0172ULL, 0xfbb8264797811adfULL, 0x19573841af96503bULL,
                                 0xafb4737da84c6140ULL, 0x6043dd5a5802d8c4ULL, 0x09e950fc52a02f86ULL, 0x14fef0833aea7b6bULL,
                                 0x619dfa9d886be9f6ULL, 0xfe7fd297f59e9b78ULL, 0xff9e1a62231b7dfeULL, 0x28fd7eebae9e4206ULL,
                                 0x64095b56c71856eeULL, 0xdc57f922327d3cbbULL, 0x55f935be33351076ULL, 0x0da4a0e693fd6482ULL};
  (void)dev;
  G2 g; memcpy(g.w.data(), W, 128); return g;
}
// normalised Jacobian (x, y, 1 | 1, 1, 0) -> affine encoding
G1 jac_to_g1(const uint64_t j[12]) {
  G1 r;
  if (j[8] | j[9] | j[10] | j[11]) memcpy(r.w.data(), j, 64);
  return r;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ kzg
namespace kzg {

std::string KZGError::to_string() const {
  return "Can't commit to polynomial: polynomial has degree " + std::to_string(degree) + " but max degree is " + std::to_string(max_degree);
}

KZGSetup::~KZGSetup() {
  if (chunk_ && dev_) keaki_hip_srs_g1_free(dev_->ctx(), chunk_);
  if (srs_ && dev_) keaki_hip_srs_g1_free(dev_->ctx(), srs_);
  if (srs_g2_ && dev_) keaki_hip_srs_g2_free(dev_->ctx(), srs_g2_);
  if (gsrs_ && dev_) keaki_hip_group_srs_g1_free(dev_->group(), gsrs_);
  if (gfk_ && dev_) keaki_hip_group_fk_free(dev_->group(), gfk_);
}
KZGSetup::KZGSetup(KZGSetup&& o) noexcept
    : dev_(std::move(o.dev_)), g1_aff_(std::move(o.g1_aff_)), tau_g2_(o.tau_g2_), srs_(o.srs_), gsrs_(o.gsrs_), gfk_(o.gfk_), gfk_log2d_(o.gfk_log2d_),
      tables_(o.tables_), g2_pow_(std::move(o.g2_pow_)), srs_g2_(o.srs_g2_), chunk_(o.chunk_), chunk_lo_(o.chunk_lo_), chunk_hi_(o.chunk_hi_) {
  o.srs_g2_ = nullptr;
  o.srs_ = nullptr; o.chunk_ = nullptr; o.gsrs_ = nullptr; o.gfk_ = nullptr;
}
keaki_hip_group_fk* KZGSetup::group_fk(unsigned log2d) const {
  if (gfk_ && gfk_log2d_ == log2d) return gfk_;
  if (gfk_) { keaki_hip_group_fk_free(dev_->group(), gfk_); gfk_ = nullptr; }
  vec::Radix2Domain d2 = vec::Radix2Domain::create((size_t)2 << log2d);
  dev_->check_group(keaki_hip_group_fk_create(dev_->group(), g1_aff_[0].w.data(), log2d, d2.group_gen.l, d2.group_gen_inv.l, d2.size_inv.l, &gfk_));
  gfk_log2d_ = log2d;
  return gfk_;
}
keaki_hip_srs_g1* KZGSetup::srs() const {
  if (!srs_) dev_->check(keaki_hip_srs_g1_upload(dev_->ctx(), g1_aff_.empty() ? nullptr : g1_aff_[0].w.data(), g1_aff_.size(), &srs_));
  return srs_;
}

// window tables are an optimisation: when they do not fit (KEAKI_ERR_OOM) the handle keeps working through the generic path
static bool try_precompute(const Device& dev, keaki_hip_srs_g1* srs) {
  const int st = keaki_hip_srs_g1_precompute(dev.ctx(), srs, nullptr);
  if (st == KEAKI_ERR_OOM) return false;
  dev.check(st);
  return true;
}

keaki_hip_srs_g1* KZGSetup::chunk_srs(size_t lo, size_t hi) const {
  if (lo == 0 && hi == g1_aff_.size()) return srs();            // one rank: the chunk is the SRS, its tables are there already
  if (chunk_ && chunk_lo_ == lo && chunk_hi_ == hi) return chunk_;
  if (chunk_) { keaki_hip_srs_g1_free(dev_->ctx(), chunk_); chunk_ = nullptr; }
  dev_->check(keaki_hip_srs_g1_slice(dev_->ctx(), srs(), lo, hi - lo, &chunk_));
  chunk_lo_ = lo; chunk_hi_ = hi;
  if (tables_ && hi > lo) (void)try_precompute(*dev_, chunk_);
  return chunk_;
}

KZGSetup KZGSetup::from_powers(std::shared_ptr<Device> dev, std::vector<G1> g1_aff, const G2& tau_g2) {
  KZGSetup s;
  s.dev_ = std::move(dev);
  s.g1_aff_ = std::move(g1_aff);
  s.tau_g2_ = tau_g2;
  if (s.dev_->group()) {
    // several GPUs in this process: chunk i of the SRS and its window tables live on member i from now on (src/kzg.rs:98 reads them)
    s.dev_->check_group(keaki_hip_group_srs_g1_upload(s.dev_->group(), s.g1_aff_.empty() ? nullptr : s.g1_aff_[0].w.data(), s.g1_aff_.size(), 1, &s.gsrs_));
    s.tables_ = keaki_hip_group_srs_g1_has_tables(s.gsrs_) != 0;    // a member whose table build ran out of memory keeps the generic MSM
    return s;
  }
  s.dev_->check(keaki_hip_srs_g1_upload(s.dev_->ctx(), s.g1_aff_.empty() ? nullptr : s.g1_aff_[0].w.data(), s.g1_aff_.size(), &s.srs_));
  // The SRS never changes after setup: tabulate [2^(window offset)] tau^i G1 once so that every later commit/open runs the
  // shared-bucket MSM (W x the SRS in HBM). It pays at every size: a 1000-coefficient commit takes 0.64 ms with tables, 1.98 ms
  // without (the per-window sums need ~250 serial doublings). KEAKI_PRECOMPUTE_MIN raises the smallest SRS that gets tables.
  const char* pm = getenv("KEAKI_PRECOMPUTE_MIN");
  const size_t pre_min = pm ? (size_t)atoll(pm) : (size_t)1;
  if (s.g1_aff_.size() >= pre_min) s.tables_ = try_precompute(*s.dev_, s.srs_);
  return s;
}

KZGSetup KZGSetup::setup(std::shared_ptr<Device> dev, const Fr& secret, size_t max_d) {
  // g1_pow[i] = g1 * secret^i (src/kzg.rs:59-61), tau_g2 = g2 * secret (:57); batched on the GPU
  std::vector<Fr> pw(max_d);
  Fr acc = Fr::one();
  for (size_t i = 0; i < max_d; i++) { pw[i] = acc; acc = acc * secret; }
  std::vector<G1> pts(max_d);
  G1 g1 = g1_generator();
  if (max_d) dev->check(keaki_hip_g1_mul_batch(dev->ctx(), g1.w.data(), 0, pw[0].l, max_d, pts[0].w.data()));
  G2 g2 = g2_generator(*dev), tau;
  dev->check(keaki_hip_g2_mul_batch(dev->ctx(), g2.w.data(), 0, secret.l, 1, tau.w.data()));
  return from_powers(std::move(dev), std::move(pts), tau);
}

static void trim(DensePolynomial& p);
KZGSetup KZGSetup::from_powers_g2(std::shared_ptr<Device> dev, std::vector<G1> g1_aff, std::vector<G2> g2_pow) {
  if (g2_pow.size() < 2) throw SetError("from_powers_g2: needs at least g2 and [tau]_2");
  KZGSetup s = from_powers(std::move(dev), std::move(g1_aff), g2_pow[1]);
  s.g2_pow_ = std::move(g2_pow);
  return s;
}
KZGSetup KZGSetup::setup_with_g2(std::shared_ptr<Device> dev, const Fr& secret, size_t max_d, size_t max_set) {
  // g2_pow[i] = g2 * secret^i, i <= max_set (at least g2 and [tau]_2), batched on the GPU like the G1 powers of `setup`
  const size_t n2 = std::max<size_t>(max_set, 1) + 1;
  std::vector<Fr> pw(n2);
  Fr acc = Fr::one();
  for (size_t i = 0; i < n2; i++) { pw[i] = acc; acc = acc * secret; }
  std::vector<G2> g2s(n2);
  G2 g2 = g2_generator(*dev);
  dev->check(keaki_hip_g2_mul_batch(dev->ctx(), g2.w.data(), 0, pw[0].l, n2, g2s[0].w.data()));
  KZGSetup s = setup(std::move(dev), secret, max_d);
  s.g2_pow_ = std::move(g2s);
  return s;
}
keaki_hip_srs_g2* KZGSetup::srs_g2() const {
  if (g2_pow_.empty()) throw SetError("this KZGSetup holds no G2 powers: build it with setup_with_g2, from_powers_g2 or new_from_file_g2");
  if (!srs_g2_) dev_->check(keaki_hip_srs_g2_upload(dev_->ctx(), g2_pow_[0].w.data(), g2_pow_.size(), &srs_g2_));
  return srs_g2_;
}

// ---- set openings ---------------------------------------------------------------------------------------------------------------------------
namespace {
// the device library does not look for repeated points: this layer does (sort a copy, compare neighbours)
void check_set(const char* what, const std::vector<Fr>& points, size_t n_values) {
  if (points.empty() || points.size() > (size_t)KEAKI_SET_MAX) throw SetError(std::string(what) + ": a set holds 1 .. " + std::to_string((int)KEAKI_SET_MAX) + " points");
  if (n_values != points.size()) throw SetError(std::string(what) + ": one value (or proof) per point");
  std::vector<std::array<uint64_t, 4>> z(points.size());
  for (size_t i = 0; i < z.size(); i++) z[i] = {points[i].l[3], points[i].l[2], points[i].l[1], points[i].l[0]};
  std::sort(z.begin(), z.end());
  if (std::adjacent_find(z.begin(), z.end()) != z.end()) throw SetError(std::string(what) + ": repeated point in the set");
}
}  // namespace
Result<std::pair<G1, std::vector<Fr>>> open_set(const KZGSetup& setup, const DensePolynomial& p_in, const std::vector<Fr>& points) {
  typedef Result<std::pair<G1, std::vector<Fr>>> Res;
  check_set("open_set", points, points.size());
  DensePolynomial p = p_in;
  trim(p);
  const size_t qlen = p.size() > 1 ? p.size() - 1 : 0;
  if (qlen > setup.g1_pow().size()) return Res::Err(KZGError{KZGError::PolynomialTooLarge, qlen, setup.g1_pow().size()});
  uint64_t jac[12];
  std::vector<Fr> values(points.size());
  setup.device()->check(keaki_hip_kzg_open_multi(setup.device()->ctx(), setup.srs(), p.empty() ? nullptr : p[0].l, p.size(), points[0].l, points.size(), jac, values[0].l));
  return Res::Ok({jac_to_g1(jac), std::move(values)});
}
bool verify_set(const KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points, const std::vector<Fr>& values, const G1& proof) {
  check_set("verify_set", points, values.size());
  const Device& dev = *setup.device();
  int32_t ok = 0;
  dev.check(keaki_hip_kzg_verify_multi(dev.ctx(), setup.srs(), setup.srs_g2(), commitment.w.data(), points[0].l, values[0].l, points.size(), proof.w.data(), &ok, nullptr));
  return ok != 0;
}
G1 aggregate_proofs(const KZGSetup& setup, const std::vector<Fr>& points, const std::vector<G1>& proofs) {
  check_set("aggregate_proofs", points, proofs.size());
  uint64_t jac[12];
  setup.device()->check(keaki_hip_kzg_aggregate(setup.device()->ctx(), points[0].l, proofs[0].w.data(), points.size(), jac));
  return jac_to_g1(jac);
}
std::pair<G1, G2> set_pair(const KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points, const std::vector<Fr>& values) {
  check_set("set_pair", points, values.size());
  // keaki_hip_kzg_verify_multi hands out the two points its predicate is evaluated on; the proof slot takes any curve point (the verdict is not used)
  const Device& dev = *setup.device();
  int32_t ok = 0;
  uint64_t pair[24];
  G1 any = g1_generator();
  dev.check(keaki_hip_kzg_verify_multi(dev.ctx(), setup.srs(), setup.srs_g2(), commitment.w.data(), points[0].l, values[0].l, points.size(), any.w.data(), &ok, pair));
  std::pair<G1, G2> out;
  memcpy(out.first.w.data(), pair, 64);
  memcpy(out.second.w.data(), pair + 8, 128);
  return out;
}

Result<G1> commit(const KZGSetup& setup, const DensePolynomial& p) {
  if (p.size() > setup.g1_pow().size())
    return Result<G1>::Err(KZGError{KZGError::PolynomialTooLarge, p.size(), setup.g1_pow().size()});
  uint64_t jac[12];
  if (setup.group_srs())
    setup.device()->check_group(keaki_hip_group_msm_g1(setup.device()->group(), setup.group_srs(), p.empty() ? nullptr : p[0].l, p.size(), jac));
  else
    setup.device()->check(keaki_hip_msm_g1(setup.device()->ctx(), setup.srs(), p.empty() ? nullptr : p[0].l, p.size(), jac));
  return Result<G1>::Ok(jac_to_g1(jac));
}

constexpr size_t OPEN_HOST_QUOTIENT_MAX = 8192;
// DensePolynomial semantics: trailing zero coefficients are not part of the polynomial
static void trim(DensePolynomial& p) { while (!p.empty() && p.back().is_zero()) p.pop_back(); }

Result<G1> open(const KZGSetup& setup, const DensePolynomial& p_in, const Fr& point) {
  // quotient (p(x) - p(point)) / (x - point) and its commitment in one device call (keaki_hip_kzg_open: blockwise Horner recurrence
  // in front of the MSM). The quotient has p.len() - 1 coefficients and its leading one is p's, so it needs no trimming.
  DensePolynomial p = p_in;
  trim(p);
  const size_t qlen = p.size() > 1 ? p.size() - 1 : 0;
  if (qlen > setup.g1_pow().size())                       // the commit inside open fails with the QUOTIENT's length (src/kzg.rs:123,91-96)
    return Result<G1>::Err(KZGError{KZGError::PolynomialTooLarge, qlen, setup.g1_pow().size()});
  uint64_t jac[12];
  if (setup.group_srs()) {
    setup.device()->check_group(keaki_hip_group_kzg_open(setup.device()->group(), setup.group_srs(), p.empty() ? nullptr : p[0].l, p.size(), point.l, jac, nullptr));
  } else if (qlen && qlen <= OPEN_HOST_QUOTIENT_MAX) {
    // SHORT polynomials: the synthetic division is a chain (q_(i-1) = p_i + point q_i), 40 ns a step on the host, while the device's blockwise
    // recurrence waits for its three launches (0.7 ms at 1,000 coefficients against 0.04 here); the MSM is the device's either way (src/kzg.rs:109-123)
    std::vector<Fr> q(qlen);
    q[qlen - 1] = p[qlen];
    for (size_t i = qlen - 1; i > 0; i--) q[i - 1] = p[i] + point * q[i];
    setup.device()->check(keaki_hip_msm_g1(setup.device()->ctx(), setup.srs(), q[0].l, qlen, jac));
  } else {
    setup.device()->check(keaki_hip_kzg_open(setup.device()->ctx(), setup.srs(), p.empty() ? nullptr : p[0].l, p.size(), point.l, jac, nullptr));
  }
  return Result<G1>::Ok(jac_to_g1(jac));
}

// rows zero-padded to n coefficients each, as the batch entries read them (stride = n)
static std::vector<uint64_t> pack_rows(const std::vector<DensePolynomial>& polys, size_t n) {
  std::vector<uint64_t> rows(polys.size() * n * 4 + 4, 0);
  for (size_t j = 0; j < polys.size(); j++)
    for (size_t i = 0; i < polys[j].size() && i < n; i++) memcpy(&rows[(j * n + i) * 4], polys[j][i].l, 32);
  return rows;
}

Result<std::vector<G1>> commit_batch(const KZGSetup& setup, const std::vector<DensePolynomial>& polys) {
  typedef Result<std::vector<G1>> Res;
  const size_t m = polys.size(), len = setup.g1_pow().size();
  size_t n = 0;
  for (const DensePolynomial& p : polys) {
    if (p.size() > len) return Res::Err(KZGError{KZGError::PolynomialTooLarge, p.size(), len});
    n = std::max(n, p.size());
  }
  std::vector<G1> out(m);
  if (m < COMMIT_BATCH_MIN || setup.group_srs()) {
    for (size_t j = 0; j < m; j++) out[j] = commit(setup, polys[j]).value;
    return Res::Ok(std::move(out));
  }
  const std::vector<uint64_t> rows = pack_rows(polys, n);
  std::vector<uint64_t> jac(m * 12);
  setup.device()->check(keaki_hip_msm_g1_batch(setup.device()->ctx(), setup.srs(), rows.data(), n, m, n, jac.data()));
  for (size_t j = 0; j < m; j++) out[j] = jac_to_g1(&jac[12 * j]);
  return Res::Ok(std::move(out));
}

Result<std::vector<G1>> open_batch(const KZGSetup& setup, const std::vector<DensePolynomial>& polys_in, const std::vector<Fr>& points) {
  typedef Result<std::vector<G1>> Res;
  if (points.size() != polys_in.size()) throw std::invalid_argument("open_batch: one point per polynomial");
  std::vector<DensePolynomial> polys = polys_in;
  const size_t m = polys.size(), len = setup.g1_pow().size();
  size_t n = 0;
  for (DensePolynomial& p : polys) {
    trim(p);
    const size_t qlen = p.size() > 1 ? p.size() - 1 : 0;
    if (qlen > len) return Res::Err(KZGError{KZGError::PolynomialTooLarge, qlen, len});
    n = std::max(n, p.size());
  }
  std::vector<G1> out(m);
  if (m < COMMIT_BATCH_MIN || setup.group_srs()) {
    for (size_t j = 0; j < m; j++) out[j] = open(setup, polys[j], points[j]).value;
    return Res::Ok(std::move(out));
  }
  const std::vector<uint64_t> rows = pack_rows(polys, n);
  std::vector<uint64_t> jac(m * 12);
  setup.device()->check(keaki_hip_kzg_open_batch(setup.device()->ctx(), setup.srs(), rows.data(), n, m, n, points[0].l, jac.data(), nullptr));
  for (size_t j = 0; j < m; j++) out[j] = jac_to_g1(&jac[12 * j]);
  return Res::Ok(std::move(out));
}

Result<bool> verify(const KZGSetup& setup, const G1& commitment, const Fr& point, const Fr& value, const G1& proof) {
  // src/kzg.rs:127-146, evaluated on the device in the same form (include/keaki_hip.h)
  const Device& dev = *setup.device();
  int32_t ok = 0;
  dev.check(keaki_hip_kzg_verify(dev.ctx(), commitment.w.data(), setup.tau_g2().w.data(), point.l, value.l, proof.w.data(), &ok));
  return Result<bool>::Ok(ok != 0);
}

bool verify_batch_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values,
                       const uint64_t* proofs, size_t n) {
  if (n_coms != 1 && n_coms != n) throw std::invalid_argument("verify_batch: one commitment, or one per item");
  std::vector<Fr> gammas(n);
  for (size_t i = 0; i < n; i++) gammas[i] = fr_rand(rng);       // one draw per item in index order, whichever path follows
  const Device& dev = *setup.device();
  if (n < VERIFY_BATCH_MIN) {
    // a batch call costs two MSM tails and a scalar-mult whatever n is; a few single checks are cheaper (profiles/verify_batch.txt)
    Fr z = Fr::one();
    for (size_t i = 0; i < n; i++) {
      int32_t ok = 0;
      dev.check(keaki_hip_kzg_verify(dev.ctx(), coms + (n_coms == 1 ? 0 : 8 * i), setup.tau_g2().w.data(), roots_of_unity ? z.l : points[i].l, values[i].l,
                                     proofs + 8 * i, &ok));
      if (!ok) return false;
      if (roots_of_unity) z = z * points[0];
    }
    return true;
  }
  int32_t ok = 0;
  dev.check(keaki_hip_kzg_verify_batch(dev.ctx(), coms, n_coms == 1 ? 0 : 1, setup.tau_g2().w.data(), points[0].l, roots_of_unity ? 1 : 0, values[0].l, proofs,
                                       gammas[0].l, n, &ok, nullptr));
  return ok != 0;
}
Result<bool> verify_batch(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points,
                          const std::vector<Fr>& values, const std::vector<G1>& proofs) {
  static_assert(sizeof(G1) == 64 && sizeof(Fr) == 32, "G1 is eight u64 words, Fr four");
  const size_t n = values.size();
  if (points.size() != n || proofs.size() != n || (commitments.size() != 1 && commitments.size() != n))
    throw std::invalid_argument("verify_batch: points, values and proofs must have one entry per item, commitments one or n");
  return Result<bool>::Ok(verify_batch_flat(rng, setup, commitments.empty() ? nullptr : commitments[0].w.data(), commitments.size(), points.data(), false, values.data(),
                                            n ? proofs[0].w.data() : nullptr, n));
}

size_t verify_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values, const uint64_t* proofs,
                        size_t n, uint8_t* status_out) {
  if (n_coms != 1 && n_coms != n) throw std::invalid_argument("verify_each: one commitment, or one per item");
  if (n == 0) return 0;
  const Device& dev = *setup.device();
  uint64_t bad = 0;
  dev.check(keaki_hip_kzg_verify_each(dev.ctx(), coms, n_coms == 1 ? 0 : 1, setup.tau_g2().w.data(), points[0].l, roots_of_unity ? 1 : 0, values[0].l, proofs, n,
                                      status_out, &bad, nullptr, nullptr));
  return (size_t)bad;
}
Result<std::vector<uint8_t>> verify_each(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points, const std::vector<Fr>& values,
                                         const std::vector<G1>& proofs) {
  const size_t n = values.size();
  if (points.size() != n || proofs.size() != n || (commitments.size() != 1 && commitments.size() != n))
    throw std::invalid_argument("verify_each: points, values and proofs must have one entry per item, commitments one or n");
  std::vector<uint8_t> status(n);
  verify_each_flat(setup, commitments.empty() ? nullptr : commitments[0].w.data(), commitments.size(), points.data(), false, values.data(), n ? proofs[0].w.data() : nullptr, n, status.data());
  return Result<std::vector<uint8_t>>::Ok(std::move(status));
}
std::vector<size_t> locate_invalid_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* points, bool roots_of_unity, const Fr* values,
                                        const uint64_t* proofs, size_t n) {
  std::vector<size_t> out;
  if (verify_batch_flat(rng, setup, coms, n_coms, points, roots_of_unity, values, proofs, n)) return out;
  std::vector<uint8_t> status(n);
  out.reserve(verify_each_flat(setup, coms, n_coms, points, roots_of_unity, values, proofs, n, status.data()));
  for (size_t i = 0; i < n; i++) if (status[i]) out.push_back(i);
  return out;
}
std::vector<size_t> locate_invalid(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& points, const std::vector<Fr>& values,
                                   const std::vector<G1>& proofs) {
  const size_t n = values.size();
  if (points.size() != n || proofs.size() != n || (commitments.size() != 1 && commitments.size() != n))
    throw std::invalid_argument("locate_invalid: points, values and proofs must have one entry per item, commitments one or n");
  return locate_invalid_flat(rng, setup, commitments.empty() ? nullptr : commitments[0].w.data(), commitments.size(), points.data(), false, values.data(), n ? proofs[0].w.data() : nullptr, n);
}

namespace {
const char* wire_reason(int r) {
  return r == 1 ? "malformed encoding (flags, or a coordinate >= p)" : r == 2 ? "no point of the curve has this x" : r == 3 ? "outside the order-r subgroup" : "rejected";
}
[[noreturn]] void throw_wire(const char* what, size_t index, int reason) {
  throw WireError(index, reason, std::string(what) + ": item " + std::to_string(index) + ": " + wire_reason(reason));
}
}  // namespace
void proofs_to_bytes_flat(const KZGSetup& setup, const uint64_t* proofs, size_t n, uint8_t* wire_out) {
  const Device& dev = *setup.device();
  dev.check(keaki_hip_g1_compress(dev.ctx(), proofs, n, wire_out));
}
void proofs_from_bytes_flat(const KZGSetup& setup, const uint8_t* wire, size_t n, uint64_t* proofs_out) {
  const Device& dev = *setup.device();
  std::vector<uint8_t> status(n);
  uint64_t bad = 0, first = 0;
  dev.check(keaki_hip_g1_decompress(dev.ctx(), wire, n, proofs_out, status.data(), &bad, &first));
  if (bad) throw_wire("proofs_from_bytes", (size_t)first, status[(size_t)first]);
}
std::vector<uint8_t> proofs_to_bytes(const KZGSetup& setup, const std::vector<G1>& proofs) {
  static_assert(sizeof(G1) == 64, "G1 is eight u64 words");
  std::vector<uint8_t> out(proofs.size() * 32);
  proofs_to_bytes_flat(setup, proofs.empty() ? nullptr : proofs[0].w.data(), proofs.size(), out.data());
  return out;
}
std::vector<G1> proofs_from_bytes(const KZGSetup& setup, const std::vector<uint8_t>& bytes) {
  if (bytes.size() % 32) throw std::invalid_argument("proofs_from_bytes: the length is not a multiple of 32");
  std::vector<G1> out(bytes.size() / 32);
  proofs_from_bytes_flat(setup, bytes.data(), out.size(), out.empty() ? nullptr : out[0].w.data());
  return out;
}

void precompute_open_fk(const KZGSetup& setup, size_t d) {
  if (d < 1 || (d & (d - 1)) != 0 || d > setup.g1_pow().size()) return;   // open_fk falls back to per-point openings for such shapes
  unsigned log2d = 0;
  while ((size_t(1) << log2d) < d) log2d++;
  if (setup.device()->group()) { (void)setup.group_fk(log2d); return; }      // every member's part of the SRS-only transform
  vec::Radix2Domain d2 = vec::Radix2Domain::create(2 * d);
  setup.device()->check(keaki_hip_srs_g1_precompute_fk(setup.device()->ctx(), setup.srs(), log2d, d2.group_gen.l));
}

Result<std::vector<G1>> open_fk(const KZGSetup& setup, const std::vector<Fr>& p, size_t domain_size) {
  const size_t d = p.size();
  const bool pow2 = d >= 1 && (d & (d - 1)) == 0;
  if (pow2 && domain_size == d && d <= setup.g1_pow().size()) {
    // FK23 (src/kzg.rs:157-203): the scalar-field DFT, the three group FFTs and the 2d scalar-mults all run on the GPU.
    unsigned log2d = 0;
    while ((size_t(1) << log2d) < d) log2d++;
    // hat_a = DFT_2d(0,..,0,p) / 2d and every twiddle table are derived on the device from omega_2d (keaki_hip_open_fk_poly)
    vec::Radix2Domain d2 = vec::Radix2Domain::create(2 * d);
    std::vector<G1> out(d);
    const Device& dev = *setup.device();
    if (dev.group())       // the group FFTs and the 2d scalar-mults split over the members, exchanges inside the library
      dev.check_group(keaki_hip_group_fk_open(dev.group(), setup.group_fk(log2d), p[0].l, out[0].w.data()));
    else
      dev.check(keaki_hip_open_fk_poly(dev.ctx(), setup.srs(), log2d, p[0].l, d2.group_gen.l, d2.group_gen_inv.l, d2.size_inv.l, out[0].w.data()));
    return Result<std::vector<G1>>::Ok(std::move(out));
  }
  // shapes FK23 does not cover (the reference would panic on them): one opening per root of unity
  vec::Radix2Domain dd = vec::Radix2Domain::create(domain_size);
  std::vector<Fr> el = dd.elements();
  std::vector<G1> out;
  out.reserve(el.size());
  for (const Fr& z : el) {
    Result<G1> r = open(setup, p, z);
    if (!r.ok) return Result<std::vector<G1>>::Err(r.error);
    out.push_back(r.value);
  }
  return Result<std::vector<G1>>::Ok(std::move(out));
}

std::vector<G1> open_fk_cosets(const KZGSetup& setup, const std::vector<Fr>& p, size_t domain_size, size_t l) {
  const size_t d = domain_size;
  if (d < 1 || (d & (d - 1)) != 0 || l < 1 || (l & (l - 1)) != 0 || l > d) throw SetError("open_fk_cosets: the domain and the coset size are powers of two, l <= d");
  if (l > (size_t)KEAKI_SET_MAX) throw SetError("open_fk_cosets: more than KEAKI_SET_MAX points in a coset");
  if (p.size() > d) throw SetError("open_fk_cosets: more coefficients than the domain holds");
  if (d > setup.g1_pow().size()) throw SetError("open_fk_cosets: the domain is larger than the SRS");
  unsigned log2d = 0, log2l = 0;
  while ((size_t(1) << log2d) < d) log2d++;
  while ((size_t(1) << log2l) < l) log2l++;
  std::vector<Fr> c(p);
  c.resize(d, Fr::zero());
  const vec::Radix2Domain d2 = vec::Radix2Domain::create(2 * (d / l));     // omega_2r = omega_2d^l
  std::vector<G1> out(d / l);
  const Device& dev = *setup.device();
  dev.check(keaki_hip_open_fk_cosets_poly(dev.ctx(), setup.srs(), log2d, log2l, c[0].l, d2.group_gen.l, d2.group_gen_inv.l, d2.size_inv.l, out[0].w.data()));
  return out;
}

bool verify_cosets_flat(Rng& rng, const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values,
                        size_t item_stride, size_t t_stride, size_t l, const uint64_t* proofs, size_t n) {
  if (l < 1 || (l & (l - 1)) != 0) throw SetError("verify_cosets: the coset size is a power of two");
  if (l > (size_t)KEAKI_SET_MAX) throw SetError("verify_cosets: more than KEAKI_SET_MAX points in a coset");
  if (l > setup.g1_pow().size()) throw SetError("verify_cosets: the coset is larger than the SRS");
  if (n_coms != 1 && n_coms != n) throw SetError("verify_cosets: one commitment, or one per item");
  if (setup.g2_pow().size() <= l) throw SetError("verify_cosets: this KZGSetup holds no [tau^l]_2: build it with G2 powers beyond l (setup_with_g2, from_powers_g2)");
  const Device& dev = *setup.device();
  if (dev.group()) throw SetError("verify_cosets: single device only");
  if (!roots_of_unity)
    for (size_t k = 0; k < n; k++)
      if (shifts[k] == Fr::zero()) throw SetError("verify_cosets: a zero shift is no coset");
  std::vector<Fr> gammas(n);
  for (size_t k = 0; k < n; k++) gammas[k] = fr_rand(rng);       // one draw per item in index order
  if (n == 0) return true;
  unsigned log2l = 0;
  while ((size_t(1) << log2l) < l) log2l++;
  const vec::Radix2Domain dl = vec::Radix2Domain::create(l);
  int32_t ok = 0;
  dev.check(keaki_hip_kzg_verify_cosets(dev.ctx(), setup.srs(), coms, n_coms == 1 ? 0 : 1, setup.g2_pow()[l].w.data(), shifts[0].l, roots_of_unity ? 1 : 0,
                                        values[0].l, item_stride, t_stride, log2l, dl.group_gen_inv.l, dl.size_inv.l, proofs, gammas[0].l, n, &ok, nullptr));
  return ok != 0;
}
namespace {
// the refusals the three coset calls share; -> log2 l
unsigned coset_call_check(const char* what, const KZGSetup& setup, size_t n_coms, const Fr* shifts, bool roots_of_unity, size_t l, size_t n, bool need_g2) {
  const std::string w(what);
  if (l < 1 || (l & (l - 1)) != 0) throw SetError(w + ": the coset size is a power of two");
  if (l > (size_t)KEAKI_SET_MAX) throw SetError(w + ": more than KEAKI_SET_MAX points in a coset");
  if (l > setup.g1_pow().size()) throw SetError(w + ": the coset is larger than the SRS");
  if (n_coms != 1 && n_coms != n) throw SetError(w + ": one commitment, or one per item");
  if (need_g2 && setup.g2_pow().size() <= l) throw SetError(w + ": this KZGSetup holds no [tau^l]_2: build it with G2 powers beyond l (setup_with_g2, from_powers_g2)");
  if (setup.device()->group()) throw SetError(w + ": single device only");
  if (!roots_of_unity)
    for (size_t k = 0; k < n; k++)
      if (shifts[k] == Fr::zero()) throw SetError(w + ": a zero shift is no coset");
  unsigned log2l = 0;
  while ((size_t(1) << log2l) < l) log2l++;
  return log2l;
}
}  // namespace
void coset_pairs_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values, size_t item_stride,
                      size_t t_stride, size_t l, size_t n, uint64_t* lhs_out, Fr* c_out) {
  const unsigned log2l = coset_call_check("coset_pairs", setup, n_coms, shifts, roots_of_unity, l, n, false);
  if (n == 0) return;
  const Device& dev = *setup.device();
  const vec::Radix2Domain dl = vec::Radix2Domain::create(l);
  dev.check(keaki_hip_kzg_coset_pairs(dev.ctx(), setup.srs(), coms, n_coms == 1 ? 0 : 1, shifts[0].l, roots_of_unity ? 1 : 0, values[0].l, item_stride, t_stride,
                                      log2l, dl.group_gen_inv.l, dl.size_inv.l, n, lhs_out, c_out[0].l));
}
std::vector<uint8_t> verify_cosets_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const Fr* shifts, bool roots_of_unity, const Fr* values,
                                             size_t item_stride, size_t t_stride, size_t l, const uint64_t* proofs, size_t n) {
  const unsigned log2l = coset_call_check("verify_cosets_each", setup, n_coms, shifts, roots_of_unity, l, n, true);
  std::vector<uint8_t> status(n);
  if (n == 0) return status;
  const Device& dev = *setup.device();
  const vec::Radix2Domain dl = vec::Radix2Domain::create(l);
  uint64_t n_bad = 0;
  dev.check(keaki_hip_kzg_verify_cosets_each(dev.ctx(), setup.srs(), coms, n_coms == 1 ? 0 : 1, setup.g2_pow()[l].w.data(), shifts[0].l, roots_of_unity ? 1 : 0,
                                             values[0].l, item_stride, t_stride, log2l, dl.group_gen_inv.l, dl.size_inv.l, proofs, n, status.data(), &n_bad, nullptr,
                                             nullptr));
  return status;
}
bool verify_cosets(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<Fr>& shifts, size_t l, const std::vector<Fr>& values,
                   const std::vector<G1>& proofs) {
  const size_t n = shifts.size();
  if (l == 0 || values.size() != n * l || proofs.size() != n || (commitments.size() != 1 && commitments.size() != n))
    throw SetError("verify_cosets: l values and one proof per item, commitments one or n");
  return verify_cosets_flat(rng, setup, commitments.empty() ? nullptr : commitments[0].w.data(), commitments.size(), shifts.data(), false, values.data(), l, 1, l, n ? proofs[0].w.data() : nullptr, n);
}

bool verify_sets_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k,
                      const uint64_t* proofs, const Fr* gammas, size_t n) {
  if (k < 1 || k > (size_t)KEAKI_VERIFY_SETS_K_MAX) throw SetError("verify_sets: a set holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " points");
  if (k > setup.g1_pow().size()) throw SetError("verify_sets: the set is larger than the SRS");
  if (n_coms != 1 && n_coms != n) throw SetError("verify_sets: one commitment, or one per item");
  if (setup.g2_pow().size() <= k) throw SetError("verify_sets: this KZGSetup holds no [tau^k]_2: build it with G2 powers beyond k (setup_with_g2, from_powers_g2)");
  const Device& dev = *setup.device();
  if (dev.group()) throw SetError("verify_sets: single device only");
  if (n == 0) return true;
  int32_t ok = 0;
  dev.check(keaki_hip_kzg_verify_sets(dev.ctx(), setup.srs(), setup.srs_g2(), coms, n_coms == 1 ? 0 : 1, points, omega ? 1 : 0, omega ? omega->l : nullptr, values[0].l,
                                      k, k, proofs, gammas[0].l, n, &ok, nullptr));
  return ok != 0;
}
namespace {
// Items of unequal size in one call per size: `sizes[i]` = k of item i; `fill(i, dst)` appends item i's k point words (32 B each, or 4 B indices) to the
// group's flat buffer. The gammas were drawn by the caller, one per item in index order; the verdict is the AND over the groups (every group runs).
template <class Elem, class Fill>
bool verify_sets_grouped(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<size_t>& sizes, Fill fill, const Fr* omega,
                         const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs, const std::vector<Fr>& gammas) {
  std::map<size_t, std::vector<size_t>> groups;
  for (size_t i = 0; i < sizes.size(); i++) groups[sizes[i]].push_back(i);
  bool all = true;
  for (const auto& [k, items] : groups) {
    const size_t m = items.size();
    std::vector<Elem> pts;
    std::vector<Fr> vals, gam(m);
    std::vector<G1> pr(m), coms(commitments.size() == 1 ? 1 : m);
    pts.reserve(m * k);
    vals.reserve(m * k);
    for (size_t t = 0; t < m; t++) {
      const size_t i = items[t];
      fill(i, pts);
      vals.insert(vals.end(), values[i].begin(), values[i].end());
      gam[t] = gammas[i];
      pr[t] = proofs[i];
      if (commitments.size() != 1) coms[t] = commitments[i];
    }
    if (commitments.size() == 1) coms[0] = commitments[0];
    all &= verify_sets_flat(setup, coms[0].w.data(), coms.size(), pts.data(), omega, vals.data(), k, pr[0].w.data(), gam.data(), m);
  }
  return all;
}
}  // namespace
bool verify_sets(Rng& rng, const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                 const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const size_t n = points.size();
  if (values.size() != n || proofs.size() != n || (commitments.size() != 1 && commitments.size() != n))
    throw SetError("verify_sets: points, values and proofs must have one entry per item, commitments one or n");
  std::vector<Fr> gammas(n);
  for (size_t i = 0; i < n; i++) gammas[i] = fr_rand(rng);       // one draw per item in index order
  std::vector<size_t> sizes(n);
  for (size_t i = 0; i < n; i++) {
    if (points[i].empty() || points[i].size() > (size_t)KEAKI_VERIFY_SETS_K_MAX)
      throw SetError("verify_sets: a set holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " points");
    check_set("verify_sets", points[i], values[i].size());
    sizes[i] = points[i].size();
  }
  if (setup.device()->group()) throw SetError("verify_sets: single device only");
  return verify_sets_grouped<Fr>(setup, commitments, sizes, [&](size_t i, std::vector<Fr>& dst) { dst.insert(dst.end(), points[i].begin(), points[i].end()); }, nullptr,
                                 values, proofs, gammas);
}
bool verify_sets_indexed(Rng& rng, const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                         const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const size_t n = idx_rows.size();
  if (values.size() != n || proofs.size() != n) throw SetError("vec_verify_subsets: idx_rows, values and proofs must have one entry per item");
  std::vector<Fr> gammas(n);
  for (size_t i = 0; i < n; i++) gammas[i] = fr_rand(rng);       // one draw per item in index order
  std::vector<size_t> sizes(n);
  for (size_t i = 0; i < n; i++) {
    const std::vector<size_t>& row = idx_rows[i];
    if (row.empty() || row.size() > (size_t)KEAKI_VERIFY_SETS_K_MAX)
      throw SetError("vec_verify_subsets: a subset holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " positions");
    if (values[i].size() != row.size()) throw SetError("vec_verify_subsets: one value per position");
    std::vector<size_t> s(row);
    std::sort(s.begin(), s.end());
    if (s.back() >= domain || s.back() > 0xFFFFFFFFull) throw SetError("vec_verify_subsets: index outside the domain");
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) throw SetError("vec_verify_subsets: repeated index in a subset");
    sizes[i] = row.size();
  }
  if (setup.device()->group()) throw SetError("vec_verify_subsets: single device only");
  return verify_sets_grouped<uint32_t>(setup, {com}, sizes, [&](size_t i, std::vector<uint32_t>& dst) { for (size_t e : idx_rows[i]) dst.push_back((uint32_t)e); }, &omega,
                                       values, proofs, gammas);
}

namespace {
void sets_flat_check(const char* what, const KZGSetup& setup, size_t n_coms, size_t k, size_t n) {
  const std::string w(what);
  if (k < 1 || k > (size_t)KEAKI_VERIFY_SETS_K_MAX) throw SetError(w + ": a set holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " points");
  if (k > setup.g1_pow().size()) throw SetError(w + ": the set is larger than the SRS");
  if (n_coms != 1 && n_coms != n) throw SetError(w + ": one commitment, or one per item");
  if (setup.g2_pow().size() <= k) throw SetError(w + ": this KZGSetup holds no [tau^k]_2: build it with G2 powers beyond k (setup_with_g2, from_powers_g2)");
  if (setup.device()->group()) throw SetError(w + ": single device only");
}
// what the grouping layers refuse, before any device call (and before any draw of their callers): -> the size of every item
std::vector<size_t> sets_rows_check(const char* what, const KZGSetup& setup, size_t n_coms, const std::vector<std::vector<Fr>>& points,
                                    const std::vector<std::vector<Fr>>& values, size_t n_proofs) {
  const std::string w(what);
  const size_t n = points.size();
  if (values.size() != n || n_proofs != n || (n_coms != 1 && n_coms != n)) throw SetError(w + ": points, values and proofs must have one entry per item, commitments one or n");
  std::vector<size_t> sizes(n);
  for (size_t i = 0; i < n; i++) {
    if (points[i].empty() || points[i].size() > (size_t)KEAKI_VERIFY_SETS_K_MAX)
      throw SetError(w + ": a set holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " points");
    check_set(what, points[i], values[i].size());
    sizes[i] = points[i].size();
    sets_flat_check(what, setup, n_coms, sizes[i], n);
  }
  if (setup.device()->group()) throw SetError(w + ": single device only");
  return sizes;
}
std::vector<size_t> sets_idx_check(const char* what, const KZGSetup& setup, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                                   const std::vector<std::vector<Fr>>& values, size_t n_proofs) {
  const std::string w(what);
  const size_t n = idx_rows.size();
  if (values.size() != n || n_proofs != n) throw SetError(w + ": idx_rows, values and proofs must have one entry per item");
  std::vector<size_t> sizes(n);
  for (size_t i = 0; i < n; i++) {
    const std::vector<size_t>& row = idx_rows[i];
    if (row.empty() || row.size() > (size_t)KEAKI_VERIFY_SETS_K_MAX) throw SetError(w + ": a subset holds 1 .. " + std::to_string((int)KEAKI_VERIFY_SETS_K_MAX) + " positions");
    if (values[i].size() != row.size()) throw SetError(w + ": one value per position");
    std::vector<size_t> s(row);
    std::sort(s.begin(), s.end());
    if (s.back() >= domain || s.back() > 0xFFFFFFFFull) throw SetError(w + ": index outside the domain");
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) throw SetError(w + ": repeated index in a subset");
    sizes[i] = row.size();
    sets_flat_check(what, setup, 1, sizes[i], n);
  }
  if (setup.device()->group()) throw SetError(w + ": single device only");
  return sizes;
}
// One call of `run(k, items, coms, n_coms, pts, vals)` per set size: items = the indices of the group's items in the caller's order, the buffers flat as the
// _flat entries take them. `fill(i, dst)` appends item i's point words (Fr, or u32 indices).
template <class Elem, class Fill, class Run>
void sets_each_group(const std::vector<G1>& commitments, const std::vector<size_t>& sizes, Fill fill, const std::vector<std::vector<Fr>>& values, Run run) {
  std::map<size_t, std::vector<size_t>> groups;
  for (size_t i = 0; i < sizes.size(); i++) groups[sizes[i]].push_back(i);
  for (const auto& [k, items] : groups) {
    const size_t m = items.size();
    std::vector<Elem> pts;
    std::vector<Fr> vals;
    std::vector<G1> coms(commitments.size() == 1 ? 1 : m);
    pts.reserve(m * k);
    vals.reserve(m * k);
    for (size_t t = 0; t < m; t++) {
      fill(items[t], pts);
      vals.insert(vals.end(), values[items[t]].begin(), values[items[t]].end());
      if (commitments.size() != 1) coms[t] = commitments[items[t]];
    }
    if (commitments.size() == 1) coms[0] = commitments[0];
    run(k, items, coms[0].w.data(), coms.size(), (const void*)pts.data(), vals.data());
  }
}
template <class Elem, class Fill>
void set_pairs_grouped(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<size_t>& sizes, Fill fill, const Fr* omega,
                       const std::vector<std::vector<Fr>>& values, uint64_t* lhs_out, uint64_t* z2_out) {
  sets_each_group<Elem>(commitments, sizes, fill, values, [&](size_t k, const std::vector<size_t>& items, const uint64_t* coms, size_t n_coms, const void* pts, const Fr* vals) {
    const size_t m = items.size();
    std::vector<uint64_t> a(m * 8), z(m * 16);
    set_pairs_flat(setup, coms, n_coms, pts, omega, vals, k, m, a.data(), z.data());
    for (size_t t = 0; t < m; t++) {
      memcpy(lhs_out + 8 * items[t], a.data() + 8 * t, 64);
      memcpy(z2_out + 16 * items[t], z.data() + 16 * t, 128);
    }
  });
}
template <class Elem, class Fill>
std::vector<uint8_t> verify_sets_each_grouped(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<size_t>& sizes, Fill fill, const Fr* omega,
                                              const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  std::vector<uint8_t> status(sizes.size());
  sets_each_group<Elem>(commitments, sizes, fill, values, [&](size_t k, const std::vector<size_t>& items, const uint64_t* coms, size_t n_coms, const void* pts, const Fr* vals) {
    const size_t m = items.size();
    std::vector<G1> pr(m);
    for (size_t t = 0; t < m; t++) pr[t] = proofs[items[t]];
    const std::vector<uint8_t> st = verify_sets_each_flat(setup, coms, n_coms, pts, omega, vals, k, pr[0].w.data(), m);
    for (size_t t = 0; t < m; t++) status[items[t]] = st[t];
  });
  return status;
}
}  // namespace
void set_pairs_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k, size_t n,
                    uint64_t* lhs_out, uint64_t* z2_out) {
  sets_flat_check("set_pairs", setup, n_coms, k, n);
  if (n == 0) return;
  const Device& dev = *setup.device();
  dev.check(keaki_hip_kzg_set_pairs(dev.ctx(), setup.srs(), setup.srs_g2(), coms, n_coms == 1 ? 0 : 1, points, omega ? 1 : 0, omega ? omega->l : nullptr, values[0].l, k, k,
                                    n, lhs_out, z2_out));
}
std::vector<uint8_t> verify_sets_each_flat(const KZGSetup& setup, const uint64_t* coms, size_t n_coms, const void* points, const Fr* omega, const Fr* values, size_t k,
                                           const uint64_t* proofs, size_t n) {
  sets_flat_check("verify_sets_each", setup, n_coms, k, n);
  std::vector<uint8_t> status(n);
  if (n == 0) return status;
  const Device& dev = *setup.device();
  uint64_t n_bad = 0;
  dev.check(keaki_hip_kzg_verify_sets_each(dev.ctx(), setup.srs(), setup.srs_g2(), coms, n_coms == 1 ? 0 : 1, points, omega ? 1 : 0, omega ? omega->l : nullptr,
                                           values[0].l, k, k, proofs, n, status.data(), &n_bad, nullptr, nullptr, nullptr));
  return status;
}
void set_pairs(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points, const std::vector<std::vector<Fr>>& values,
               uint64_t* lhs_out, uint64_t* z2_out) {
  const std::vector<size_t> sizes = sets_rows_check("set_pairs", setup, commitments.size(), points, values, points.size());
  set_pairs_grouped<Fr>(setup, commitments, sizes, [&](size_t i, std::vector<Fr>& dst) { dst.insert(dst.end(), points[i].begin(), points[i].end()); }, nullptr, values,
                        lhs_out, z2_out);
}
void set_pairs_indexed(const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                       const std::vector<std::vector<Fr>>& values, uint64_t* lhs_out, uint64_t* z2_out) {
  const std::vector<size_t> sizes = sets_idx_check("set_pairs", setup, domain, idx_rows, values, idx_rows.size());
  set_pairs_grouped<uint32_t>(setup, {com}, sizes, [&](size_t i, std::vector<uint32_t>& dst) { for (size_t e : idx_rows[i]) dst.push_back((uint32_t)e); }, &omega, values,
                              lhs_out, z2_out);
}
std::vector<uint8_t> verify_sets_each(const KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                                      const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const std::vector<size_t> sizes = sets_rows_check("verify_sets_each", setup, commitments.size(), points, values, proofs.size());
  return verify_sets_each_grouped<Fr>(setup, commitments, sizes, [&](size_t i, std::vector<Fr>& dst) { dst.insert(dst.end(), points[i].begin(), points[i].end()); }, nullptr,
                                      values, proofs);
}
std::vector<uint8_t> verify_sets_each_indexed(const KZGSetup& setup, const G1& com, const Fr& omega, size_t domain, const std::vector<std::vector<size_t>>& idx_rows,
                                              const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const std::vector<size_t> sizes = sets_idx_check("vec_verify_subsets_each", setup, domain, idx_rows, values, proofs.size());
  return verify_sets_each_grouped<uint32_t>(setup, {com}, sizes, [&](size_t i, std::vector<uint32_t>& dst) { for (size_t e : idx_rows[i]) dst.push_back((uint32_t)e); },
                                            &omega, values, proofs);
}

}  // namespace kzg

// ------------------------------------------------------------------------------------------------ kem / enc
namespace kem {

std::pair<G2, std::vector<uint8_t>> encapsulate(Rng& rng, const kzg::KZGSetup& setup, const G1& commitment, const Fr& point,
                                                const Fr& value, size_t msg_len) {
  Fr r = fr_rand(rng);  // src/kem.rs:26
  G2 ct; std::vector<uint8_t> key(msg_len), gt(384);
  setup.device()->check(keaki_hip_encap_batch(setup.device()->ctx(), commitment.w.data(), setup.tau_g2().w.data(), point.l, value.l, r.l, 1,
                                              ct.w.data(), gt.data(), msg_len ? key.data() : nullptr, msg_len));
  return {ct, key};
}
std::vector<uint8_t> decapsulate(const kzg::KZGSetup& setup, const G1& proof, const G2& ciphertext, size_t msg_len) {
  std::vector<uint8_t> key(msg_len), gt(384);
  setup.device()->check(keaki_hip_decap_batch(setup.device()->ctx(), proof.w.data(), ciphertext.w.data(), 1, gt.data(),
                                              msg_len ? key.data() : nullptr, msg_len));
  return key;
}

namespace {
// (ct, key) for the pair (A, Zq) = (C - [I]_1, [Z]_2) and the scalar r: ct = r Zq, key = KDF(e(r A, g2)), from the library's existing entries
std::pair<G2, std::vector<uint8_t>> encap_pair(const kzg::KZGSetup& setup, const std::pair<G1, G2>& az, const Fr& r, size_t msg_len) {
  const Device& dev = *setup.device();
  G2 ct; G1 pt;
  dev.check(keaki_hip_g2_mul_batch(dev.ctx(), az.second.w.data(), 0, r.l, 1, ct.w.data()));
  dev.check(keaki_hip_g1_mul_batch(dev.ctx(), az.first.w.data(), 0, r.l, 1, pt.w.data()));
  return {ct, decapsulate(setup, pt, g2_generator(dev), msg_len)};
}
}  // namespace
std::pair<G2, std::vector<uint8_t>> encapsulate_set(Rng& rng, const kzg::KZGSetup& setup, const G1& commitment, const std::vector<Fr>& points,
                                                    const std::vector<Fr>& values, size_t msg_len) {
  const std::pair<G1, G2> az = kzg::set_pair(setup, commitment, points, values);      // throws before the draw: a refused call leaves `rng` alone
  const Fr r = fr_rand(rng);
  return encap_pair(setup, az, r, msg_len);
}

void seal_pairs(Rng& rng, const kzg::KZGSetup& setup, const uint64_t* lhs, const uint64_t* z2, size_t n, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out,
                uint8_t* bodies_out) {
  if (!n) return;
  const Device& dev = *setup.device();
  std::vector<Fr> rs(n), zeros(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);      // one r per item in index order, as everywhere else
  std::vector<uint64_t> offsets(n + 1);
  for (size_t i = 0; i <= n; i++) offsets[i] = i;
  // n groups of one item with coms := A, points = values = 0: key_i = KDF(e(r_i A_i, g2)); the G2 output of this call (r_i [tau]_2) is replaced below
  const uint64_t* tau = setup.tau_g2().w.data();
  if (msgs && msg_len) {
    dev.check(keaki_hip_encrypt_multi(dev.ctx(), lhs, offsets.data(), n, tau, zeros[0].l, zeros[0].l, rs[0].l, msgs, n, ct_g2_out, bodies_out, msg_len));
  } else {
    std::vector<uint8_t> gt_unused(n * 384);
    dev.check(keaki_hip_encap_multi(dev.ctx(), lhs, offsets.data(), n, tau, zeros[0].l, zeros[0].l, rs[0].l, n, ct_g2_out, gt_unused.data(), msg_len ? bodies_out : nullptr,
                                    msg_len));
  }
  dev.check(keaki_hip_g2_mul_batch(dev.ctx(), z2, 1, rs[0].l, n, ct_g2_out));      // ct_i = r_i Z2_i
}
std::vector<std::pair<G2, std::vector<uint8_t>>> encapsulate_sets(Rng& rng, const kzg::KZGSetup& setup, const std::vector<G1>& commitments,
                                                                  const std::vector<std::vector<Fr>>& points, const std::vector<std::vector<Fr>>& values, size_t msg_len) {
  const size_t n = points.size();
  std::vector<uint64_t> a(n * 8), z(n * 16), ct(n * 16);
  std::vector<uint8_t> keys(n * msg_len);
  kzg::set_pairs(setup, commitments, points, values, a.data(), z.data());      // throws before the draws: a refused call leaves `rng` alone
  seal_pairs(rng, setup, a.data(), z.data(), n, nullptr, msg_len, ct.data(), keys.data());
  std::vector<std::pair<G2, std::vector<uint8_t>>> out(n);
  for (size_t i = 0; i < n; i++) {
    memcpy(out[i].first.w.data(), ct.data() + 16 * i, 128);
    out[i].second.assign(keys.begin() + i * msg_len, keys.begin() + (i + 1) * msg_len);
  }
  return out;
}

void prepare(const kzg::KZGSetup& setup, size_t batch_hint) {
  const Device& dev = *setup.device();
  if (dev.group() && batch_hint >= GROUP_MIN_ITEMS) {
    const size_t N = dev.members(), share = (batch_hint + N - 1) / N;
    for (size_t i = 0; i < N; i++) {
      keaki_hip_ctx* c = keaki_hip_group_ctx(dev.group(), i);
      const int st = keaki_hip_encap_prepare(c, setup.tau_g2().w.data(), share);
      if (st != KEAKI_OK) throw HipError(st, keaki_hip_last_error(c));
    }
    return;
  }
  dev.check(keaki_hip_encap_prepare(dev.ctx(), setup.tau_g2().w.data(), batch_hint));
}
}  // namespace kem

namespace enc {
Ciphertext encrypt(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr& point, const Fr& value, const std::vector<uint8_t>& msg) {
  auto kc = kem::encapsulate(rng, setup, com, point, value, msg.size());
  std::vector<uint8_t> ct(msg.size());
  for (size_t i = 0; i < msg.size(); i++) ct[i] = kc.second[i] ^ msg[i];
  return {kc.first, ct};
}
Ciphertext encrypt_set(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& points, const std::vector<Fr>& values,
                       const std::vector<uint8_t>& msg) {
  auto kc = kem::encapsulate_set(rng, setup, com, points, values, msg.size());
  std::vector<uint8_t> ct(msg.size());
  for (size_t i = 0; i < msg.size(); i++) ct[i] = kc.second[i] ^ msg[i];
  return {kc.first, ct};
}
std::vector<Ciphertext> encrypt_sets(Rng& rng, const kzg::KZGSetup& setup, const std::vector<G1>& commitments, const std::vector<std::vector<Fr>>& points,
                                     const std::vector<std::vector<Fr>>& values, const std::vector<std::vector<uint8_t>>& messages) {
  const size_t n = points.size(), len = messages.empty() ? 0 : messages[0].size();
  if (messages.size() != n) throw kzg::SetError("encrypt_sets: one message per item");
  for (const auto& m : messages)
    if (m.size() != len) throw kzg::SetError("encrypt_sets: all messages of one length");
  auto kc = kem::encapsulate_sets(rng, setup, commitments, points, values, len);
  std::vector<Ciphertext> out(n);
  for (size_t i = 0; i < n; i++) {
    out[i].first = kc[i].first;
    out[i].second.resize(len);
    for (size_t j = 0; j < len; j++) out[i].second[j] = kc[i].second[j] ^ messages[i][j];
  }
  return out;
}
std::vector<uint8_t> decrypt(const kzg::KZGSetup& setup, const G1& proof, const Ciphertext& ct) {
  std::vector<uint8_t> key = kem::decapsulate(setup, proof, ct.first, ct.second.size());
  for (size_t i = 0; i < key.size(); i++) key[i] ^= ct.second[i];
  return key;
}
// wire = n x (64 B point | body): the points are gathered into one contiguous array for the device call and scattered back
void ciphertexts_to_bytes_flat(const kzg::KZGSetup& setup, const uint64_t* ct_g2, const uint8_t* bodies, size_t n, size_t msg_len, uint8_t* wire_out) {
  const Device& dev = *setup.device();
  std::vector<uint8_t> pts(n * 64);
  dev.check(keaki_hip_g2_compress(dev.ctx(), ct_g2, n, pts.data()));
  const size_t item = 64 + msg_len;
  for (size_t i = 0; i < n; i++) {
    memcpy(wire_out + i * item, pts.data() + i * 64, 64);
    if (msg_len) memcpy(wire_out + i * item + 64, bodies + i * msg_len, msg_len);
  }
}
void ciphertexts_from_bytes_flat(const kzg::KZGSetup& setup, const uint8_t* wire, size_t n, size_t msg_len, uint64_t* ct_g2_out, uint8_t* bodies_out) {
  const Device& dev = *setup.device();
  const size_t item = 64 + msg_len;
  std::vector<uint8_t> pts(n * 64), status(n);
  for (size_t i = 0; i < n; i++) memcpy(pts.data() + i * 64, wire + i * item, 64);
  uint64_t bad = 0, first = 0;
  dev.check(keaki_hip_g2_decompress(dev.ctx(), pts.data(), n, 1, ct_g2_out, status.data(), &bad, &first));
  if (bad) kzg::throw_wire("ciphertexts_from_bytes", (size_t)first, status[(size_t)first]);
  for (size_t i = 0; i < n; i++)
    if (msg_len) memcpy(bodies_out + i * msg_len, wire + i * item + 64, msg_len);
}
std::vector<uint8_t> ciphertexts_to_bytes(const kzg::KZGSetup& setup, const std::vector<Ciphertext>& cts) {
  const size_t n = cts.size(), msg_len = n ? cts[0].second.size() : 0;
  std::vector<uint64_t> g2(n * 16);
  std::vector<uint8_t> bodies(n * msg_len), out(n * (64 + msg_len));
  for (size_t i = 0; i < n; i++) {
    if (cts[i].second.size() != msg_len) throw std::invalid_argument("ciphertexts_to_bytes: the bodies of one batch must have one length");
    memcpy(g2.data() + 16 * i, cts[i].first.w.data(), 128);
    if (msg_len) memcpy(bodies.data() + i * msg_len, cts[i].second.data(), msg_len);
  }
  ciphertexts_to_bytes_flat(setup, g2.data(), bodies.data(), n, msg_len, out.data());
  return out;
}
std::vector<Ciphertext> ciphertexts_from_bytes(const kzg::KZGSetup& setup, const std::vector<uint8_t>& bytes, size_t msg_len) {
  if (bytes.size() % (64 + msg_len)) throw std::invalid_argument("ciphertexts_from_bytes: the length is not a multiple of 64 + msg_len");
  const size_t n = bytes.size() / (64 + msg_len);
  std::vector<uint64_t> g2(n * 16);
  std::vector<uint8_t> bodies(n * msg_len);
  ciphertexts_from_bytes_flat(setup, bytes.data(), n, msg_len, g2.data(), bodies.data());
  std::vector<Ciphertext> out(n);
  for (size_t i = 0; i < n; i++) {
    memcpy(out[i].first.w.data(), g2.data() + 16 * i, 128);
    out[i].second.assign(bodies.begin() + i * msg_len, bodies.begin() + (i + 1) * msg_len);
  }
  return out;
}
}  // namespace enc

// ------------------------------------------------------------------------------------------------ vec
namespace vec {
namespace {
// the loop bodies of src/vec.rs:63-66 / :75-78 as one batched call: over all members of a group device for large batches
void encap_many(const kzg::KZGSetup& setup, const G1& com, const uint64_t* points, const uint64_t* values, const uint64_t* rs, size_t n,
                uint64_t* ct, uint8_t* key, size_t msg_len) {
  const Device& dev = *setup.device();
  if (dev.group() && n >= GROUP_MIN_ITEMS)
    dev.check_group(keaki_hip_group_encap_batch(dev.group(), com.w.data(), setup.tau_g2().w.data(), points, values, rs, n, ct, nullptr, key, msg_len));
  else
    dev.check(keaki_hip_encap_batch(dev.ctx(), com.w.data(), setup.tau_g2().w.data(), points, values, rs, n, ct, nullptr, key, msg_len));
}
// enc::encrypt / enc::decrypt per item (src/enc.rs:19-55) as one batched call: KEM + the XOR DEM on the device(s)
void encrypt_many(const kzg::KZGSetup& setup, const G1& com, const uint64_t* points, const uint64_t* values, const uint64_t* rs, const uint8_t* msgs,
                  size_t n, uint64_t* ct, uint8_t* body, size_t msg_len) {
  const Device& dev = *setup.device();
  if (dev.group() && n >= GROUP_MIN_ITEMS)
    dev.check_group(keaki_hip_group_encrypt_batch(dev.group(), com.w.data(), setup.tau_g2().w.data(), points, values, rs, msgs, n, ct, body, msg_len));
  else
    dev.check(keaki_hip_encrypt_batch(dev.ctx(), com.w.data(), setup.tau_g2().w.data(), points, values, rs, msgs, n, ct, body, msg_len));
}
void decrypt_many(const kzg::KZGSetup& setup, const uint64_t* proofs, const uint64_t* cts, const uint8_t* bodies, size_t n, uint8_t* msgs, size_t msg_len) {
  const Device& dev = *setup.device();
  if (dev.group() && n >= GROUP_MIN_ITEMS) dev.check_group(keaki_hip_group_decrypt_batch(dev.group(), proofs, cts, bodies, n, msgs, msg_len));
  else dev.check(keaki_hip_decrypt_batch(dev.ctx(), proofs, cts, bodies, n, msgs, msg_len));
}
void decap_many(const kzg::KZGSetup& setup, const uint64_t* proofs, const uint64_t* cts, size_t n, uint8_t* key, size_t msg_len) {
  const Device& dev = *setup.device();
  if (dev.group() && n >= GROUP_MIN_ITEMS)
    dev.check_group(keaki_hip_group_decap_batch(dev.group(), proofs, cts, n, nullptr, key, msg_len));   // keys only: no 384 B/item GT download
  else
    dev.check(keaki_hip_decap_batch(dev.ctx(), proofs, cts, n, nullptr, key, msg_len));
}
}  // namespace

Radix2Domain Radix2Domain::create(size_t min_size) {
  size_t size = 1; unsigned log = 0;
  while (size < min_size) { size <<= 1; log++; }
  if (log > FR_TWO_ADICITY) throw std::invalid_argument("domain larger than 2^28");
  Fr g; memcpy(g.l, FR_TWO_ADIC_ROOT, 32);
  for (unsigned i = log; i < FR_TWO_ADICITY; i++) g = g * g;
  Radix2Domain d;
  d.size = size; d.group_gen = g; d.group_gen_inv = g.inverse(); d.size_inv = Fr::from_u64(size).inverse();
  return d;
}
std::vector<Fr> Radix2Domain::elements() const {
  std::vector<Fr> e(size);
  Fr acc = Fr::one();
  for (size_t i = 0; i < size; i++) { e[i] = acc; acc = acc * group_gen; }
  return e;
}
static void fft_in_place(std::vector<Fr>& a, const Fr& root) {
  size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; i++) {  // bit reversal
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    Fr w = root;
    for (size_t k = len; k < n; k <<= 1) w = w * w;
    for (size_t i = 0; i < n; i += len) {
      Fr x = Fr::one();
      for (size_t j = 0; j < len / 2; j++) {
        Fr u = a[i + j], v = a[i + j + len / 2] * x;
        a[i + j] = u + v; a[i + j + len / 2] = u - v;
        x = x * w;
      }
    }
  }
}
std::vector<Fr> Radix2Domain::fft(std::vector<Fr> c) const { c.resize(size); fft_in_place(c, group_gen); return c; }
std::vector<Fr> Radix2Domain::ifft(std::vector<Fr> e) const {
  e.resize(size);
  fft_in_place(e, group_gen_inv);
  for (auto& x : e) x = x * size_inv;
  return e;
}

// src/vec.rs:27-44: everything of vec_commit in front of the final commit -> (coefficients as a DensePolynomial, proofs)
std::vector<Fr> vec_commit_coeffs(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v) {
  size_t d = v.size() + PADDING_LEN;
  std::vector<Fr> padded(v);
  padded.push_back(fr_rand(rng));                    // src/vec.rs:31-33
  Radix2Domain domain = Radix2Domain::create(d);     // :36
  if (d < (size_t(1) << 12)) return domain.ifft(padded);
  // :37 on the device for large domains (keaki_hip_fr_fft), same values
  padded.resize(domain.size);
  unsigned log_size = 0;
  while ((size_t(1) << log_size) < domain.size) log_size++;
  setup.device()->check(keaki_hip_fr_fft(setup.device()->ctx(), padded[0].l, log_size, domain.group_gen_inv.l, domain.size_inv.l));
  return padded;
}
static DensePolynomial trimmed(std::vector<Fr> c) {
  while (!c.empty() && c.back().is_zero()) c.pop_back();  // from_coefficients_vec trims
  return c;
}
std::pair<DensePolynomial, std::vector<G1>> vec_commit_openings(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v) {
  std::vector<Fr> p_coeff = vec_commit_coeffs(rng, setup, v);
  std::vector<G1> proofs = kzg::open_fk(setup, p_coeff, p_coeff.size()).unwrap();  // :40
  return {trimmed(std::move(p_coeff)), std::move(proofs)};
}
G1 vec_commit_flat(Rng& rng, const kzg::KZGSetup& setup, const Fr* v, size_t n, uint64_t* proofs_out) {
  const size_t d = n + PADDING_LEN;
  Radix2Domain domain = Radix2Domain::create(d);     // src/vec.rs:36
  const Device& dev = *setup.device();
  if (!dev.group() && domain.size >= (size_t(1) << 12) && domain.size <= setup.g1_pow().size()) {
    const Fr pad = fr_rand(rng);                     // :31-33, the only draw
    unsigned log_size = 0;
    while ((size_t(1) << log_size) < domain.size) log_size++;
    Radix2Domain d2 = Radix2Domain::create(2 * domain.size);
    uint64_t jac[12];
    dev.check(keaki_hip_vec_commit(dev.ctx(), setup.srs(), n ? v[0].l : nullptr, n, pad.l, log_size, domain.group_gen_inv.l, domain.size_inv.l,
                                   d2.group_gen.l, d2.group_gen_inv.l, d2.size_inv.l, jac, proofs_out));
    return jac_to_g1(jac);
  }
  auto cp = vec_commit_openings(rng, setup, std::vector<Fr>(v, v + n));
  for (size_t i = 0; i < cp.second.size(); i++) memcpy(proofs_out + 8 * i, cp.second[i].w.data(), 64);
  return kzg::commit(setup, cp.first).unwrap();      // :46
}
std::pair<G1, std::vector<G1>> vec_commit(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v) {
  static_assert(sizeof(G1) == 64, "a G1 is eight u64 words");
  std::vector<G1> proofs(Radix2Domain::create(v.size() + PADDING_LEN).size);
  G1 com = vec_commit_flat(rng, setup, v.data(), v.size(), proofs.empty() ? nullptr : proofs[0].w.data());
  return {com, std::move(proofs)};
}

std::vector<std::pair<G1, std::vector<G1>>> vec_commit_batch(Rng& rng, const kzg::KZGSetup& setup, const std::vector<std::vector<Fr>>& vecs) {
  const Device& dev = *setup.device();
  if (dev.group()) throw std::invalid_argument("vec_commit_batch: a group device commits vector by vector (vec_commit)");
  size_t longest = 0;
  for (const auto& v : vecs) longest = std::max(longest, v.size());
  const size_t n = longest + PADDING_LEN, m = vecs.size();
  const Radix2Domain domain = Radix2Domain::create(n), d2 = Radix2Domain::create(2 * domain.size);
  unsigned log_size = 0;
  while ((size_t(1) << log_size) < domain.size) log_size++;
  // row j = vecs[j] | its padding scalar (src/vec.rs:31-33, drawn in index order) | zeros: the evaluations ark-poly's ifft would pad with
  std::vector<Fr> rows(m * n);
  for (size_t j = 0; j < m; j++) {
    std::copy(vecs[j].begin(), vecs[j].end(), rows.begin() + j * n);
    rows[j * n + vecs[j].size()] = fr_rand(rng);
  }
  std::vector<uint64_t> jac(12 * m);
  std::vector<std::pair<G1, std::vector<G1>>> out(m);
  std::vector<G1> proofs(m * domain.size);
  if (m)
    dev.check(keaki_hip_vec_commit_batch(dev.ctx(), setup.srs(), rows[0].l, n, m, n, log_size, domain.group_gen_inv.l, domain.size_inv.l, d2.group_gen.l,
                                         d2.group_gen_inv.l, d2.size_inv.l, jac.data(), proofs[0].w.data()));
  for (size_t j = 0; j < m; j++)
    out[j] = {jac_to_g1(&jac[12 * j]), std::vector<G1>(proofs.begin() + j * domain.size, proofs.begin() + (j + 1) * domain.size)};
  return out;
}

namespace {
// (domain, log2 of its size) of an update over `domain_size` evaluations: a power of two, on a single device
std::pair<Radix2Domain, unsigned> update_domain(const kzg::KZGSetup& setup, size_t domain_size, const char* what) {
  if (setup.device()->group()) throw std::invalid_argument(std::string(what) + ": a group device has no update tables (single device only)");
  if (domain_size < 1 || (domain_size & (domain_size - 1)) != 0) throw std::invalid_argument(std::string(what) + ": the domain size is not a power of two");
  unsigned log_size = 0;
  while ((size_t(1) << log_size) < domain_size) log_size++;
  return {Radix2Domain::create(domain_size), log_size};
}
}  // namespace
void precompute_vec_update(const kzg::KZGSetup& setup, size_t domain_size) {
  const auto dl = update_domain(setup, domain_size, "precompute_vec_update");
  const Device& dev = *setup.device();
  dev.check(keaki_hip_srs_g1_precompute_update(dev.ctx(), setup.srs(), dl.second, dl.first.group_gen.l, dl.first.group_gen_inv.l, dl.first.size_inv.l));
}
void vec_update_flat(const kzg::KZGSetup& setup, size_t domain_size, const uint32_t* idx, const Fr* deltas, size_t k, uint64_t* com_inout, uint64_t* proofs_inout) {
  const auto dl = update_domain(setup, domain_size, "vec_update");
  const Device& dev = *setup.device();
  uint64_t jac[12];
  if (com_inout) {                               // affine -> normalised Jacobian (x, y, 1 | 1, 1, 0)
    G1 c; memcpy(c.w.data(), com_inout, 64);
    const bool inf = c.is_zero();
    for (int i = 0; i < 3; i++) memcpy(jac + 4 * i, G1_GEN_W, 32);      // G1_GEN_W[0..4) is x = 1: the Montgomery one of Fq
    if (inf) memset(jac + 8, 0, 32); else memcpy(jac, com_inout, 64);
  }
  dev.check(keaki_hip_vec_update(dev.ctx(), setup.srs(), dl.second, dl.first.group_gen.l, dl.first.group_gen_inv.l, dl.first.size_inv.l, idx, k ? deltas[0].l : nullptr, k,
                                 com_inout ? jac : nullptr, proofs_inout));
  if (com_inout && k) { const G1 c = jac_to_g1(jac); memcpy(com_inout, c.w.data(), 64); }
}
void vec_update(const kzg::KZGSetup& setup, G1& com, std::vector<G1>& proofs, const std::vector<size_t>& idx, const std::vector<Fr>& old_values,
                const std::vector<Fr>& new_values) {
  if (idx.size() != old_values.size() || idx.size() != new_values.size()) throw std::invalid_argument("vec_update: idx, old_values and new_values differ in length");
  std::vector<uint32_t> ix(idx.size());
  std::vector<Fr> deltas(idx.size());
  for (size_t t = 0; t < idx.size(); t++) {
    if (idx[t] >= proofs.size()) throw std::invalid_argument("vec_update: index " + std::to_string(idx[t]) + " is outside the domain of " + std::to_string(proofs.size()));
    ix[t] = (uint32_t)idx[t];
    deltas[t] = new_values[t] - old_values[t];
  }
  vec_update_flat(setup, proofs.size(), ix.data(), deltas.data(), ix.size(), com.w.data(), proofs.empty() ? nullptr : proofs[0].w.data());
}

bool vec_verify_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* v, size_t n, const uint64_t* proofs) {
  const Radix2Domain domain = Radix2Domain::create(n + PADDING_LEN);      // the domain vec_commit interpolated over (src/vec.rs:36)
  return kzg::verify_batch_flat(rng, setup, com.w.data(), 1, &domain.group_gen, true, v, proofs, n);
}
size_t vec_verify_each_flat(const kzg::KZGSetup& setup, const G1& com, const Fr* v, size_t n, const uint64_t* proofs, uint8_t* status_out) {
  const Radix2Domain domain = Radix2Domain::create(n + PADDING_LEN);
  return kzg::verify_each_flat(setup, com.w.data(), 1, &domain.group_gen, true, v, proofs, n, status_out);
}
std::vector<uint8_t> vec_verify_each(const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& v, const std::vector<G1>& proofs) {
  if (proofs.size() < v.size()) throw std::invalid_argument("vec_verify_each: fewer proofs than values");
  std::vector<uint8_t> status(v.size());
  vec_verify_each_flat(setup, com, v.data(), v.size(), v.empty() ? nullptr : proofs[0].w.data(), status.data());
  return status;
}
bool vec_verify(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& v, const std::vector<G1>& proofs) {
  if (proofs.size() < v.size()) throw std::invalid_argument("vec_verify: fewer proofs than values");
  return vec_verify_flat(rng, setup, com, v.data(), v.size(), v.empty() ? nullptr : proofs[0].w.data());
}

std::vector<enc::Ciphertext> vec_encrypt(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& points,
                                         const std::vector<Fr>& values, const std::vector<std::vector<uint8_t>>& messages) {
  size_t n = messages.size();
  std::vector<enc::Ciphertext> out(n);
  if (!n) return out;
  // the reference draws one r per item in index order inside the loop (src/vec.rs:63-66 -> src/kem.rs:26)
  std::vector<Fr> rs(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);
  size_t max_len = 0;
  for (auto& m : messages) max_len = std::max(max_len, m.size());
  std::vector<uint64_t> ct(16 * n);
  std::vector<uint8_t> key(n * std::max<size_t>(max_len, 1));
  encap_many(setup, com, points[0].l, values[0].l, rs[0].l, n, ct.data(), key.data(), max_len);
  for (size_t i = 0; i < n; i++) {
    memcpy(out[i].first.w.data(), &ct[16 * i], 128);
    out[i].second.resize(messages[i].size());
    // BLAKE3 XOF: a shorter key is a prefix of a longer one, so one max_len call serves ragged messages
    for (size_t j = 0; j < messages[i].size(); j++) out[i].second[j] = key[i * max_len + j] ^ messages[i][j];
  }
  return out;
}

// The same two loops on contiguous buffers of n equal-length messages: identical draws and bytes, no per-item containers (what an FFI
// caller with 2^20 items wants).
void vec_encrypt_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* points, const Fr* values, const uint8_t* msgs, size_t n,
                      size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  if (!n) return;
  // One r per item, in index order (src/vec.rs:63-66 -> src/kem.rs:26): the draws are the host's and serial by the reference's semantics
  // (13.5 ms for 2^20 items, twice the rate of the device). Large vectors go in PIECES of growing size -- 1/16, 1/8, 1/4, the rest: a helper
  // thread draws the r of piece k + 1 while the device works on piece k, and only the first, small piece is drawn with the device idle
  // (the stream of draws is the same; only one thread touches `rng` at a time). Inside a piece the C ABI overlaps its own copies with its
  // kernels (api.hip: pipelined).
  static const size_t SIXTEENTHS[5] = {0, 1, 3, 7, 16};
  const size_t pieces = n >= ((size_t)1 << 18) ? 4 : 1;
  auto bound = [&](size_t k) { return k >= pieces ? n : std::min(n, ((n * SIXTEENTHS[k] / 16) + 63) & ~(size_t)63); };
  // the draws land in memory nobody has touched or cleared: a value-initialised std::vector<Fr>(n) spends 6 ms at n = 2^20 writing zeros into
  // fresh 4 KB pages before the first draw. Huge pages where the kernel offers them on request (the first touch is the helper thread's).
  struct RawFr {
    Fr* p = nullptr;
    explicit RawFr(size_t count) {
      const size_t HP = (size_t)2 << 20, bytes = count * sizeof(Fr);
      if (bytes >= HP) {
        p = static_cast<Fr*>(aligned_alloc(HP, (bytes + HP - 1) & ~(HP - 1)));
        if (p) (void)madvise(p, (bytes + HP - 1) & ~(HP - 1), MADV_HUGEPAGE);
      } else {
        p = static_cast<Fr*>(malloc(bytes));
      }
      if (!p) throw std::bad_alloc();
    }
    ~RawFr() { free(p); }
    RawFr(const RawFr&) = delete;
    RawFr& operator=(const RawFr&) = delete;
  } rs_mem(n);
  Fr* rs = rs_mem.p;
  auto draw = [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) rs[i] = fr_rand(rng); };
  std::vector<uint8_t> gt_unused;
  draw(0, bound(1));
  for (size_t k = 0; k < pieces; k++) {
    const size_t lo = bound(k), hi = bound(k + 1), m = hi - lo;
    std::thread ahead;
    if (k + 1 < pieces) ahead = std::thread(draw, hi, bound(k + 2));
    try {
      if (m && msg_len)                                                                                         // src/enc.rs:32-36 on the device
        encrypt_many(setup, com, points[lo].l, values[lo].l, rs[lo].l, msgs + msg_len * lo, m, ct_g2_out + 16 * lo, ct_msg_out + msg_len * lo, msg_len);
      else if (m) {
        gt_unused.resize(m * 384);       // the ABI wants at least one of gt / key
        setup.device()->check(keaki_hip_encap_batch(setup.device()->ctx(), com.w.data(), setup.tau_g2().w.data(), points[lo].l, values[lo].l, rs[lo].l, m,
                                                    ct_g2_out + 16 * lo, gt_unused.data(), nullptr, 0));
      }
    } catch (...) {
      if (ahead.joinable()) ahead.join();
      throw;
    }
    if (ahead.joinable()) ahead.join();
  }
}
// vec_encrypt to m commitments in ONE device call (keaki_hip_encrypt_multi): group j = the next counts[j] items, under coms[j]. One r per item
// in global index order -- the stream m consecutive vec_encrypt calls draw -- so points and bodies equal those of that loop.
void vec_encrypt_batch(Rng& rng, const kzg::KZGSetup& setup, const G1* coms, const size_t* counts, size_t m, const Fr* points, const Fr* values,
                       const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  const Device& dev = *setup.device();
  if (dev.group()) throw std::invalid_argument("vec_encrypt_batch: a group device encrypts commitment by commitment (vec_encrypt)");
  std::vector<uint64_t> offsets(m + 1, 0), cw(8 * std::max<size_t>(m, 1));
  for (size_t j = 0; j < m; j++) {
    offsets[j + 1] = offsets[j] + counts[j];
    memcpy(&cw[8 * j], coms[j].w.data(), 64);
  }
  const size_t n = (size_t)offsets[m];
  if (!n) return;
  std::vector<Fr> rs(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);
  if (msg_len) {
    dev.check(keaki_hip_encrypt_multi(dev.ctx(), cw.data(), offsets.data(), m, setup.tau_g2().w.data(), points[0].l, values[0].l, rs[0].l, msgs, n, ct_g2_out,
                                      ct_msg_out, msg_len));
  } else {
    std::vector<uint8_t> gt_unused(n * 384);       // the ABI wants at least one of gt / key
    dev.check(keaki_hip_encap_multi(dev.ctx(), cw.data(), offsets.data(), m, setup.tau_g2().w.data(), points[0].l, values[0].l, rs[0].l, n, ct_g2_out,
                                    gt_unused.data(), nullptr, 0));
  }
}
namespace {
std::vector<Fr> subset_points(size_t domain_size, const std::vector<size_t>& idx, const char* what) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  std::vector<Fr> z(idx.size());
  for (size_t j = 0; j < idx.size(); j++) {
    if (idx[j] >= dom.size) throw kzg::SetError(std::string(what) + ": index outside the domain");
    z[j] = dom.group_gen.pow(idx[j]);
  }
  return z;            // a repeated index is a repeated point: the kzg layer refuses it
}
}  // namespace
G1 vec_open_subset(const kzg::KZGSetup& setup, size_t domain_size, const std::vector<size_t>& idx, const std::vector<G1>& proofs) {
  const std::vector<Fr> z = subset_points(domain_size, idx, "vec_open_subset");
  std::vector<G1> sel(idx.size());
  for (size_t j = 0; j < idx.size(); j++) {
    if (idx[j] >= proofs.size()) throw kzg::SetError("vec_open_subset: no proof for an index");
    sel[j] = proofs[idx[j]];
  }
  return kzg::aggregate_proofs(setup, z, sel);
}
bool vec_verify_subset(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<size_t>& idx, const std::vector<Fr>& values, const G1& proof) {
  return kzg::verify_set(setup, com, subset_points(domain_size, idx, "vec_verify_subset"), values, proof);
}
bool vec_verify_subsets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                        const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  return kzg::verify_sets_indexed(rng, setup, com, dom.group_gen, dom.size, idx_rows, values, proofs);
}
std::vector<uint8_t> vec_verify_subsets_each(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                                             const std::vector<std::vector<Fr>>& values, const std::vector<G1>& proofs) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  return kzg::verify_sets_each_indexed(setup, com, dom.group_gen, dom.size, idx_rows, values, proofs);
}
void vec_encrypt_subsets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<std::vector<size_t>>& idx_rows,
                         const std::vector<std::vector<Fr>>& values, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  const size_t n = idx_rows.size();
  std::vector<uint64_t> a(n * 8), z(n * 16);
  kzg::set_pairs_indexed(setup, com, dom.group_gen, dom.size, idx_rows, values, a.data(), z.data());      // every refusal comes before the first draw from rng
  if (msg_len) {
    kem::seal_pairs(rng, setup, a.data(), z.data(), n, msgs, msg_len, ct_g2_out, ct_msg_out);
  } else {
    kem::seal_pairs(rng, setup, a.data(), z.data(), n, nullptr, 0, ct_g2_out, nullptr);
  }
}
std::vector<G1> vec_open_cosets(const kzg::KZGSetup& setup, const std::vector<Fr>& evals, size_t l) {
  if (evals.empty()) throw kzg::SetError("vec_open_cosets: no evaluations");
  const Radix2Domain dom = Radix2Domain::create(evals.size());
  return kzg::open_fk_cosets(setup, dom.ifft(evals), dom.size, l);
}
std::vector<size_t> vec_coset_indices(size_t domain_size, size_t l, size_t i) {
  const size_t d = Radix2Domain::create(domain_size).size;
  if (l < 1 || (l & (l - 1)) != 0 || l > d || i >= d / l) throw kzg::SetError("vec_coset_indices: l is a power of two <= the domain, i < domain / l");
  std::vector<size_t> idx(l);
  for (size_t t = 0; t < l; t++) idx[t] = i + t * (d / l);
  return idx;
}
bool vec_verify_cosets_flat(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* evals, size_t domain_size, size_t l, const uint64_t* proofs) {
  const size_t d = domain_size;
  if (d < 1 || (d & (d - 1)) != 0 || l < 1 || (l & (l - 1)) != 0 || l > d) throw kzg::SetError("vec_verify_cosets: the domain and the coset size are powers of two, l <= d");
  const Radix2Domain dom = Radix2Domain::create(d);
  return kzg::verify_cosets_flat(rng, setup, com.w.data(), 1, &dom.group_gen, true, evals, 1, d / l, l, proofs, d / l);
}
bool vec_verify_cosets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& evals, size_t l, const std::vector<G1>& proofs) {
  if (evals.empty()) throw kzg::SetError("vec_verify_cosets: no evaluations");
  const size_t d = Radix2Domain::create(evals.size()).size;
  if (l < 1 || (l & (l - 1)) != 0 || l > d || proofs.size() != d / l) throw kzg::SetError("vec_verify_cosets: l is a power of two <= the domain, one proof per coset");
  std::vector<Fr> e(evals);
  e.resize(d, Fr::zero());
  return vec_verify_cosets_flat(rng, setup, com, e.data(), d, l, proofs[0].w.data());
}
bool vec_verify_cosets_subset(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets,
                              const std::vector<Fr>& values, const std::vector<G1>& proofs) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  if (l < 1 || (l & (l - 1)) != 0 || l > dom.size) throw kzg::SetError("vec_verify_cosets_subset: l is a power of two <= the domain");
  if (values.size() != cosets.size() * l || proofs.size() != cosets.size()) throw kzg::SetError("vec_verify_cosets_subset: l values and one proof per listed coset");
  std::vector<Fr> h(cosets.size());
  for (size_t k = 0; k < cosets.size(); k++) {
    if (cosets[k] >= dom.size / l) throw kzg::SetError("vec_verify_cosets_subset: coset index outside domain / l");
    h[k] = dom.group_gen.pow(cosets[k]);
  }
  return kzg::verify_cosets_flat(rng, setup, com.w.data(), 1, h.data(), false, values.data(), l, 1, l, proofs.empty() ? nullptr : proofs[0].w.data(), cosets.size());
}
std::vector<uint8_t> vec_verify_cosets_each(const kzg::KZGSetup& setup, const G1& com, const std::vector<Fr>& evals, size_t l, const std::vector<G1>& proofs) {
  if (evals.empty()) throw kzg::SetError("vec_verify_cosets_each: no evaluations");
  const Radix2Domain dom = Radix2Domain::create(evals.size());
  const size_t d = dom.size;
  if (l < 1 || (l & (l - 1)) != 0 || l > d || proofs.size() != d / l) throw kzg::SetError("vec_verify_cosets_each: l is a power of two <= the domain, one proof per coset");
  std::vector<Fr> e(evals);
  e.resize(d, Fr::zero());
  return kzg::verify_cosets_each_flat(setup, com.w.data(), 1, &dom.group_gen, true, e.data(), 1, d / l, l, proofs[0].w.data(), d / l);
}
namespace {
// the shifts omega_d^i of the listed cosets, with the argument checks of vec_verify_cosets_subset
std::vector<Fr> coset_shifts(const char* what, size_t domain_size, size_t l, const std::vector<size_t>& cosets) {
  const Radix2Domain dom = Radix2Domain::create(domain_size);
  if (l < 1 || (l & (l - 1)) != 0 || l > dom.size) throw kzg::SetError(std::string(what) + ": l is a power of two <= the domain");
  std::vector<Fr> h(cosets.size());
  for (size_t k = 0; k < cosets.size(); k++) {
    if (cosets[k] >= dom.size / l) throw kzg::SetError(std::string(what) + ": coset index outside domain / l");
    h[k] = dom.group_gen.pow(cosets[k]);
  }
  return h;
}
}  // namespace
std::vector<uint8_t> vec_verify_cosets_each_subset(const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets,
                                                   const std::vector<Fr>& values, const std::vector<G1>& proofs) {
  const std::vector<Fr> h = coset_shifts("vec_verify_cosets_each_subset", domain_size, l, cosets);
  if (values.size() != cosets.size() * l || proofs.size() != cosets.size()) throw kzg::SetError("vec_verify_cosets_each_subset: l values and one proof per listed coset");
  return kzg::verify_cosets_each_flat(setup, com.w.data(), 1, h.data(), false, values.data(), l, 1, l, proofs.empty() ? nullptr : proofs[0].w.data(), cosets.size());
}
void vec_encrypt_cosets(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, size_t l, const std::vector<size_t>& cosets, const Fr* values,
                        const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  // every refusal comes before the first draw from rng
  const std::vector<Fr> h = coset_shifts("vec_encrypt_cosets", domain_size, l, cosets);
  const size_t n = cosets.size();
  if (setup.g2_pow().size() <= l) throw kzg::SetError("vec_encrypt_cosets: this KZGSetup holds no [tau^l]_2: build it with G2 powers beyond l (setup_with_g2, from_powers_g2)");
  std::vector<uint64_t> coms(n * 8);
  std::vector<Fr> c(n), zeros(n);
  kzg::coset_pairs_flat(setup, com.w.data(), 1, h.data(), false, values, l, 1, l, n, coms.data(), c.data());
  if (!n) return;
  const Device& dev = *setup.device();
  std::vector<Fr> rs(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);      // one r per item in index order, as everywhere else
  std::vector<uint64_t> offsets(n + 1);
  for (size_t i = 0; i <= n; i++) offsets[i] = i;
  // item k: ct = r_k ([tau^l]_2 - c_k g2), key = KDF(e(r_k A_k, g2)): n groups of one item with coms := A, points := c, values := 0
  const uint64_t* tau_l = setup.g2_pow()[l].w.data();
  if (msg_len) {
    dev.check(keaki_hip_encrypt_multi(dev.ctx(), coms.data(), offsets.data(), n, tau_l, c[0].l, zeros[0].l, rs[0].l, msgs, n, ct_g2_out, ct_msg_out, msg_len));
  } else {
    std::vector<uint8_t> gt_unused(n * 384);
    dev.check(keaki_hip_encap_multi(dev.ctx(), coms.data(), offsets.data(), n, tau_l, c[0].l, zeros[0].l, rs[0].l, n, ct_g2_out, gt_unused.data(), nullptr, 0));
  }
}
void vec_encrypt_subset_batch(Rng& rng, const kzg::KZGSetup& setup, const G1& com, size_t domain_size, const std::vector<size_t>& idx, const Fr* values,
                              size_t n, const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  const Device& dev = *setup.device();
  const size_t k = idx.size();
  const std::vector<Fr> z = subset_points(domain_size, idx, "vec_encrypt_subset_batch");
  if (!n) return;
  // [Z]_2 (and the argument checks: set size, repeated index, G2 powers) from the first tuple's pair
  const std::pair<G1, G2> az0 = kzg::set_pair(setup, com, z, std::vector<Fr>(values, values + k));
  if (dev.group()) throw kzg::SetError("vec_encrypt_subset_batch: single device only");
  // Z and the weights once; q_j = Z / (x - z_j) on the host; row i = -I_i = -sum_j (y_ij c_j) q_j
  std::vector<Fr> zc(k + 1), w(k);
  dev.check(keaki_hip_kzg_set_polys(dev.ctx(), z[0].l, nullptr, k, zc[0].l, w[0].l, nullptr));
  std::vector<Fr> q(k * k);
  for (size_t j = 0; j < k; j++) {
    Fr carry = Fr::one();                                  // q_(k-1) = Z_k = 1, q_(t-1) = Z_t + z_j q_t
    for (size_t t = k; t-- > 0;) { q[j * k + t] = carry; carry = zc[t] + z[j] * carry; }
  }
  std::vector<Fr> rows(n * k);
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < k; j++) {
      const Fr sj = -(values[i * k + j] * w[j]);
      for (size_t t = 0; t < k; t++) rows[i * k + t] = rows[i * k + t] + sj * q[j * k + t];
    }
  std::vector<uint64_t> jac(n * 12), coms(n * 8);
  dev.check(keaki_hip_msm_g1_batch(dev.ctx(), setup.srs(), rows[0].l, k, n, k, jac.data()));
  uint64_t two[24], sum[12];
  const G1 one = g1_generator();                            // its x is the Montgomery form of 1
  if (com.is_zero()) { memcpy(two, one.w.data(), 32); memcpy(two + 4, one.w.data(), 32); memset(two + 8, 0, 32); }
  else { memcpy(two, com.w.data(), 64); memcpy(two + 8, one.w.data(), 32); }
  for (size_t i = 0; i < n; i++) {
    memcpy(two + 12, &jac[12 * i], 96);
    dev.check(keaki_hip_g1_sum(dev.ctx(), two, 2, sum));
    const G1 ci = jac_to_g1(sum);
    memcpy(&coms[8 * i], ci.w.data(), 64);
  }
  std::vector<Fr> rs(n), zeros(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);      // one r per item in index order, as everywhere else
  std::vector<uint64_t> offsets(n + 1);
  for (size_t i = 0; i <= n; i++) offsets[i] = i;
  if (msg_len) {
    dev.check(keaki_hip_encrypt_multi(dev.ctx(), coms.data(), offsets.data(), n, az0.second.w.data(), zeros[0].l, zeros[0].l, rs[0].l, msgs, n, ct_g2_out, ct_msg_out, msg_len));
  } else {
    std::vector<uint8_t> gt_unused(n * 384);
    dev.check(keaki_hip_encap_multi(dev.ctx(), coms.data(), offsets.data(), n, az0.second.w.data(), zeros[0].l, zeros[0].l, rs[0].l, n, ct_g2_out, gt_unused.data(), nullptr, 0));
  }
}
void vec_decrypt_flat(const kzg::KZGSetup& setup, const uint64_t* proofs, const uint64_t* ct_g2, const uint8_t* ct_msgs, size_t n, size_t msg_len,
                      uint8_t* msgs_out) {
  if (!n || !msg_len) return;
  decrypt_many(setup, proofs, ct_g2, ct_msgs, n, msgs_out, msg_len);                                          // src/enc.rs:48-52 on the device
}
std::vector<std::vector<uint8_t>> vec_decrypt(const kzg::KZGSetup& setup, const std::vector<G1>& proofs,
                                              const std::vector<const enc::Ciphertext*>& cts) {
  size_t n = cts.size();
  std::vector<std::vector<uint8_t>> out(n);
  if (!n) return out;
  size_t max_len = 0;
  for (auto* c : cts) max_len = std::max(max_len, c->second.size());
  std::vector<uint64_t> pr(8 * n), ct(16 * n);
  for (size_t i = 0; i < n; i++) { memcpy(&pr[8 * i], proofs[i].w.data(), 64); memcpy(&ct[16 * i], cts[i]->first.w.data(), 128); }
  std::vector<uint8_t> key(n * std::max<size_t>(max_len, 1));
  decap_many(setup, pr.data(), ct.data(), n, key.data(), max_len);
  for (size_t i = 0; i < n; i++) {
    out[i].resize(cts[i]->second.size());
    for (size_t j = 0; j < out[i].size(); j++) out[i][j] = key[i * max_len + j] ^ cts[i]->second[j];
  }
  return out;
}

}  // namespace vec

// ------------------------------------------------------------------------------------------------ dist
namespace dist {

std::pair<size_t, size_t> Shard::bounds(size_t n) const {
  const size_t base = n / world, rem = n % world;
  const size_t lo = rank * base + std::min(rank, rem);
  return {lo, lo + base + (rank < rem ? 1 : 0)};
}

void prepare(const kzg::KZGSetup& setup, const Shard& sh) {
  auto b = sh.bounds(setup.g1_pow().size());
  (void)setup.chunk_srs(b.first, b.second);
}

kzg::Result<Partial> commit_partial(const kzg::KZGSetup& setup, const DensePolynomial& p, const Shard& sh) {
  const size_t len = setup.g1_pow().size();
  if (p.size() > len) return kzg::Result<Partial>::Err(kzg::KZGError{kzg::KZGError::PolynomialTooLarge, p.size(), len});
  // the ranges follow the SRS, not the polynomial: a rank's window tables are built once per setup and serve every polynomial
  auto b = sh.bounds(len);
  const size_t lo = std::min(b.first, p.size()), hi = std::min(b.second, p.size());
  Partial out;
  setup.device()->check(keaki_hip_msm_g1(setup.device()->ctx(), setup.chunk_srs(b.first, b.second), hi > lo ? p[lo].l : nullptr, hi - lo, out.data()));
  return kzg::Result<Partial>::Ok(out);
}

std::pair<Partial, std::vector<G1>> vec_commit_partial(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v, const Shard& sh) {
  auto cp = vec::vec_commit_openings(rng, setup, v);                 // replicated on every rank: same rng stream, same values
  return {commit_partial(setup, cp.first, sh).unwrap(), std::move(cp.second)};
}

static unsigned log2_of(size_t n) {
  unsigned l = 0;
  while ((size_t(1) << l) < n) l++;
  return l;
}
bool ShardedOpenFk::can_shard(const kzg::KZGSetup& setup, size_t domain_size, const Shard& sh) {
  const size_t w = sh.world;
  return w >= 2 && (w & (w - 1)) == 0 && domain_size >= w * w && (domain_size & (domain_size - 1)) == 0 && domain_size <= setup.g1_pow().size();
}
ShardedOpenFk::ShardedOpenFk(const kzg::KZGSetup& setup, size_t domain_size, const Shard& sh) : setup_(setup), dev_(setup.device()), d_(domain_size) {
  vec::Radix2Domain d2 = vec::Radix2Domain::create(2 * domain_size);
  const Device& dev = *setup.device();
  dev.check(keaki_hip_fk_shard_create(dev.ctx(), setup.srs(), log2_of(domain_size), (uint32_t)sh.rank, (uint32_t)sh.world, d2.group_gen.l,
                                      d2.group_gen_inv.l, d2.size_inv.l, &fk_));
  dev.check(keaki_hip_fk_shard_sizes(fk_, sizes_));
}
ShardedOpenFk::~ShardedOpenFk() { keaki_hip_fk_shard_free(dev_->ctx(), fk_); }
void ShardedOpenFk::prepare(void* d_send, void* d_recv, const FkExchange& ex) {
  if (prepared_) return;
  const Device& dev = *setup_.device();
  dev.check(keaki_hip_fk_shard_setup(dev.ctx(), fk_, 0, d_send, nullptr));
  dev.check(keaki_hip_synchronize(dev.ctx()));
  if (ex.all_to_all(ex.user, d_send, d_recv, sizes_[1])) throw std::runtime_error("ShardedOpenFk: the caller's all-to-all failed");
  dev.check(keaki_hip_fk_shard_setup(dev.ctx(), fk_, 1, nullptr, d_recv));
  dev.check(keaki_hip_synchronize(dev.ctx()));
  prepared_ = true;
}
std::vector<G1> ShardedOpenFk::open(const std::vector<Fr>& p, void* d_send, void* d_recv, const FkExchange& ex) {
  if (p.size() != d_) throw std::runtime_error("ShardedOpenFk::open: the polynomial must have domain_size coefficients");
  prepare(d_send, d_recv, ex);
  const Device& dev = *setup_.device();
  dev.check(keaki_hip_fk_shard_open(dev.ctx(), fk_, 0, p[0].l, d_send, nullptr, nullptr));
  dev.check(keaki_hip_synchronize(dev.ctx()));
  if (ex.all_to_all(ex.user, d_send, d_recv, sizes_[2])) throw std::runtime_error("ShardedOpenFk: the caller's all-to-all failed");
  dev.check(keaki_hip_fk_shard_open(dev.ctx(), fk_, 1, nullptr, d_send, d_recv, nullptr));
  dev.check(keaki_hip_synchronize(dev.ctx()));
  if (ex.all_to_all(ex.user, d_send, d_recv, sizes_[2])) throw std::runtime_error("ShardedOpenFk: the caller's all-to-all failed");
  dev.check(keaki_hip_fk_shard_open(dev.ctx(), fk_, 2, nullptr, d_send, d_recv, nullptr));
  dev.check(keaki_hip_synchronize(dev.ctx()));
  if (ex.all_gather(ex.user, d_send, d_recv, sizes_[3])) throw std::runtime_error("ShardedOpenFk: the caller's all-gather failed");
  std::vector<G1> out(d_);
  dev.check(keaki_hip_fk_shard_open(dev.ctx(), fk_, 3, nullptr, nullptr, d_recv, out[0].w.data()));
  return out;
}
std::pair<Partial, std::vector<G1>> vec_commit_partial_fk(Rng& rng, const kzg::KZGSetup& setup, const std::vector<Fr>& v, const Shard& sh,
                                                          ShardedOpenFk& fk, void* d_send, void* d_recv, const FkExchange& ex) {
  std::vector<Fr> coeffs = vec::vec_commit_coeffs(rng, setup, v);       // replicated: same rng stream, same values
  std::vector<G1> proofs = fk.open(coeffs, d_send, d_recv, ex);
  while (!coeffs.empty() && coeffs.back().is_zero()) coeffs.pop_back();
  return {commit_partial(setup, coeffs, sh).unwrap(), std::move(proofs)};
}

G1 commit_combine(const kzg::KZGSetup& setup, const Partial* partials, size_t world) {
  uint64_t jac[12];
  setup.device()->check(keaki_hip_g1_sum(setup.device()->ctx(), world ? partials[0].data() : nullptr, world, jac));
  return jac_to_g1(jac);
}

void vec_encrypt_flat_shard(Rng& rng, const kzg::KZGSetup& setup, const G1& com, const Fr* points, const Fr* values, const uint8_t* msgs, size_t n,
                            size_t msg_len, const Shard& sh, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  if (!n) return;
  std::vector<Fr> rs(n);
  for (size_t i = 0; i < n; i++) rs[i] = fr_rand(rng);        // the whole stream, as the serial loop would draw it (src/vec.rs:63-66 -> src/kem.rs:26)
  auto b = sh.bounds(n);
  const size_t lo = b.first, m = b.second - b.first;
  if (!m) return;
  setup.device()->check(keaki_hip_encap_batch(setup.device()->ctx(), com.w.data(), setup.tau_g2().w.data(), points[lo].l, values[lo].l, rs[lo].l, m,
                                              ct_g2_out, nullptr, msg_len ? ct_msg_out : nullptr, msg_len));
  for (size_t i = 0; i < m * msg_len; i++) ct_msg_out[i] ^= msgs[lo * msg_len + i];
}

}  // namespace dist
}  // namespace keaki
