// Flat C front-end of the C++ host mirror (keaki.hpp) so the pytest harness and other FFI users can
// drive kzg / kem / enc / vec exactly as the reference's tests do. Errors: 0 ok, 1 = KZGError
// (degree/max written to err_out[2]), negative = HipError status; message via keaki_host_last_error().
#include <algorithm>
#include <cstring>
#include <string>

#include "keaki.hpp"
#include "ptau.hpp"

using namespace keaki;

namespace {
thread_local std::string g_err;
struct CallbackRng : Rng {
  uint64_t (*fn)(void*); void* user;
  uint64_t next_u64() override { return fn(user); }
};
struct SplitMix64Rng : Rng {  // deterministic stand-in for ark_std::test_rng() in the harness
  uint64_t s;
  explicit SplitMix64Rng(uint64_t seed) : s(seed) {}
  uint64_t next_u64() override {
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
};
struct Setup { std::shared_ptr<Device> dev; kzg::KZGSetup s; };

template <class F>
int guard(F&& f) {
  try { return f(); }
  catch (const HipError& e) { g_err = e.what(); return e.status; }
  catch (const kzg::SetError& e) { g_err = e.what(); return 3; }          // a set call refused: repeated point, no G2 powers, bad sizes
  catch (const std::exception& e) { g_err = e.what(); return -1000; }
}
// bytes that do not decode (WireError): status 2, the index of the first rejected item and the reason in bad_out[0], [1]
template <class F>
int wire_guard(uint64_t* bad_out, F&& f) {
  return guard([&] {
    try { f(); return 0; }
    catch (const WireError& e) {
      if (bad_out) { bad_out[0] = e.index; bad_out[1] = (uint64_t)e.reason; }
      g_err = e.what();
      return 2;
    }
  });
}
Fr fr_of(const uint64_t* p) { Fr r; memcpy(r.l, p, 32); return r; }
std::vector<Fr> frs_of(const uint64_t* p, size_t n) { std::vector<Fr> v(n); for (size_t i = 0; i < n; i++) v[i] = fr_of(p + 4 * i); return v; }
G1 g1_of(const uint64_t* p) { G1 r; memcpy(r.w.data(), p, 64); return r; }
G2 g2_of(const uint64_t* p) { G2 r; memcpy(r.w.data(), p, 128); return r; }
int kzg_err(const kzg::KZGError& e, uint64_t* err_out) { if (err_out) { err_out[0] = e.degree; err_out[1] = e.max_degree; } g_err = e.to_string(); return 1; }
}  // namespace

extern "C" {

const char* keaki_host_last_error(void) { return g_err.c_str(); }

void* keaki_host_rng_splitmix(uint64_t seed) { return new SplitMix64Rng(seed); }
void* keaki_host_rng_callback(uint64_t (*fn)(void*), void* user) { auto* r = new CallbackRng(); r->fn = fn; r->user = user; return r; }
void keaki_host_rng_free(void* rng) { delete (Rng*)rng; }
void keaki_host_fr_rand(void* rng, uint64_t* out) { Fr r = fr_rand(*(Rng*)rng); memcpy(out, r.l, 32); }
// n consecutive draws (what a loop of `Fr::rand(rng)` consumes), for harnesses that replay the stream of vec_encrypt
void keaki_host_fr_rand_many(void* rng, size_t n, uint64_t* out) { for (size_t i = 0; i < n; i++) { Fr r = fr_rand(*(Rng*)rng); memcpy(out + 4 * i, r.l, 32); } }

// Fr helpers for the harness (Fr::from(i64), arithmetic, polynomial evaluation)
void keaki_host_fr_from_i64(int64_t v, uint64_t* out) { Fr r = Fr::from_i64(v); memcpy(out, r.l, 32); }
void keaki_host_fr_mul(const uint64_t* a, const uint64_t* b, uint64_t* out) { Fr r = fr_of(a) * fr_of(b); memcpy(out, r.l, 32); }
void keaki_host_fr_add(const uint64_t* a, const uint64_t* b, uint64_t* out) { Fr r = fr_of(a) + fr_of(b); memcpy(out, r.l, 32); }
void keaki_host_fr_sub(const uint64_t* a, const uint64_t* b, uint64_t* out) { Fr r = fr_of(a) - fr_of(b); memcpy(out, r.l, 32); }
void keaki_host_fr_inv(const uint64_t* a, uint64_t* out) { Fr r = fr_of(a).inverse(); memcpy(out, r.l, 32); }
void keaki_host_poly_eval(const uint64_t* coeffs, size_t n, const uint64_t* x, uint64_t* out) {
  Fr acc = Fr::zero(), xx = fr_of(x);
  for (size_t i = n; i-- > 0;) acc = acc * xx + fr_of(coeffs + 4 * i);
  memcpy(out, acc.l, 32);
}
size_t keaki_host_domain(size_t min_size, uint64_t* elements_out /* may be NULL */) {
  auto d = vec::Radix2Domain::create(min_size);
  if (elements_out) { auto e = d.elements(); for (size_t i = 0; i < e.size(); i++) memcpy(elements_out + 4 * i, e[i].l, 32); }
  return d.size;
}
void keaki_host_ifft(const uint64_t* evals, size_t n, size_t domain_min, uint64_t* out) {
  auto d = vec::Radix2Domain::create(domain_min);
  auto c = d.ifft(frs_of(evals, n));
  for (size_t i = 0; i < c.size(); i++) memcpy(out + 4 * i, c[i].l, 32);
}
void keaki_host_fft(const uint64_t* coeffs, size_t n, size_t domain_min, uint64_t* out) {
  auto d = vec::Radix2Domain::create(domain_min);
  auto c = d.fft(frs_of(coeffs, n));
  for (size_t i = 0; i < c.size(); i++) memcpy(out + 4 * i, c[i].l, 32);
}

// ---- Device objects: one GPU, or a list of ordinals = several GPUs of this process behind one object (keaki::Device) ---------------
// A handle is a std::shared_ptr<Device>*: setups created on it keep the device alive after the handle is freed.
int keaki_host_device_new(const int* ordinals, size_t n, void** out) {
  return guard([&] {
    if (n == 1) *out = new std::shared_ptr<Device>(std::make_shared<Device>(ordinals[0]));
    else *out = new std::shared_ptr<Device>(std::make_shared<Device>(std::vector<int>(ordinals, ordinals + n)));
    return 0;
  });
}
void keaki_host_device_free(void* dev) { delete (std::shared_ptr<Device>*)dev; }
size_t keaki_host_device_members(void* dev) { return (*(std::shared_ptr<Device>*)dev)->members(); }
// the keaki_hip_ctx of a member (member 0 for a single-GPU device): for the debug / option / memory calls of the C ABI
void* keaki_host_device_ctx(void* dev, size_t member) {
  auto& d = *(std::shared_ptr<Device>*)dev;
  return d->group() ? (void*)keaki_hip_group_ctx(d->group(), member) : (member == 0 ? (void*)d->ctx() : nullptr);
}
int keaki_host_setup_on(void* dev, const uint64_t* secret, size_t max_d, void** out) {
  return guard([&] {
    auto d = *(std::shared_ptr<Device>*)dev;
    *out = new Setup{d, kzg::KZGSetup::setup(d, fr_of(secret), max_d)};
    return 0;
  });
}
int keaki_host_setup_from_powers_on(void* dev, const uint64_t* g1_aff, size_t n, const uint64_t* tau_g2, void** out) {
  return guard([&] {
    auto d = *(std::shared_ptr<Device>*)dev;
    std::vector<G1> pts(n);
    for (size_t i = 0; i < n; i++) pts[i] = g1_of(g1_aff + 8 * i);
    *out = new Setup{d, kzg::KZGSetup::from_powers(d, std::move(pts), g2_of(tau_g2))};
    return 0;
  });
}

// KZGSetup::setup(secret, max_d)
int keaki_host_setup(int device, const uint64_t* secret, size_t max_d, void** out) {
  return guard([&] {
    auto dev = std::make_shared<Device>(device);
    auto* s = new Setup{dev, kzg::KZGSetup::setup(dev, fr_of(secret), max_d)};
    *out = s; return 0;
  });
}
int keaki_host_setup_from_powers(int device, const uint64_t* g1_aff, size_t n, const uint64_t* tau_g2, void** out) {
  return guard([&] {
    auto dev = std::make_shared<Device>(device);
    std::vector<G1> pts(n);
    for (size_t i = 0; i < n; i++) pts[i] = g1_of(g1_aff + 8 * i);
    *out = new Setup{dev, kzg::KZGSetup::from_powers(dev, std::move(pts), g2_of(tau_g2))};
    return 0;
  });
}
// ---- .ptau ingest (src/kzg/ptau.rs, src/kzg.rs:33-52). Status 2 = SetupFileError: kind / payload in err_out[3], text via last_error.
static int file_err(const ptau::SetupFileError& e, uint64_t* err_out) {
  if (err_out) { err_out[0] = (uint64_t)e.kind; err_out[1] = e.a; err_out[2] = e.b; }
  g_err = e.to_string();
  return 2;
}
// parse only (no GPU): header (modulus bytes up to mod_cap, power, ceremony power), section table, and the point counts; with
// g1_out / g2_out non-null the limbs of sections 2 / 3 are copied out (call once with nulls for the counts)
int keaki_host_ptau_parse(const char* path, uint8_t* modulus_out, size_t mod_cap, uint32_t* mod_len, uint32_t* power, uint32_t* ceremony_power,
                          uint64_t* sections_out /* 11 x (id, size, position) */, size_t* file_len, size_t* n_g1, size_t* n_g2, uint64_t* g1_out,
                          uint64_t* g2_out, uint64_t* err_out) {
  return guard([&] {
    auto data = ptau::load(path);
    if (!data.ok) return file_err(data.error, err_out);
    if (file_len) *file_len = data.value.size();
    auto md = ptau::verify_metadata(data.value);
    if (!md.ok) return file_err(md.error, err_out);
    auto secs = ptau::parse_sections(data.value);
    if (!secs.ok) return file_err(secs.error, err_out);
    if (sections_out) for (size_t i = 0; i < ptau::N_SECTIONS; i++) {
      sections_out[3 * i] = secs.value.sections[i].id; sections_out[3 * i + 1] = secs.value.sections[i].size; sections_out[3 * i + 2] = secs.value.sections[i].position;
    }
    auto hdr = ptau::parse_header(data.value, secs.value);
    if (!hdr.ok) return file_err(hdr.error, err_out);
    if (mod_len) *mod_len = (uint32_t)hdr.value.field_modulus.size();
    if (modulus_out) memcpy(modulus_out, hdr.value.field_modulus.data(), std::min(mod_cap, hdr.value.field_modulus.size()));
    if (power) *power = hdr.value.power;
    if (ceremony_power) *ceremony_power = hdr.value.ceremony_power;
    auto g1 = ptau::parse_tau_g1(data.value, secs.value, hdr.value.power);
    if (!g1.ok) return file_err(g1.error, err_out);
    auto g2 = ptau::parse_tau_g2(data.value, secs.value, hdr.value.power);
    if (!g2.ok) return file_err(g2.error, err_out);
    if (n_g1) *n_g1 = g1.value.size();
    if (n_g2) *n_g2 = g2.value.size();
    if (g1_out) for (size_t i = 0; i < g1.value.size(); i++) memcpy(g1_out + 8 * i, g1.value[i].w.data(), 64);
    if (g2_out) for (size_t i = 0; i < g2.value.size(); i++) memcpy(g2_out + 16 * i, g2.value[i].w.data(), 128);
    return 0;
  });
}
int keaki_host_ptau_section_info(const uint8_t* header12, size_t offset, uint64_t* out3, uint64_t* err_out) {
  return guard([&] {
    auto si = ptau::section_info_from_data(header12, offset);
    if (!si.ok) return file_err(si.error, err_out);
    out3[0] = si.value.id; out3[1] = si.value.size; out3[2] = si.value.position;
    return 0;
  });
}
int keaki_host_ptau_section_index(uint8_t id) { return ptau::section_index(id); }
// KZGSetup::new_from_file
int keaki_host_setup_from_file(int device, const char* path, void** out, uint64_t* err_out) {
  return guard([&] {
    auto dev = std::make_shared<Device>(device);
    auto r = kzg::new_from_file(dev, path);
    if (!r.ok) return file_err(r.error, err_out);
    *out = new Setup{dev, std::move(*r.setup)};
    return 0;
  });
}
// ---- set openings: setups with G2 powers (dev: a Device handle, or NULL for a context of its own on `device`) ----
static std::shared_ptr<Device> dev_of(void* dev, int device) { return dev ? *(std::shared_ptr<Device>*)dev : std::make_shared<Device>(device); }
int keaki_host_setup_with_g2(void* dev, int device, const uint64_t* secret, size_t max_d, size_t max_set, void** out) {
  return guard([&] {
    auto d = dev_of(dev, device);
    *out = new Setup{d, kzg::KZGSetup::setup_with_g2(d, fr_of(secret), max_d, max_set)};
    return 0;
  });
}
int keaki_host_setup_from_powers_g2(void* dev, int device, const uint64_t* g1_aff, size_t n, const uint64_t* g2_pow, size_t n2, void** out) {
  return guard([&] {
    auto d = dev_of(dev, device);
    std::vector<G1> pts(n);
    for (size_t i = 0; i < n; i++) pts[i] = g1_of(g1_aff + 8 * i);
    std::vector<G2> g2s(n2);
    for (size_t i = 0; i < n2; i++) g2s[i] = g2_of(g2_pow + 16 * i);
    *out = new Setup{d, kzg::KZGSetup::from_powers_g2(d, std::move(pts), std::move(g2s))};
    return 0;
  });
}
int keaki_host_setup_from_file_g2(int device, const char* path, void** out, uint64_t* err_out) {
  return guard([&] {
    auto dev = std::make_shared<Device>(device);
    auto r = kzg::new_from_file_g2(dev, path);
    if (!r.ok) return file_err(r.error, err_out);
    *out = new Setup{dev, std::move(*r.setup)};
    return 0;
  });
}
size_t keaki_host_setup_g2_len(void* s) { return ((Setup*)s)->s.g2_pow().size(); }
void keaki_host_setup_g2_all(void* s, uint64_t* out) {
  const auto& v = ((Setup*)s)->s.g2_pow();
  for (size_t i = 0; i < v.size(); i++) memcpy(out + 16 * i, v[i].w.data(), 128);
}
static std::vector<size_t> idx_of(const uint64_t* idx, size_t k) { return std::vector<size_t>(idx, idx + k); }
int keaki_host_open_set(void* s, const uint64_t* coeffs, size_t n, const uint64_t* points, size_t k, uint64_t* out_g1, uint64_t* values_out, uint64_t* err_out) {
  return guard([&] {
    auto r = kzg::open_set(((Setup*)s)->s, frs_of(coeffs, n), frs_of(points, k));
    if (!r.ok) return kzg_err(r.error, err_out);
    memcpy(out_g1, r.value.first.w.data(), 64);
    for (size_t j = 0; j < k; j++) memcpy(values_out + 4 * j, r.value.second[j].l, 32);
    return 0;
  });
}
int keaki_host_verify_set(void* s, const uint64_t* com, const uint64_t* points, const uint64_t* values, size_t k, const uint64_t* proof, int* out_ok) {
  return guard([&] { *out_ok = kzg::verify_set(((Setup*)s)->s, g1_of(com), frs_of(points, k), frs_of(values, k), g1_of(proof)) ? 1 : 0; return 0; });
}
int keaki_host_aggregate_proofs(void* s, const uint64_t* points, const uint64_t* proofs, size_t k, uint64_t* out_g1) {
  return guard([&] {
    std::vector<G1> pr(k);
    for (size_t j = 0; j < k; j++) pr[j] = g1_of(proofs + 8 * j);
    G1 r = kzg::aggregate_proofs(((Setup*)s)->s, frs_of(points, k), pr);
    memcpy(out_g1, r.w.data(), 64);
    return 0;
  });
}
int keaki_host_encapsulate_set(void* rng, void* s, const uint64_t* com, const uint64_t* points, const uint64_t* values, size_t k, size_t msg_len,
                               uint64_t* ct_out, uint8_t* key_out) {
  return guard([&] {
    auto r = kem::encapsulate_set(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), frs_of(points, k), frs_of(values, k), msg_len);
    memcpy(ct_out, r.first.w.data(), 128);
    if (msg_len) memcpy(key_out, r.second.data(), msg_len);
    return 0;
  });
}
int keaki_host_encrypt_set(void* rng, void* s, const uint64_t* com, const uint64_t* points, const uint64_t* values, size_t k, const uint8_t* msg, size_t len,
                           uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    auto c = enc::encrypt_set(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), frs_of(points, k), frs_of(values, k), std::vector<uint8_t>(msg, msg + len));
    memcpy(ct_g2_out, c.first.w.data(), 128);
    if (len) memcpy(ct_msg_out, c.second.data(), len);
    return 0;
  });
}
// FK23 coset openings: out_proofs holds domain_size / l (vec_open_cosets: next power of two >= n, / l) affine points; out_idx holds l indices
int keaki_host_open_fk_cosets(void* s, const uint64_t* coeffs, size_t n, size_t domain_size, size_t l, uint64_t* out_proofs) {
  return guard([&] {
    std::vector<G1> r = kzg::open_fk_cosets(((Setup*)s)->s, frs_of(coeffs, n), domain_size, l);
    for (size_t i = 0; i < r.size(); i++) memcpy(out_proofs + 8 * i, r[i].w.data(), 64);
    return 0;
  });
}
int keaki_host_vec_open_cosets(void* s, const uint64_t* evals, size_t n, size_t l, uint64_t* out_proofs) {
  return guard([&] {
    std::vector<G1> r = vec::vec_open_cosets(((Setup*)s)->s, frs_of(evals, n), l);
    for (size_t i = 0; i < r.size(); i++) memcpy(out_proofs + 8 * i, r[i].w.data(), 64);
    return 0;
  });
}
int keaki_host_vec_coset_indices(size_t domain_size, size_t l, size_t i, uint64_t* out_idx) {
  return guard([&] {
    const std::vector<size_t> r = vec::vec_coset_indices(domain_size, l, i);
    for (size_t t = 0; t < r.size(); t++) out_idx[t] = r[t];
    return 0;
  });
}
int keaki_host_vec_open_subset(void* s, size_t domain_size, const uint64_t* idx, size_t k, const uint64_t* proofs, size_t n_proofs, uint64_t* out_g1) {
  return guard([&] {
    std::vector<G1> pr(n_proofs);
    for (size_t j = 0; j < n_proofs; j++) pr[j] = g1_of(proofs + 8 * j);
    G1 r = vec::vec_open_subset(((Setup*)s)->s, domain_size, idx_of(idx, k), pr);
    memcpy(out_g1, r.w.data(), 64);
    return 0;
  });
}
// coset batch verification (include/keaki_hip.h: keaki_hip_kzg_verify_cosets). n_coms: 1 or n; values: n rows of l; the gammas are drawn from rng
int keaki_host_verify_cosets(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* shifts, size_t l, const uint64_t* values, const uint64_t* proofs,
                             size_t n, int* out_ok) {
  return guard([&] {
    std::vector<G1> c(n_coms), pr(n);
    for (size_t i = 0; i < n_coms; i++) c[i] = g1_of(coms + 8 * i);
    for (size_t i = 0; i < n; i++) pr[i] = g1_of(proofs + 8 * i);
    *out_ok = kzg::verify_cosets(*(Rng*)rng, ((Setup*)s)->s, c, frs_of(shifts, n), l, frs_of(values, n * l), pr) ? 1 : 0;
    return 0;
  });
}
// set batch verification (include/keaki_hip.h: keaki_hip_kzg_verify_sets). Item i has sizes[i] points; points / values (idx / values): the items' rows one
// behind the other (sum of sizes entries); n_coms: 1 or n; the gammas are drawn from rng, one per item
int keaki_host_verify_sets(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* values,
                           const uint64_t* proofs, size_t n, int* out_ok) {
  return guard([&] {
    std::vector<G1> c(n_coms), pr(n);
    std::vector<std::vector<Fr>> z(n), y(n);
    for (size_t i = 0; i < n_coms; i++) c[i] = g1_of(coms + 8 * i);
    for (size_t i = 0, at = 0; i < n; at += sizes[i], i++) {
      pr[i] = g1_of(proofs + 8 * i);
      z[i] = frs_of(points + 4 * at, sizes[i]);
      y[i] = frs_of(values + 4 * at, sizes[i]);
    }
    *out_ok = kzg::verify_sets(*(Rng*)rng, ((Setup*)s)->s, c, z, y, pr) ? 1 : 0;
    return 0;
  });
}
// the per-item side (include/keaki_hip.h: keaki_hip_kzg_set_pairs, keaki_hip_kzg_verify_sets_each); arrays as keaki_host_verify_sets. status_out: n bytes, 0 = valid;
// a_out n x 8 words, z2_out n x 16 words; msgs n x msg_len; ct_g2_out n x 16 words, bodies n x msg_len
namespace {
struct SetRows { std::vector<G1> c; std::vector<std::vector<Fr>> z, y; std::vector<std::vector<size_t>> rows; };
SetRows set_rows(const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* idx, const uint64_t* values, size_t n) {
  SetRows r;
  r.c.resize(n_coms); r.z.resize(n); r.y.resize(n); r.rows.resize(n);
  for (size_t i = 0; i < n_coms; i++) r.c[i] = g1_of(coms + 8 * i);
  for (size_t i = 0, at = 0; i < n; at += sizes[i], i++) {
    if (points) r.z[i] = frs_of(points + 4 * at, sizes[i]);
    if (idx) r.rows[i] = idx_of(idx + at, sizes[i]);
    r.y[i] = frs_of(values + 4 * at, sizes[i]);
  }
  return r;
}
std::vector<G1> g1s_of(const uint64_t* p, size_t n) {
  std::vector<G1> v(n);
  for (size_t i = 0; i < n; i++) v[i] = g1_of(p + 8 * i);
  return v;
}
}  // namespace
int keaki_host_set_pairs(void* s, const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* values, size_t n, uint64_t* a_out,
                         uint64_t* z2_out) {
  return guard([&] {
    const SetRows r = set_rows(coms, n_coms, sizes, points, nullptr, values, n);
    kzg::set_pairs(((Setup*)s)->s, r.c, r.z, r.y, a_out, z2_out);
    return 0;
  });
}
int keaki_host_verify_sets_each(void* s, const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* values, const uint64_t* proofs,
                                size_t n, uint8_t* status_out) {
  return guard([&] {
    const SetRows r = set_rows(coms, n_coms, sizes, points, nullptr, values, n);
    const std::vector<uint8_t> st = kzg::verify_sets_each(((Setup*)s)->s, r.c, r.z, r.y, g1s_of(proofs, n));
    if (n) memcpy(status_out, st.data(), n);
    return 0;
  });
}
int keaki_host_vec_verify_subsets_each(void* s, const uint64_t* com, size_t domain_size, const uint64_t* sizes, const uint64_t* idx, const uint64_t* values,
                                       const uint64_t* proofs, size_t n, uint8_t* status_out) {
  return guard([&] {
    const SetRows r = set_rows(com, 1, sizes, nullptr, idx, values, n);
    const std::vector<uint8_t> st = vec::vec_verify_subsets_each(((Setup*)s)->s, r.c[0], domain_size, r.rows, r.y, g1s_of(proofs, n));
    if (n) memcpy(status_out, st.data(), n);
    return 0;
  });
}
int keaki_host_encapsulate_sets(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* values, size_t n,
                                size_t msg_len, uint64_t* ct_g2_out, uint8_t* keys_out) {
  return guard([&] {
    const SetRows r = set_rows(coms, n_coms, sizes, points, nullptr, values, n);
    const auto kc = kem::encapsulate_sets(*(Rng*)rng, ((Setup*)s)->s, r.c, r.z, r.y, msg_len);
    for (size_t i = 0; i < n; i++) {
      memcpy(ct_g2_out + 16 * i, kc[i].first.w.data(), 128);
      if (msg_len) memcpy(keys_out + i * msg_len, kc[i].second.data(), msg_len);
    }
    return 0;
  });
}
int keaki_host_encrypt_sets(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* sizes, const uint64_t* points, const uint64_t* values, size_t n,
                            const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    const SetRows r = set_rows(coms, n_coms, sizes, points, nullptr, values, n);
    std::vector<std::vector<uint8_t>> m(n);
    for (size_t i = 0; i < n; i++) m[i].assign(msgs + i * msg_len, msgs + (i + 1) * msg_len);
    const auto cts = enc::encrypt_sets(*(Rng*)rng, ((Setup*)s)->s, r.c, r.z, r.y, m);
    for (size_t i = 0; i < n; i++) {
      memcpy(ct_g2_out + 16 * i, cts[i].first.w.data(), 128);
      if (msg_len) memcpy(ct_msg_out + i * msg_len, cts[i].second.data(), msg_len);
    }
    return 0;
  });
}
int keaki_host_vec_encrypt_subsets(void* rng, void* s, const uint64_t* com, size_t domain_size, const uint64_t* sizes, const uint64_t* idx, const uint64_t* values, size_t n,
                                   const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    const SetRows r = set_rows(com, 1, sizes, nullptr, idx, values, n);
    vec::vec_encrypt_subsets(*(Rng*)rng, ((Setup*)s)->s, r.c[0], domain_size, r.rows, r.y, msgs, msg_len, ct_g2_out, ct_msg_out);
    return 0;
  });
}
int keaki_host_vec_verify_subsets(void* rng, void* s, const uint64_t* com, size_t domain_size, const uint64_t* sizes, const uint64_t* idx, const uint64_t* values,
                                  const uint64_t* proofs, size_t n, int* out_ok) {
  return guard([&] {
    std::vector<G1> pr(n);
    std::vector<std::vector<size_t>> rows(n);
    std::vector<std::vector<Fr>> y(n);
    for (size_t i = 0, at = 0; i < n; at += sizes[i], i++) {
      pr[i] = g1_of(proofs + 8 * i);
      rows[i] = idx_of(idx + at, sizes[i]);
      y[i] = frs_of(values + 4 * at, sizes[i]);
    }
    *out_ok = vec::vec_verify_subsets(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), domain_size, rows, y, pr) ? 1 : 0;
    return 0;
  });
}
// all cosets of a vector: evals n <= domain Fr (zero-padded to the next power of two d), proofs d / l affine points
int keaki_host_vec_verify_cosets(void* rng, void* s, const uint64_t* com, const uint64_t* evals, size_t n, size_t l, const uint64_t* proofs, size_t n_proofs,
                                 int* out_ok) {
  return guard([&] {
    std::vector<G1> pr(n_proofs);
    for (size_t i = 0; i < n_proofs; i++) pr[i] = g1_of(proofs + 8 * i);
    *out_ok = vec::vec_verify_cosets(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), frs_of(evals, n), l, pr) ? 1 : 0;
    return 0;
  });
}
int keaki_host_vec_verify_cosets_subset(void* rng, void* s, const uint64_t* com, size_t domain_size, size_t l, const uint64_t* cosets, size_t k, const uint64_t* values,
                                        const uint64_t* proofs, int* out_ok) {
  return guard([&] {
    std::vector<G1> pr(k);
    for (size_t i = 0; i < k; i++) pr[i] = g1_of(proofs + 8 * i);
    *out_ok = vec::vec_verify_cosets_subset(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), domain_size, l, idx_of(cosets, k), frs_of(values, k * l), pr) ? 1 : 0;
    return 0;
  });
}
// one verdict per coset (include/keaki_hip.h: keaki_hip_kzg_verify_cosets_each): status_out d / l (or k) bytes, 0 = valid
int keaki_host_vec_verify_cosets_each(void* s, const uint64_t* com, const uint64_t* evals, size_t n, size_t l, const uint64_t* proofs, size_t n_proofs,
                                      uint8_t* status_out) {
  return guard([&] {
    std::vector<G1> pr(n_proofs);
    for (size_t i = 0; i < n_proofs; i++) pr[i] = g1_of(proofs + 8 * i);
    const std::vector<uint8_t> st = vec::vec_verify_cosets_each(((Setup*)s)->s, g1_of(com), frs_of(evals, n), l, pr);
    memcpy(status_out, st.data(), st.size());
    return 0;
  });
}
int keaki_host_vec_verify_cosets_each_subset(void* s, const uint64_t* com, size_t domain_size, size_t l, const uint64_t* cosets, size_t k, const uint64_t* values,
                                             const uint64_t* proofs, uint8_t* status_out) {
  return guard([&] {
    std::vector<G1> pr(k);
    for (size_t i = 0; i < k; i++) pr[i] = g1_of(proofs + 8 * i);
    const std::vector<uint8_t> st = vec::vec_verify_cosets_each_subset(((Setup*)s)->s, g1_of(com), domain_size, l, idx_of(cosets, k), frs_of(values, k * l), pr);
    memcpy(status_out, st.data(), st.size());
    return 0;
  });
}
// message k to the l claimed values of coset cosets[k]: values k rows of l, msgs k x msg_len
int keaki_host_vec_encrypt_cosets(void* rng, void* s, const uint64_t* com, size_t domain_size, size_t l, const uint64_t* cosets, size_t k, const uint64_t* values,
                                  const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    const std::vector<Fr> v = frs_of(values, k * l);
    vec::vec_encrypt_cosets(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), domain_size, l, idx_of(cosets, k), v.data(), msgs, msg_len, ct_g2_out, ct_msg_out);
    return 0;
  });
}
int keaki_host_vec_verify_subset(void* s, const uint64_t* com, size_t domain_size, const uint64_t* idx, const uint64_t* values, size_t k, const uint64_t* proof,
                                 int* out_ok) {
  return guard([&] {
    *out_ok = vec::vec_verify_subset(((Setup*)s)->s, g1_of(com), domain_size, idx_of(idx, k), frs_of(values, k), g1_of(proof)) ? 1 : 0;
    return 0;
  });
}
int keaki_host_vec_encrypt_subset_batch(void* rng, void* s, const uint64_t* com, size_t domain_size, const uint64_t* idx, size_t k, const uint64_t* values, size_t n,
                                        const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    const std::vector<Fr> v = frs_of(values, n * k);
    vec::vec_encrypt_subset_batch(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), domain_size, idx_of(idx, k), v.data(), n, msgs, msg_len, ct_g2_out, ct_msg_out);
    return 0;
  });
}
void keaki_host_setup_free(void* s) { delete (Setup*)s; }
size_t keaki_host_setup_len(void* s) { return ((Setup*)s)->s.g1_pow().size(); }
void keaki_host_setup_g1_pow(void* s, size_t i, uint64_t* out) { memcpy(out, ((Setup*)s)->s.g1_pow()[i].w.data(), 64); }
void keaki_host_setup_g1_all(void* s, uint64_t* out) {   // all of g1_pow at once: len x 8 words
  const auto& v = ((Setup*)s)->s.g1_pow();
  for (size_t i = 0; i < v.size(); i++) memcpy(out + 8 * i, v[i].w.data(), 64);
}
void keaki_host_setup_tau_g2(void* s, uint64_t* out) { memcpy(out, ((Setup*)s)->s.tau_g2().w.data(), 128); }

int keaki_host_commit(void* s, const uint64_t* coeffs, size_t n, uint64_t* out_g1, uint64_t* err_out) {
  return guard([&] {
    auto r = kzg::commit(((Setup*)s)->s, frs_of(coeffs, n));
    if (!r.ok) return kzg_err(r.error, err_out);
    memcpy(out_g1, r.value.w.data(), 64); return 0;
  });
}
int keaki_host_open(void* s, const uint64_t* coeffs, size_t n, const uint64_t* point, uint64_t* out_g1, uint64_t* err_out) {
  return guard([&] {
    auto r = kzg::open(((Setup*)s)->s, frs_of(coeffs, n), fr_of(point));
    if (!r.ok) return kzg_err(r.error, err_out);
    memcpy(out_g1, r.value.w.data(), 64); return 0;
  });
}
// m rows of n coefficients at coeffs + 4 * stride * j words (zero-padded rows: trailing zeros are not part of a polynomial); out_g1: m affine points
static std::vector<DensePolynomial> rows_of(const uint64_t* coeffs, size_t n, size_t m, size_t stride) {
  std::vector<DensePolynomial> polys(m);
  for (size_t j = 0; j < m; j++) polys[j] = frs_of(coeffs + 4 * stride * j, n);
  return polys;
}
int keaki_host_commit_batch(void* s, const uint64_t* coeffs, size_t n, size_t m, size_t stride, uint64_t* out_g1, uint64_t* err_out) {
  return guard([&] {
    auto r = kzg::commit_batch(((Setup*)s)->s, rows_of(coeffs, n, m, stride));
    if (!r.ok) return kzg_err(r.error, err_out);
    for (size_t j = 0; j < m; j++) memcpy(out_g1 + 8 * j, r.value[j].w.data(), 64);
    return 0;
  });
}
int keaki_host_open_batch(void* s, const uint64_t* coeffs, size_t n, size_t m, size_t stride, const uint64_t* points, uint64_t* out_g1, uint64_t* err_out) {
  return guard([&] {
    std::vector<Fr> z(m);
    for (size_t j = 0; j < m; j++) z[j] = fr_of(points + 4 * j);
    auto r = kzg::open_batch(((Setup*)s)->s, rows_of(coeffs, n, m, stride), z);
    if (!r.ok) return kzg_err(r.error, err_out);
    for (size_t j = 0; j < m; j++) memcpy(out_g1 + 8 * j, r.value[j].w.data(), 64);
    return 0;
  });
}
int keaki_host_commit_batch_min(void) { return (int)kzg::COMMIT_BATCH_MIN; }
int keaki_host_verify(void* s, const uint64_t* com, const uint64_t* point, const uint64_t* value, const uint64_t* proof, int* out_ok) {
  return guard([&] {
    auto r = kzg::verify(((Setup*)s)->s, g1_of(com), fr_of(point), fr_of(value), g1_of(proof));
    *out_ok = r.value ? 1 : 0; return 0;
  });
}
// n_coms: 1 or n; point_mode 1: `points` is ONE Fr omega, item i is opened at omega^i
int keaki_host_verify_batch(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* points, int point_mode, const uint64_t* values,
                            const uint64_t* proofs, size_t n, int* out_ok) {
  return guard([&] {
    static_assert(sizeof(Fr) == 32, "Fr is four u64 limbs");
    *out_ok = kzg::verify_batch_flat(*(Rng*)rng, ((Setup*)s)->s, coms, n_coms, reinterpret_cast<const Fr*>(points), point_mode != 0,
                                     reinterpret_cast<const Fr*>(values), proofs, n) ? 1 : 0;
    return 0;
  });
}
// one verdict per item: status_out[i] = 0 valid / 1 invalid, *out_bad = the number of ones
int keaki_host_verify_each(void* s, const uint64_t* coms, size_t n_coms, const uint64_t* points, int point_mode, const uint64_t* values, const uint64_t* proofs,
                           size_t n, uint8_t* status_out, uint64_t* out_bad) {
  return guard([&] {
    *out_bad = kzg::verify_each_flat(((Setup*)s)->s, coms, n_coms, reinterpret_cast<const Fr*>(points), point_mode != 0, reinterpret_cast<const Fr*>(values), proofs,
                                     n, status_out);
    return 0;
  });
}
// verify_batch, then verify_each if it rejects: idx_out (room for n) receives the invalid indices, *out_count how many
int keaki_host_locate_invalid(void* rng, void* s, const uint64_t* coms, size_t n_coms, const uint64_t* points, int point_mode, const uint64_t* values,
                              const uint64_t* proofs, size_t n, uint64_t* idx_out, uint64_t* out_count) {
  return guard([&] {
    const std::vector<size_t> bad = kzg::locate_invalid_flat(*(Rng*)rng, ((Setup*)s)->s, coms, n_coms, reinterpret_cast<const Fr*>(points), point_mode != 0,
                                                             reinterpret_cast<const Fr*>(values), proofs, n);
    for (size_t i = 0; i < bad.size(); i++) idx_out[i] = bad[i];
    *out_count = bad.size();
    return 0;
  });
}
int keaki_host_vec_verify_each(void* s, const uint64_t* com, const uint64_t* v, size_t n, const uint64_t* proofs, uint8_t* status_out, uint64_t* out_bad) {
  return guard([&] {
    *out_bad = vec::vec_verify_each_flat(((Setup*)s)->s, g1_of(com), reinterpret_cast<const Fr*>(v), n, proofs, status_out);
    return 0;
  });
}
int keaki_host_vec_verify(void* rng, void* s, const uint64_t* com, const uint64_t* v, size_t n, const uint64_t* proofs, int* out_ok) {
  return guard([&] {
    *out_ok = vec::vec_verify_flat(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), reinterpret_cast<const Fr*>(v), n, proofs) ? 1 : 0;
    return 0;
  });
}
// the wire format (compressed points). Return 2: bytes that do not decode; bad_out[0] = index of the first rejected item, bad_out[1] = reason
// (1 malformed, 2 not on the curve, 3 outside the subgroup)
int keaki_host_proofs_to_bytes(void* s, const uint64_t* proofs, size_t n, uint8_t* wire_out) {
  return guard([&] { kzg::proofs_to_bytes_flat(((Setup*)s)->s, proofs, n, wire_out); return 0; });
}
int keaki_host_proofs_from_bytes(void* s, const uint8_t* wire, size_t n, uint64_t* proofs_out, uint64_t* bad_out) {
  return wire_guard(bad_out, [&] { kzg::proofs_from_bytes_flat(((Setup*)s)->s, wire, n, proofs_out); });
}
int keaki_host_ciphertexts_to_bytes(void* s, const uint64_t* ct_g2, const uint8_t* bodies, size_t n, size_t msg_len, uint8_t* wire_out) {
  return guard([&] { enc::ciphertexts_to_bytes_flat(((Setup*)s)->s, ct_g2, bodies, n, msg_len, wire_out); return 0; });
}
int keaki_host_ciphertexts_from_bytes(void* s, const uint8_t* wire, size_t n, size_t msg_len, uint64_t* ct_g2_out, uint8_t* bodies_out, uint64_t* bad_out) {
  return wire_guard(bad_out, [&] { enc::ciphertexts_from_bytes_flat(((Setup*)s)->s, wire, n, msg_len, ct_g2_out, bodies_out); });
}
int keaki_host_precompute_open_fk(void* s, size_t domain_size) {
  return guard([&] { kzg::precompute_open_fk(((Setup*)s)->s, domain_size); return 0; });
}
int keaki_host_open_fk(void* s, const uint64_t* coeffs, size_t n, size_t domain_size, uint64_t* out_g1s, uint64_t* err_out) {
  return guard([&] {
    auto r = kzg::open_fk(((Setup*)s)->s, frs_of(coeffs, n), domain_size);
    if (!r.ok) return kzg_err(r.error, err_out);
    for (size_t i = 0; i < r.value.size(); i++) memcpy(out_g1s + 8 * i, r.value[i].w.data(), 64);
    return 0;
  });
}
int keaki_host_encapsulate(void* rng, void* s, const uint64_t* com, const uint64_t* point, const uint64_t* value, size_t msg_len,
                           uint64_t* ct_out, uint8_t* key_out) {
  return guard([&] {
    auto r = kem::encapsulate(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), fr_of(point), fr_of(value), msg_len);
    memcpy(ct_out, r.first.w.data(), 128);
    if (msg_len) memcpy(key_out, r.second.data(), msg_len);
    return 0;
  });
}
int keaki_host_kem_prepare(void* s, size_t batch_hint) {
  return guard([&] { kem::prepare(((Setup*)s)->s, batch_hint); return 0; });
}
int keaki_host_decapsulate(void* s, const uint64_t* proof, const uint64_t* ct, size_t msg_len, uint8_t* key_out) {
  return guard([&] {
    auto k = kem::decapsulate(((Setup*)s)->s, g1_of(proof), g2_of(ct), msg_len);
    if (msg_len) memcpy(key_out, k.data(), msg_len);
    return 0;
  });
}
int keaki_host_encrypt(void* rng, void* s, const uint64_t* com, const uint64_t* point, const uint64_t* value, const uint8_t* msg, size_t len,
                       uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    auto c = enc::encrypt(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), fr_of(point), fr_of(value), std::vector<uint8_t>(msg, msg + len));
    memcpy(ct_g2_out, c.first.w.data(), 128);
    if (len) memcpy(ct_msg_out, c.second.data(), len);
    return 0;
  });
}
int keaki_host_decrypt(void* s, const uint64_t* proof, const uint64_t* ct_g2, const uint8_t* ct_msg, size_t len, uint8_t* msg_out) {
  return guard([&] {
    enc::Ciphertext c{g2_of(ct_g2), std::vector<uint8_t>(ct_msg, ct_msg + len)};
    auto m = enc::decrypt(((Setup*)s)->s, g1_of(proof), c);
    if (len) memcpy(msg_out, m.data(), len);
    return 0;
  });
}
// vec_commit: v has n scalars; outputs commitment and `domain_size` proofs (caller sizes proofs_out with keaki_host_domain(n+1))
int keaki_host_vec_commit(void* rng, void* s, const uint64_t* v, size_t n, uint64_t* com_out, uint64_t* proofs_out) {
  return guard([&] {
    static_assert(sizeof(Fr) == 32, "Fr is four u64 limbs");
    G1 com = vec::vec_commit_flat(*(Rng*)rng, ((Setup*)s)->s, reinterpret_cast<const Fr*>(v), n, proofs_out);      // straight into the caller's array
    memcpy(com_out, com.w.data(), 64);
    return 0;
  });
}
// vec_commit_batch: m vectors of `lens[j]` scalars, concatenated in v; com_out: m x 8 words, proofs_out: m x keaki_host_domain(longest + 1) x 8 words
int keaki_host_vec_commit_batch(void* rng, void* s, const uint64_t* v, const size_t* lens, size_t m, uint64_t* com_out, uint64_t* proofs_out) {
  return guard([&] {
    std::vector<std::vector<Fr>> vecs(m);
    size_t at = 0;
    for (size_t j = 0; j < m; at += lens[j], j++) vecs[j] = frs_of(v + 4 * at, lens[j]);
    auto r = vec::vec_commit_batch(*(Rng*)rng, ((Setup*)s)->s, vecs);
    for (size_t j = 0; j < m; j++) {
      memcpy(com_out + 8 * j, r[j].first.w.data(), 64);
      const size_t d = r[j].second.size();
      if (d) memcpy(proofs_out + 8 * d * j, r[j].second[0].w.data(), 64 * d);
    }
    return 0;
  });
}
// vec_update: positions idx[t] (t < k) of a committed vector go from old_values[t] to new_values[t]; com (8 words) and proofs (domain_size x 8 words) in place
int keaki_host_vec_update(void* s, const uint64_t* idx, const uint64_t* old_values, const uint64_t* new_values, size_t k, size_t domain_size, uint64_t* com_inout,
                          uint64_t* proofs_inout) {
  return guard([&] {
    G1 com = g1_of(com_inout);
    std::vector<G1> proofs(domain_size);
    if (domain_size) memcpy(proofs[0].w.data(), proofs_inout, 64 * domain_size);
    vec::vec_update(((Setup*)s)->s, com, proofs, std::vector<size_t>(idx, idx + k), frs_of(old_values, k), frs_of(new_values, k));
    memcpy(com_inout, com.w.data(), 64);
    if (domain_size) memcpy(proofs_inout, proofs[0].w.data(), 64 * domain_size);
    return 0;
  });
}
// the same from the differences, on the caller's arrays (either of com / proofs may be null)
int keaki_host_vec_update_flat(void* s, size_t domain_size, const uint32_t* idx, const uint64_t* deltas, size_t k, uint64_t* com_inout, uint64_t* proofs_inout) {
  return guard([&] {
    static_assert(sizeof(Fr) == 32, "Fr is four u64 limbs");
    vec::vec_update_flat(((Setup*)s)->s, domain_size, idx, reinterpret_cast<const Fr*>(deltas), k, com_inout, proofs_inout);
    return 0;
  });
}
int keaki_host_precompute_vec_update(void* s, size_t domain_size) {
  return guard([&] { vec::precompute_vec_update(((Setup*)s)->s, domain_size); return 0; });
}
// vec_encrypt with equal-length messages (msg_len each, concatenated)
int keaki_host_vec_encrypt(void* rng, void* s, const uint64_t* com, const uint64_t* points, const uint64_t* values, const uint8_t* msgs,
                           size_t n, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    static_assert(sizeof(Fr) == 32, "Fr is four u64 limbs");
    vec::vec_encrypt_flat(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), reinterpret_cast<const Fr*>(points), reinterpret_cast<const Fr*>(values), msgs, n, msg_len,
                          ct_g2_out, ct_msg_out);
    return 0;
  });
}
// vec_encrypt_batch: m commitments (m x 8 words), counts[j] items each, item-major arrays over all n = sum(counts) items
int keaki_host_vec_encrypt_batch(void* rng, void* s, const uint64_t* coms, const size_t* counts, size_t m, const uint64_t* points, const uint64_t* values,
                                 const uint8_t* msgs, size_t msg_len, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    std::vector<G1> cs(m);
    for (size_t j = 0; j < m; j++) cs[j] = g1_of(coms + 8 * j);
    vec::vec_encrypt_batch(*(Rng*)rng, ((Setup*)s)->s, cs.data(), counts, m, reinterpret_cast<const Fr*>(points), reinterpret_cast<const Fr*>(values), msgs,
                           msg_len, ct_g2_out, ct_msg_out);
    return 0;
  });
}
int keaki_host_vec_decrypt(void* s, const uint64_t* proofs, const uint64_t* ct_g2, const uint8_t* ct_msgs, size_t n, size_t msg_len,
                           uint8_t* msgs_out) {
  return guard([&] {
    vec::vec_decrypt_flat(((Setup*)s)->s, proofs, ct_g2, ct_msgs, n, msg_len, msgs_out);
    return 0;
  });
}

// ---- keaki::dist: one process per GPU (rank / world), the exchange of the 96-byte partials is the caller's ------------------------
int keaki_host_prepare_shard(void* s, size_t rank, size_t world) {
  return guard([&] { dist::prepare(((Setup*)s)->s, dist::Shard{rank, world}); return 0; });
}
int keaki_host_setup_has_tables(void* s) { return ((Setup*)s)->s.has_window_tables() ? 1 : 0; }
int keaki_host_commit_partial(void* s, const uint64_t* coeffs, size_t n, size_t rank, size_t world, uint64_t* out_jac12, uint64_t* err_out) {
  return guard([&] {
    auto r = dist::commit_partial(((Setup*)s)->s, frs_of(coeffs, n), dist::Shard{rank, world});
    if (!r.ok) return kzg_err(r.error, err_out);
    memcpy(out_jac12, r.value.data(), 96); return 0;
  });
}
// vec_commit with the commit left as this rank's partial; proofs_out sized with keaki_host_domain(n + 1)
int keaki_host_vec_commit_partial(void* rng, void* s, const uint64_t* v, size_t n, size_t rank, size_t world, uint64_t* out_jac12, uint64_t* proofs_out) {
  return guard([&] {
    auto r = dist::vec_commit_partial(*(Rng*)rng, ((Setup*)s)->s, frs_of(v, n), dist::Shard{rank, world});
    memcpy(out_jac12, r.first.data(), 96);
    for (size_t i = 0; i < r.second.size(); i++) memcpy(proofs_out + 8 * i, r.second[i].w.data(), 64);
    return 0;
  });
}
// ---- open_fk sharded (dist::ShardedOpenFk): the two callbacks are the caller's collectives over device memory
typedef int (*keaki_host_a2a_fn)(void* user, void* d_send, void* d_recv, size_t bytes_per_peer);
int keaki_host_fk_shard_can(void* s, size_t domain_size, size_t rank, size_t world) {
  return dist::ShardedOpenFk::can_shard(((Setup*)s)->s, domain_size, dist::Shard{rank, world}) ? 1 : 0;
}
int keaki_host_fk_shard_new(void* s, size_t domain_size, size_t rank, size_t world, void** out) {
  return guard([&] { *out = new dist::ShardedOpenFk(((Setup*)s)->s, domain_size, dist::Shard{rank, world}); return 0; });
}
void keaki_host_fk_shard_free(void* fk) { delete (dist::ShardedOpenFk*)fk; }
size_t keaki_host_fk_shard_buffer_bytes(void* fk) { return ((dist::ShardedOpenFk*)fk)->buffer_bytes(); }
int keaki_host_fk_shard_prepare(void* fk, void* d_send, void* d_recv, keaki_host_a2a_fn all_to_all, keaki_host_a2a_fn all_gather, void* user) {
  return guard([&] { ((dist::ShardedOpenFk*)fk)->prepare(d_send, d_recv, dist::FkExchange{all_to_all, all_gather, user}); return 0; });
}
int keaki_host_fk_shard_open(void* fk, const uint64_t* coeffs, size_t n, void* d_send, void* d_recv, keaki_host_a2a_fn all_to_all,
                             keaki_host_a2a_fn all_gather, void* user, uint64_t* out_g1s) {
  return guard([&] {
    auto r = ((dist::ShardedOpenFk*)fk)->open(frs_of(coeffs, n), d_send, d_recv, dist::FkExchange{all_to_all, all_gather, user});
    for (size_t i = 0; i < r.size(); i++) memcpy(out_g1s + 8 * i, r[i].w.data(), 64);
    return 0;
  });
}
int keaki_host_vec_commit_partial_fk(void* rng, void* s, const uint64_t* v, size_t n, size_t rank, size_t world, void* fk, void* d_send, void* d_recv,
                                     keaki_host_a2a_fn all_to_all, keaki_host_a2a_fn all_gather, void* user, uint64_t* out_jac12, uint64_t* proofs_out) {
  return guard([&] {
    auto r = dist::vec_commit_partial_fk(*(Rng*)rng, ((Setup*)s)->s, frs_of(v, n), dist::Shard{rank, world}, *(dist::ShardedOpenFk*)fk, d_send, d_recv,
                                         dist::FkExchange{all_to_all, all_gather, user});
    memcpy(out_jac12, r.first.data(), 96);
    for (size_t i = 0; i < r.second.size(); i++) memcpy(proofs_out + 8 * i, r.second[i].w.data(), 64);
    return 0;
  });
}
int keaki_host_commit_combine(void* s, const uint64_t* partials_jac12, size_t world, uint64_t* out_g1) {
  return guard([&] {
    static_assert(sizeof(dist::Partial) == 96, "a partial is twelve u64 words");
    G1 g = dist::commit_combine(((Setup*)s)->s, reinterpret_cast<const dist::Partial*>(partials_jac12), world);
    memcpy(out_g1, g.w.data(), 64); return 0;
  });
}
// vec_encrypt for the items of rank `rank` only (outputs sized for that rank's hi - lo items)
int keaki_host_vec_encrypt_shard(void* rng, void* s, const uint64_t* com, const uint64_t* points, const uint64_t* values, const uint8_t* msgs,
                                 size_t n, size_t msg_len, size_t rank, size_t world, uint64_t* ct_g2_out, uint8_t* ct_msg_out) {
  return guard([&] {
    dist::vec_encrypt_flat_shard(*(Rng*)rng, ((Setup*)s)->s, g1_of(com), reinterpret_cast<const Fr*>(points), reinterpret_cast<const Fr*>(values), msgs, n,
                                 msg_len, dist::Shard{rank, world}, ct_g2_out, ct_msg_out);
    return 0;
  });
}

}  // extern "C"
