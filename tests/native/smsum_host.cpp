// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// CPU restatement of kernels/k_smsg.hip's k_smsum and of the host-side plan of a
// same-message call: the identical bodies (bls/smsum.hpp, bls/plan.hpp
// plan_same_message / check_same_message) compiled for the host, the kernel's wavefront
// replaced by a loop over the 64 lanes of every step.  For job sizes at the lane-stride
// and wavefront-tail edges, with some sets not live, the tree's two sums must equal a
// plain left-to-right sum after conversion to affine, and smsum_finish must leave the
// unit and the virtual set k_uset / vset_write would.  A stand-alone program (its own
// main), so it also runs under -fsanitize=address,undefined.
//
//   smsum_host            prints "ok <checks>" and exits 0, or the first mismatch and 1
#include <stdio.h>
#include <string.h>

#include <vector>

#define BLS_LAZY_POW 1
#include "bls/plan.hpp"
#include "bls/smsum.hpp"

unsigned long long bls_fpm_counter = 0;
unsigned long long bls_lz_norm_counter = 0;

using namespace bls;

static int g_checks = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    ++g_checks;                          \
    if (!(cond)) {                       \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
      return 1;                          \
    }                                    \
  } while (0)

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <class F>
static bool aff_eq(const Aff<F>& a, const Aff<F>& b) {
  if (a.inf || b.inf) return a.inf && b.inf;
  return f_eq(a.x, b.x) && f_eq(a.y, b.y);
}

static const uint32_t LANES = 64;

static int run_jobs(const std::vector<uint32_t>& sizes, uint64_t seed, bool cancel_first_job) {
  // the call: jobs back to back, every set a one-set request
  uint32_t n = 0;
  std::vector<uint32_t> off(1, 0);
  for (uint32_t s : sizes) off.push_back(n += s);
  std::vector<uint8_t> roots(32 * sizes.size(), 0x5a), sigs(96 * (size_t)n, 0);
  std::vector<uint32_t> idx(n, 0);
  std::vector<int32_t> verdicts(n, 0);
  bls_same_msg_batch in;
  memset(&in, 0, sizeof(in));
  in.n_jobs = (uint32_t)sizes.size();
  in.n_sets = n;
  in.job_set_offsets = off.data();
  in.messages = roots.data();
  in.pk_indices = idx.data();
  in.signatures = sigs.data();
  CHECK(check_same_message(&in, verdicts.data()) == nullptr, "shape check refused a good batch");
  SameMsgPlan sm;
  plan_same_message(&in, sm);
  const BatchPlan& plan = sm.plan;
  uint32_t batched = 0, singles = 0;
  for (uint32_t s : sizes) (s == 1 ? singles : batched) += 1;
  const uint32_t C = (uint32_t)plan.chunk_off.size() - 1;
  CHECK(C == batched && plan.nonbatch_reqs.size() == singles, "plan: %u chunks, %zu alone", C,
        plan.nonbatch_reqs.size());
  for (uint32_t c = 0, j = 0; c < C; ++c, ++j) {
    while (sizes[j] == 1) ++j;
    CHECK(plan.chunk_off[c + 1] - plan.chunk_off[c] == sizes[j], "chunk %u is not job %u", c, j);
    for (uint32_t k = plan.chunk_off[c]; k < plan.chunk_off[c + 1]; ++k)
      CHECK(plan.chunk_reqs[k] == off[j] + (k - plan.chunk_off[c]), "chunk %u request %u", c, k);
  }

  // chain entries: RP = [a] g1, RS = [b] g2 per set, ~1 set in 5 not live
  const uint32_t unit_base = n + C, n_total = unit_base + C;
  std::vector<Fp> chain((size_t)CHAIN_WORDS * n_total);
  std::vector<uint32_t> live(n_total, 0);
  std::vector<Fp12> f(n_total);
  G1A g1;
  g1.x = c_g1_x();
  g1.y = c_g1_y();
  g1.inf = false;
  G2A g2;
  g2.x = c_g2_x();
  g2.y = c_g2_y();
  g2.inf = false;
  std::vector<G1J> rp(n);
  std::vector<G2J> rs(n);
  uint64_t st = seed;
  for (uint32_t i = 0; i < n; ++i) {
    rp[i] = aff_mul_u64(g1, splitmix(st) >> 40);  // 24-bit scalars: short chains, distinct points
    rs[i] = aff_mul_u64(g2, splitmix(st) >> 40);
    live[i] = splitmix(st) % 5 != 0;
  }
  if (cancel_first_job && C > 0 && plan.chunk_off[1] >= 2) {
    // the first batched job: P, -P and nothing else live -> both sums are the point at infinity
    for (uint32_t k = plan.chunk_off[0]; k < plan.chunk_off[1]; ++k) live[plan.chunk_reqs[k]] = 0;
    const uint32_t a = plan.chunk_reqs[plan.chunk_off[0]], b = plan.chunk_reqs[plan.chunk_off[1] - 1];
    rp[b] = jac_neg(rp[a]);
    rs[b] = jac_neg(rs[a]);
    live[a] = live[b] = 1;
  }
  for (uint32_t i = 0; i < n; ++i) {
    Fp* o = chain.data() + (size_t)CHAIN_WORDS * i;
    for (int k = 0; k < 4; ++k) o[CH_HQ + k] = fp_add(c_one(), rp[i].x);  // a marker for the HQ copy
    memcpy(o + CH_RP, &rp[i], sizeof(G1J));
    memcpy(o + CH_RS, &rs[i], sizeof(G2J));
  }
  PipeBufs b;
  memset(&b, 0, sizeof(b));
  b.n_sets = n;
  b.n_chunks = C;
  b.n_units = C;
  b.unit_base = unit_base;
  b.chain = chain.data();
  b.chain_live = live.data();
  b.f = f.data();
  b.chunk_off = plan.chunk_off.data();
  b.chunk_reqs = plan.chunk_reqs.data();

  for (uint32_t c = 0; c < C; ++c) {
    const uint32_t beg = plan.chunk_off[c], end = plan.chunk_off[c + 1];
    // the kernel's order: strided partial sums, six tree steps, G1 then G2
    std::vector<G1J> s1(LANES);
    std::vector<G2J> s2(LANES);
    for (uint32_t l = 0; l < LANES; ++l)
      s1[l] = smsum_partial<Fp>(b.chain, b.chain_live, b.chunk_reqs, beg, end, l, LANES, CH_RP);
    smsum_tree(s1.data(), LANES);
    for (uint32_t l = 0; l < LANES; ++l)
      s2[l] = smsum_partial<Fp2>(b.chain, b.chain_live, b.chunk_reqs, beg, end, l, LANES, CH_RS);
    smsum_tree(s2.data(), LANES);
    // the reference: left to right over the live sets
    G1J r1 = jac_infinity<Fp>();
    G2J r2 = jac_infinity<Fp2>();
    uint32_t n_live = 0;
    for (uint32_t k = beg; k < end; ++k) {
      const uint32_t i = plan.chunk_reqs[k];
      if (!live[i]) continue;
      r1 = jac_add(r1, rp[i]);
      r2 = jac_add(r2, rs[i]);
      ++n_live;
    }
    CHECK(aff_eq(jac_to_aff(s1[0]), jac_to_aff(r1)), "job %u (%u sets, %u live): G1 sum", c, end - beg, n_live);
    CHECK(aff_eq(jac_to_aff(s2[0]), jac_to_aff(r2)), "job %u (%u sets, %u live): G2 sum", c, end - beg, n_live);
    if (cancel_first_job && c == 0)
      CHECK(jac_is_inf(s1[0]) && jac_is_inf(s2[0]), "job 0: P + (-P) must be the point at infinity");

    const uint32_t rep = plan.chunk_reqs[beg], u = unit_base + c, v = n + c;
    smsum_finish(b, c, s1[0], s2[0], rep);
    if (jac_is_inf(r1)) {
      CHECK(live[u] == 0 && fp12_is_one(f[u]), "job %u: an infinity unit is not live, f = 1", c);
    } else {
      const Fp* o = chain.data() + (size_t)CHAIN_WORDS * u;
      G1J got;
      memcpy(&got, o + CH_RP, sizeof(G1J));
      CHECK(live[u] == 1 && jac_eq(got, r1), "job %u: unit RP", c);
      CHECK(memcmp(o + CH_HQ, chain.data() + (size_t)CHAIN_WORDS * rep + CH_HQ, 4 * sizeof(Fp)) == 0,
            "job %u: unit HQ is the representative set's", c);
    }
    if (jac_is_inf(r2)) {
      CHECK(live[v] == 0 && fp12_is_one(f[v]), "job %u: an infinity signature sum is not live, f = 1", c);
    } else {
      const Fp* o = chain.data() + (size_t)CHAIN_WORDS * v;
      const G2A a = jac_to_aff(r2);
      CHECK(live[v] == 1 && f_eq(Fp2{o[CH_HQ], o[CH_HQ + 1]}, a.x) && f_eq(Fp2{o[CH_HQ + 2], o[CH_HQ + 3]}, a.y),
            "job %u: virtual set HQ = affine sum", c);
      CHECK(f_eq(o[CH_RP], c_g1_x()) && f_eq(o[CH_RP + 1], c_g1_negy()) && f_eq(o[CH_RP + 2], c_one()),
            "job %u: virtual set RP = -g1", c);
    }
  }
  return 0;
}

static int bad_batches() {
  const uint32_t off_empty[] = {0, 2, 2, 5}, off_short[] = {0, 2, 4}, off_back[] = {0, 3, 2, 5};
  uint8_t roots[96] = {0}, sigs[96 * 5] = {0};
  uint32_t idx[5] = {0};
  int32_t v[5];
  bls_same_msg_batch in;
  memset(&in, 0, sizeof(in));
  in.n_jobs = 3;
  in.n_sets = 5;
  in.messages = roots;
  in.pk_indices = idx;
  in.signatures = sigs;
  in.job_set_offsets = off_empty;
  CHECK(check_same_message(&in, v) != nullptr, "an empty job must be refused");
  in.job_set_offsets = off_back;
  CHECK(check_same_message(&in, v) != nullptr, "offsets that go back must be refused");
  in.n_jobs = 2;
  in.job_set_offsets = off_short;
  CHECK(check_same_message(&in, v) != nullptr, "offsets that stop short of n_sets must be refused");
  in.n_sets = 4;
  CHECK(check_same_message(&in, v) == nullptr, "a good batch");
  CHECK(check_same_message(&in, nullptr) != nullptr, "NULL verdicts");
  in.signatures = nullptr;
  CHECK(check_same_message(&in, v) != nullptr, "NULL signatures");
  return 0;
}

int main() {
  if (run_jobs({1, 2, 63, 64, 65, 129}, 1, false)) return 1;
  if (run_jobs({129, 1, 65, 1, 2}, 2, true)) return 1;
  if (bad_batches()) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
