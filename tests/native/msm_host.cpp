// TEST INFRASTRUCTURE ONLY -- never linked into the product library.
//
// CPU restatement of the Pippenger signature sum (kernels/k_msm.hip and the roles of
// kernels/k_mlq.hip's k_mlq_msm / k_mlf_msm): the identical stage bodies (bls/msm.hpp)
// compiled for the host, a wavefront replaced by a loop over its 64 lanes and a launch by
// a loop over its blocks.  For n = 2, 63, 64, 65 and 256 sets [k] g2 with the pipeline's
// set_scalar / glv_split scalars, some sets not live, a bucket that spans several
// segments (a few scalars repeated) and a cancelling pair:
//   - the virtual set's affine point equals a plain left-to-right sum of [r_i] sig_i;
//   - with the f-side launch's 16 bucket blocks run forward, in reverse and in shuffled
//     orders, exactly one block per window runs the window body and one the final sum,
//     the four window sums and the final point are bit-identical, and every ticket and
//     bucket count is back at zero.
// A stand-alone program (its own main), so it also runs under -fsanitize=address,undefined.
//
//   msm_host            prints "ok <checks>" and exits 0, or the first mismatch and 1
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define BLS_LAZY_POW 1
#include "bls/msm.hpp"

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

static bool aff_eq(const G2A& a, const G2A& b) {
  if (a.inf || b.inf) return a.inf && b.inf;
  return f_eq(a.x, b.x) && f_eq(a.y, b.y);
}

enum Mode { PLAIN, REPEAT, CANCEL, NONE_LIVE };

// the sum's buffers for a pass of n sets and C chunk groups
struct Pass {
  uint32_t n, C, seg;
  std::vector<G2A> sig;
  std::vector<uint32_t> live, seed, state, off, seg_off, ent, sorted;
  std::vector<uint64_t> r;
  std::vector<G2J> seg_sum, bucket, win;
  std::vector<Fp> chain;
  std::vector<Fp12> f;
  PipeBufs b;
  MsmBufs m;
  Pass(uint32_t n_, uint32_t C_)
      : n(n_), C(C_), seg(msm_seg_len(n_)), sig(n_), live(n_ + C_, 0), seed(8), state(MSM_NB + MSM_TICKETS, 0),
        off(MSM_NB + 1), seg_off(MSM_NB + 1), ent(8ull * n_), sorted(8ull * n_), r(n_),
        seg_sum(8ull * n_ / seg + MSM_NB + 1), bucket(MSM_NB), win(MSM_W), chain((size_t)CHAIN_WORDS * (n_ + C_)),
        f(n_ + C_) {
    memset(&b, 0, sizeof(b));
    b.n_sets = n;
    b.n_chunks = C;
    b.sig = sig.data();
    b.chain_live = live.data();
    b.seed = seed.data();
    b.chain = chain.data();
    b.f = f.data();
    m.cnt = state.data();
    m.ticket = state.data() + MSM_NB;
    m.off = off.data();
    m.seg_off = seg_off.data();
    m.ent = ent.data();
    m.sorted = sorted.data();
    m.seg_sum = seg_sum.data();
    m.bucket = bucket.data();
    m.win = win.data();
  }
};

// k_msm_bin's scan as plain prefix sums; the counts go back to zero as the kernel leaves them
static uint32_t offsets(Pass& p) {
  uint32_t a = 0, c = 0, deepest = 0;
  for (uint32_t k = 0; k < MSM_NB; ++k) {
    p.off[k] = a;
    p.seg_off[k] = c;
    a += p.state[k];
    c += (p.state[k] + p.seg - 1) / p.seg;
    deepest = std::max(deepest, p.state[k]);
    p.state[k] = 0;
  }
  p.off[MSM_NB] = a;
  p.seg_off[MSM_NB] = c;
  return deepest;
}

// the f-side launch's bucket blocks in the given order, as k_mlf_msm runs a block
static int bucket_blocks(Pass& p, const std::vector<uint32_t>& order, uint32_t ran[MSM_W], uint32_t& finals) {
  std::vector<G2J> L(MSM_LANES);
  for (uint32_t j : order) {
    const uint32_t w = msm_bucket_block_window(j);
    for (uint32_t l = 0; l < MSM_LANES; ++l) msm_bucket_block_lane(p.m, j, l);
    if (!msm_last_block(p.m.ticket + 2 + w, MSM_BKT_BLOCKS)) continue;
    ++ran[w];
    msm_window_host(p.m, w, L.data());
    if (!msm_last_block(p.m.ticket + 1, MSM_W)) continue;
    ++finals;
    for (uint32_t l = 0; l < MSM_LANES; ++l) msm_final_lane(p.b, p.m, l, p.C, p.n);
  }
  return 0;
}

static int run_case(uint32_t n, Mode mode, uint64_t seed0) {
  const uint32_t C = 3;
  Pass p(n, C);
  uint64_t st = seed0;
  for (int k = 0; k < 8; ++k) p.seed[k] = (uint32_t)splitmix(st);
  G2A g2;
  g2.x = c_g2_x();
  g2.y = c_g2_y();
  g2.inf = false;
  for (uint32_t i = 0; i < n; ++i) {
    p.sig[i] = jac_to_aff(aff_mul_u64(g2, (splitmix(st) >> 40) | 1ull));  // 24-bit scalars: short chains
    p.r[i] = set_scalar(p.seed.data(), p.b.scalar_base + i);
    p.live[i] = mode == NONE_LIVE ? 0u : (mode == PLAIN && n > 2 ? splitmix(st) % 5 != 0 : 1u);
  }
  if (mode == REPEAT) {
    // 3 seg + 1 sets with set 0's scalar: each of its 8 buckets spans four segments; every
    // fourth of them not live
    for (uint32_t i = 1; i < n && i <= 3 * p.seg; ++i) p.r[i] = p.r[0];
    for (uint32_t i = 3; i < n; i += 4) p.live[i] = 0;
  }
  if (mode == CANCEL) {
    // P and -P with one scalar and nothing else live: the sum is the point at infinity
    for (uint32_t i = 0; i < n; ++i) p.live[i] = 0;
    p.sig[n - 1] = p.sig[0];
    p.sig[n - 1].y = fp2_neg(p.sig[0].y);
    p.r[n - 1] = p.r[0];
    p.live[0] = p.live[n - 1] = 1;
  }

  // the reference: left to right over the live sets
  G2J ref = jac_infinity<Fp2>();
  uint32_t n_live = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!p.live[i]) continue;
    ref = jac_add(ref, jac_mul_set_scalar(jac_from_aff(p.sig[i]), p.r[i]));
    ++n_live;
  }
  const G2A ref_aff = jac_to_aff(ref);

  // k_msm_bin, k_msm_scatter, then the segments (k_msm_seg / k_mlq_msm's first blocks)
  for (uint32_t i = 0; i < n; ++i) msm_bin_entries(p.b, p.m, i, p.r[i]);
  const uint32_t deepest = offsets(p);
  if (mode == REPEAT && n > 3 * p.seg)
    CHECK(deepest > 2 * p.seg, "n %u: the repeated scalars must fill a bucket past two segments (%u)", n, deepest);
  CHECK(p.seg_off[MSM_NB] <= p.seg_sum.size(), "n %u: %u segments exceed the capacity", n, p.seg_off[MSM_NB]);
  for (uint32_t i = 0; i < n; ++i) msm_scatter_lane(p.m, i);
  const uint32_t seg_lanes = (p.seg_off[MSM_NB] + MSM_LANES - 1) / MSM_LANES * MSM_LANES;
  for (uint32_t s = 0; s < seg_lanes; ++s) msm_seg_lane(p.b, p.m, p.seg, s);

  // the bucket blocks in several orders
  std::vector<std::vector<uint32_t>> orders;
  std::vector<uint32_t> fwd(MSM_W * MSM_BKT_BLOCKS);
  for (uint32_t j = 0; j < fwd.size(); ++j) fwd[j] = j;
  orders.push_back(fwd);
  orders.push_back(std::vector<uint32_t>(fwd.rbegin(), fwd.rend()));
  for (int k = 0; k < 4; ++k) {
    std::vector<uint32_t> o(fwd);
    for (size_t j = o.size() - 1; j > 0; --j) std::swap(o[j], o[splitmix(st) % (j + 1)]);
    orders.push_back(o);
  }
  std::vector<G2J> win0;
  std::vector<Fp> chain0;
  std::vector<uint32_t> live0;
  for (size_t k = 0; k < orders.size(); ++k) {
    // nothing of an earlier order may stand in for this one's results
    memset((void*)p.bucket.data(), 0xA5, sizeof(G2J) * p.bucket.size());
    memset((void*)p.win.data(), 0xA5, sizeof(G2J) * p.win.size());
    memset((void*)p.chain.data(), 0xA5, sizeof(Fp) * p.chain.size());
    for (uint32_t g = 0; g < C; ++g) p.live[n + g] = 7u;
    uint32_t ran[MSM_W] = {0, 0, 0, 0}, finals = 0;
    if (bucket_blocks(p, orders[k], ran, finals)) return 1;
    for (uint32_t w = 0; w < MSM_W; ++w)
      CHECK(ran[w] == 1, "n %u order %zu: window %u ran %u times", n, k, w, ran[w]);
    CHECK(finals == 1, "n %u order %zu: %u final sums", n, k, finals);
    for (uint32_t t = 0; t < MSM_NB + MSM_TICKETS; ++t)
      CHECK(p.state[t] == 0, "n %u order %zu: state word %u is %u afterwards", n, k, t, p.state[t]);
    // the virtual sets: group 0 the sum, the others empty
    const Fp* o = p.chain.data() + (size_t)CHAIN_WORDS * n;
    if (ref_aff.inf) {
      CHECK(p.live[n] == 0 && fp12_is_one(p.f[n]), "n %u order %zu: an infinity sum is not live, f = 1", n, k);
    } else {
      G2A got;
      got.x = Fp2{o[CH_HQ], o[CH_HQ + 1]};
      got.y = Fp2{o[CH_HQ + 2], o[CH_HQ + 3]};
      got.inf = false;
      CHECK(p.live[n] == 1 && aff_eq(got, ref_aff), "n %u (%u live) order %zu: the sum", n, n_live, k);
      CHECK(f_eq(o[CH_RP], c_g1_x()) && f_eq(o[CH_RP + 1], c_g1_negy()) && f_eq(o[CH_RP + 2], c_one()),
            "n %u order %zu: virtual set RP = -g1", n, k);
    }
    for (uint32_t g = 1; g < C; ++g)
      CHECK(p.live[n + g] == 0 && fp12_is_one(p.f[n + g]), "n %u order %zu: group %u is empty", n, k, g);
    if (k == 0) {
      win0 = p.win;
      chain0 = p.chain;
      live0 = p.live;
    } else {
      CHECK(memcmp((const void*)win0.data(), (const void*)p.win.data(), sizeof(G2J) * MSM_W) == 0,
            "n %u order %zu: the window sums differ from the forward order's", n, k);
      CHECK(memcmp((const void*)chain0.data(), (const void*)p.chain.data(), sizeof(Fp) * p.chain.size()) == 0 &&
                live0 == p.live,
            "n %u order %zu: the final point differs from the forward order's", n, k);
    }
  }
  if (mode == CANCEL || mode == NONE_LIVE) CHECK(ref_aff.inf, "n %u: the case must sum to infinity", n);
  return 0;
}

int main() {
  const uint32_t sizes[] = {2, 63, 64, 65, 256};
  uint64_t seed = 1;
  for (uint32_t n : sizes) {
    if (run_case(n, PLAIN, seed++)) return 1;   // ~1 set in 5 not live (n = 2: both live)
    if (run_case(n, REPEAT, seed++)) return 1;  // a bucket over several segments
    if (run_case(n, CANCEL, seed++)) return 1;
  }
  if (run_case(64, NONE_LIVE, seed++)) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
