// The Pippenger signature sum's stage bodies (kernels/k_msm.hip has the method and the
// serial launches), shared by k_msm.hip, by the Miller-loop launches that run the long
// stages as roles of their own blocks (kernels/k_mlq.hip k_mlq_msm / k_mlf_msm) and by
// the CPU restatement (tests/native/msm_host.cpp, which loops the lanes of each step).
//
//   msm_bin_lane / msm_scatter_lane   one lane per set (msm_bin_entries: the same for a given
//                     64-bit scalar, for the host test's repeated scalars)
//   msm_seg_lane      one lane per segment of <= seg points of one bucket
//   msm_bucket_lane   one lane per bucket; msm_bucket_block_lane: the same with the
//                     buckets laid out MSM_BKT_BLOCKS blocks per window, so that a
//                     window's buckets are complete when its blocks have all arrived
//   msm_win_*         the steps of one window's wavefront (lane sums, suffix scan, weights,
//                     tree, scaling): the device runs them with a barrier between the
//                     steps (msm_window_wave), the host one lane after the other
//                     (msm_window_host)
//   msm_final_lane    the four windows' sum into the chunk groups' virtual sets
//   msm_last_block    the ticket: true in the block that arrives last of `expected`
// Every Fp2 product's output is canonical whichever primitive the translation unit
// selects (BLS_FP2_PRIM), and the additions are curve.hpp's complete ones, so every
// stage's result is the same Jacobian triple in each of the three builds.
#pragma once

#include "msm_bufs.hpp"
#include "pipeline.hpp"

namespace bls {

// one out-of-line copy of each addition per kernel (the bodies are large)
#if defined(__HIPCC__)
#define BLS_MSM_ADD static __host__ __device__ __attribute__((noinline))
#else
#define BLS_MSM_ADD static inline
#endif
BLS_MSM_ADD void msm_madd(G2J* acc, const G2A* p) { *acc = jac_add_aff(*acc, *p); }
BLS_MSM_ADD void msm_add(G2J* acc, const G2J* p) { *acc = jac_add(*acc, *p); }
BLS_MSM_ADD void msm_dbl(G2J* acc) { *acc = jac_dbl(*acc); }

// point reference: set index, top bit = the mu image
BLS_HD G2A msm_point(const PipeBufs& b, uint32_t ref) {
  const G2A s = b.sig[ref & 0x7FFFFFFFu];
  if (!(ref >> 31)) return s;
  const G2J m = g2_mu(jac_from_aff(s));  // z stays 1: psi conjugates it
  G2A r;
  r.x = m.x;
  r.y = m.y;
  r.inf = false;
  return r;
}

// set i's 8 (window, digit) entries, each with its slot in the bucket (a count per bucket:
// atomic on the device; the host runs the lanes one by one)
// (r64: the set's 64-bit random value, set_scalar)
BLS_HD void msm_bin_entries(const PipeBufs& b, const MsmBufs& m, uint32_t i, uint64_t r64) {
  uint32_t* ent = m.ent + 8ull * i;
  if (!b.chain_live[i]) {
    for (int j = 0; j < 8; ++j) ent[j] = MSM_ENT_NONE;
    return;
  }
  uint32_t sc[2];
  glv_split(r64, sc[0], sc[1]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 8; ++j) {
    const uint32_t w = (uint32_t)j >> 1, d = (sc[j & 1] >> (8 * w)) & 255u;
    if (d == 0) {
      ent[j] = MSM_ENT_NONE;
      continue;
    }
    const uint32_t key = w * MSM_D + d - 1;
#if defined(__HIP_DEVICE_COMPILE__)
    ent[j] = (key << 22) | atomicAdd(&m.cnt[key], 1u);
#else
    ent[j] = (key << 22) | m.cnt[key]++;
#endif
  }
}

BLS_HD void msm_bin_lane(const PipeBufs& b, const MsmBufs& m, uint32_t i) {
  msm_bin_entries(b, m, i, b.chain_live[i] ? set_scalar(b.seed, b.scalar_base + i) : 0ull);
}

BLS_HD void msm_scatter_lane(const MsmBufs& m, uint32_t i) {
  const uint32_t* ent = m.ent + 8ull * i;
  for (int j = 0; j < 8; ++j) {
    const uint32_t e = ent[j];
    if (e == MSM_ENT_NONE) continue;
    m.sorted[m.off[e >> 22] + (e & 0x3FFFFFu)] = i | ((uint32_t)(j & 1) << 31);
  }
}

// lane s: segment s of the bucket whose [seg_off[k], seg_off[k + 1]) holds it
BLS_HD void msm_seg_lane(const PipeBufs& b, const MsmBufs& m, uint32_t seg, uint32_t s) {
  if (s >= m.seg_off[MSM_NB]) return;
  uint32_t lo = 0, hi = MSM_NB;  // largest k with seg_off[k] <= s
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (m.seg_off[mid] <= s) lo = mid;
    else hi = mid;
  }
  const uint32_t beg = m.off[lo] + (s - m.seg_off[lo]) * seg;
  const uint32_t end = beg + seg < m.off[lo + 1] ? beg + seg : m.off[lo + 1];
  G2J acc = jac_infinity<Fp2>();
  for (uint32_t e = beg; e < end; ++e) {
    const G2A p = msm_point(b, m.sorted[e]);
    msm_madd(&acc, &p);
  }
  m.seg_sum[s] = acc;
}

BLS_HD void msm_bucket_lane(const MsmBufs& m, uint32_t k) {
  if (k >= MSM_NB) return;
  G2J acc = jac_infinity<Fp2>();
  for (uint32_t s = m.seg_off[k]; s < m.seg_off[k + 1]; ++s) {
    const G2J p = m.seg_sum[s];
    msm_add(&acc, &p);
  }
  m.bucket[k] = acc;
}

// bucket block j of MSM_W * MSM_BKT_BLOCKS: window j / MSM_BKT_BLOCKS, its buckets
// MSM_LANES (j % MSM_BKT_BLOCKS) + lane (the 256th lane of a window idles)
BLS_HD uint32_t msm_bucket_block_window(uint32_t j) { return j / MSM_BKT_BLOCKS; }
BLS_HD void msm_bucket_block_lane(const MsmBufs& m, uint32_t j, uint32_t lane) {
  const uint32_t d1 = MSM_LANES * (j % MSM_BKT_BLOCKS) + lane;
  if (d1 < MSM_D) msm_bucket_lane(m, msm_bucket_block_window(j) * MSM_D + d1);
}

// One wavefront per window w: T_w = sum_{d=1..255} d B_{w,d}.  Lane l owns digits
// d = 4 l + j (j = 0..3, B_0 = O):
//   S_l = sum_j B_{4l+j},  W_l = sum_j j B_{4l+j}  (running sums, 5 additions)
//   T_w = sum_l (4 l S_l + W_l) = sum_l ([4] U_l + W_l),  U_l = sum_{k >= l, k >= 1} S_k
// U by a suffix scan over the lanes (L: one G2J per lane), then one tree; lane 0 scales by
// 2^(8 w).
BLS_HD void msm_win_lane_sums(const MsmBufs& m, uint32_t w, uint32_t l, G2J& s, G2J& wl) {
  // suffix sums within the lane: s = B3, B3 + B2, ...; W = B3 + (B3 + B2) + (B3 + B2 + B1)
  s = m.bucket[w * MSM_D + 4 * l + 3 - 1];
  wl = s;
  for (int j = 2; j >= 0; --j) {
    const uint32_t d = 4 * l + (uint32_t)j;
    const G2J bj = d ? m.bucket[w * MSM_D + d - 1] : jac_infinity<Fp2>();
    msm_add(&s, &bj);
    if (j > 0) msm_add(&wl, &s);
  }
}
// a suffix-scan step reads ...
BLS_HD G2J msm_win_scan_read(const G2J* L, uint32_t l, uint32_t off) {
  return l + off < MSM_LANES ? L[l + off] : jac_infinity<Fp2>();
}
// ... and, once every lane has read, adds and writes: U_l = sum_{k >= l} S_k after off = 1 .. 32
BLS_HD void msm_win_scan_write(G2J* L, uint32_t l, G2J& u, const G2J& y) {
  msm_add(&u, &y);
  L[l] = u;
}
// [4] U_l + W_l, U over the lanes l >= 1 only
BLS_HD G2J msm_win_weight(uint32_t l, const G2J& u_in, const G2J& wl) {
  G2J u = l == 0 ? jac_infinity<Fp2>() : u_in;
  msm_dbl(&u);
  msm_dbl(&u);
  msm_add(&u, &wl);
  return u;
}
BLS_HD void msm_win_tree_step(G2J* L, uint32_t l, uint32_t off) {
  if (l < off) {
    const G2J y = L[l + off];
    G2J z = L[l];
    msm_add(&z, &y);
    L[l] = z;
  }
}
BLS_HD void msm_win_scale(const MsmBufs& m, uint32_t w, const G2J& t_in) {
  G2J t = t_in;
  for (uint32_t k = 0; k < 8 * w; ++k) msm_dbl(&t);
  m.win[w] = t;
}

// S = sum_w [2^(8w)] T_w: the chunk group 0's virtual set; the other groups are empty
BLS_HD void msm_final_lane(const PipeBufs& b, const MsmBufs& m, uint32_t l, uint32_t groups, uint32_t vbase) {
  if (l == 0) {
    G2J acc = m.win[0];
    for (uint32_t k = 1; k < MSM_W; ++k) {
      const G2J p = m.win[k];
      msm_add(&acc, &p);
    }
    vset_write(b, acc, vbase);
  }
  for (uint32_t g = 1 + l; g < groups; g += MSM_LANES) vset_write(b, jac_infinity<Fp2>(), vbase + g);
}

#if defined(__HIPCC__)
// last block of `expected` to arrive: true in every lane of that block; the others'
// writes are visible to it (device-scope release / acquire fences around a device-scope
// ticket, reset for the next pass).  Block-uniform: every lane of the block calls it.
static __device__ __forceinline__ bool msm_last_block(uint32_t* ticket, uint32_t expected) {
  __shared__ uint32_t last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == expected - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return false;  // (a block's next ticket writes the flag only after its first barrier)
  __threadfence();
  if (threadIdx.x == 0) (void)atomicExch(ticket, 0u);
  return true;
}

// window w on the calling wavefront (a block of MSM_LANES lanes), L in LDS
static __device__ __forceinline__ void msm_window_wave(const MsmBufs& m, uint32_t w, G2J* L) {
  const uint32_t l = threadIdx.x;
  G2J s, wl;
  msm_win_lane_sums(m, w, l, s, wl);
  L[l] = s;
  __syncthreads();
  G2J u = s;
  for (uint32_t off = 1; off < MSM_LANES; off <<= 1) {
    const G2J y = msm_win_scan_read(L, l, off);
    __syncthreads();
    msm_win_scan_write(L, l, u, y);
    __syncthreads();
  }
  L[l] = msm_win_weight(l, u, wl);
  __syncthreads();
  for (uint32_t off = MSM_LANES / 2; off >= 1; off >>= 1) {
    msm_win_tree_step(L, l, off);
    __syncthreads();
  }
  if (l == 0) msm_win_scale(m, w, L[0]);
}
#else
// the host's ticket: blocks run one after the other
static inline bool msm_last_block(uint32_t* ticket, uint32_t expected) {
  if (++*ticket != expected) return false;
  *ticket = 0;
  return true;
}

// window w with the wavefront's steps as loops over the lanes, in the kernel's order
static inline void msm_window_host(const MsmBufs& m, uint32_t w, G2J* L) {
  G2J u[MSM_LANES], wl[MSM_LANES], y[MSM_LANES];
  for (uint32_t l = 0; l < MSM_LANES; ++l) {
    msm_win_lane_sums(m, w, l, u[l], wl[l]);
    L[l] = u[l];
  }
  for (uint32_t off = 1; off < MSM_LANES; off <<= 1) {
    for (uint32_t l = 0; l < MSM_LANES; ++l) y[l] = msm_win_scan_read(L, l, off);
    for (uint32_t l = 0; l < MSM_LANES; ++l) msm_win_scan_write(L, l, u[l], y[l]);
  }
  for (uint32_t l = 0; l < MSM_LANES; ++l) L[l] = msm_win_weight(l, u[l], wl[l]);
  for (uint32_t off = MSM_LANES / 2; off >= 1; off >>= 1)
    for (uint32_t l = 0; l < MSM_LANES; ++l) msm_win_tree_step(L, l, off);
  msm_win_scale(m, w, L[0]);
}
#endif

// segment length for a pass of n_sets: ~sqrt(entries per bucket), so the per-segment mixed
// additions and the per-bucket segment additions are about equally deep
static inline uint32_t msm_seg_len(uint32_t n_sets) {
  const uint32_t per_bucket = (8u * n_sets + MSM_NB - 1) / MSM_NB;
  uint32_t seg = 8;
  while (seg * seg < per_bucket) seg *= 2;
  return seg;
}

}  // namespace bls
