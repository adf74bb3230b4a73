// Miller loops split in two SIMT kernels (the aggregated-signature path's default):
//
//   k_mlq  one lane per item: the twist point T runs from Q = HQ through the 63
//          doubling and 5 addition steps of |x| = 0xd201000000010000 (bls/pairing.hpp
//          miller_dbl_step / miller_add_step) and writes each step's line, already
//          evaluated at P = RP made affine (l0, l2 x, l3 y: 6 Fp), to a line buffer -- 68
//          lines x 288 B per item, laid out line-major and lane-minor so a wavefront's
//          stores and loads are 256-byte rows;
//   k_mlf  one lane per TWO items of one product domain (a chunk, or a non-batchable
//          request: PipeBufs::ml_dom): f = prod over both pairs' lines with ONE
//          squaring of f per bit (blst's miller_loop_n likewise shares the
//          squarings), conjugated (x < 0); f of the first item, 1 in the second.  Items
//          of different domains, or the individually verified pass (units_paired = 0),
//          run one f per item.
//
// Against a fused one-lane loop (6,803 Fp products per pair, f + T + lines live together
// in one lane, 512 registers and spills; removed in round 4): the line side takes ~1,920
// products per pair with T, P and Q only; the f side 62 squarings (36) per two pairs
// plus 68 sparse line products (39) per pair -> ~5,700 products per pair, each kernel
// with half the live state.
//
// The Fp2 products and squares of both sides are the out-of-line lazy primitives
// (BLS_FP2_PRIM: field.hpp fp2_mul_w / fp2_sqr_w, one call and one reduction per
// coefficient instead of three Fp products; the second operand of a product travels
// through a lane-private LDS slot, 6 KB per block).  store_line's Fp2 x Fp keeps the two Fp
// products: it has two reductions either way, and the Fp2 primitive would add 392
// multiply-adds.
#define BLS_FP_D28 1
#define BLS_FP2_PRIM 1
#include <stdlib.h>

#include "../launchers.hpp"
#include "bls/knobs.hpp"
#include "bls/msm.hpp"
#include "bls/pairing.hpp"
#include "tower_op_ids.hpp"

using namespace bls;

static_assert(BLS_BLOCK == BLS_FP2_SLOT_LANES, "the Fp2 primitive's LDS slot holds one wavefront per block");

namespace {

constexpr int ML_EVENTS = 68;          // 63 doublings + 5 additions
constexpr int LINE_WORDS = 6 * 12;     // l0, l2, l3 (Fp2 each) as 32-bit words

__device__ __forceinline__ bool ml_live(const PipeBufs& b, uint32_t i, uint32_t units_paired) {
  if (!b.chain_live[i]) return false;
  return !(units_paired && b.set_unit && i < b.n_sets && b.set_unit[i] != UNIT_NONE);
}

// word w of line e of item k (stride = the launch's item count, padded to a wavefront)
__device__ __forceinline__ size_t line_at(uint32_t stride, uint32_t k, int e, int w) {
  return ((size_t)e * LINE_WORDS + w) * stride + k;
}

// P affine (g1_eval_affine_from_jac, z3 = 1): l0 is c0 itself
__device__ __forceinline__ void store_line(uint32_t* L, uint32_t stride, uint32_t k, int e, const G1Eval& P,
                                           const Fp2& c0, const Fp2& c1, const Fp2& c2) {
  const Fp2 l[3] = {c0, fp2_mul_fp(c1, P.xz), fp2_mul_fp(c2, P.y)};
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int w = 0; w < 12; ++w) {
      L[line_at(stride, k, e, 24 * j + w)] = l[j].c0.l[w];
      L[line_at(stride, k, e, 24 * j + 12 + w)] = l[j].c1.l[w];
    }
}

__device__ __forceinline__ void load_line(const uint32_t* L, uint32_t stride, uint32_t k, int e, Fp2& l0, Fp2& l2,
                                          Fp2& l3) {
  Fp2* l[3] = {&l0, &l2, &l3};
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int w = 0; w < 12; ++w) {
      l[j]->c0.l[w] = L[line_at(stride, k, e, 24 * j + w)];
      l[j]->c1.l[w] = L[line_at(stride, k, e, 24 * j + 12 + w)];
    }
}

// Inlined copies of field.hpp's fp12_sqr / fp12_mul_line (out of line there, which puts
// f on the stack at every call): here f stays in registers and only the Fp products are
// calls.
__device__ __forceinline__ Fp12 sqr12(const Fp12& a) {
  const Fp6 ab = fp6_mul(a.c0, a.c1);
  const Fp6 s = fp6_mul(fp6_add(a.c0, a.c1), fp6_add(a.c0, fp6_mul_v(a.c1)));
  return Fp12{fp6_sub(fp6_sub(s, ab), fp6_mul_v(ab)), fp6_add(ab, ab)};
}

__device__ __forceinline__ Fp12 mul_line12(const Fp12& f, const Fp2& l0, const Fp2& l2, const Fp2& l3) {
  const Fp6 aa = fp6_mul_01(f.c0, l0, l2);
  const Fp6 bb = fp6_mul_1(f.c1, l3);
  const Fp6 c1 = fp6_sub(fp6_sub(fp6_mul_01(fp6_add(f.c0, f.c1), l0, fp2_add(l2, l3)), aa), bb);
  return Fp12{fp6_add(aa, fp6_mul_v(bb)), c1};
}

// prod over n consecutive items k0 .. k0 + n - 1 of their line products, one squaring of f
// per bit (n at run time: one copy of the line product, whatever the sharing)
__device__ __forceinline__ Fp12 ml_f(const uint32_t* L, uint32_t stride, uint32_t k0, uint32_t n) {
  Fp12 f = fp12_one();
  int e = 0;
  const uint64_t X = BLS_X_ABS;
  for (int bit = 62; bit >= 0; --bit) {
    if (bit != 62) f = sqr12(f);
    const int adds = (int)((X >> bit) & 1ull);
    for (int a = 0; a <= adds; ++a) {
      uint32_t g = 0;
      // two items' lines at once (fp12_mul_line2: 23 Fp2 products instead of 26; +4 % at
      // the plateau, profiles/r03_ab_mlq_mlf.json)
#pragma unroll 1
      for (; g + 1 < n; g += 2) {
        Fp2 l0, l2, l3, m0, m2, m3;
        load_line(L, stride, k0 + g, e, l0, l2, l3);
        load_line(L, stride, k0 + g + 1, e, m0, m2, m3);
        f = fp12_mul_line2(f, l0, l2, l3, m0, m2, m3);
      }
#pragma unroll 1
      for (; g < n; ++g) {
        Fp2 l0, l2, l3;
        load_line(L, stride, k0 + g, e, l0, l2, l3);
        f = mul_line12(f, l0, l2, l3);
      }
      ++e;
    }
  }
  return fp12_conj(f);
}

// Item k of a launch: items[k] of a list, else first + k, with the items from gap_at on
// moved up by gap (the overlapped first pass runs the sets and the units and leaves out
// the chunk groups' virtual sets between them; every other launch has gap = 0).
struct MlItems {
  uint32_t first, count, gap_at, gap;
  const uint32_t* items;
  __device__ __forceinline__ uint32_t at(uint32_t k) const {
    return items ? items[k] : first + k + (k >= gap_at ? gap : 0u);
  }
};

// the line side of item k (lane k of the launch's Miller-loop blocks)
__device__ __forceinline__ void mlq_lane(const PipeBufs& b, const MlItems& it, uint32_t k, uint32_t units_paired,
                                         uint32_t* L, uint32_t stride) {
  if (k >= it.count) return;
  const uint32_t i = it.at(k);
  if (!ml_live(b, i, units_paired)) return;
  const Fp* ch = b.chain + (size_t)CHAIN_WORDS * i;
  G1J rp;
  rp.x = ch[CH_RP + 0];
  rp.y = ch[CH_RP + 1];
  rp.z = ch[CH_RP + 2];
  const G1Eval P = g1_eval_affine_from_jac(rp);
  G2A q;
  q.x = Fp2{ch[CH_HQ + 0], ch[CH_HQ + 1]};
  q.y = Fp2{ch[CH_HQ + 2], ch[CH_HQ + 3]};
  q.inf = false;
  G2Proj T;
  T.x = q.x;
  T.y = q.y;
  T.z = fp2_one();
  Fp2 c0, c1, c2;
  int e = 0;
  const uint64_t X = BLS_X_ABS;
  for (int bit = 62; bit >= 0; --bit) {
    miller_dbl_step(T, c0, c1, c2);
    store_line(L, stride, k, e++, P, c0, c1, c2);
    if ((X >> bit) & 1ull) {
      miller_add_step(T, q, c0, c1, c2);
      store_line(L, stride, k, e++, P, c0, c1, c2);
    }
  }
}

// the f side of lane t: per_lane items k0 .. k0 + per_lane - 1.  When all are live and of
// one product domain they share one f (one squaring per bit for all of them), else each
// runs its own; items (an index list, the individually verified pass) never share
__device__ __forceinline__ void mlf_lane(const PipeBufs& b, const MlItems& it, uint32_t t, uint32_t units_paired,
                                         const uint32_t* L, uint32_t stride, uint32_t per_lane) {
  const uint32_t k0 = per_lane * t;
  if (k0 >= it.count) return;
  const uint32_t n = min(per_lane, it.count - k0);
  const uint32_t i0 = it.at(k0);
  // ml_dom covers the first-pass items [0, indiv_vbase) only: the individually verified
  // requests' signature sums after it never share (reading past it paired two requests'
  // sums into one f -- the verdict bug test_verify_many_merged_signature_sum_fails found)
  bool share = n > 1 && units_paired && b.ml_dom && !it.items && ml_live(b, i0, units_paired);
  for (uint32_t g = 1; share && g < n; ++g) {
    const uint32_t i = it.at(k0 + g);
    share = ml_live(b, i, units_paired) && i < b.indiv_vbase && b.ml_dom[i] == b.ml_dom[i0];
  }
  if (share) {
    b.f[i0] = ml_f(L, stride, k0, n);
    for (uint32_t g = 1; g < n; ++g) b.f[it.at(k0 + g)] = fp12_one();
    return;
  }
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t i = it.at(k0 + g);
    if (ml_live(b, i, units_paired)) b.f[i] = ml_f(L, stride, k0 + g, 1);
  }
}

}  // namespace

template <int W>
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(W, W))) void k_mlq(
    PipeBufs b, uint32_t first, uint32_t count, uint32_t units_paired, uint32_t* L, uint32_t stride,
    const uint32_t* items) {
  mlq_lane(b, MlItems{first, count, 0xFFFFFFFFu, 0u, items}, blockIdx.x * BLS_BLOCK + threadIdx.x, units_paired, L,
           stride);
}

template <int W>
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(W, W))) void k_mlf(
    PipeBufs b, uint32_t first, uint32_t count, uint32_t units_paired, const uint32_t* L, uint32_t stride,
    const uint32_t* items, uint32_t per_lane) {
  mlf_lane(b, MlItems{first, count, 0xFFFFFFFFu, 0u, items}, blockIdx.x * BLS_BLOCK + threadIdx.x, units_paired, L,
           stride, per_lane);
}

// ---------------------------------------------------------------------------
// The overlapped form of a first pass that sums its signatures by the Pippenger method
// (kernels/k_msm.hip, bls/msm.hpp).  Nothing needs the sum before the chunk groups'
// virtual sets are paired, and the sets' and units' own Miller loops do not depend on it,
// so the sum's long stages run as roles of these two launches' lowest blocks instead of
// as three nearly empty launches in front of them (192, 16 and 4 wavefronts, each waiting
// for a free wave slot among the other passes' 512-register waves):
//   k_mlq_msm  blocks [0, seg_blocks): k_msm_seg's body, one lane per segment; the blocks
//              after them: k_mlq's body over the sets [0, n) and the units (MlItems gap:
//              never the virtual sets [n, n + C), which do not exist yet)
//   k_mlf_msm  blocks [0, 16): k_msm_bucket's body, four blocks per window; the last of a
//              window's four to arrive (a ticket per window) runs k_msm_window's body as
//              its one wavefront, and the last of the four windows (the ticket of the
//              serial form) sums them and writes the virtual sets; the blocks after them:
//              k_mlf<1>'s body over the same items as k_mlq_msm
// The role branches are uniform over a block.  No wavefront waits for another: the only
// ordering inside a launch is "the last arriver continues", everything else is the order
// of the launches on the stream (k_mlq_msm's segment sums are complete before k_mlf_msm
// starts).  The MSM blocks come first in the grid so that they are dispatched first; they
// raise their priority as the serial kernels do.  LDS per block: the Fp2 primitive's slot
// (6 KB) + the window's lane array (18 KB) + flags < 25 KB, four blocks (one per SIMD) per
// CU under 100 KB of its 160 KB.
// ---------------------------------------------------------------------------
constexpr uint32_t MSM_BUCKET_BLOCKS = MSM_W * MSM_BKT_BLOCKS;
// every block of k_mlf_msm is charged the window role's lane array beside the Fp2 slot:
// four blocks (one wavefront per SIMD) must fit a CU's 160 KB of LDS
static_assert(4 * (sizeof(G2J) * MSM_LANES + 12 * BLS_FP2_SLOT_LANES * sizeof(uint64_t) + 64) <= 160 * 1024,
              "k_mlf_msm: LDS per CU no longer holds one wavefront per SIMD");

// The MSM blocks' bodies, out of line: the kernels' own registers and scratch accesses are
// then the Miller-loop role's, as in k_mlq / k_mlf (inlined, the bucket role cost k_mlf's
// per-item line loop two more scratch loads and stores per line; profiles/ab_msm_overlap.json)
static __device__ __attribute__((noinline)) void msm_seg_role(const PipeBufs& b, const MsmBufs& m, uint32_t seg) {
  BLS_TAIL_PRIO();
  msm_seg_lane(b, m, seg, blockIdx.x * BLS_BLOCK + threadIdx.x);
}

static __device__ __attribute__((noinline)) void msm_bucket_role(const PipeBufs& b, const MsmBufs& m, uint32_t groups,
                                                                 uint32_t vbase) {
  BLS_TAIL_PRIO();
  __shared__ G2J lanes[MSM_LANES];
  const uint32_t w = msm_bucket_block_window(blockIdx.x);
  msm_bucket_block_lane(m, blockIdx.x, threadIdx.x);
  if (!msm_last_block(m.ticket + 2 + w, MSM_BKT_BLOCKS)) return;
  msm_window_wave(m, w, lanes);
  if (!msm_last_block(m.ticket + 1, MSM_W)) return;
  msm_final_lane(b, m, threadIdx.x, groups, vbase);
}

template <int W>
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(W, W))) void k_mlq_msm(
    PipeBufs b, MsmBufs m, uint32_t seg, uint32_t seg_blocks, uint32_t count, uint32_t gap_at, uint32_t gap,
    uint32_t* L, uint32_t stride) {
  if (blockIdx.x < seg_blocks) {
    msm_seg_role(b, m, seg);
    return;
  }
  mlq_lane(b, MlItems{0u, count, gap_at, gap, nullptr}, (blockIdx.x - seg_blocks) * BLS_BLOCK + threadIdx.x, 1u, L,
           stride);
}

template <int W>
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(W, W))) void k_mlf_msm(
    PipeBufs b, MsmBufs m, uint32_t count, uint32_t gap_at, uint32_t gap, const uint32_t* L, uint32_t stride,
    uint32_t per_lane) {
  if (blockIdx.x < MSM_BUCKET_BLOCKS) {
    msm_bucket_role(b, m, gap, gap_at);  // the gap is the chunk groups' virtual sets
    return;
  }
  mlf_lane(b, MlItems{0u, count, gap_at, gap, nullptr}, (blockIdx.x - MSM_BUCKET_BLOCKS) * BLS_BLOCK + threadIdx.x,
           1u, L, stride, per_lane);
}

// ---------------------------------------------------------------------------
// k_mlf2: the f side with two lanes per item, for few sets in flight (a pass of 16,384
// sets runs as 544 wavefronts instead of 272, each with half of the f chain's products).  Lanes 2k and 2k + 1 hold the same f; per step each computes
// one of the squaring's two Fp6 products and one of the line's two mul_by_01 products
// (plus one of the Fp2 products of f.c1 l3, and both the third), swaps its products with
// its partner (DPP quad_perm [1,0,3,2]: one move per word), and both finish the step --
// 39 Fp products per lane per doubling step instead of 75 (field.hpp fp12_sqr_half_* /
// fp12_line_half_*).  Same f as ml_f(.., 1) (test_gpu_parity runs every shape).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
}
__device__ __forceinline__ Fp pair_swap(const Fp& a) {
  Fp r;
#pragma unroll
  for (int w = 0; w < 12; ++w) r.l[w] = pair_swap(a.l[w]);
  return r;
}
__device__ __forceinline__ Fp2 pair_swap(const Fp2& a) { return Fp2{pair_swap(a.c0), pair_swap(a.c1)}; }
__device__ __forceinline__ Fp6 pair_swap(const Fp6& a) { return Fp6{pair_swap(a.c0), pair_swap(a.c1), pair_swap(a.c2)}; }

__device__ __forceinline__ Fp12 sqr12_pair(const Fp12& a, bool h) {
  const Fp6 m = fp12_sqr_half_prod(a, h);
  return fp12_sqr_half_join(m, pair_swap(m), h);
}

__device__ __forceinline__ Fp12 mul_line12_pair(const Fp12& f, const Fp2& l0, const Fp2& l2, const Fp2& l3, bool h) {
  const LineHalf own = fp12_line_half_prod(f, l0, l2, l3, h);
  return fp12_line_half_join(own, pair_swap(own.m), pair_swap(own.p), h);
}


template <int W>
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(W, W))) void k_mlf2(
    PipeBufs b, uint32_t first, uint32_t count, uint32_t units_paired, const uint32_t* L, uint32_t stride,
    const uint32_t* items) {
  const uint32_t t = blockIdx.x * BLS_BLOCK + threadIdx.x;
  const uint32_t k = t >> 1;
  const bool h = (t & 1u) != 0u;
  // both lanes of a pair take the same exits: the partner of every swap is active
  if (k >= count) return;
  const uint32_t i = items ? items[k] : first + k;
  if (!ml_live(b, i, units_paired)) return;
  Fp12 f = fp12_one();
  int e = 0;
  const uint64_t X = BLS_X_ABS;
  for (int bit = 62; bit >= 0; --bit) {
    if (bit != 62) f = sqr12_pair(f, h);
    const int adds = (int)((X >> bit) & 1ull);
    for (int a = 0; a <= adds; ++a) {
      Fp2 l0, l2, l3;
      load_line(L, stride, k, e, l0, l2, l3);
      f = mul_line12_pair(f, l0, l2, l3, h);
      ++e;
    }
  }
  if (!h) b.f[i] = fp12_conj(f);
}

// line buffer words for a launch of `count` items (stride padded to a wavefront)
size_t mlq_line_words(uint32_t count) {
  const size_t stride = ((size_t)count + BLS_BLOCK - 1) / BLS_BLOCK * BLS_BLOCK;
  return stride * ML_EVENTS * LINE_WORDS;
}

hipError_t launch_k_mlqf(const PipeBufs& b, uint32_t first, uint32_t count, bool own_only, uint32_t* lines,
                         hipStream_t s, const uint32_t* items) {
  if (count == 0) return hipSuccess;
  const uint32_t stride = (count + BLS_BLOCK - 1) / BLS_BLOCK * BLS_BLOCK;
  // k_mlq / k_mlf at one wavefront per SIMD (512 registers, no spills around the products:
  // +3 % at 12 x 16 over two per SIMD, profiles/r03_ab_mlq_mlf.json)
  const uint32_t up = (own_only || items) ? 0u : 1u;
  k_mlq<1><<<bls_grid_for(count), BLS_BLOCK, 0, s>>>(b, first, count, up, lines, stride, items);
  // items per k_mlf lane, or two lanes per item (k_mlf2): bls/knobs.hpp mlf_per_lane
  const bls::Knobs& kn = bls::knobs();
  const uint32_t per_lane = b.mlf_pl ? b.mlf_pl : bls::mlf_per_lane(kn, bls_sets_in_flight());
  if (per_lane == MLF_PAIR) {
    if (kn.mlf2_waves == 2) k_mlf2<2><<<bls_grid_for(2 * count), BLS_BLOCK, 0, s>>>(b, first, count, up, lines, stride, items);
    else k_mlf2<1><<<bls_grid_for(2 * count), BLS_BLOCK, 0, s>>>(b, first, count, up, lines, stride, items);
    return hipGetLastError();
  }
  const uint32_t lanes = (count + per_lane - 1) / per_lane;
  k_mlf<1><<<bls_grid_for(lanes), BLS_BLOCK, 0, s>>>(b, first, count, up, lines, stride, items, per_lane);
  return hipGetLastError();
}

hipError_t launch_k_mlqf_msm(const PipeBufs& b, const MsmBufs& m, uint32_t groups, uint32_t n_units, uint32_t* lines,
                             hipStream_t s) {
  const uint32_t n = b.n_sets, count = n + n_units, per_lane = b.mlf_pl;
  if (n == 0 || groups == 0 || !(per_lane == 1 || per_lane == 2 || per_lane == 4)) return hipErrorInvalidValue;
  const uint32_t stride = (count + BLS_BLOCK - 1) / BLS_BLOCK * BLS_BLOCK;
  const uint32_t seg_blocks = bls_grid_for((uint32_t)msm_seg_cap(n));
  k_mlq_msm<1><<<seg_blocks + bls_grid_for(count), BLS_BLOCK, 0, s>>>(b, m, msm_seg_len(n), seg_blocks, count, n,
                                                                      groups, lines, stride);
  const uint32_t lanes = (count + per_lane - 1) / per_lane;
  k_mlf_msm<1><<<MSM_BUCKET_BLOCKS + bls_grid_for(lanes), BLS_BLOCK, 0, s>>>(b, m, count, n, groups, lines, stride,
                                                                            per_lane);
  return hipGetLastError();
}

// k_mlq<1> alone over items [0, count), each its own: the line buffer of the tower-op
// self-test's TOP_MLQ_LINES (bls_gpu.hip tower_lines_test)
hipError_t launch_k_mlq_lines(const PipeBufs& b, uint32_t count, uint32_t* lines, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const uint32_t stride = (count + BLS_BLOCK - 1) / BLS_BLOCK * BLS_BLOCK;
  k_mlq<1><<<bls_grid_for(count), BLS_BLOCK, 0, s>>>(b, 0u, count, 0u, lines, stride, nullptr);
  return hipGetLastError();
}

// Tower-op self-test (kernels/tower_ops.hpp), the ops whose functions are local to this file
// or exist only in this flavour: one lane per record calls sqr12, mul_line12 or
// fp12_mul_line2 as ml_f does; for the pair ops lanes 2k and 2k + 1 both load record k, each
// runs its half with pair_swap as k_mlf2 does, and both write their result (2k, 2k + 1).
// Both lanes of a pair take the same exit, and the lanes past the last record are idle as
// k_mlf2's are.  k_mlf<1>'s launch bounds and occupancy; one wavefront per block (the Fp2
// primitive's LDS slot).
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tower_op_mlq(
    uint32_t op, const Fp* in, uint32_t n, Fp12* out) {
  const uint32_t t = blockIdx.x * BLS_BLOCK + threadIdx.x;
  const bool pair = tower_op_is_pair(op);
  const uint32_t k = pair ? t >> 1 : t;
  const bool h = pair && (t & 1u) != 0u;
  if (k >= n) return;
  const Fp* r = in + (size_t)tower_op_in_fps(op) * k;
  const Fp12 f = *reinterpret_cast<const Fp12*>(r);
  const Fp2* l = reinterpret_cast<const Fp2*>(r + 12);
  if (op == TOP_MLQ_SQR12) out[t] = sqr12(f);
  else if (op == TOP_MLQ_MUL_LINE12) out[t] = mul_line12(f, l[0], l[1], l[2]);
  else if (op == TOP_MLQ_MUL_LINE2) out[t] = fp12_mul_line2(f, l[0], l[1], l[2], l[3], l[4], l[5]);
  else if (op == TOP_MLQ_SQR12_PAIR) out[t] = sqr12_pair(f, h);
  else out[t] = mul_line12_pair(f, l[0], l[1], l[2], h);
}

hipError_t launch_k_tower_op_mlq(uint32_t op, const Fp* in, uint32_t n, Fp* out, hipStream_t s) {
  if (!tower_op_in_mlq_tu(op)) return hipErrorInvalidValue;
  const uint32_t lanes = tower_op_is_pair(op) ? 2u * n : n;
  k_tower_op_mlq<<<bls_grid_for(lanes), BLS_BLOCK, 0, s>>>(op, in, n, reinterpret_cast<Fp12*>(out));
  return hipGetLastError();
}
