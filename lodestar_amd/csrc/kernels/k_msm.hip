// The merged signature sum S = sum_i [r_i] sig_i over a pass's live sets as a Pippenger
// multi-scalar multiplication (bucket method), replacing k_chain role 2 ([r] sig per set,
// ~1.6k Fp products) and the k_gsum levels in the merged-check path.
//
// Scalars: the set's batch scalar is r_i = a_i + b_i mu (curve.hpp glv_split / jac_mul_glv:
// a, b the two 32-bit halves of set_scalar, mu = -x^2 with [mu]Q = -psi^2(Q) on G2), so
//   S = sum_i [a_i] sig_i + [b_i] mu(sig_i):
// 2 n affine points with 32-bit scalars, four 8-bit windows, 255 buckets per window.
//
//   k_msm_bin      one lane per set: its 8 (window, digit) entries, bucket slot by atomic
//                  count; the last workgroup to finish (ticket) turns the counts into
//                  bucket and level-0 segment offsets and zeroes them for the next pass
//   k_msm_scatter  one lane per set: point references into bucket order
//   k_msm_seg      one lane per segment of <= seg points of one bucket: mixed additions
//   k_msm_bucket   one lane per bucket: the sum of its segments
//   k_msm_window   one wavefront per window: T_w = sum_d d B_{w,d} from per-lane running
//                  sums of 4 buckets, a suffix scan and a tree over the lanes in LDS,
//                  then [2^(8w)] T_w; the last window to finish (ticket) sums the four
//                  into the pass's signature sum and writes the chunk groups' virtual
//                  sets (group 0 the sum, the others infinity: f = 1; vset_write)
// Each fused step saves a dispatch: under load a one-wave kernel waits milliseconds for
// a free slot among the other passes' long waves (profiles/r03_ab_streams.json).
// The counters and tickets live in a per-context buffer zeroed once (MsmBufs::cnt).
//
// The stage bodies are bls/msm.hpp's.  These five launches one after the other are the
// serial form (launch_k_msm).  The overlapped form keeps k_msm_bin and k_msm_scatter here
// (launch_k_msm_sort) and runs the segment, bucket, window and final stages as roles of
// the first pass's Miller-loop launches, whose own items do not need the sum
// (kernels/k_mlq.hip launch_k_mlqf_msm).
//
// Work per pass of n sets: ~8 n mixed additions (29 Fp products each) + n/seg * ... + a
// fixed ~4k additions for the windows -- ~300 Fp products per set against ~1.6k for the
// per-set [r] sig chains.  The per-set RS are still produced (k_chain role 2 alone) when
// the merged check fails and the chunks' own sums are needed (bls_gpu.hip ensure_rs).
#define BLS_FP_D28 1
#include "../launchers.hpp"
#include "bls/msm.hpp"

using namespace bls;

__global__ __launch_bounds__(BLS_BLOCK) void k_msm_bin(PipeBufs b, MsmBufs m, uint32_t seg) {
  BLS_TAIL_PRIO();
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i < b.n_sets) msm_bin_lane(b, m, i);
  if (!msm_last_block(m.ticket, gridDim.x)) return;
  // the scan, one wavefront: lane t owns buckets [16 t, 16 t + 16); off[k] = sum_{j<k}
  // cnt[j], seg_off likewise over ceil(cnt / seg) segments per bucket
  __shared__ uint32_t a[64], c[64];
  const uint32_t t = threadIdx.x, k0 = 16u * t;
  uint32_t sa = 0, sc = 0;
  for (uint32_t k = k0; k < k0 + 16u && k < MSM_NB; ++k) {
    const uint32_t n = __hip_atomic_load(&m.cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sa += n;
    sc += (n + seg - 1) / seg;
  }
  a[t] = sa;
  c[t] = sc;
  __syncthreads();
  for (uint32_t off = 1; off < 64; off <<= 1) {  // inclusive Hillis-Steele scan
    const uint32_t x = t >= off ? a[t - off] : 0u, y = t >= off ? c[t - off] : 0u;
    __syncthreads();
    a[t] += x;
    c[t] += y;
    __syncthreads();
  }
  uint32_t pa = a[t] - sa, pc = c[t] - sc;  // exclusive prefixes of this lane's buckets
  for (uint32_t k = k0; k < k0 + 16u && k < MSM_NB; ++k) {
    const uint32_t n = __hip_atomic_load(&m.cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m.off[k] = pa;
    m.seg_off[k] = pc;
    pa += n;
    pc += (n + seg - 1) / seg;
    __hip_atomic_store(&m.cnt[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // zero for the next pass
  }
  if (t == 63) {
    m.off[MSM_NB] = a[63];
    m.seg_off[MSM_NB] = c[63];
  }
}

__global__ __launch_bounds__(BLS_BLOCK) void k_msm_scatter(PipeBufs b, MsmBufs m) {
  BLS_TAIL_PRIO();
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i < b.n_sets) msm_scatter_lane(m, i);
}

// two wavefronts per SIMD (256 VGPRs, 864 B/lane of scratch) rather than the one that
// 352 registers gave: cfg2 +0.6 % in five alternated pairs, the signature-sum stage
// ~0.7 ms shorter (profiles/r06_ab_msm_occ.json)
#ifndef BLS_MSM_WAVES
#define BLS_MSM_WAVES 2
#endif
__global__ __launch_bounds__(BLS_BLOCK) __attribute__((amdgpu_waves_per_eu(BLS_MSM_WAVES))) void k_msm_seg(PipeBufs b, MsmBufs m, uint32_t seg) {
  BLS_TAIL_PRIO();
  msm_seg_lane(b, m, seg, blockIdx.x * BLS_BLOCK + threadIdx.x);
}

__global__ __launch_bounds__(BLS_BLOCK) void k_msm_bucket(MsmBufs m) {
  BLS_TAIL_PRIO();
  msm_bucket_lane(m, blockIdx.x * BLS_BLOCK + threadIdx.x);
}

// one wavefront per window w (a 256-lane workgroup waited for a whole free CU under
// load; the steps: bls/msm.hpp msm_window_wave); the last window to finish sums the four
__global__ __launch_bounds__(64) void k_msm_window(PipeBufs b, MsmBufs m, uint32_t groups, uint32_t vbase) {
  BLS_TAIL_PRIO();
  __shared__ G2J L[MSM_LANES];
  msm_window_wave(m, blockIdx.x, L);
  if (!msm_last_block(m.ticket + 1, gridDim.x)) return;
  msm_final_lane(b, m, threadIdx.x, groups, vbase);
}

size_t msm_seg_cap(uint32_t n_sets) { return (8ull * n_sets) / msm_seg_len(n_sets) + MSM_NB + 1; }

hipError_t launch_k_msm_sort(const PipeBufs& b, const MsmBufs& m, hipStream_t s) {
  const uint32_t n = b.n_sets;
  if (n == 0) return hipErrorInvalidValue;
  k_msm_bin<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(b, m, msm_seg_len(n));
  k_msm_scatter<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(b, m);
  return hipGetLastError();
}

hipError_t launch_k_msm(const PipeBufs& b, const MsmBufs& m, uint32_t groups, uint32_t vbase, hipStream_t s) {
  const uint32_t n = b.n_sets;
  const hipError_t e = launch_k_msm_sort(b, m, s);
  if (e != hipSuccess) return e;
  k_msm_seg<<<bls_grid_for((uint32_t)msm_seg_cap(n)), BLS_BLOCK, 0, s>>>(b, m, msm_seg_len(n));
  k_msm_bucket<<<bls_grid_for(MSM_NB), BLS_BLOCK, 0, s>>>(m);
  k_msm_window<<<MSM_W, 64, 0, s>>>(b, m, groups, vbase);
  return hipGetLastError();
}
