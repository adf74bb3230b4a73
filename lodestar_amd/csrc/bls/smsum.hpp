// Same-message jobs (bls_gpu_verify_same_message): the reduction that turns one job's
// [r_i] pk_i and [r_i] sig_i (b.chain, CH_RP / CH_RS, after k_chain) into the job's two
// pairing inputs in one step, shared by kernels/k_smsg.hip (k_smsum: one wavefront per
// job, the scratch array in LDS, a barrier between the steps) and its CPU restatement
// (tests/native/smsum_host.cpp, which loops the lanes of each step).
//
//   smsum_partial   lane l of `lanes` sums the job's live sets l, l + lanes, ...
//   smsum_step      one level of the tree over the lanes' partial sums in `scratch`:
//                   lane l < half adds scratch[l + half] into scratch[l]
//   smsum_tree      (host) the levels half = lanes / 2 .. 1, the order the kernel runs
//   smsum_finish    lane 0: the job's unit (RP = sum r_i pk_i, HQ of the root's
//                   representative set) and its virtual set (affine sum r_i sig_i,
//                   RP = -g1; vset_write), a sum at infinity giving f = 1 and not live
//                   as k_uset / vset_write do
// The additions are curve.hpp's complete jac_add, so equal, opposite and infinity
// partial sums need no special path.
#pragma once

#include "pipeline.hpp"

namespace bls {

// one out-of-line copy of each group's addition per kernel (the pattern of
// kernels/k_gsum.hip g2_add_p: the body is large)
#if defined(__HIPCC__)
#define BLS_SMSUM_ADD __host__ __device__ __noinline__
#else
#define BLS_SMSUM_ADD static inline
#endif
template <class F>
BLS_SMSUM_ADD void smsum_add(Jac<F>* acc, const Jac<F>* p) {
  *acc = jac_add(*acc, *p);
}

// the point at word `at` (CH_RP: G1 Jacobian, CH_RS: G2 Jacobian) of set i's chain entry
template <class F>
BLS_HD Jac<F> smsum_load(const Fp* chain, uint32_t i, int at) {
  Jac<F> p;
  const Fp* c = chain + (size_t)CHAIN_WORDS * i + at;
  Fp* d = reinterpret_cast<Fp*>(&p);
  for (int k = 0; k < (int)(sizeof(Jac<F>) / sizeof(Fp)); ++k) d[k] = c[k];
  return p;
}

// sets[beg, end): the job's sets; lanes: the stride (a power of two)
template <class F>
BLS_HD Jac<F> smsum_partial(const Fp* chain, const uint32_t* chain_live, const uint32_t* sets, uint32_t beg,
                            uint32_t end, uint32_t lane, uint32_t lanes, int at) {
  Jac<F> acc = jac_infinity<F>();
  for (uint32_t k = beg + lane; k < end; k += lanes) {
    const uint32_t i = sets[k];
    if (!chain_live[i]) continue;
    const Jac<F> p = smsum_load<F>(chain, i, at);
    smsum_add(&acc, &p);
  }
  return acc;
}

template <class F>
BLS_HD void smsum_step(Jac<F>* scratch, uint32_t lane, uint32_t half) {
  if (lane < half) smsum_add(&scratch[lane], &scratch[lane + half]);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the whole tree on the host: scratch[0] = the sum of scratch[0, lanes)
template <class F>
static inline void smsum_tree(Jac<F>* scratch, uint32_t lanes) {
  for (uint32_t half = lanes / 2; half; half >>= 1)
    for (uint32_t lane = 0; lane < lanes; ++lane) smsum_step(scratch, lane, half);
}
#endif

// job c of the call: unit b.unit_base + c and virtual set b.n_sets + c
BLS_HD void smsum_finish(const PipeBufs& b, uint32_t c, const G1J& rp, const G2J& rs, uint32_t rep) {
  const uint32_t v = b.unit_base + c;
  if (jac_is_inf(rp)) {  // no live set (errors, exact path) or a cancelling sum: f = 1
    b.chain_live[v] = 0u;
    Fp* d = reinterpret_cast<Fp*>(&b.f[v]);
    d[0] = c_one();
    for (int k = 1; k < 12; ++k) d[k] = fp_zero();
  } else {
    Fp* o = b.chain + (size_t)CHAIN_WORDS * v;
    const Fp* h = b.chain + (size_t)CHAIN_WORDS * rep + CH_HQ;
    for (int k = 0; k < 4; ++k) o[CH_HQ + k] = h[k];
    o[CH_RP + 0] = rp.x;
    o[CH_RP + 1] = rp.y;
    o[CH_RP + 2] = rp.z;
    b.chain_live[v] = 1u;
  }
  vset_write(b, rs, b.n_sets + c);
}

}  // namespace bls
