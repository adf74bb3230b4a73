// Same-message jobs (bls_gpu_verify_same_message), the first pass's sums:
//
//   k_smsum  one wavefront per job (chunk c of the call's plan; its sets are
//            b.chunk_reqs[b.chunk_off[c] .. b.chunk_off[c + 1]), every request one set).
//            Lane l sums the job's live sets l, l + 64, .. from b.chain (CH_RP as G1
//            Jacobian, then CH_RS as G2 Jacobian), the 64 partial sums are reduced in six
//            steps through LDS, and lane 0 writes the job's Miller-loop unit
//            (e(sum r_i pk_i, H(root))) and its virtual set (e(-g1, sum r_i sig_i)):
//            the job's two pairing inputs.  It replaces, for these calls, the k_gsum /
//            k_vset and k_gsum1 / k_uset levels (kernels/k_gsum.hip): about ten
//            dependent launches of single-lane additions for a 128-set job.
//
// The two groups are reduced one after the other in the same 18 KB of LDS (64 G2
// Jacobian points; the G1 sums take its first half).  The body is bls/smsum.hpp, shared
// with the CPU restatement under tests/native/.
#define BLS_FP_INLINE 1
#include "../bls/smsum.hpp"
#include "../launchers.hpp"

using namespace bls;

#define SMSUM_LANES 64u
static_assert(SMSUM_LANES == BLS_BLOCK, "k_smsum: one wavefront per job");

__global__ __launch_bounds__(BLS_BLOCK) void k_smsum(PipeBufs b, const uint32_t* unit_rep) {
  BLS_TAIL_PRIO();
  __shared__ G2J sh2[SMSUM_LANES];
  G1J* sh1 = reinterpret_cast<G1J*>(sh2);
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  if (c >= b.n_chunks) return;  // (uniform over the block)
  const uint32_t beg = b.chunk_off[c], end = b.chunk_off[c + 1];

  sh1[lane] = smsum_partial<Fp>(b.chain, b.chain_live, b.chunk_reqs, beg, end, lane, SMSUM_LANES, CH_RP);
  __syncthreads();
  for (uint32_t half = SMSUM_LANES / 2; half; half >>= 1) {
    smsum_step(sh1, lane, half);
    __syncthreads();
  }
  G1J rp = jac_infinity<Fp>();
  if (lane == 0) rp = sh1[0];
  __syncthreads();

  sh2[lane] = smsum_partial<Fp2>(b.chain, b.chain_live, b.chunk_reqs, beg, end, lane, SMSUM_LANES, CH_RS);
  __syncthreads();
  for (uint32_t half = SMSUM_LANES / 2; half; half >>= 1) {
    smsum_step(sh2, lane, half);
    __syncthreads();
  }
  if (lane == 0) smsum_finish(b, c, rp, sh2[0], unit_rep[c]);
}

// one unit per chunk: b.n_units == b.n_chunks (bls_gpu.hip plan_same_message)
hipError_t launch_k_smsum(const PipeBufs& b, const uint32_t* unit_rep, hipStream_t s) {
  if (b.n_chunks == 0) return hipSuccess;
  if (b.n_units != b.n_chunks) return hipErrorInvalidValue;
  k_smsum<<<b.n_chunks, BLS_BLOCK, 0, s>>>(b, unit_rep);
  return hipGetLastError();
}
