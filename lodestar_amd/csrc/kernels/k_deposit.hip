// Front kernel of a deposit call (bls_gpu_verify_deposits): takes k_pk's place in the
// verify pass.  Per deposit it decompresses and KeyValidates the untrusted 48-byte key
// into b.pk / b.pk_status (stage_deposit_pk) and computes the DepositMessage signing root
// into the pass's message buffer (stage_deposit_root); bls/deposit.hpp holds both bodies.
//
// Two roles, one per wavefront (as k_chain's roles): blocks [0, ceil(n / 64)) validate keys
// -- one Fp square root and Scott's test, ~1.7k dependent Fp products, the stage's latency
// -- and the blocks behind them hash roots, 10 SHA-256 compressions each, which hide under
// the Fp chains; no wavefront mixes the two instruction streams.  k_deposit_fused is the
// plain shape, one lane per deposit doing both ($BLS_DEPOSIT_FUSED=1), kept for the A/B of
// DESIGN.md section 7k.
//
// Like k_pk it is the first kernel of its pass, so it also resets the call's device-side
// words: set_flag, flag_count and the next call's first_bad_pk slot.
#include <stdlib.h>

#include "../bls/deposit.hpp"
#include "../launchers.hpp"

using namespace bls;

namespace {

__device__ __forceinline__ void deposit_resets(const PipeBufs& b, uint32_t i) {
  if (i < b.n_sets) b.set_flag[i] = b.init_set_flag;
  if (i == 0) {
    *b.flag_count = 0u;
    if (b.first_bad_pk_next) *b.first_bad_pk_next = 0xFFFFFFFFu;
  }
}

__device__ __forceinline__ void deposit_root(const PipeBufs& b, const DepositBufs& d, uint32_t i) {
  if (i >= b.n_sets) return;
  stage_deposit_root(d.pubkeys48 + 48ull * i, d.wc + 32ull * i, d.amounts + 8ull * i, d.domain, d.roots + 32ull * i);
}

}  // namespace

__global__ __launch_bounds__(BLS_BLOCK) void k_deposit(PipeBufs b, DepositBufs d) {
  const uint32_t key_blocks = (b.n_sets + BLS_BLOCK - 1) / BLS_BLOCK;
  if (blockIdx.x < key_blocks) {
    const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
    deposit_resets(b, i);
    stage_deposit_pk(b, d, i);
  } else {
    deposit_root(b, d, (blockIdx.x - key_blocks) * BLS_BLOCK + threadIdx.x);
  }
}

__global__ __launch_bounds__(BLS_BLOCK) void k_deposit_fused(PipeBufs b, DepositBufs d) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  deposit_resets(b, i);
  deposit_root(b, d, i);
  stage_deposit_pk(b, d, i);
}

hipError_t launch_k_deposit(const PipeBufs& b, const DepositBufs& d, hipStream_t s) {
  // read per launch: the A/B tool alternates the two shapes in one process
  const char* e = getenv("BLS_DEPOSIT_FUSED");
  if (e && e[0] == '1') k_deposit_fused<<<bls_grid_for(b.n_sets), BLS_BLOCK, 0, s>>>(b, d);
  else k_deposit<<<2 * bls_grid_for(b.n_sets), BLS_BLOCK, 0, s>>>(b, d);
  return hipGetLastError();
}
