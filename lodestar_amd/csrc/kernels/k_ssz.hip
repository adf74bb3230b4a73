// SSZ signing roots on the GPU (the step before the verify path):
// computeSigningRoot(type, obj, domain) = hash_tree_root(SigningData{hash_tree_root(obj),
// domain}) (state-transition/src/util/signingRoot.ts:7-13) for the fixed-size containers
// the signature-set producers sign (state-transition/src/signatureSets/*.ts).
//
// One lane per object.  An object's leaves are 32-byte chunks of its serialization
// (integers little-endian, zero padded) or nested container roots; every internal node
// is one 64-byte SHA-256 input = two compressions, the second over the constant padding
// block.  The work is a few dozen compressions per object -- latency-bound integer ALU
// work, no HBM pressure (<= 160 B in, 32 B out per object).
#include "../bls/ssz_tree.hpp"
#include "../launchers.hpp"

using namespace bls;

__global__ __launch_bounds__(BLS_BLOCK) void k_ssz_roots(uint32_t kind, const uint8_t* objs, uint32_t n,
                                                         const uint8_t* domains, uint32_t domain_stride,
                                                         uint8_t* out32) {
  const uint32_t i = blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  bool ok;
  Chunk r = object_root(kind, objs + (size_t)BLS_SSZ_SIZE(kind) * i, ok);
  if (domains) r = hash_pair(r, load_chunk(domains + (size_t)domain_stride * i, 32));
  store_chunk(r, out32 + 32ull * i);
}

bool ssz_kind_known(uint32_t kind) {
  switch (kind) {
    case BLS_SSZ_ROOT:
    case BLS_SSZ_UINT64:
    case BLS_SSZ_CHECKPOINT:
    case BLS_SSZ_ATTESTATION_DATA:
    case BLS_SSZ_TWO_UINT64:
    case BLS_SSZ_BEACON_BLOCK_HEADER:
    case BLS_SSZ_DEPOSIT_MESSAGE:
    case BLS_SSZ_FORK_DATA:
    case BLS_SSZ_SIGNING_DATA:
      return true;
    default:
      return false;
  }
}

hipError_t launch_k_ssz_roots(uint32_t kind, const uint8_t* objs, uint32_t n, const uint8_t* domains,
                              uint32_t domain_stride, uint8_t* out32, hipStream_t s) {
  k_ssz_roots<<<bls_grid_for(n), BLS_BLOCK, 0, s>>>(kind, objs, n, domains, domain_stride, out32);
  return hipGetLastError();
}
