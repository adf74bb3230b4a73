// The Pippenger signature sum's buffers and sizes (kernels/k_msm.hip): what the host code
// and the launchers need.  The stage bodies are in bls/msm.hpp, which only the kernels that
// run them and the host test include.
#pragma once

#include "curve.hpp"

namespace bls {

struct MsmBufs {
  uint32_t* cnt;      // 1020 bucket counts + the tickets: per context, zero between passes
  uint32_t* ticket;   // cnt + 1020: [0] k_msm_bin, [1] the windows, [2 + w] window w's bucket blocks
  uint32_t* off;      // 1021 bucket offsets into sorted
  uint32_t* seg_off;  // 1021 segment offsets
  uint32_t* ent;      // 8 n_sets (bucket << 22 | slot) entries
  uint32_t* sorted;   // 8 n_sets point references in bucket order
  G2J* seg_sum;       // msm_seg_cap(n_sets)
  G2J* bucket;        // 1020
  G2J* win;           // 4
};

constexpr uint32_t MSM_W = 4, MSM_D = 255, MSM_NB = MSM_W * MSM_D;
constexpr uint32_t MSM_LANES = 64;       // lanes of a block
constexpr uint32_t MSM_BKT_BLOCKS = 4;   // bucket blocks per window: 4 x 64 lanes for its 255 buckets
constexpr uint32_t MSM_ENT_NONE = 0xFFFFFFFFu;
constexpr uint32_t MSM_TICKETS = 2 + MSM_W;

}  // namespace bls
