// Constants that fix the shape of a pass's host-side plans (bls/plan.hpp) and that the
// kernels reading those plans share: one definition for both sides.
#pragma once

#define GSUM_FAN 4u   // points per k_gsum segment (a 16-set chunk: two levels of 3 additions)
#define BLS_FOLD 16u  // sets per k_fold group (what k_indiv strides by)
#define BLS_FOLD1 4u  // sets per first-level k_fold group
#define UNIT_NONE 0xFFFFFFFFu  // PipeBufs::set_unit: the set runs its own Miller loop
// GroupBufs::ref[g]: REF_CHUNK | c = compare with chunk c's checked value ref_fe[c]
#define REF_CHUNK 0x80000000u
#define REF_NONE 0xFFFFFFFFu  // no comparison (the chunk indices stay far below 2^31 - 1)
