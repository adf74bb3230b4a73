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
#define BLS_AGG_WAVE_MIN 16u  // aggregate sets of at least this many keys: k_pk_agg
// k_msm_bin: 22-bit bucket slots, <= 2 entries per set and bucket
#define MSM_MAX_SETS (1u << 21)
// items per k_mlf lane (bls/knobs.hpp mlf_per_lane): one item per TWO f lanes (kernels/k_mlq.hip k_mlf2)
#define MLF_PAIR 3u
