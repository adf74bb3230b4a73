// Host-side launchers, one per kernel translation unit (lodestar_amd/csrc/kernels/*.hip).
// Each heavy kernel lives in its own TU so the build compiles them in parallel.
#pragma once

#include <hip/hip_runtime.h>

#include "bls/pipeline.hpp"
#include "bls/plan_shape.hpp"

#define BLS_BLOCK 64

// Serial tails of a pass (signature sums, their affine form, the product tree and the
// final exponentiations, status) run few wavefronts whose chains set the pass latency;
// with other passes' wide kernels on the same SIMDs they raise their wave priority so the
// SIMD issues them first (s_setprio 3; +3.6 % at 4 x 16, profiles/r03_ab_tail_prio.json).
#define BLS_TAIL_PRIO() __builtin_amdgcn_s_setprio(3)

static inline unsigned bls_grid_for(uint32_t n) { return (n + BLS_BLOCK - 1) / BLS_BLOCK; }

hipError_t launch_k_pk(const bls::PipeBufs& b, hipStream_t s);
hipError_t launch_k_pk_agg(const bls::PipeBufs& b, hipStream_t s);
// committee sets (bls/committee.hpp): b.bits_sets' sums, and a group's totals at registration
hipError_t launch_k_pk_bits(const bls::PipeBufs& b, hipStream_t s);
hipError_t launch_k_pk_span(const bls::PipeBufs& b, hipStream_t s);  // b.span_sets' sums
hipError_t launch_k_committee_totals(const bls::CommitteeGroupDev& grp, bls::G1J* totals, const bls::G1A* table,
                                     uint32_t table_n, hipStream_t s);
hipError_t launch_k_aggregate(const bls::PipeBufs& b, uint8_t* out96, hipStream_t s);
hipError_t launch_k_load_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len, bls::G1A* out, int32_t* codes,
                                 hipStream_t s);
// comb rows of n table keys (curve.hpp g1_comb_build): tmp = 15 n G1J of workspace
hipError_t launch_k_comb_build(const bls::G1A* keys, uint32_t n, bls::G1J* tmp, bls::Fp* rows, uint8_t* ok,
                               hipStream_t s);
hipError_t launch_k_status(const bls::PipeBufs& b, hipStream_t s);
hipError_t launch_k_validate_pubkeys(const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes, hipStream_t s);
// the front kernel of a deposit call, in k_pk's place (kernels/k_deposit.hip, bls/deposit.hpp)
namespace bls {
struct DepositBufs;
}
hipError_t launch_k_deposit(const bls::PipeBufs& b, const bls::DepositBufs& d, hipStream_t s);
hipError_t launch_k_pre(const bls::PipeBufs& b, hipStream_t s);
hipError_t launch_k_exact(const bls::PipeBufs& b, hipStream_t s);
// roles: bit k runs k_chain role k (0 H, 1 subgroup, 2 [r] sig, 3 [r] pk); k_chain_done
// follows unless only role 2 runs (the merged check's fallback needs the per-set RS)
hipError_t launch_k_chain(const bls::PipeBufs& b, hipStream_t s, uint32_t roles = 0xFu);
// Pippenger sum of [r_i] sig_i over the live sets (kernels/k_msm.hip; stage bodies in bls/msm.hpp)
#include "bls/msm_bufs.hpp"
using bls::MsmBufs;
#define MSM_BUCKETS 1020u
size_t msm_seg_cap(uint32_t n_sets);
// bucket counts, then the tickets: k_msm_bin's, the windows', one per window's bucket blocks
#define MSM_STATE_WORDS (MSM_BUCKETS + 6u)
static_assert(MSM_BUCKETS == bls::MSM_NB && MSM_STATE_WORDS == bls::MSM_NB + bls::MSM_TICKETS, "bls/msm_bufs.hpp");
// the merged signature sum into the chunk groups' virtual sets vbase .. vbase + groups:
// the serial form, five launches
hipError_t launch_k_msm(const bls::PipeBufs& b, const MsmBufs& m, uint32_t groups, uint32_t vbase, hipStream_t s);
// ... and its first two alone (k_msm_bin, k_msm_scatter) for the overlapped form
hipError_t launch_k_msm_sort(const bls::PipeBufs& b, const MsmBufs& m, hipStream_t s);
// The overlapped form (kernels/k_mlq.hip): the first pass's Miller loops of the sets
// [0, n_sets) and the units [n_sets + groups, n_sets + groups + n_units) in k_mlq's and
// k_mlf<1>'s bodies, with the sum's segment stage on the lowest blocks of the line-side
// launch and its bucket, window and final stages on the lowest 16 blocks of the f-side
// launch; the virtual sets n_sets .. n_sets + groups exist when the f-side launch ends (the
// caller pairs them after it).  b.mlf_pl = 1, 2 or 4 (hipErrorInvalidValue otherwise).
hipError_t launch_k_mlqf_msm(const bls::PipeBufs& b, const MsmBufs& m, uint32_t groups, uint32_t n_units,
                             uint32_t* lines, hipStream_t s);
hipError_t launch_k_gsum(const bls::PipeBufs& b, const uint32_t* seg, uint32_t n_seg, const bls::G2J* in,
                         bls::G2J* out, hipStream_t s);
hipError_t launch_k_vset(const bls::PipeBufs& b, const bls::G2J* sums, uint32_t n_groups, uint32_t vbase,
                         hipStream_t s);
hipError_t launch_k_gsum1(const bls::PipeBufs& b, const uint32_t* seg, uint32_t n_seg, const bls::G1J* in,
                          bls::G1J* out, hipStream_t s);
hipError_t launch_k_uset(const bls::PipeBufs& b, const bls::G1J* sums, const uint32_t* unit_rep, hipStream_t s);
// same-message jobs (kernels/k_smsg.hip): chunk c's sum r_i pk_i -> unit b.unit_base + c and
// sum r_i sig_i -> virtual set b.n_sets + c, one wavefront per chunk (one unit per chunk)
hipError_t launch_k_smsum(const bls::PipeBufs& b, const uint32_t* unit_rep, hipStream_t s);
hipError_t launch_k_hash_to_g2(const uint8_t* msgs, uint32_t n, uint8_t* out192, hipStream_t s);
hipError_t launch_k_sig_aggregate(const uint8_t* in96, uint32_t n, const uint32_t* off, uint32_t n_lists,
                                  bls::G2A* pts, int32_t* sig_codes, uint8_t* out96, int32_t* codes, hipStream_t s);
hipError_t launch_k_g2_decompress(const uint8_t* in96, uint32_t n, int validate, uint8_t* out192, int32_t* codes,
                                  hipStream_t s);
hipError_t launch_k_ssz_roots(uint32_t kind, const uint8_t* objs, uint32_t n, const uint8_t* domains,
                              uint32_t domain_stride, uint8_t* out32, hipStream_t s);
bool ssz_kind_known(uint32_t kind);
hipError_t launch_k_sk_to_pk(const uint8_t* sks, uint32_t n, uint8_t* out48, hipStream_t s);
hipError_t launch_k_sign(const uint8_t* sks, const uint8_t* msgs, uint32_t n, uint8_t* out96, hipStream_t s);
hipError_t launch_k_mad_peak(uint64_t* out, uint32_t blocks, uint32_t iters, hipStream_t s);
hipError_t launch_k_fp_mul_test(const uint8_t* a, const uint8_t* b, uint32_t n, uint8_t* out, hipStream_t s);
// field-op self-test (kernels/field_ops.hpp): op = base id | FOP_D28_FLAG for the
// 28-bit-digit translation unit; field_op_shape: record sizes in words, -2 unknown op
int field_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);
hipError_t launch_k_field_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s);
hipError_t launch_k_field_op_d28(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s);
// curve-op self-test (kernels/curve_ops.hpp): op = base id | COP_D28_FLAG; curve_op_shape:
// record sizes in words, -2 for an unknown op or a flavour the op does not exist in;
// ws: curve_op_ws_bytes(op, n) of zeroed device memory (COP_CHAIN_H's chain rows and bytes)
int curve_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);
size_t curve_op_ws_bytes(uint32_t op, uint32_t n);
hipError_t launch_k_curve_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, void* ws, hipStream_t s);
hipError_t launch_k_curve_op_d28(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s);
hipError_t launch_k_curve_op_chain(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, void* ws,
                                   hipStream_t s);
// tower-op self-test (kernels/tower_ops.hpp): op = base id | TOP_D28_FLAG; tower_op_shape:
// record sizes in words, -2 for an unknown op or a flavour the op does not exist in.  The
// _fin and _mlq launchers run the file-local functions of kernels/k_fin_simt.hip and
// kernels/k_mlq.hip; launch_k_mlq_lines is k_mlq<1> alone over items [0, count), each its
// own (launch_k_mlqf's first launch, units not paired)
int tower_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);
hipError_t launch_k_tower_op(uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s);
hipError_t launch_k_tower_op_d28(uint32_t op, const bls::Fp* in, uint32_t n, bls::Fp* out, hipStream_t s);
hipError_t launch_k_tower_op_fin(uint32_t op, const bls::Fp* in, uint32_t n, bls::Fp* out, hipStream_t s);
hipError_t launch_k_tower_op_mlq(uint32_t op, const bls::Fp* in, uint32_t n, bls::Fp* out, hipStream_t s);
hipError_t launch_k_mlq_lines(const bls::PipeBufs& b, uint32_t count, uint32_t* lines, hipStream_t s);
hipError_t launch_k_fpm_chain(bls::Fp* io, uint32_t lanes, uint32_t iters, hipStream_t s);
size_t kernel_probe_out_bytes(const char* name);
hipError_t launch_kernel_probe(const char* name, void* out, uint32_t lanes, hipStream_t s);
#include "bls/coop.hpp"
hipError_t launch_k_chunk_coop(const bls::PipeBufs& b, const bls::CoopEnv& env, hipStream_t s);
hipError_t launch_k_indiv_coop(const bls::PipeBufs& b, const bls::CoopEnv& env, const bls::GroupBufs& g,
                              hipStream_t s);
hipError_t launch_k_group_coop(const bls::PipeBufs& b, const bls::CoopEnv& env, const bls::GroupBufs& g,
                              hipStream_t s);
hipError_t launch_k_fold(const bls::PipeBufs& b, const bls::CoopEnv& env, const uint32_t* groups, uint32_t n_groups,
                         uint32_t step, hipStream_t s);
// SIMT final exponentiations, one lane per chunk / request (kernels/k_fin_simt.hip), for
// a failing pass's many tasks: save = 4 Fp12 of device memory per task
hipError_t launch_k_chunk_simt(const bls::PipeBufs& b, bls::Fp12* save, hipStream_t s);
hipError_t launch_k_indiv_simt(const bls::PipeBufs& b, const bls::GroupBufs& g, bls::Fp12* save, hipStream_t s);
hipError_t launch_k_coop_probe(const bls::CoopEnv& env, bls::CoopProg pg, uint32_t blocks, uint32_t reps,
                               uint32_t* sink, uint64_t* stamps, hipStream_t s);
// test: run program pg once on n_frames caller frames of `frame` slots (the program's own
// frame size: 256, COOP_FRAME2 or COOP_FRAME3), two wavefronts per frame when w2
hipError_t launch_k_coop_run_test(const bls::CoopEnv& env, bls::CoopProg pg, uint32_t frame, bool w2,
                                  const bls::Fp* in, uint32_t n_frames, bls::Fp* out, uint32_t* flags, hipStream_t s);
#define FPROD_FAN 16u
hipError_t launch_k_fprod(const bls::Fp12* in, uint32_t n, bls::Fp12* out, int32_t* verdict,
                          const bls::CoopEnv& env, hipStream_t s);
hipError_t launch_k_pset(const bls::PipeBufs& b, const bls::CoopEnv& env, hipStream_t s);
hipError_t launch_k_mln(const bls::PipeBufs& b, const bls::CoopEnv& env, uint32_t first, uint32_t count,
                        hipStream_t s, bool own_only = false);
// own Miller loops of the listed items (items[0, count)) in one launch: the split SIMT
// kernels only (k_mln_list_ok); the individually verified pass uses it for every set of
// the failed chunks at once
bool k_mln_list_ok(const bls::PipeBufs& b);
hipError_t launch_k_mln_list(const bls::PipeBufs& b, const uint32_t* items, uint32_t count, hipStream_t s);
// cooperative single-pair loops of [first, first + count) or of items[0, count), one
// wavefront each, for a failing pass's later launches; hipErrorNotSupported above
// $BLS_COOP_ML_MAX items (kernels/k_pset.hip)
hipError_t launch_k_mln_coop(const bls::PipeBufs& b, const bls::CoopEnv& env, uint32_t first, uint32_t count,
                             const uint32_t* items, hipStream_t s);
size_t mlq_line_words(uint32_t count);
// sets in the verify calls currently running in this process (every context)
uint64_t bls_sets_in_flight();
hipError_t launch_k_mlqf(const bls::PipeBufs& b, uint32_t first, uint32_t count, bool own_only, uint32_t* lines,
                         hipStream_t s, const uint32_t* items = nullptr);
