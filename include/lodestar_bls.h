/*
 * lodestar_bls.h -- C-ABI of the MI355X BLS12-381 signature-set verifier.
 *
 * Drop-in boundary for Lodestar's BLS verification hot path.  The reference
 * crosses JS -> native inside @chainsafe/blst (SWIG N-API, [ext]); the seam this
 * library replaces is the worker RPC
 *     WorkerApi.verifyManySignatureSets(BlsWorkReq[]) -> BlsWorkResult
 * (packages/beacon-node/src/chain/bls/multithread/index.ts:59-61, worker.ts:26-108,
 *  types.ts:8-38), which sits behind
 *     IBlsVerifier.verifySignatureSets(sets, opts) (chain/bls/interface.ts:20-46).
 * The N-API binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes; the caller owns every buffer for the
 * duration of the call (the library copies into pinned staging); no call throws
 * across the ABI -- functions return 0 on success and a negative value on a
 * runtime failure (message via bls_gpu_last_error).  Per-request verdicts use
 *     1 = valid, 0 = invalid, < 0 = -(BLST-style error code)
 * with the codes below (values 1..7 follow blst's BLST_ERROR enum).
 */
#ifndef LODESTAR_BLS_H
#define LODESTAR_BLS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  BLS_CODE_OK = 0,
  BLS_CODE_BAD_ENCODING = 1,         /* "BLST_BAD_ENCODING" */
  BLS_CODE_POINT_NOT_ON_CURVE = 2,   /* "BLST_POINT_NOT_ON_CURVE" */
  BLS_CODE_POINT_NOT_IN_GROUP = 3,   /* "BLST_POINT_NOT_IN_GROUP" */
  BLS_CODE_PK_IS_INFINITY = 6,       /* "BLST_PK_IS_INFINITY" */
  BLS_CODE_INVALID_SIZE = 8,         /* "BLST_INVALID_SIZE" (multithread.test.ts:100) */
  BLS_CODE_ZERO_SIGNATURE = 9,       /* infinity signature on the 1-set path */
  BLS_CODE_EMPTY_SET = 10,           /* "Empty signature set" (maybeBatch.ts:29-31) */
  BLS_CODE_EMPTY_AGGREGATE = 11      /* "EMPTY_AGGREGATE_ARRAY" (PublicKey.aggregate([])) */
};

/* One verifyManySignatureSets() call: n_reqs BlsWorkReq, n_sets SerializedSet in
 * request order (types.ts:8-17).  Request r owns sets [req_set_offsets[r],
 * req_set_offsets[r+1]).  Public keys come either raw (96-byte uncompressed
 * affine, what index.ts:160 sends the worker) or as index lists into the
 * context's device-resident pubkey table (bls_gpu_load_pubkeys); an index list
 * of length k > 1 is an aggregate set, summed on the GPU (chain/bls/utils.ts:5-16). */
typedef struct bls_batch {
  uint32_t n_sets;
  uint32_t n_reqs;
  const uint32_t* req_set_offsets; /* n_reqs + 1 */
  const uint8_t* req_batchable;    /* n_reqs, 0/1 (VerifySignatureOpts.batchable) */
  const uint8_t* pubkeys;          /* n_sets * 96; used when set_pk_offsets == NULL */
  const uint32_t* set_pk_offsets;  /* n_sets + 1 into pk_indices, or NULL */
  const uint32_t* pk_indices;      /* device pubkey-table indices */
  const uint8_t* messages;         /* n_sets * 32 (signing roots) */
  const uint8_t* signatures;       /* n_sets * 96 (compressed G2; bytes past signature_lens[i] ignored) */
  const uint32_t* signature_lens;  /* n_sets, or NULL = all 96 */
  const uint8_t* seed;             /* 32 bytes for the random scalars, or NULL = fresh OS randomness */
} bls_batch;

/* BlsWorkResult bookkeeping (types.ts:26-38) */
typedef struct bls_stats {
  uint32_t batch_retries;      /* batchable chunks that failed and were re-verified per request */
  uint32_t batch_sigs_success; /* sets accepted by a successful batch */
  uint32_t n_chunks;           /* batchable chunks (chunkifyMaximizeChunkSize(reqs, 16)) */
  uint32_t n_individual;       /* requests verified on their own */
  uint32_t n_flagged;          /* sets finished by the exact single-lane path */
  double device_ms;            /* device time of the call (HIP events) */
  double stage_ms[8];          /* per stage (HIP events on the context's stream): h2d, pk, pre (SSWU + sig decode),
                                  k_chain (or k_pset), signature sums, Miller loops (k_mlq + k_mlf),
                                  status + merged / chunk checks, individual */
  uint32_t n_unique_msgs;      /* distinct signing roots hashed to the curve (== n_sets without dedup) */
  uint32_t merged_check;       /* 0 not run, 1 passed (per-chunk checks skipped), 2 failed (chunks checked),
                                  3 skipped: the context's previous pass failed it, chunks checked straight away */
  uint32_t n_ml_units;         /* Miller-loop units (chunk x shared signing root pairings), 0 = one per set */
  uint32_t pass_shape;         /* how the aggregated path ran (0 on the per-set path): bit 0 the merged signature
                                  sum by Pippenger MSM, bit 1 its long stages inside the Miller-loop launches
                                  (0: five launches in front of them); bits 8-15 items per lane of the f side of the Miller loops
                                  (1, 2, 4; 3 = one item per two lanes) */
} bls_stats;

typedef struct bls_gpu_ctx bls_gpu_ctx;

/* Number of visible HIP devices (0 when there is no GPU). */
int bls_gpu_device_count(void);

/* Create a verifier bound to one device (one process per GPU; the device index is
 * local to the process).  Replaces BlsMultiThreadWorkerPool's worker creation
 * (multithread/index.ts:199-233). */
int bls_gpu_init(int device, bls_gpu_ctx** out);

/* The same with a stream priority: BLS_PRIORITY_HIGH puts the context's kernels ahead
 * of normal-priority contexts' queued work on the device -- the latency lane of
 * verifyOnMainThread calls (multithread/index.ts:138-151: the reference runs them on the
 * main thread, outside the worker queue).  BLS_PRIORITY_NORMAL = bls_gpu_init.
 *
 * Both admit a context only while the scratch the HIP runtime reserves for the
 * process's contexts fits a budget (see bls_admission below); otherwise they return
 * BLS_ERR_ADMISSION without creating anything, and bls_gpu_init_error() says why.  Any
 * other failure returns -1 (-2 for bad arguments) with its message there too.  The
 * reference's pool likewise records a worker that fails to start and keeps the others
 * (multithread/index.ts:221-229). */
#define BLS_PRIORITY_NORMAL 0
#define BLS_PRIORITY_HIGH 1
#define BLS_ERR_ADMISSION (-4)
int bls_gpu_init_priority(int device, int priority, bls_gpu_ctx** out);

/* Message of the last failed bls_gpu_init / bls_gpu_init_priority on the calling thread
 * ("" after a successful one). */
const char* bls_gpu_init_error(void);

/* Scratch admission.  The HIP runtime backs each hardware queue with private-segment
 * memory for a full device of the deepest kernel dispatched on it and aborts the queues
 * (HSA_STATUS_ERROR_OUT_OF_RESOURCES, every call of the process failing) past ~8 GiB.
 * A process's streams of one priority map onto at most GPU_MAX_HW_QUEUES hardware
 * queues (HIP's default 4), per priority level, so
 *   queues_in_use    = min(contexts_normal, hw_queues) + min(contexts_high, hw_queues)
 *   scratch_reserved = queues_in_use x scratch_per_queue
 * where scratch_per_queue is the deepest verify-path kernel's reservation (scratch
 * bytes per lane x 64 x resident waves per SIMD x 1024 SIMDs, from the kernels' resource
 * usage at build time; bls_scratch_worst_kernel names it).  A context is admitted while
 * scratch_reserved <= scratch_budget (default 6 GiB; $BLS_SCRATCH_BUDGET_MIB or
 * bls_gpu_set_scratch_budget). */
typedef struct bls_admission {
  uint32_t contexts_normal, contexts_high; /* open contexts on the device */
  uint32_t hw_queues;                      /* the runtime's hardware queues per priority (below) */
  uint32_t queues_in_use;
  uint64_t scratch_per_queue, scratch_reserved, scratch_budget; /* bytes */
  uint32_t hw_queues_known;                /* 1: hw_queues is the runtime's count (the variable's value when the
                                              runtime initialised under this library's first context, or the
                                              caller's argument); 0: unknown -- HIP was initialised before that
                                              context, hw_queues is the variable's value now (4 when unset);
                                              2: no context yet, hw_queues is what the runtime will read */
} bls_admission;

/* The accounting alone (no device needed): 0 if n_normal + n_high contexts are
 * admissible with hw_queues hardware queues per priority (0 = $GPU_MAX_HW_QUEUES), else
 * BLS_ERR_ADMISSION; *out (nullable) receives the figures. */
int bls_scratch_plan(uint32_t n_normal, uint32_t n_high, uint32_t hw_queues, bls_admission* out);
/* The figures for the contexts open on `device` now. */
int bls_gpu_admission(int device, bls_admission* out);
const char* bls_scratch_worst_kernel(void);
/* Override the budget for this process (0 restores the default / environment). */
void bls_gpu_set_scratch_budget(uint64_t bytes);

/* Ask the HIP runtime for n hardware queues per priority (one per verifier context, so
 * contexts do not serialise on HIP's default 4: 12 contexts x 22 calls run 2.27M sets/s
 * on 4 queues, 3.65M on 24).  The runtime reads GPU_MAX_HW_QUEUES once, when it
 * initialises; this sets the variable to n when it is unset and the runtime is not up
 * yet.  The library never writes the environment on its own: call this before any HIP
 * use in the process, from one thread (setenv).  Returns 0 applied, 1 left alone (the
 * variable is already set: the host's choice stands), 2 too late (the runtime is up and
 * keeps its count), -2 for n == 0.  The Python and JS wrappers call it (or set the
 * variable) as they load the library unless $BLS_KEEP_HW_QUEUES=1. */
int bls_gpu_request_hw_queues(uint32_t n);

/* Release device memory and streams (IBlsVerifier.close, index.ts:176-197). */
void bls_gpu_close(bls_gpu_ctx* ctx);

const char* bls_gpu_last_error(const bls_gpu_ctx* ctx);

/* Load / append trusted validator pubkeys into the device table (Index2PubkeyCache,
 * state-transition/src/cache/pubkeyCache.ts:56-77).  pk_len is 48 (compressed) or 96
 * (uncompressed).  codes (nullable, n entries) receive a per-key decode code; keys
 * are not subgroup-checked (trusted, pubkeyCache.ts:72-75).  All or nothing: when any
 * key fails to decode, no key is appended (the table keeps its size, so indices stay
 * aligned across contexts).  Returns the new table size (>= 0) or < 0 on failure.
 * Beside the 100 B table entry the load builds 1,440 B of comb rows per key (15 affine
 * multiples; [r] pk of a single-key set runs on them), up to $BLS_PK_COMB_MAX_MB MiB per
 * table (default 4096; keys past it, or every key if that memory cannot be had, verify
 * through the per-set chain as before; $BLS_PK_COMB=0: no rows).
 * A context created by bls_gpu_init owns a private table.  When contexts share one
 * (bls_gpu_share_pubkeys) a load through any of them appends for all of them, the return
 * value is the shared size, and all-or-nothing holds for every sharer at once.  Loads of
 * one table run one at a time; calls in flight on the other contexts are not blocked and
 * see the table as it was when they began -- the new keys (and a table that had to grow)
 * are published only after they are complete on the device. */
int64_t bls_gpu_load_pubkeys(bls_gpu_ctx* ctx, const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes);

/* Make ctx use the key table of `with` (same device): one table per device instead of one
 * replica per context (the reference has one Index2PubkeyCache per process).  ctx must
 * hold no keys; it may already share an (empty) table with other contexts, which keep it.
 * Afterwards the two are peers: a load through either appends for both, every verify call
 * of either reads the same device memory, and the table lives until the last context
 * using it is closed, in any order of closes.  $BLS_PK_COMB_MAX_MB then caps the rows per
 * table, not per context; BLS_DEBUG_NO_PK_COMB stays a per-context flag.  Returns 0 on
 * success and when the two already share; -2 for a NULL argument, ctx == with, contexts
 * on different devices, or a ctx whose table is not empty (message in
 * bls_gpu_last_error(ctx)).  The function takes both contexts' locks, so it waits for a
 * call in flight on either. */
int bls_gpu_share_pubkeys(bls_gpu_ctx* ctx, bls_gpu_ctx* with);

/* The key table ctx uses. */
typedef struct bls_pubkeys_info {
  uint64_t table_id;      /* equal for contexts sharing a table; unique per table in the process; never 0 */
  uint32_t n_keys;        /* keys loaded (the next key's index) */
  uint32_t capacity;      /* keys the current buffers have room for */
  uint32_t comb_keys;     /* keys [0, comb_keys) were offered comb rows */
  uint32_t n_contexts;    /* open contexts using the table */
  uint64_t device_bytes;  /* table + rows + comb_ok of the current generation, counted once */
} bls_pubkeys_info;
int bls_gpu_pubkeys_info(bls_gpu_ctx* ctx, bls_pubkeys_info* out);

/* KeyValidate for n public keys (blst PublicKey.fromBytes(bytes, validate=true) [ext],
 * the check deposits get before a key enters the registry, state-transition
 * block/processDeposit.ts:56-65 -> index2pubkey, pubkeyCache.ts:56-77): decode
 * (48 compressed / 96 uncompressed), then BLST_PK_IS_INFINITY for the point at
 * infinity and BLST_POINT_NOT_IN_GROUP outside G1 (Scott's endomorphism test).
 * codes: n entries, 0 = valid.  Does not touch the device table. */
int bls_gpu_validate_pubkeys(bls_gpu_ctx* ctx, const uint8_t* pks, uint32_t n, uint32_t pk_len, int32_t* codes);

/* verifyManySignatureSets (worker.ts:32-108) on the GPU: per-request verdicts with
 * the reference's batch / fallback semantics:
 *   - batchable requests are grouped by chunkifyMaximizeChunkSize(reqs, 16) and each
 *     chunk is checked by one random-scalar batch (maybeBatch.ts:18-25);
 *   - a failing or erroring chunk is re-verified request by request;
 *   - non-batchable requests are verified on their own (maybeBatch.ts:16-39).
 * verdicts: n_reqs int32 (see top of file).  stats nullable. */
int bls_gpu_verify(bls_gpu_ctx* ctx, const bls_batch* batch, int32_t* verdicts, bls_stats* stats);

/* Several verifyManySignatureSets messages submitted together (the pool handing one
 * GPU context every message that is ready): the same verdicts and worker semantics as
 * n_batches bls_gpu_verify calls -- each message's batchable requests are chunked on
 * their own -- computed in one pass over the concatenated sets when every message
 * carries table-index pubkeys (messages with raw pubkeys run one after another).
 * verdicts: the messages' n_reqs entries concatenated; stats (nullable, one struct):
 * totals over the messages. */
int bls_gpu_verify_many(bls_gpu_ctx* ctx, const bls_batch* batches, uint32_t n_batches, int32_t* verdicts,
                        bls_stats* stats);

/* IBlsVerifier.verifySignatureSetsSameMessage(sets, message) -> boolean[]: jobs of
 * {publicKey, signature} pairs that all sign ONE root (unaggregated gossip
 * attestations).  The reference checks a job with aggregateWithRandomness -- one
 * pairing equation e(sum r_i pk_i, H(m)) e(-g1, sum r_i sig_i) == 1 -- and verifies
 * every set on its own when that fails.  Several jobs go in one call (the pool handing
 * a context every same-message job that is ready).  Job j owns sets
 * [job_set_offsets[j], job_set_offsets[j + 1]), each >= 1 and <= BLS_SAME_MSG_MAX_JOB
 * sets; public keys are device-table indices. */
#define BLS_SAME_MSG_MAX_JOB 4096u
typedef struct bls_same_msg_batch {
  uint32_t n_jobs, n_sets;
  const uint32_t* job_set_offsets; /* n_jobs + 1, from 0 to n_sets */
  const uint8_t* messages;         /* n_jobs * 32: one signing root per job */
  const uint32_t* pk_indices;      /* n_sets: one device-table index per set */
  const uint8_t* signatures;       /* n_sets * 96 compressed G2 */
  const uint8_t* seed;             /* 32 bytes or NULL, as in bls_batch */
} bls_same_msg_batch;

/* set_verdicts: n_sets int32.
 *   - A job is one random-scalar batch over all of its sets, whatever its size (it is
 *     not chunked at 16); set i of the call draws its scalar from the seed at index i.
 *     Two Miller loops and one final exponentiation per job, one hash-to-curve per
 *     distinct root (two jobs carrying the same root share H(m) and stay two batches).
 *   - A passing job gives every set 1.
 *   - A job fails when its check fails or any of its sets has a decode or group error;
 *     each of its sets then gets the verdict bls_gpu_verify gives a one-set request of
 *     that key index, root and signature: 1, 0 or -code under the one-set rules (an
 *     index past the table BLS_CODE_BAD_ENCODING, an infinity signature
 *     BLS_CODE_ZERO_SIGNATURE), found by the individual pass and its group tests.
 *   - A 1-set job is verified on its own directly.
 * n_jobs == 0 returns 0 and writes nothing; an empty or oversized job, offsets that do
 * not run monotonically from 0 to n_sets, or a NULL pointer where one is needed
 * return -2.  stats (nullable): n_chunks = jobs batched (>= 2 sets), batch_retries =
 * failed jobs, batch_sigs_success = sets of passing jobs, n_ml_units = one per batched
 * job, n_unique_msgs = distinct roots in the call, n_individual = sets verified on
 * their own. */
int bls_gpu_verify_same_message(bls_gpu_ctx* ctx, const bls_same_msg_batch* batch, int32_t* set_verdicts,
                                bls_stats* stats);

/* Deposit signatures (state-transition/src/block/processDeposit.ts:48-65): the one
 * signature check of the beacon node outside IBlsVerifier.  For a deposit of an unknown
 * validator the reference runs, inside one try block whose catch skips the deposit,
 *     PublicKey.fromBytes(pubkey, CoordType.affine, true)      -- KeyValidate, untrusted key
 *     Signature.fromBytes(signature, CoordType.affine, true)
 *     verify(publicKey, computeSigningRoot(DepositMessage, deposit, domain), signature)
 * with domain = computeDomain(DOMAIN_DEPOSIT, fork_version, ZERO_HASH) (:52).  One call
 * checks n deposits given by their four fields. */
#define BLS_DEPOSITS_MAX_CALL 65536u
typedef struct bls_deposit_batch {
  uint32_t n;
  const uint8_t* pubkeys48;               /* n * 48 compressed G1, untrusted */
  const uint8_t* withdrawal_credentials;  /* n * 32 */
  const uint8_t* amounts;                 /* n * 8, little-endian Gwei as in the SSZ serialization */
  const uint8_t* signatures;              /* n * 96 compressed G2 */
  const uint8_t* domain;                  /* 32 bytes: compute_domain(DOMAIN_DEPOSIT, fork_version, zero root) */
  const uint8_t* seed;                    /* as in bls_batch */
} bls_deposit_batch;

/* verdicts: n int32.  verdicts[i] is what the reference's try block gives deposit i on its
 * own: 1 valid, 0 invalid, -code when a step throws.  The order of the steps fixes the code:
 *   1. KeyValidate of the key: BLS_CODE_BAD_ENCODING, POINT_NOT_ON_CURVE, PK_IS_INFINITY or
 *      POINT_NOT_IN_GROUP;
 *   2. the signature decoded with validation: BAD_ENCODING, POINT_NOT_ON_CURVE,
 *      POINT_NOT_IN_GROUP;
 *   3. the one-set rules of bls_gpu_verify: an infinity signature BLS_CODE_ZERO_SIGNATURE;
 *   4. verify(pk, signing_root), the root being hash_tree_root(SigningData{
 *      hash_tree_root(DepositMessage{pubkey, withdrawal_credentials, amount}), domain}),
 *      computed on the device (signingRoot.ts:7-13).
 * An invalid deposit is legal: it never makes the call fail, and no verdict depends on
 * another deposit of the call.  The device table is neither read nor written.
 *
 * Internally every deposit is one batchable one-set request of the bls_gpu_verify pass:
 * chunks of chunkifyMaximizeChunkSize(n, 16), the merged check, the per-request fallback
 * and the group tests, so the verdicts are those of per-deposit verification apart from
 * the 2^-64 of a random-scalar batch.  Soundness of batching untrusted keys: a random-
 * scalar batch is sound only over points of the prime-order groups, so a deposit whose
 * key or signature has an error code gives its request that status before any product is
 * formed -- the key stage hands on the point at infinity for it -- and a key outside G1
 * never enters a batch.
 *
 * stats (nullable): those of bls_gpu_verify over n one-set batchable requests;
 * n_unique_msgs == n (the roots are made on the device, so there is no signing-root
 * dedup).  Like a same-message call, a deposit call neither reads nor writes the
 * context's merged-check history: invalid deposits are normal and must not change the
 * shape of the next gossip pass.
 * n == 0 returns 0 and writes nothing; n > BLS_DEPOSITS_MAX_CALL, or a NULL pointer other
 * than seed or stats, returns -2. */
int bls_gpu_verify_deposits(bls_gpu_ctx* ctx, const bls_deposit_batch* batch, int32_t* verdicts, bls_stats* stats);

/* Sharded call across GPUs (north_star "each GPU reduces its shard to
 * an Fp12 partial, the partials are combined over RCCL/xGMI, and one final
 * exponentiation follows").  The reference verifies one call as ONE random-scalar
 * batch (maybeBatch.ts:18-25, blst verifyMultipleSignatures [ext]); here each rank
 * holds a contiguous shard of the call's sets and computes
 *     P_rank = prod_{i in shard} e(r_i pk_i, H(m_i)) e(-g1, r_i sig_i)   (Miller loops only)
 * with r_i drawn from the call's shared seed at index set_index_base + i, so the
 * scalars of all shards are distinct draws of one batch.  batch->seed must be set
 * (the same 32 bytes on every rank).  out576 receives P_rank as 12 Fp (opaque device
 * form: 12 x 48-byte Montgomery limbs; only bls_gpu_final_check reads it).  The shard is
 * verified with the rules of a multi-set call (no single-set rules, even for a 1-set
 * shard).  status: 0 if every set decoded, else -(code) of the shard's first error in
 * the reference's order -- class 0 a pubkey that does not decode / aggregate
 * (deserializeSet, worker.ts:45), class 1 a signature that does not decode
 * (maybeBatch.ts:19-24), class 2 an infinity pubkey -- and err_info (nullable,
 * 2 words) receives {class, shard-local set index} (class 3: none) so the ranks can
 * pick the call's first error; the whole call then rejects (rule 2 of SURVEY §8a) and
 * out576 is undefined.  The shard must hold >= 1 set. */
int bls_gpu_partial(bls_gpu_ctx* ctx, const bls_batch* batch, uint32_t set_index_base, uint8_t* out576,
                    int32_t* status, uint32_t* err_info, bls_stats* stats);

/* The combine step after the all-gather: *verdict = 1 iff FE(prod_k partials[k]) == 1,
 * one final exponentiation for the whole call (n >= 1 partials of 576 bytes). */
int bls_gpu_final_check(bls_gpu_ctx* ctx, const uint8_t* partials576, uint32_t n, int32_t* verdict);

/* getAggregatedPubkey (chain/bls/utils.ts:5-16) for n_sets index lists over the device
 * table; out: n_sets * 96 bytes uncompressed (PointFormat.uncompressed, index.ts:126,160);
 * codes: n_sets (0 ok, BLS_CODE_EMPTY_AGGREGATE for an empty list). */
int bls_gpu_aggregate_pubkeys(bls_gpu_ctx* ctx, const uint32_t* set_pk_offsets, const uint32_t* pk_indices,
                              uint32_t n_sets, uint8_t* out96, int32_t* codes);

/* Committee groups: aggregate sets as they arrive on the wire, a committee plus a bitfield
 * (Attestation.aggregation_bits over a beacon committee, SyncAggregate.sync_committee_bits
 * over the sync committee), instead of the index list the host would expand them into.  The
 * committees are fixed for an epoch or a sync-committee period, so their member lists are
 * registered once and kept on the device with each committee's total key: a set whose field
 * has c of n bits set costs min(c, n - c + 1) point additions, not c, and its call ships
 * n / 8 bytes, not 4 c.
 *
 * A group is what the host holds as one unit -- one epoch's shuffling, or one sync
 * committee -- and is registered and replaced wholesale.  Groups belong to the context
 * (each context of a device registers them for itself; holding them beside the shared key
 * table of bls_gpu_share_pubkeys is a follow-up). */
#define BLS_COMMITTEE_GROUPS 8u               /* previous/current/next shuffling, current/next sync committee, spare */
#define BLS_COMMITTEE_MAX_MEMBERS 131072u     /* per committee */
#define BLS_SET_NO_COMMITTEE 0xFFFFFFFFu
#define BLS_COMMITTEE_REF(group, index) (((uint32_t)(group) << 24) | (uint32_t)(index))  /* index < 2^24 */

/* Replace group `group` (0..7) by n committees; committee c = table indices
 * members[member_offsets[c] .. member_offsets[c+1]), in committee order, duplicates allowed
 * (sync committees repeat validators).  n == 0 drops the group.  The call copies both arrays
 * to the device and sums every committee's members there (with multiplicity); the key
 * table is append-only, so the totals stay valid after later bls_gpu_load_pubkeys calls.
 * It holds the context's lock: no call of the context is in flight while a group changes.
 * Returns 0; -2 with nothing changed and a bls_gpu_last_error message naming the committee
 * for group >= BLS_COMMITTEE_GROUPS, member_offsets that do not run monotonically from 0, an
 * empty committee, one of more than BLS_COMMITTEE_MAX_MEMBERS members, or a member at or past
 * the table's size; -1 (nothing changed either) for a device failure. */
int bls_gpu_set_committee_group(bls_gpu_ctx* ctx, uint32_t group, uint32_t n,
                                const uint32_t* member_offsets, const uint32_t* members);
typedef struct bls_committee_info { uint32_t n_committees; uint32_t n_members; uint64_t device_bytes; } bls_committee_info;
/* What group `group` holds (all zero: not registered); -2 for group >= BLS_COMMITTEE_GROUPS. */
int bls_gpu_committee_group_info(bls_gpu_ctx* ctx, uint32_t group, bls_committee_info* out);

typedef struct bls_committee_sets {
  const uint32_t* set_committee;  /* n_sets: BLS_COMMITTEE_REF(group, index), or BLS_SET_NO_COMMITTEE:
                                     the set uses batch->set_pk_offsets / pk_indices as before */
  const uint32_t* set_bits_off;   /* n_sets + 1 byte offsets into bits (equal for a NO_COMMITTEE set) */
  const uint8_t* bits;            /* member j of the committee = bit (j & 7) of byte j >> 3 (SSZ order),
                                     without a Bitlist delimiter bit */
} bls_committee_sets;

/* bls_gpu_verify for a batch some of whose sets name a committee.  A committee set is
 * exactly the aggregate set whose index list is the committee's members at the set bits, in
 * order: the same verdicts and bls_stats counters as bls_gpu_verify on the expanded lists.
 * Its status follows the index-list path: no bit set BLS_CODE_EMPTY_AGGREGATE; an
 * unregistered group, an index past the group, a byte count other than ceil(members / 8) or
 * a set bit at or past the member count BLS_CODE_BAD_ENCODING.  The batch must be in table
 * mode (set_pk_offsets != NULL) and a committee set's own index list empty; the call may mix
 * both kinds of set.  -2 otherwise, and for set_bits_off that does not run monotonically
 * from 0 or a NO_COMMITTEE set that carries bits. */
int bls_gpu_verify_committees(bls_gpu_ctx* ctx, const bls_batch* batch, const bls_committee_sets* cs,
                              int32_t* verdicts, bls_stats* stats);
/* bls_gpu_aggregate_pubkeys for n_sets committee sets (every set names a committee): the
 * same bytes and codes as the expanded index lists give. */
int bls_gpu_aggregate_committee_bits(bls_gpu_ctx* ctx, const bls_committee_sets* cs, uint32_t n_sets,
                                     uint8_t* out96, int32_t* codes);

/* Spans: an aggregate over several committees under one field.  Since Electra (EIP-7549) an
 * on-chain Attestation selects up to 64 committees of its slot with committee_bits, and its
 * aggregation_bits run over those committees' members concatenated in committee order.
 * Committee sizes are no multiples of 8, so every committee after the first starts mid-byte
 * and the field cannot be cut into bls_committee_sets fields.  A span set names its
 * committees (its segments) in order and carries the field as it is: segment k of sizes
 * n_0, n_1, ... starts at bit n_0 + ... + n_{k-1}.  Each segment by itself is summed from
 * its set bits or as its total minus its clear bits, so a set costs
 * sum_k min(c_k, n_k - c_k + 1) point additions.
 *
 * A span set is exactly the aggregate set whose index list is the members of its segments,
 * concatenated in order, at the set bits: a one-segment span is a committee set; segments
 * may repeat a committee and come from different groups; a key in several segments counts
 * with multiplicity.  Its status: no bit set in the whole field BLS_CODE_EMPTY_AGGREGATE (a
 * segment without a set bit beside one that has some is legal here -- Electra's "every
 * selected committee has an attester" is a state-transition rule and stays with the host);
 * a segment of an unregistered group, an index past its group, a byte count other than
 * ceil(sum n_k / 8) or a set bit at or past sum n_k BLS_CODE_BAD_ENCODING. */
#define BLS_SPAN_MAX_COMMITTEES 64u           /* MAX_COMMITTEES_PER_SLOT */
typedef struct bls_span_sets {
  const uint32_t* set_span_off;  /* n_sets + 1 into span_refs, monotone from 0; an empty range: the set
                                    is an index-list set (batch->set_pk_offsets / pk_indices) */
  const uint32_t* span_refs;     /* BLS_COMMITTEE_REF(group, index) per segment, in order */
  const uint32_t* set_bits_off;  /* n_sets + 1 byte offsets into bits (equal for an index-list set) */
  const uint8_t* bits;           /* bit j of the concatenation = bit (j & 7) of byte j >> 3; no delimiter bit */
} bls_span_sets;

/* bls_gpu_verify for a batch some of whose sets are spans: the verdicts and every bls_stats
 * counter of bls_gpu_verify on the expanded lists with the same seed.  -2 with a
 * bls_gpu_last_error message naming the set, and nothing run, for a set of more than
 * BLS_SPAN_MAX_COMMITTEES segments, offsets that do not run monotonically from 0, a span
 * set that also carries an index list, an index-list set that carries bits, a raw-key batch
 * (set_pk_offsets == NULL), or a NULL array where one is needed. */
int bls_gpu_verify_spans(bls_gpu_ctx* ctx, const bls_batch* batch, const bls_span_sets* ss,
                         int32_t* verdicts, bls_stats* stats);
/* bls_gpu_aggregate_pubkeys for n_sets span sets (every set has at least one segment, -2
 * otherwise): the same bytes and codes as the expanded index lists give.  n_sets == 0
 * returns 0 and writes nothing. */
int bls_gpu_aggregate_spans(bls_gpu_ctx* ctx, const bls_span_sets* ss, uint32_t n_sets,
                            uint8_t* out96, int32_t* codes);

/* G2 signature aggregation for the op pools:
 * Signature.aggregate(sigs.map((s) => Signature.fromBytes(s, undefined, true))) for each
 * of n_lists lists (aggregatedAttestationPool.ts:320-327 aggregateInto,
 * syncContributionAndProofPool.ts:181-185, syncCommitteeMessagePool.ts:122-129).
 * List l holds the 96-byte compressed signatures [list_offsets[l], list_offsets[l+1]).
 * out96: n_lists compressed sums; codes: 0, BLS_CODE_EMPTY_AGGREGATE for an empty list,
 * or the code of the list's first signature that does not decode / is outside G2. */
int bls_gpu_aggregate_signatures(bls_gpu_ctx* ctx, const uint8_t* sigs96, const uint32_t* list_offsets,
                                 uint32_t n_lists, uint8_t* out96, int32_t* codes);

/* Signature.fromBytes(bytes, CoordType.affine, validate) ([ext] @chainsafe/blst, as
 * maybeBatch.ts:23,36 call it): n 96-byte compressed G2 points -> out192 (uncompressed
 * ZCash order x.c1 || x.c0 || y.c1 || y.c0; the infinity encoding for the point at
 * infinity) and codes (0, or BLS_CODE_BAD_ENCODING / POINT_NOT_ON_CURVE /
 * POINT_NOT_IN_GROUP; the subgroup test only when validate != 0). */
int bls_gpu_g2_decompress(bls_gpu_ctx* ctx, const uint8_t* in96, uint32_t n, int validate, uint8_t* out192,
                          int32_t* codes);

/* hash_to_G2 with the POP DST for n 32-byte messages; out: n * 192 bytes (uncompressed
 * ZCash order x.c1 || x.c0 || y.c1 || y.c0). */
int bls_gpu_hash_to_g2(bls_gpu_ctx* ctx, const uint8_t* msgs, uint32_t n, uint8_t* out192);

/* SSZ object kinds of bls_gpu_ssz_roots: the fixed-size containers whose signing roots
 * the signature-set producers compute (state-transition/src/signatureSets/), given
 * in their SSZ serialization (fields concatenated, integers little-endian).  The value
 * is the serialized size in bytes in the low 8 bits. */
enum {
  BLS_SSZ_ROOT = 0x000 | 32,                /* Root / Bytes32: sync committee messages (block root), or an
                                               object root computed elsewhere (e.g. AggregateAndProof) */
  BLS_SSZ_UINT64 = 0x100 | 8,               /* Epoch / Slot: randao reveal, aggregate selection proof */
  BLS_SSZ_CHECKPOINT = 0x200 | 40,          /* Checkpoint{epoch, root} */
  BLS_SSZ_ATTESTATION_DATA = 0x300 | 128,   /* AttestationData: attestations, indexed attestations, slashings */
  BLS_SSZ_TWO_UINT64 = 0x400 | 16,          /* VoluntaryExit{epoch, validator_index},
                                               SyncAggregatorSelectionData{slot, subcommittee_index} */
  BLS_SSZ_BEACON_BLOCK_HEADER = 0x500 | 112, /* BeaconBlockHeader (== the block's root given its body root):
                                               proposer signatures, proposer slashings */
  BLS_SSZ_DEPOSIT_MESSAGE = 0x600 | 88,     /* DepositMessage{pubkey 48, withdrawal_credentials, amount} */
  BLS_SSZ_FORK_DATA = 0x700 | 36,           /* ForkData{current_version 4, genesis_validators_root}:
                                               computeForkDataRoot (util/domain.ts:40-45) */
  BLS_SSZ_SIGNING_DATA = 0x800 | 64         /* SigningData{object_root, domain} */
};
#define BLS_SSZ_SIZE(kind) ((uint32_t)(kind) & 0xFFu)

/* computeSigningRoot(type, obj, domain) (state-transition/src/util/signingRoot.ts:7-13)
 * for n serialized objects of one kind: out32[i] = hash_tree_root(SigningData{
 * hash_tree_root(obj_i), domain_i}); with domains == NULL, out32[i] = hash_tree_root(obj_i)
 * instead.  objs: n * BLS_SSZ_SIZE(kind) bytes; domain_stride 0 = one 32-byte domain for
 * every object, 32 = one per object.  Returns -2 for an unknown kind or stride. */
int bls_gpu_ssz_roots(bls_gpu_ctx* ctx, uint32_t kind, const uint8_t* objs, uint32_t n, const uint8_t* domains,
                      uint32_t domain_stride, uint8_t* out32);

/* Fixture helpers (signing is out of the verify path; used to synthesise inputs).
 * sks: n * 32 bytes big-endian scalars. */
int bls_gpu_sk_to_pk(bls_gpu_ctx* ctx, const uint8_t* sks, uint32_t n, uint8_t* out48);
int bls_gpu_sign(bls_gpu_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, uint32_t n, uint8_t* out96);

/* Roofline probe: measured rate of v_mad_u64_u32 (32x32+64 multiply-add, the unit of
 * every Fp Montgomery product) on this device, with every CU at 8 waves/SIMD. */
int bls_gpu_mad_peak(bls_gpu_ctx* ctx, double* mads_per_s, double* ms);

/* Field self-test: out = a * b mod p for n pairs of canonical 48-byte big-endian
 * elements (exercises to/from Montgomery and the device Montgomery product). */
int bls_gpu_fp_mul_test(bls_gpu_ctx* ctx, const uint8_t* a48, const uint8_t* b48, uint32_t n, uint8_t* out48);

/* Device field-op self-test: one lane per record runs ONE field primitive on raw
 * little-endian 32-bit words (Fp = 12 limbs, lazy28 = 14 signed digits) and writes its
 * raw result; nothing converts to or from Montgomery form or reduces around it, so
 * non-canonical operands reach the primitive untouched.  `in` holds n records of
 * in_words words, `out` receives n records of out_words (bls_gpu_field_op_shape).
 * op: a base id (lodestar_amd/csrc/kernels/field_ops.hpp FOP_*, tests/_fieldvec.py),
 * ORed with BLS_FIELD_OP_D28 for the kernels built over the 28-bit-digit product the
 * verify path uses; without it the 32-bit column product.  -2: unknown op.
 * Ops: 0..28 the arithmetic primitives and the interpreter's linear combination, 29..31
 * the out-of-line Fp2 products, 32 (FOP_PREDS, both flavours) the comparison predicates
 * on one raw pair (c0, c1) -- 24 words in, one word of bits out: fp_plain_is_canonical,
 * fp_plain_gt_half, fp_is_zero of each and fp_eq on the words as plain values (any
 * input), then fp_lex_largest of each, fp2_lex_largest, fp2_sgn0, fp2_is_zero on them as
 * Montgomery forms (canonical input only). */
#define BLS_FIELD_OP_D28 0x100u
int bls_gpu_field_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out);
int bls_gpu_field_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);

/* Device curve-op self-test: one lane per record runs ONE curve-level function of the verify
 * path, the production function itself in the translation-unit flavour production compiles
 * it in, one launch per call.  Fp values travel as 12 little-endian 32-bit words in
 * Montgomery form, exactly what production passes between these kernels; nothing on the
 * device converts or canonicalises them.  `in` holds n records of in_words words, `out`
 * receives n records of out_words (bls_gpu_curve_op_shape).  op: a base id
 * (lodestar_amd/csrc/kernels/curve_op_ids.hpp COP_*, tests/_curvevec.py), ORed with
 * BLS_CURVE_OP_D28 for the 28-bit-digit flavours.  -2: unknown op, or an op in a flavour it
 * does not exist in.
 *   0 FROM_BE64       fp_from_be64_words (cols, d28)       16 big-endian words -> Fp
 *   1 H2F             hash_to_field_fp2_x2 (cols, d28)     8 message words -> u0, u1
 *   2 SSWU            map_to_curve_sswu (cols)             u -> x, y
 *   3 SSWU_FAST       map_to_curve_sswu_fast (d28: k_pre)  u -> ok word, x, y
 *   4 ISO_AFF         iso_map_g2 (cols)                    x, y -> inf word, x, y
 *   5 ISO_JAC         k_chain.hip iso_jac_nl (d28 + Fp2 primitive)   x, y -> X, Y, Z
 *   6 CLEAR_COFACTOR  g2_clear_cofactor + jac_to_aff (cols)          inf, x, y -> inf, x, y
 *   7 CHAIN_H         k_chain.hip chain_role_h (d28 + Fp2 primitive) q0, q1 (8 Fp) ->
 *                     chain_st byte (1: H = O, HQ left zero), HQ (4 Fp)
 * Two more ops add no kernel and no arithmetic: they fill a zeroed set of pipeline buffers
 * with the records alone and call the production launchers (both BLS_CURVE_OP_D28 only).
 *   8 MILLER  the split SIMT Miller loops (k_mlq, then k_mlf or k_mlf2): record = RP (Jacobian
 *             G1: x, y, z, any z), HQ (affine G2), the item's product domain, per_lane (1, 2,
 *             4 or 3 = two lanes per item; record 0's counts) -> f (12 Fp, Fp12 memory order).
 *             Items [0, n) run as one first-pass launch: per_lane consecutive items of one
 *             domain share one f (the first holds the product, the others exactly 1).
 *             At most 1,024 items.
 *   9 FE      F (12 Fp) -> two words: FE(F) == 1 by the SIMT chunk kernel and by the
 *             cooperative one, each F its own one-request, one-set chunk */
#define BLS_CURVE_OP_D28 0x100u
int bls_gpu_curve_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out);
int bls_gpu_curve_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);

/* Device tower-op self-test: one lane per record runs ONE function of the Fp6 / Fp12 tower
 * the SIMT verify path runs in every Miller-loop step and final exponentiation, the
 * production function itself in a translation-unit flavour production compiles it in.  Fp
 * values travel as 12 little-endian 32-bit words in Montgomery form (raw value in [0, p));
 * an Fp6 is 6 Fp, an Fp12 12 Fp in memory order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2),
 * a line l0, l2, l3.  Nothing on the device converts or canonicalises around the call.  op: a
 * base id (lodestar_amd/csrc/kernels/tower_op_ids.hpp TOP_*, tests/_towervec.py), ORed
 * with BLS_TOWER_OP_D28 for the 28-bit-digit flavours.  -2: unknown op, or an op in a
 * flavour it does not exist in (nothing runs, `out` is not written).
 *   0 FP6_MUL (cols, d28)   1 FP6_MUL_01 (cols)   2 FP6_MUL_1 (cols)   3 FP6_INV (d28)
 *   4 FP12_MUL (cols)   5 FP12_SQR (cols)   6 FP12_MUL_LINE (cols)
 *   7 FP12_INV (d28)    8 FP12_FROB (d28)   9 FP12_FROB2 (d28)
 *   10 FIN_MUL12M, 11 FIN_MUL12M_CONJ, 12 FIN_CYC_SQR, 13 FIN_EXP_X_M: k_fin_simt.hip's
 *      file-local functions (d28), operands in device memory as there
 *   14 MLQ_SQR12, 15 MLQ_MUL_LINE12, 16 MLQ_MUL_LINE2 (f, line, line): k_mlq.hip (d28 + Fp2
 *      primitive); 17 MLQ_SQR12_PAIR, 18 MLQ_MUL_LINE12_PAIR: the two-lane halves, output
 *      lane 2k's Fp12 then lane 2k + 1's
 *   19 MLQ_LINES (d28): RP (Jacobian G1 x, y, z, z != 0), HQ (4 Fp) -> the 68 lines k_mlq
 *      writes for the item (event-major, l0, l2, l3 each); at most 64 items */
#define BLS_TOWER_OP_D28 0x100u
int bls_gpu_tower_op_test(bls_gpu_ctx* ctx, uint32_t op, const uint32_t* in, uint32_t n, uint32_t* out);
int bls_gpu_tower_op_shape(uint32_t op, uint32_t* in_words, uint32_t* out_words);

/* Interpreter test: the cooperative program `name` of the loaded table run once on each
 * of n_frames frames of n_slots raw Fp values (12 little-endian words each, Montgomery
 * form, any representative below 3p); frames_out receives the raw frames after the run
 * (lazy values, not canonicalised) and flags_out one zero-check flag word per frame.
 * n_slots must equal the program's frame size in the table (-2 otherwise). */
int bls_gpu_coop_run_test(bls_gpu_ctx* ctx, const char* name, const uint32_t* frames_in, uint32_t n_frames,
                          uint32_t n_slots, uint32_t* frames_out, uint32_t* flags_out);

/* Probe: `lanes` lanes each run `iters` dependent Montgomery products. */
int bls_gpu_fpm_bench(bls_gpu_ctx* ctx, uint32_t lanes, uint32_t iters, double* ns_per_fpm, double* fpm_per_s);

/* Probe: time the cooperative (one wavefront per task) program `name` on `blocks`
 * tasks, `reps` runs each; us_per_step = run time / step count. */
int bls_gpu_coop_probe(bls_gpu_ctx* ctx, const char* name, uint32_t blocks, uint32_t reps, double* us_per_step,
                       double* ms_total,
                       uint64_t* step_stamps /* nullable, 2 n_steps + 1 s_memtime stamps (step start, compute done) */);

/* Design probe: launch the probe kernel `name` (kernels/k_probe.hip: "ml_simt_w1",
 * "ml_simt_w2", "fpm_d28") over `lanes` lanes `reps` times; *ms = wall time of the reps. */
int bls_gpu_kernel_probe(bls_gpu_ctx* ctx, const char* name, uint32_t lanes, uint32_t reps, double* ms);

/* Test hook: BLS_DEBUG_FORCE_EXACT routes every set through the exact single-lane
 * path (stage_exact_set) instead of the cooperative programs, so parity tests cover both. */
#define BLS_DEBUG_FORCE_EXACT 1u
/* Test / bench hook: compute hash_to_field + SSWU per set even when sets share a
 * signing root (the default dedups them, plan_msg_dedup in bls/plan.hpp). */
#define BLS_DEBUG_NO_MSG_DEDUP 2u
/* Test / bench hook: skip the merged check (one final exponentiation over every
 * chunk's sets before the per-chunk ones) and go straight to the chunk verdicts. */
#define BLS_DEBUG_NO_MERGED_CHECK 4u
/* Test / bench hook: sets per wavefront of the per-set cooperative kernel (1, 2 or 3;
 * 0 = by call size), so one process can run the same call through every packing. */
#define BLS_DEBUG_PACK(n) ((uint32_t)(n) << 8)
#define BLS_DEBUG_PACK_MASK 0x300u
/* Test / bench hook: force the aggregated-signature path (per-set chains one lane per
 * set, e(-g1, sum r_i sig_i) once per chunk, single-pair cooperative Miller loops) or
 * the all-cooperative per-set path; default: by call size (>= 512 sets: aggregated). */
#define BLS_DEBUG_SIGAGG_ON 8u
#define BLS_DEBUG_SIGAGG_OFF 16u
/* Test / bench hook: no Miller-loop units (one Miller loop per set even when sets of a
 * chunk share a signing root). */
#define BLS_DEBUG_NO_UNITS 32u
/* Test / bench hook: the merged signature sum as a Pippenger multi-scalar
 * multiplication (kernels/k_msm.hip) whatever $BLS_MSM says. */
#define BLS_DEBUG_MSM 64u
/* Test / bench hook: items per lane of the Miller loops' f side (1, 2 or 4; 3 = one item
 * per two lanes; 0 = by the process's sets in flight). */
#define BLS_DEBUG_MLF_PL(n) ((uint32_t)(n) << 12)
#define BLS_DEBUG_MLF_PL_MASK 0x7000u
/* Test / bench hook: group-test failed chunks of >= 4 requests whatever
 * $BLS_GROUP_TEST_MIN says (its default is 4 too; 0 turns group testing off). */
#define BLS_DEBUG_GROUP_TEST 128u
/* Test hook: run the merged check on every pass, also after a pass that failed it (by
 * default such a context's next pass checks its chunks straight away, merged_check 3). */
#define BLS_DEBUG_MERGED_EVERY_PASS 0x8000u
/* Test / bench hook: [r] pk by the GLV chain for every set of this context, also where the
 * key's comb rows exist (bls_gpu_load_pubkeys builds them; $BLS_PK_COMB=0 turns them off
 * for the process), so one process can run the same call through both. */
#define BLS_DEBUG_NO_PK_COMB 0x10000u
/* Test / bench hook: the Pippenger signature sum as five launches of its own in front of
 * the Miller loops (the serial form) also where its long stages would run inside the
 * Miller-loop launches (pass_shape bit 1; $BLS_MSM_OVERLAP=0 does the same for the
 * process), so one process can run the same call through both. */
#define BLS_DEBUG_MSM_SERIAL 0x20000u
int bls_gpu_set_debug_flags(bls_gpu_ctx* ctx, uint32_t flags);

/* Test hook: the group-test rounds of the context's last verify pass (zero when it group-
 * tested nothing; bls_stats does not say which round decided a failed chunk):
 *   out[0] chunks group-tested (with a request of status OK)
 *   out[1] ... whose whole value came from the failed chunk check's own final exponentiation
 *   out[2] tests run in pass A        out[3] chunks decided by pass A's decode
 *   out[4] tests run in pass B        out[5] chunks decided by pass B
 *   out[6] tests run in pass C (= requests tested alone)
 *   out[7] 1 when a chunk's pass A did not fit the group-sum workspace even on its own
 *          (its requests went to pass C), else 0; chunks that do not fit together are
 *          tested in several rounds, which the counters do not tell apart
 * Returns 0, or -2 on a null argument. */
int bls_gpu_group_test_counts(bls_gpu_ctx* ctx, uint32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* LODESTAR_BLS_H */
