/*
 * Thin N-API addon over the C-ABI of include/lodestar_bls.h: what Lodestar's
 * `GpuBlsVerifier` (integration/js/gpuBlsVerifier.js) loads in place of the
 * @chainsafe/blst worker pool (beacon-node/src/chain/bls/multithread/index.ts).
 *
 *   init(device, highPriority?) -> handle   (highPriority: bls_gpu_init_priority HIGH; throws an
 *          Error with code "BLS_ERR_ADMISSION" when the scratch admission refuses the context)
 *   loadPubkeys(handle, Uint8Array pks, pkLen) -> Int32Array codes
 *   verify(handle, {reqSetOffsets, reqBatchable, messages, signatures,
 *                   setPkOffsets?, pkIndices?, pubkeys?, signatureLens?, seed?})
 *          -> Promise<Int32Array verdicts>   (1 valid, 0 invalid, -code error)
 *   verifySync(handle, request) -> Int32Array   (the same on the calling thread)
 *   partial(handle, request, setIndexBase) -> Promise<{partial: Uint8Array(576) | null, status,
 *          errClass, errIndex}>   (bls_gpu_partial: a shard of a call split across devices;
 *          request.seed must hold the call's 32-byte seed)
 *   finalCheck(handle, Uint8Array partials (576 B each)) -> Promise<boolean>   (bls_gpu_final_check)
 *   verifySameMessage(handle, {jobSetOffsets, messages, pkIndices, signatures, seed?})
 *          -> Promise<Int32Array set verdicts>   (bls_gpu_verify_same_message: jobs of table-index
 *          sets that sign one root each, IBlsVerifier.verifySignatureSetsSameMessage; the array
 *          also carries nChunks = jobs batched and nIndividual = sets verified on their own)
 *   verifyDeposits(handle, {pubkeys, withdrawalCredentials, amounts, signatures, domain, seed?})
 *          -> Promise<Int32Array verdicts>   (bls_gpu_verify_deposits: n = pubkeys.length / 48
 *          deposits by their four fields, amounts 8 B little-endian each; one code per deposit,
 *          1 valid, 0 invalid, -code a step that throws in processDeposit.ts:48-65; an invalid
 *          deposit never rejects the promise)
 *   close(handle)
 *
 * The verdict array carries the worker's BlsWorkResult bookkeeping (types.ts:26-38) as
 * properties: batchRetries, batchSigsSuccess, deviceMs, and workerStartNs / workerEndNs
 * (CLOCK_MONOTONIC ns as Numbers, the clock of process.hrtime.bigint(), taken on the
 * thread that ran the call) -- what the pool turns into its metrics
 * (multithread/index.ts:330-366: latencyToWorker, latencyFromWorker, batchRetries,
 * batchSigsSuccess, jobsWorkerTime).
 *
 * verify runs bls_gpu_verify on a libuv worker thread (napi_async_work): the JS
 * main thread never blocks on the GPU.  Input buffers are referenced until the
 * call completes (the library copies them into pinned staging at the start).
 *
 * Build (no node-gyp needed):
 *   gcc -O2 -shared -fPIC -I/usr/include/node -I include integration/napi/lodestar_bls_napi.c \
 *       -L lodestar_amd/_native -llodestar_bls -Wl,-rpath,'$ORIGIN' -o lodestar_amd/_native/lodestar_bls.node
 */
#define NAPI_VERSION 4
#include <execinfo.h>
#include <node_api.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "lodestar_bls.h"

#define CHECK(env, call)                                            \
  do {                                                              \
    if ((call) != napi_ok) {                                        \
      napi_throw_error((env), NULL, "lodestar_bls: N-API failure"); \
      return NULL;                                                  \
    }                                                               \
  } while (0)

/* One handle per JS verifier context.  Every entry point runs on the JS main thread
 * (verify_execute only touches ctx on a libuv worker), so the counters need no
 * locking.  close() while verifies are queued or running only marks the handle; the
 * last completing verify releases the device context.  Each queued job also holds a
 * reference to the handle object, so the GC finalizer cannot run under it; close()
 * removes the wrap, so a closed handle has no finalizer at all. */
typedef struct {
  bls_gpu_ctx* ctx;
  uint32_t inflight;
  int closed;
} bls_handle;

/* a closed handle with nothing in flight: release its device context and free it (the
 * caller does not touch h afterwards) */
static void handle_release_if_idle(bls_handle* h) {
  if (h->closed && h->inflight == 0) {
    if (h->ctx) bls_gpu_close(h->ctx);
    h->ctx = NULL;
    free(h);
  }
}

/* GC of a handle that was never closed (jobs hold a reference to the handle object, so
 * nothing is in flight then) */
static void handle_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  bls_handle* h = (bls_handle*)data;
  h->closed = 1;
  handle_release_if_idle(h);
}

static napi_value js_init(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t dev = 0;
  bool high = false;
  if (argc > 0) CHECK(env, napi_get_value_int32(env, argv[0], &dev));
  if (argc > 1) {
    napi_valuetype t;
    CHECK(env, napi_typeof(env, argv[1], &t));
    if (t == napi_boolean) CHECK(env, napi_get_value_bool(env, argv[1], &high));
  }
  bls_gpu_ctx* ctx = NULL;
  const int rc = bls_gpu_init_priority(dev, high ? BLS_PRIORITY_HIGH : BLS_PRIORITY_NORMAL, &ctx);
  if (rc != 0 || !ctx) {
    /* the library's reason; error.code "BLS_ERR_ADMISSION" when the scratch admission
     * refused the context (the adapter then runs on the contexts it has, as the reference
     * pool keeps the workers that started, multithread/index.ts:221-229) */
    const char* why = bls_gpu_init_error();
    char msg[600];
    snprintf(msg, sizeof(msg), "%s", why && *why ? why : "bls_gpu_init failed (no HIP device?)");
    napi_throw_error(env, rc == BLS_ERR_ADMISSION ? "BLS_ERR_ADMISSION" : "BLS_ERR_INIT", msg);
    return NULL;
  }
  bls_handle* h = (bls_handle*)calloc(1, sizeof(bls_handle));
  h->ctx = ctx;
  /* the handle is a plain object wrapping h: close() removes the wrap, so a closed
   * handle leaves no finalizer for V8 to run at environment teardown (Node 12 ran such
   * finalizers during FreeEnvironment and crashed the process at exit, 1 run in ~3 of
   * the 16-context N-API bench; profiles/r06_napi_exit_crash.txt) */
  napi_value obj;
  CHECK(env, napi_create_object(env, &obj));
  if (napi_wrap(env, obj, h, handle_finalize, NULL, NULL) != napi_ok) {
    bls_gpu_close(ctx);
    free(h);
    napi_throw_error(env, NULL, "lodestar_bls: N-API failure");
    return NULL;
  }
  return obj;
}

/* the live handle behind v, or NULL (not a handle, or closed: use after close) */
static bls_handle* get_handle(napi_env env, napi_value v) {
  void* p = NULL;
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_object) return NULL;
  if (napi_unwrap(env, v, &p) != napi_ok || !p) return NULL;
  bls_handle* h = (bls_handle*)p;
  return h->closed ? NULL : h;
}

static napi_value js_close(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = get_handle(env, argv[0]);
  if (h) {
    void* p = NULL;
    (void)napi_remove_wrap(env, argv[0], &p);  /* no finalizer from here on */
    h->closed = 1;
    handle_release_if_idle(h);  /* now, or when its last call completes */
  }
  return NULL;
}

/* typed array / buffer data pointer and byte length (NULL for undefined / null) */
static int view_of(napi_env env, napi_value v, void** data, size_t* bytes) {
  napi_valuetype t;
  *data = NULL;
  *bytes = 0;
  if (napi_typeof(env, v, &t) != napi_ok) return -1;
  if (t == napi_undefined || t == napi_null) return 0;
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type tt;
    size_t len, off;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &tt, &len, data, &ab, &off) != napi_ok) return -1;
    size_t el = (tt == napi_uint32_array || tt == napi_int32_array) ? 4 : 1;
    *bytes = len * el;
    return 0;
  }
  return napi_get_buffer_info(env, v, data, bytes) == napi_ok ? 0 : -1;
}

static napi_value js_load_pubkeys(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = get_handle(env, argv[0]);
  void* pks;
  size_t bytes;
  uint32_t pk_len = 48;
  if (!h || view_of(env, argv[1], &pks, &bytes)) {
    napi_throw_type_error(env, NULL, "loadPubkeys(handle, Uint8Array, pkLen)");
    return NULL;
  }
  if (argc > 2) CHECK(env, napi_get_value_uint32(env, argv[2], &pk_len));
  uint32_t n = (uint32_t)(bytes / pk_len);
  napi_value ab, out;
  void* codes;
  CHECK(env, napi_create_arraybuffer(env, 4 * (size_t)(n ? n : 1), &codes, &ab));
  CHECK(env, napi_create_typedarray(env, napi_int32_array, n, ab, 0, &out));
  if (bls_gpu_load_pubkeys(h->ctx, (const uint8_t*)pks, n, pk_len, (int32_t*)codes) < 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  return out;
}

/* sharePubkeys(handle, withHandle): handle uses withHandle's key table from here on
 * (bls_gpu_share_pubkeys; synchronous -- it only waits for calls in flight on the two) */
static napi_value js_share_pubkeys(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc > 0 ? get_handle(env, argv[0]) : NULL;
  bls_handle* with = argc > 1 ? get_handle(env, argv[1]) : NULL;
  if (!h || !with) {
    napi_throw_type_error(env, NULL, "sharePubkeys(handle, withHandle)");
    return NULL;
  }
  if (bls_gpu_share_pubkeys(h->ctx, with->ctx) != 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  return NULL;
}

/* pubkeysInfo(handle) -> {tableId, nKeys, capacity, combKeys, nContexts, deviceBytes}
 * (bls_pubkeys_info; tableId and deviceBytes as numbers: both stay far below 2^53) */
static napi_value js_pubkeys_info(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc > 0 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "pubkeysInfo(handle)");
    return NULL;
  }
  bls_pubkeys_info pi;
  if (bls_gpu_pubkeys_info(h->ctx, &pi) != 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  const char* names[6] = {"tableId", "nKeys", "capacity", "combKeys", "nContexts", "deviceBytes"};
  const double vals[6] = {(double)pi.table_id,  (double)pi.n_keys,     (double)pi.capacity,
                          (double)pi.comb_keys, (double)pi.n_contexts, (double)pi.device_bytes};
  napi_value obj;
  CHECK(env, napi_create_object(env, &obj));
  for (int i = 0; i < 6; ++i) {
    napi_value v;
    CHECK(env, napi_create_double(env, vals[i], &v));
    CHECK(env, napi_set_named_property(env, obj, names[i], v));
  }
  return obj;
}

enum { JOB_VERIFY = 0, JOB_PARTIAL = 1, JOB_FINAL = 2, JOB_SAME_MSG = 3, JOB_DEPOSITS = 4, JOB_COMMITTEES = 5,
       JOB_SET_GROUP = 6, JOB_SPANS = 7, JOB_AGG_SPANS = 8 };

typedef struct {
  int kind;
  bls_handle* h;
  bls_gpu_ctx* ctx;
  bls_batch batch;
  bls_same_msg_batch same;  /* JOB_SAME_MSG */
  bls_deposit_batch dep;    /* JOB_DEPOSITS */
  bls_committee_sets cs;    /* JOB_COMMITTEES (with batch) */
  bls_span_sets ss;         /* JOB_SPANS (with batch), JOB_AGG_SPANS */
  uint32_t n_span_sets;     /* JOB_AGG_SPANS */
  uint8_t* agg_out;         /* JOB_AGG_SPANS: 96 B per set, then the codes in verdicts */
  uint32_t group, n_committees;          /* JOB_SET_GROUP */
  const uint32_t *member_offsets, *members;
  napi_ref keep;          /* the request object: keeps the input buffers alive */
  napi_ref keep_handle;   /* the handle object: no finalizer while the job is out */
  int32_t* verdicts;
  bls_stats stats;
  double t_start_ns, t_end_ns;
  int rc;
  /* JOB_PARTIAL / JOB_FINAL */
  uint32_t base;
  uint8_t part[576];
  int32_t status;
  uint32_t err_info[2];
  const uint8_t* partials;
  uint32_t n_partials;
  int32_t verdict;
  napi_deferred deferred;
  napi_async_work work;
} verify_job;

static double mono_ns(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec * 1e9 + (double)t.tv_nsec;
}

/* the BlsWorkResult bookkeeping as properties of the verdict array */
static void attach_stats(napi_env env, napi_value out, const bls_stats* st, double t0, double t1) {
  napi_value v;
  napi_create_uint32(env, st->batch_retries, &v);
  napi_set_named_property(env, out, "batchRetries", v);
  napi_create_uint32(env, st->batch_sigs_success, &v);
  napi_set_named_property(env, out, "batchSigsSuccess", v);
  napi_create_double(env, st->device_ms, &v);
  napi_set_named_property(env, out, "deviceMs", v);
  napi_create_double(env, t0, &v);
  napi_set_named_property(env, out, "workerStartNs", v);
  napi_create_double(env, t1, &v);
  napi_set_named_property(env, out, "workerEndNs", v);
}

static void verify_execute(napi_env env, void* data) {
  (void)env;
  verify_job* j = (verify_job*)data;
  j->t_start_ns = mono_ns();
  if (j->kind == JOB_PARTIAL)
    j->rc = bls_gpu_partial(j->ctx, &j->batch, j->base, j->part, &j->status, j->err_info, &j->stats);
  else if (j->kind == JOB_FINAL)
    j->rc = bls_gpu_final_check(j->ctx, j->partials, j->n_partials, &j->verdict);
  else if (j->kind == JOB_SAME_MSG)
    j->rc = bls_gpu_verify_same_message(j->ctx, &j->same, j->verdicts, &j->stats);
  else if (j->kind == JOB_DEPOSITS)
    j->rc = bls_gpu_verify_deposits(j->ctx, &j->dep, j->verdicts, &j->stats);
  else if (j->kind == JOB_COMMITTEES)
    j->rc = bls_gpu_verify_committees(j->ctx, &j->batch, &j->cs, j->verdicts, &j->stats);
  else if (j->kind == JOB_SPANS)
    j->rc = bls_gpu_verify_spans(j->ctx, &j->batch, &j->ss, j->verdicts, &j->stats);
  else if (j->kind == JOB_AGG_SPANS)
    j->rc = bls_gpu_aggregate_spans(j->ctx, &j->ss, j->n_span_sets, j->agg_out, j->verdicts);
  else if (j->kind == JOB_SET_GROUP)
    j->rc = bls_gpu_set_committee_group(j->ctx, j->group, j->n_committees, j->member_offsets, j->members);
  else
    j->rc = bls_gpu_verify(j->ctx, &j->batch, j->verdicts, &j->stats);
  j->t_end_ns = mono_ns();
}

static void verify_complete(napi_env env, napi_status status, void* data) {
  verify_job* j = (verify_job*)data;
  if (status != napi_ok || j->rc != 0) {
    napi_value msg, err;
    char text[640];
    snprintf(text, sizeof(text), "%s failed (rc %d, status %d): %s",
             j->kind == JOB_PARTIAL ? "bls_gpu_partial"
             : j->kind == JOB_FINAL ? "bls_gpu_final_check"
             : j->kind == JOB_SAME_MSG ? "bls_gpu_verify_same_message"
             : j->kind == JOB_DEPOSITS ? "bls_gpu_verify_deposits"
             : j->kind == JOB_COMMITTEES ? "bls_gpu_verify_committees"
             : j->kind == JOB_SPANS ? "bls_gpu_verify_spans"
             : j->kind == JOB_AGG_SPANS ? "bls_gpu_aggregate_spans"
             : j->kind == JOB_SET_GROUP ? "bls_gpu_set_committee_group" : "bls_gpu_verify",
             j->rc, (int)status,
             j->rc ? bls_gpu_last_error(j->ctx) : "cancelled");
    napi_create_string_utf8(env, text, NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->kind == JOB_PARTIAL) {
    napi_value out, v;
    napi_create_object(env, &out);
    if (j->status == 0) {
      napi_value ab;
      void* dst;
      napi_create_arraybuffer(env, 576, &dst, &ab);
      memcpy(dst, j->part, 576);
      napi_create_typedarray(env, napi_uint8_array, 576, ab, 0, &v);
    } else {
      napi_get_null(env, &v);
    }
    napi_set_named_property(env, out, "partial", v);
    napi_create_int32(env, j->status, &v);
    napi_set_named_property(env, out, "status", v);
    napi_create_uint32(env, j->status ? j->err_info[0] : 3u, &v);
    napi_set_named_property(env, out, "errClass", v);
    napi_create_uint32(env, j->status ? j->err_info[1] : 0u, &v);
    napi_set_named_property(env, out, "errIndex", v);
    napi_create_double(env, j->t_start_ns, &v);
    napi_set_named_property(env, out, "workerStartNs", v);
    napi_create_double(env, j->t_end_ns, &v);
    napi_set_named_property(env, out, "workerEndNs", v);
    napi_resolve_deferred(env, j->deferred, out);
  } else if (j->kind == JOB_FINAL) {
    napi_value out;
    napi_get_boolean(env, j->verdict == 1, &out);
    napi_resolve_deferred(env, j->deferred, out);
  } else if (j->kind == JOB_SET_GROUP) {
    napi_value out;
    napi_get_undefined(env, &out);
    napi_resolve_deferred(env, j->deferred, out);
  } else if (j->kind == JOB_AGG_SPANS) {
    /* {keys: Uint8Array(96 n), codes: Int32Array(n)} */
    const size_t n = j->n_span_sets;
    napi_value out, ab, v;
    void* dst;
    napi_create_object(env, &out);
    napi_create_arraybuffer(env, 96 * (n ? n : 1), &dst, &ab);
    memcpy(dst, j->agg_out, 96 * n);
    napi_create_typedarray(env, napi_uint8_array, 96 * n, ab, 0, &v);
    napi_set_named_property(env, out, "keys", v);
    napi_create_arraybuffer(env, 4 * (n ? n : 1), &dst, &ab);
    memcpy(dst, j->verdicts, 4 * n);
    napi_create_typedarray(env, napi_int32_array, n, ab, 0, &v);
    napi_set_named_property(env, out, "codes", v);
    napi_resolve_deferred(env, j->deferred, out);
  } else {
    napi_value ab, out;
    void* dst;
    uint32_t n = j->kind == JOB_SAME_MSG ? j->same.n_sets : j->kind == JOB_DEPOSITS ? j->dep.n : j->batch.n_reqs;
    napi_create_arraybuffer(env, 4 * (size_t)(n ? n : 1), &dst, &ab);
    memcpy(dst, j->verdicts, 4 * (size_t)n);
    napi_create_typedarray(env, napi_int32_array, n, ab, 0, &out);
    attach_stats(env, out, &j->stats, j->t_start_ns, j->t_end_ns);
    if (j->kind == JOB_SAME_MSG || j->kind == JOB_DEPOSITS) {
      napi_value v;
      napi_create_uint32(env, j->stats.n_chunks, &v);
      napi_set_named_property(env, out, "nChunks", v);
      napi_create_uint32(env, j->stats.n_individual, &v);
      napi_set_named_property(env, out, "nIndividual", v);
    }
    napi_resolve_deferred(env, j->deferred, out);
  }
  napi_delete_reference(env, j->keep);
  napi_delete_reference(env, j->keep_handle);
  napi_delete_async_work(env, j->work);
  j->h->inflight -= 1;
  handle_release_if_idle(j->h);
  free(j->verdicts);
  free(j->agg_out);
  free(j);
}

static int prop(napi_env env, napi_value obj, const char* name, void** data, size_t* bytes) {
  napi_value v;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return -1;
  return view_of(env, v, data, bytes);
}

/* Parse and check a request object into a bls_batch (buffers stay owned by the object). */
static int parse_request(napi_env env, napi_value req, bls_batch* b) {
  void *ro, *rb, *msg, *sig, *spo, *pki, *pks, *sl, *seed;
  size_t nro, nrb, nmsg, nsig, nspo, npki, npks, nsl, nseed;
  if (prop(env, req, "reqSetOffsets", &ro, &nro) || prop(env, req, "reqBatchable", &rb, &nrb) ||
      prop(env, req, "messages", &msg, &nmsg) || prop(env, req, "signatures", &sig, &nsig) ||
      prop(env, req, "setPkOffsets", &spo, &nspo) || prop(env, req, "pkIndices", &pki, &npki) ||
      prop(env, req, "pubkeys", &pks, &npks) || prop(env, req, "signatureLens", &sl, &nsl) ||
      prop(env, req, "seed", &seed, &nseed) || nro < 4 || !ro) {
    napi_throw_type_error(env, NULL, "verify: bad request object");
    return -1;
  }
  /* every buffer must hold what n_reqs / n_sets say: the library reads exactly that */
  const uint32_t n_reqs = (uint32_t)(nro / 4 - 1);
  const uint32_t n_sets = ((const uint32_t*)ro)[n_reqs];
  const size_t ns = n_sets;
  int ok = nrb >= n_reqs && nmsg >= 32 * ns && nsig >= 96 * ns && (!sl || nsl >= 4 * ns);
  if (spo) ok = ok && nspo >= 4 * (ns + 1) && npki >= 4 * (size_t)((const uint32_t*)spo)[n_sets];
  else ok = ok && pks && npks >= 96 * ns;
  if (!ok) {
    napi_throw_range_error(env, NULL, "verify: a buffer is shorter than n_reqs / n_sets require "
                                      "(pubkeys 96 B, messages 32 B, signatures 96 B per set)");
    return -1;
  }
  memset(b, 0, sizeof(*b));
  b->n_reqs = n_reqs;
  b->n_sets = n_sets;
  b->req_set_offsets = (const uint32_t*)ro;
  b->req_batchable = (const uint8_t*)rb;
  b->messages = (const uint8_t*)msg;
  b->signatures = (const uint8_t*)sig;
  b->set_pk_offsets = (const uint32_t*)spo;
  b->pk_indices = (const uint32_t*)pki;
  b->pubkeys = spo ? NULL : (const uint8_t*)pks;
  b->signature_lens = (const uint32_t*)sl;
  b->seed = nseed >= 32 ? (const uint8_t*)seed : NULL;
  return 0;
}

/* queue j on a libuv worker: keep = the object holding the input buffers */
static napi_value queue_job(napi_env env, bls_handle* h, verify_job* j, napi_value handle, napi_value keep) {
  j->h = h;
  j->ctx = h->ctx;
  napi_value promise, name;
  CHECK(env, napi_create_reference(env, keep, 1, &j->keep));
  CHECK(env, napi_create_reference(env, handle, 1, &j->keep_handle));
  CHECK(env, napi_create_promise(env, &j->deferred, &promise));
  CHECK(env, napi_create_string_utf8(env, "lodestar_bls_verify", NAPI_AUTO_LENGTH, &name));
  CHECK(env, napi_create_async_work(env, NULL, name, verify_execute, verify_complete, j, &j->work));
  CHECK(env, napi_queue_async_work(env, j->work));
  h->inflight += 1;
  return promise;
}

static napi_value js_verify(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verify(handle, request): no live handle (closed?)");
    return NULL;
  }
  bls_batch b;
  if (parse_request(env, argv[1], &b)) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_VERIFY;
  j->batch = b;
  j->verdicts = (int32_t*)calloc(b.n_reqs ? b.n_reqs : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* verifyCommittees(handle, request) -> Promise<Int32Array>: bls_gpu_verify_committees on a
 * libuv worker.  The request is verify's (table indices) with setCommittee (Uint32Array,
 * one BLS_COMMITTEE_REF or BLS_SET_NO_COMMITTEE per set), setBitsOff (Uint32Array, n_sets +
 * 1) and bits (Uint8Array); the library checks the offsets themselves. */
static napi_value js_verify_committees(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verifyCommittees(handle, request): no live handle (closed?)");
    return NULL;
  }
  bls_batch b;
  if (parse_request(env, argv[1], &b)) return NULL;
  void *sc, *sbo, *bits;
  size_t nsc, nsbo, nbits;
  if (prop(env, argv[1], "setCommittee", &sc, &nsc) || prop(env, argv[1], "setBitsOff", &sbo, &nsbo) ||
      prop(env, argv[1], "bits", &bits, &nbits) || !sc || !sbo) {
    napi_throw_type_error(env, NULL, "verifyCommittees: setCommittee / setBitsOff / bits missing");
    return NULL;
  }
  const size_t ns = b.n_sets;
  if (nsc < 4 * ns || nsbo < 4 * (ns + 1) || nbits < ((const uint32_t*)sbo)[ns]) {
    napi_throw_range_error(env, NULL, "verifyCommittees: setCommittee, setBitsOff or bits is shorter than n_sets "
                                      "and the last offset require");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_COMMITTEES;
  j->batch = b;
  j->cs.set_committee = (const uint32_t*)sc;
  j->cs.set_bits_off = (const uint32_t*)sbo;
  j->cs.bits = (const uint8_t*)bits;
  j->verdicts = (int32_t*)calloc(b.n_reqs ? b.n_reqs : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* The span arrays of a request into a bls_span_sets: setSpanOff (Uint32Array, n_sets + 1),
 * spanRefs (Uint32Array, one BLS_COMMITTEE_REF per segment), setBitsOff (Uint32Array, n_sets
 * + 1) and bits (Uint8Array).  Only what the library would read past a buffer's end is
 * refused here; it checks the offsets themselves and names the set. */
static int parse_spans(napi_env env, napi_value req, size_t n_sets, bls_span_sets* ss, const char* who) {
  void *so, *refs, *sbo, *bits;
  size_t nso, nrefs, nsbo, nbits;
  char text[160];
  if (prop(env, req, "setSpanOff", &so, &nso) || prop(env, req, "spanRefs", &refs, &nrefs) ||
      prop(env, req, "setBitsOff", &sbo, &nsbo) || prop(env, req, "bits", &bits, &nbits) || !so || !sbo) {
    snprintf(text, sizeof(text), "%s: setSpanOff / spanRefs / setBitsOff / bits missing", who);
    napi_throw_type_error(env, NULL, text);
    return -1;
  }
  if (nso < 4 * (n_sets + 1) || nsbo < 4 * (n_sets + 1) || nrefs < 4 * (size_t)((const uint32_t*)so)[n_sets] ||
      nbits < ((const uint32_t*)sbo)[n_sets]) {
    snprintf(text, sizeof(text), "%s: setSpanOff, spanRefs, setBitsOff or bits is shorter than n_sets and the last "
                                 "offsets require", who);
    napi_throw_range_error(env, NULL, text);
    return -1;
  }
  ss->set_span_off = (const uint32_t*)so;
  ss->span_refs = (const uint32_t*)refs;
  ss->set_bits_off = (const uint32_t*)sbo;
  ss->bits = (const uint8_t*)bits;
  return 0;
}

/* verifySpans(handle, request) -> Promise<Int32Array>: bls_gpu_verify_spans on a libuv
 * worker.  The request is verify's (table indices) with the span arrays of parse_spans. */
static napi_value js_verify_spans(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verifySpans(handle, request): no live handle (closed?)");
    return NULL;
  }
  bls_batch b;
  if (parse_request(env, argv[1], &b)) return NULL;
  bls_span_sets ss;
  if (parse_spans(env, argv[1], b.n_sets, &ss, "verifySpans")) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_SPANS;
  j->batch = b;
  j->ss = ss;
  j->verdicts = (int32_t*)calloc(b.n_reqs ? b.n_reqs : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* aggregateSpans(handle, {setSpanOff, spanRefs, setBitsOff, bits}) -> Promise<{keys, codes}>:
 * bls_gpu_aggregate_spans on a libuv worker; n_sets = setSpanOff.length - 1.  keys holds the
 * 96-byte uncompressed aggregate of each span, codes its status. */
static napi_value js_aggregate_spans(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  void* so;
  size_t nso;
  if (!h || prop(env, argv[1], "setSpanOff", &so, &nso) || !so || nso < 4) {
    napi_throw_type_error(env, NULL, "aggregateSpans(handle, {setSpanOff, spanRefs, setBitsOff, bits})");
    return NULL;
  }
  const size_t n = nso / 4 - 1;
  bls_span_sets ss;
  if (parse_spans(env, argv[1], n, &ss, "aggregateSpans")) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_AGG_SPANS;
  j->ss = ss;
  j->n_span_sets = (uint32_t)n;
  j->agg_out = (uint8_t*)calloc(n ? n : 1, 96);
  j->verdicts = (int32_t*)calloc(n ? n : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* setCommitteeGroup(handle, group, {memberOffsets, members}) -> Promise<void>:
 * bls_gpu_set_committee_group on a libuv worker (an epoch's shuffling is a few MB to copy
 * and ~2048 committees to sum); n = memberOffsets.length - 1, an empty memberOffsets drops
 * the group.  A rejected registration rejects with the library's message. */
static napi_value js_set_committee_group(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 3 ? get_handle(env, argv[0]) : NULL;
  uint32_t group = 0;
  void *mo, *mem;
  size_t nmo, nmem;
  if (!h || napi_get_value_uint32(env, argv[1], &group) != napi_ok || prop(env, argv[2], "memberOffsets", &mo, &nmo) ||
      prop(env, argv[2], "members", &mem, &nmem)) {
    napi_throw_type_error(env, NULL, "setCommitteeGroup(handle, group, {memberOffsets, members})");
    return NULL;
  }
  const uint32_t n = nmo >= 8 ? (uint32_t)(nmo / 4 - 1) : 0;
  /* members must hold what the last offset says when the offsets are monotone; the library
   * names the committee when they are not */
  if (n) {
    const uint32_t* o = (const uint32_t*)mo;
    uint32_t top = 0;
    for (uint32_t c = 0; c <= n; ++c)
      if (o[c] > top) top = o[c];
    if (nmem < 4 * (size_t)top) {
      napi_throw_range_error(env, NULL, "setCommitteeGroup: members is shorter than memberOffsets require");
      return NULL;
    }
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_SET_GROUP;
  j->group = group;
  j->n_committees = n;
  j->member_offsets = (const uint32_t*)mo;
  j->members = (const uint32_t*)mem;
  return queue_job(env, h, j, argv[0], argv[2]);
}

/* committeeGroupInfo(handle, group) -> {nCommittees, nMembers, deviceBytes} */
static napi_value js_committee_group_info(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  uint32_t group = 0;
  if (!h || napi_get_value_uint32(env, argv[1], &group) != napi_ok) {
    napi_throw_type_error(env, NULL, "committeeGroupInfo(handle, group)");
    return NULL;
  }
  bls_committee_info ci;
  if (bls_gpu_committee_group_info(h->ctx, group, &ci) != 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  const char* names[3] = {"nCommittees", "nMembers", "deviceBytes"};
  const double vals[3] = {(double)ci.n_committees, (double)ci.n_members, (double)ci.device_bytes};
  napi_value obj;
  CHECK(env, napi_create_object(env, &obj));
  for (int i = 0; i < 3; ++i) {
    napi_value v;
    CHECK(env, napi_create_double(env, vals[i], &v));
    CHECK(env, napi_set_named_property(env, obj, names[i], v));
  }
  return obj;
}

/* verifySameMessage(handle, {jobSetOffsets, messages, pkIndices, signatures, seed?}) ->
 * Promise<Int32Array>: bls_gpu_verify_same_message on a libuv worker, one verdict per set.
 * The buffer sizes are checked here; the library checks the offsets themselves (an empty
 * job rejects with its -2 and message). */
static napi_value js_verify_same_message(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verifySameMessage(handle, request): no live handle (closed?)");
    return NULL;
  }
  void *jo, *msg, *pki, *sig, *seed;
  size_t njo, nmsg, npki, nsig, nseed;
  if (prop(env, argv[1], "jobSetOffsets", &jo, &njo) || prop(env, argv[1], "messages", &msg, &nmsg) ||
      prop(env, argv[1], "pkIndices", &pki, &npki) || prop(env, argv[1], "signatures", &sig, &nsig) ||
      prop(env, argv[1], "seed", &seed, &nseed) || njo < 4 || !jo) {
    napi_throw_type_error(env, NULL, "verifySameMessage: bad request object");
    return NULL;
  }
  const uint32_t n_jobs = (uint32_t)(njo / 4 - 1);
  const uint32_t n_sets = ((const uint32_t*)jo)[n_jobs];
  if (nmsg < 32 * (size_t)n_jobs || npki < 4 * (size_t)n_sets || nsig < 96 * (size_t)n_sets) {
    napi_throw_range_error(env, NULL, "verifySameMessage: a buffer is shorter than n_jobs / n_sets require "
                                      "(messages 32 B per job, pkIndices 4 B and signatures 96 B per set)");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_SAME_MSG;
  j->same.n_jobs = n_jobs;
  j->same.n_sets = n_sets;
  j->same.job_set_offsets = (const uint32_t*)jo;
  j->same.messages = (const uint8_t*)msg;
  j->same.pk_indices = (const uint32_t*)pki;
  j->same.signatures = (const uint8_t*)sig;
  j->same.seed = nseed >= 32 ? (const uint8_t*)seed : NULL;
  j->verdicts = (int32_t*)calloc(n_sets ? n_sets : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* verifyDeposits(handle, {pubkeys, withdrawalCredentials, amounts, signatures, domain, seed?})
 * -> Promise<Int32Array>: bls_gpu_verify_deposits on a libuv worker, one code per deposit.
 * n = pubkeys.length / 48; every other buffer must hold what n says. */
static napi_value js_verify_deposits(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verifyDeposits(handle, request): no live handle (closed?)");
    return NULL;
  }
  void *pks, *wc, *amt, *sig, *dom, *seed;
  size_t npks, nwc, namt, nsig, ndom, nseed;
  if (prop(env, argv[1], "pubkeys", &pks, &npks) || prop(env, argv[1], "withdrawalCredentials", &wc, &nwc) ||
      prop(env, argv[1], "amounts", &amt, &namt) || prop(env, argv[1], "signatures", &sig, &nsig) ||
      prop(env, argv[1], "domain", &dom, &ndom) || prop(env, argv[1], "seed", &seed, &nseed) || npks % 48 != 0) {
    napi_throw_type_error(env, NULL, "verifyDeposits: bad request object");
    return NULL;
  }
  const size_t n = npks / 48;
  if (n > BLS_DEPOSITS_MAX_CALL || nwc < 32 * n || namt < 8 * n || nsig < 96 * n || ndom < 32 ||
      (n > 0 && (!pks || !wc || !amt || !sig || !dom))) {
    napi_throw_range_error(env, NULL, "verifyDeposits: more than BLS_DEPOSITS_MAX_CALL deposits, or a buffer is "
                                      "shorter than n requires (pubkeys 48 B, withdrawalCredentials 32 B, amounts "
                                      "8 B, signatures 96 B per deposit; domain 32 B)");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_DEPOSITS;
  j->dep.n = (uint32_t)n;
  j->dep.pubkeys48 = (const uint8_t*)pks;
  j->dep.withdrawal_credentials = (const uint8_t*)wc;
  j->dep.amounts = (const uint8_t*)amt;
  j->dep.signatures = (const uint8_t*)sig;
  j->dep.domain = (const uint8_t*)dom;
  j->dep.seed = nseed >= 32 ? (const uint8_t*)seed : NULL;
  j->verdicts = (int32_t*)calloc(n ? n : 1, 4);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* partial(handle, request, setIndexBase) -> Promise<{partial, status, errClass, errIndex}>:
 * bls_gpu_partial on a libuv worker -- one device's shard of a call split across the
 * devices of the node (gpuBlsVerifier.js splitCall). */
static napi_value js_partial(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 3 ? get_handle(env, argv[0]) : NULL;
  uint32_t base = 0;
  if (!h || napi_get_value_uint32(env, argv[2], &base) != napi_ok) {
    napi_throw_type_error(env, NULL, "partial(handle, request, setIndexBase): no live handle (closed?)");
    return NULL;
  }
  bls_batch b;
  if (parse_request(env, argv[1], &b)) return NULL;
  if (!b.seed || b.n_sets == 0) {
    napi_throw_range_error(env, NULL, "partial: the request needs >= 1 set and the call's 32-byte seed");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_PARTIAL;
  j->batch = b;
  j->base = base;
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* finalCheck(handle, partials) -> Promise<boolean>: FE(prod partials) == 1, bls_gpu_final_check. */
static napi_value js_final_check(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  void* p = NULL;
  size_t bytes = 0;
  if (!h || view_of(env, argv[1], &p, &bytes) || !p || bytes == 0 || bytes % 576) {
    napi_throw_type_error(env, NULL, "finalCheck(handle, Uint8Array of 576-byte partials)");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof(verify_job));
  j->kind = JOB_FINAL;
  j->partials = (const uint8_t*)p;
  j->n_partials = (uint32_t)(bytes / 576);
  return queue_job(env, h, j, argv[0], argv[1]);
}

/* verifySync(handle, request) -> Int32Array: the same call on the calling thread, for the
 * synchronous state-transition path (verifySignatureSet, state-transition
 * src/util/signatureSets.ts:24-38), which blocks the main thread as blst's verify does. */
static napi_value js_verify_sync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 2 ? get_handle(env, argv[0]) : NULL;
  if (!h) {
    napi_throw_type_error(env, NULL, "verifySync(handle, request): no live handle (closed?)");
    return NULL;
  }
  bls_batch b;
  if (parse_request(env, argv[1], &b)) return NULL;
  napi_value ab, out;
  void* dst;
  CHECK(env, napi_create_arraybuffer(env, 4 * (size_t)(b.n_reqs ? b.n_reqs : 1), &dst, &ab));
  CHECK(env, napi_create_typedarray(env, napi_int32_array, b.n_reqs, ab, 0, &out));
  bls_stats st;
  const double t0 = mono_ns();
  if (bls_gpu_verify(h->ctx, &b, (int32_t*)dst, &st) != 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  attach_stats(env, out, &st, t0, mono_ns());
  return out;
}

/* sszRoots(handle, kind, objs, domains | null) -> Uint8Array(32 n): computeSigningRoot
 * (signingRoot.ts:7-13) for n serialized objects of one BLS_SSZ_* kind on the GPU;
 * domains: 32 bytes for all, 32 per object, or null for the hash_tree_roots.  Synchronous
 * (a few SHA-256 compressions per object). */
static napi_value js_ssz_roots(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bls_handle* h = argc >= 3 ? get_handle(env, argv[0]) : NULL;
  uint32_t kind = 0;
  void *objs = NULL, *doms = NULL;
  size_t ob = 0, db = 0;
  if (!h || napi_get_value_uint32(env, argv[1], &kind) != napi_ok || view_of(env, argv[2], &objs, &ob) ||
      (argc > 3 && view_of(env, argv[3], &doms, &db))) {
    napi_throw_type_error(env, NULL, "sszRoots(handle, kind, Uint8Array, domains)");
    return NULL;
  }
  const uint32_t size = BLS_SSZ_SIZE(kind);
  if (size == 0 || ob % size) {
    napi_throw_range_error(env, NULL, "sszRoots: objects are not a whole number of the kind's size");
    return NULL;
  }
  const uint32_t n = (uint32_t)(ob / size);
  uint32_t stride = 0;
  if (doms && db == 32ull * n && n != 1) stride = 32;
  else if (doms && db != 32) {
    napi_throw_range_error(env, NULL, "sszRoots: domains must be 32 bytes or 32 bytes per object");
    return NULL;
  }
  napi_value ab, out;
  void* roots;
  CHECK(env, napi_create_arraybuffer(env, 32 * (size_t)(n ? n : 1), &roots, &ab));
  CHECK(env, napi_create_typedarray(env, napi_uint8_array, 32 * (size_t)n, ab, 0, &out));
  if (bls_gpu_ssz_roots(h->ctx, kind, (const uint8_t*)objs, n, (const uint8_t*)doms, stride, (uint8_t*)roots) < 0) {
    napi_throw_error(env, NULL, bls_gpu_last_error(h->ctx));
    return NULL;
  }
  return out;
}

/* $BLS_NAPI_SEGV_TRACE=1 (diagnostics): a native backtrace on stderr if the process takes
 * SIGSEGV / SIGABRT / SIGBUS, then the default action; and a note when the process
 * reaches exit handlers, so a crash at exit can be placed */
static void segv_trace(int sig) {
  void* fr[64];
  const int n = backtrace(fr, 64);
  static const char head[] = "lodestar_bls: fatal signal, native backtrace:\n";
  (void)!write(2, head, sizeof(head) - 1);
  backtrace_symbols_fd(fr, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
static void exit_note(void) {
  static const char msg[] = "lodestar_bls: exit handlers running\n";
  (void)!write(2, msg, sizeof(msg) - 1);
}

static napi_value module_init(napi_env env, napi_value exports) {
  const char* tr = getenv("BLS_NAPI_SEGV_TRACE");
  if (tr && *tr == '1') {
    signal(SIGSEGV, segv_trace);
    signal(SIGABRT, segv_trace);
    signal(SIGBUS, segv_trace);
    atexit(exit_note);
  }
  napi_property_descriptor d[] = {
      {"init", NULL, js_init, NULL, NULL, NULL, napi_default, NULL},
      {"close", NULL, js_close, NULL, NULL, NULL, napi_default, NULL},
      {"loadPubkeys", NULL, js_load_pubkeys, NULL, NULL, NULL, napi_default, NULL},
      {"sharePubkeys", NULL, js_share_pubkeys, NULL, NULL, NULL, napi_default, NULL},
      {"pubkeysInfo", NULL, js_pubkeys_info, NULL, NULL, NULL, napi_default, NULL},
      {"verify", NULL, js_verify, NULL, NULL, NULL, napi_default, NULL},
      {"verifySync", NULL, js_verify_sync, NULL, NULL, NULL, napi_default, NULL},
      {"sszRoots", NULL, js_ssz_roots, NULL, NULL, NULL, napi_default, NULL},
      {"partial", NULL, js_partial, NULL, NULL, NULL, napi_default, NULL},
      {"finalCheck", NULL, js_final_check, NULL, NULL, NULL, napi_default, NULL},
      {"verifySameMessage", NULL, js_verify_same_message, NULL, NULL, NULL, napi_default, NULL},
      {"verifyDeposits", NULL, js_verify_deposits, NULL, NULL, NULL, napi_default, NULL},
      {"verifyCommittees", NULL, js_verify_committees, NULL, NULL, NULL, napi_default, NULL},
      {"verifySpans", NULL, js_verify_spans, NULL, NULL, NULL, napi_default, NULL},
      {"aggregateSpans", NULL, js_aggregate_spans, NULL, NULL, NULL, napi_default, NULL},
      {"setCommitteeGroup", NULL, js_set_committee_group, NULL, NULL, NULL, napi_default, NULL},
      {"committeeGroupInfo", NULL, js_committee_group_info, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof(d) / sizeof(d[0]), d);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, module_init)
