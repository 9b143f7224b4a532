/*
 * delta_gpu.h — C ABI of the MI355X-native delta codec (libdeltagpu.so).
 *
 * Drop-in boundary for the hot path of darrelllong/Delta-Compression:
 *
 *   reference chain (src/c/main.c:257-292)          this library
 *   ---------------------------------------------   ---------------------------
 *   delta_crc64_xz(R), delta_crc64_xz(V)            \
 *     (src/c/delta.h:294-322)                        \
 *   delta_diff(ALGO_GREEDY|ALGO_ONEPASS|              > dg_encode / dg_encode_batch /
 *     ALGO_CORRECTING, ...)                          /  dg_encode_plan_run
 *     (src/c/correcting.c:499-519 -> greedy.c:88,   /
 *      onepass.c:32, correcting.c:81)              /
 *   delta_place_commands (src/c/apply.c:136-164)   /
 *   delta_encode(placed, false, |V|, src, dst)    /
 *     (src/c/encoding.c:39-90)
 *   delta_decode + delta_apply_placed(_inplace)     dg_decode / dg_decode_batch
 *     + CRC checks (encoding.c:111-178,
 *       apply.c:229-284, main.c:341-385)
 *   delta_apply_placed_inplace in the caller's      dg_update_plan_run / dg_update_batch
 *     own buffer (apply.c:253-284), after the        (the buffer that holds R becomes V;
 *     whole parse and the source CRC check           nothing is stored before both passed)
 *     (encoding.c:111-178, main.c:341-356)
 *   delta_crc64_xz (delta.h:294)                    dg_crc64_xz / dg_crc64_xz_batch_device
 *
 * Output bytes are identical to the reference's `delta encode` at the same
 * --seed-len / --table-size / --max-table (the DLT\x03 format of
 * src/c/encoding.c:39-90, README.md:125-149).
 *
 * Differences from the reference contract (src/c/delta.h), by design:
 *   - every call returns a dg_status_t instead of abort()/exit(1)
 *     (delta.h:44-79, encoding.c:119-172);
 *   - no per-command allocations: results are arenas with explicit frees;
 *   - thread-safe: constant tables are built at context creation;
 *   - DELTA_OPT_SPLAY (delta.h:222) is accepted for ALGO_GREEDY only, where
 *     it selects the smallest instead of the largest offset among the longest
 *     matches (its only effect on greedy's output, greedy.c:174-216); with
 *     onepass or correcting it is rejected with DG_ERR_UNSUPPORTED (splay
 *     changes their output);
 *   - greedy ignores q, max_table and buf_cap (as the reference's greedy
 *     does: its output does not depend on its hash table).  Each pair's R is
 *     indexed whole on the device: 4 (B + 1) + 8 S bytes for S = |R| - p + 1
 *     seeds and B = S rounded up to a power of two, at most 64 GiB per plan
 *     (DG_ERR_NOMEM above that).  Like the reference's, its time is quadratic
 *     on self-similar data (every equal seed is a candidate, each extended
 *     to its end: a long run of one byte, a short period): one such pair
 *     holds its wave for as long, while the rest of the batch proceeds;
 *   - inputs of 4 GiB or more are rejected (DG_ERR_TOO_LARGE): the format's
 *     u32 fields would silently truncate them (encoding.c:63,72-78).
 *
 * All device pointers are plain HIP device pointers; `stream` is a
 * hipStream_t passed as void* (NULL = the context's own stream).  No C++ or
 * torch types cross this boundary.
 */
#ifndef DELTA_GPU_H
#define DELTA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_ABI_VERSION 3

/* Defaults mirror src/c/delta.h:21-35. */
#define DG_SEED_LEN        16
#define DG_TABLE_SIZE      1048573UL
#define DG_MAX_TABLE_SIZE  1073741827UL
#define DG_BUF_CAP         256
#define DG_HEADER_SIZE     25
#define DG_CRC_SIZE        8

typedef enum {
	DG_OK              = 0,
	DG_ERR_INVALID_ARG = 1,
	DG_ERR_UNSUPPORTED = 2,   /* --splay with onepass or correcting, --inplace on an
	                             encode plan, a delta the device converter leaves to the host,
	                             a standard delta given to dg_update_plan_run */
	DG_ERR_TOO_LARGE   = 3,   /* a buffer >= 4 GiB */
	DG_ERR_NO_DEVICE   = 4,
	DG_ERR_HIP         = 5,
	DG_ERR_NOMEM       = 6,
	DG_ERR_CAPACITY    = 7,   /* output arena too small */
	DG_ERR_MALFORMED   = 8,   /* not a delta / truncated / bad command */
	DG_ERR_SRC_CRC     = 9,   /* reference does not match src_crc */
	DG_ERR_DST_CRC     = 10,  /* reconstructed output does not match dst_crc */
	DG_ERR_TABLE_POOL  = 11,  /* onepass: no work table came free within the
	                             wait bound (more long-epoch pairs in flight than
	                             tables; raise DG_LIMIT_TABLE_POOL_BYTES) */
	DG_ERR_INTERNAL    = 12   /* a device-side invariant failed (a library bug:
	                             segment list overflow, a member chain that ran
	                             out of members, serialiser size disagreement) */
} dg_status_t;

/* Numbering matches delta_algorithm_t (src/c/delta.h:85). */
typedef enum {
	DG_ALGO_GREEDY     = 0,
	DG_ALGO_ONEPASS    = 1,
	DG_ALGO_CORRECTING = 2
} dg_algorithm_t;

/* Option bits of delta_flags_t (src/c/delta.h:220-224). */
#define DG_OPT_VERBOSE 0
#define DG_OPT_SPLAY   1
#define DG_OPT_INPLACE 2
/* bit index of the in-place cycle policy for DG_OPT_INPLACE encodes
 * (main.c --policy): clear = localmin, set = constant (delta.h:86) */
#define DG_OPT_POLICY_CONSTANT 3

/* Layout- and meaning-identical to delta_diff_options_t (src/c/delta.h:248-257):
 * p = seed length, q = hash table size floor (--table-size), buf_cap =
 * correcting lookback capacity, max_table = correcting table ceiling. */
typedef struct {
	size_t   p;
	size_t   q;
	size_t   buf_cap;
	size_t   max_table;
	uint64_t flags;
} dg_diff_options_t;

/* DELTA_DIFF_OPTIONS_DEFAULT (src/c/delta.h:256-257). */
void dg_diff_options_default(dg_diff_options_t *opts);

/* A delta / output buffer; layout-identical to delta_buffer_t
 * (src/c/delta.h:331-334).  Free with dg_buffer_free. */
typedef struct {
	uint8_t *data;
	size_t   len;
} dg_buffer_t;

void dg_buffer_free(dg_buffer_t *buf);

/* ── context ───────────────────────────────────────────────────────────── */

typedef struct dg_context dg_context_t;

/* Binds a HIP device (device < 0: the current device) and creates one HIP
 * stream plus the constant tables.  Fails with DG_ERR_NO_DEVICE when no GPU
 * is visible: there is no CPU fallback. */
int  dg_context_create(int device, dg_context_t **out);
void dg_context_destroy(dg_context_t *ctx);
/* Current hipStream_t of the context, as void*. */
void *dg_context_stream(dg_context_t *ctx);
const char *dg_status_string(int status);
/* Last error text recorded on this context (never NULL). */
const char *dg_last_error(const dg_context_t *ctx);
int dg_abi_version(void);

/* Resource limits of a context; they apply to plans created afterwards.
 *   DG_LIMIT_TABLE_POOL_BYTES: device bytes for the onepass work tables that
 *     epochs longer than 256 steps spill into (one table = 16 B x q, held by
 *     a pair from its first long epoch to its end).  0 = automatic: enough
 *     tables for every resident wave, capped at 4 GiB (at least 1 GiB).
 *     Pairs beyond the table count wait for one; a wait longer than the
 *     bound ends the pair with DG_ERR_TABLE_POOL. */
#define DG_LIMIT_TABLE_POOL_BYTES 0
/*   DG_LIMIT_ONEPASS_MEMBERS: how onepass plans (seed length 16, 16-byte
 *     aligned pairs) run the epoch chain.  0 = automatic, 1 = verified
 *     diagonal members first (the chain walks only unverified members), 2 =
 *     the plain per-pair chain.  Output bytes are identical in every mode.
 *     Member mode needs about 1.3 B of extra device memory per position of
 *     min(|R|, |V|) (20 B for each of 129 member slots per 2 KiB chunk); when
 *     that allocation fails in automatic mode the plan falls back to the
 *     plain chain, and only a forced mode 1 returns DG_ERR_NOMEM. */
#define DG_LIMIT_ONEPASS_MEMBERS 1
int dg_context_set_limit(dg_context_t *ctx, int limit, uint64_t value);

/* ── batched, device-resident encode: the hot path ───────────────────────
 *
 * A batch is N independent (reference, version) pairs laid out in two device
 * arenas.  A plan fixes the pair geometry and options once (table sizes,
 * worst-case command capacity, work buffers, CRC segmentation) so that
 * dg_encode_plan_run is pure device work on one stream (graph-capturable:
 * no allocation, no host synchronisation).
 *
 * Output: one packed arena.  Pair i's delta occupies
 * d_out[d_offsets[i] .. d_offsets[i+1]) and is byte-identical to the
 * reference's `delta encode <algo> R_i V_i` output.  d_status[i] is a
 * dg_status_t.  d_offsets has N+1 entries (d_offsets[N] = total bytes).
 */
typedef struct {
	uint64_t r_off;   /* byte offset of R_i in the reference arena */
	uint64_t r_len;
	uint64_t v_off;   /* byte offset of V_i in the version arena */
	uint64_t v_len;
} dg_pair_t;

typedef struct dg_encode_plan dg_encode_plan_t;

int dg_encode_plan_create(dg_context_t *ctx, dg_algorithm_t algo,
                          const dg_pair_t *pairs /* host */, uint32_t n_pairs,
                          const dg_diff_options_t *opts,
                          dg_encode_plan_t **out);
/* Upper bound of the packed output (bytes): size d_out at least this. */
uint64_t dg_encode_plan_output_bound(const dg_encode_plan_t *plan);
uint32_t dg_encode_plan_num_pairs(const dg_encode_plan_t *plan);
/* Table size q actually used for pair i (onepass.c:61-62 /
 * correcting.c:116-123 sizing); 0 for a greedy plan, which has none. */
uint64_t dg_encode_plan_table_size(const dg_encode_plan_t *plan, uint32_t i);
/* One run of the plan over the bytes the arenas hold when the stream reaches
 * it; a plan is run any number of times, on other bytes of the same layout
 * each time, and no run sees anything of the runs before it.
 *   Arguments.  d_ref_arena and d_ver_arena are 16-byte aligned; d_out needs
 *     no alignment.  A NULL device pointer or a misaligned arena returns
 *     DG_ERR_INVALID_ARG before anything is enqueued.  A plan of zero pairs
 *     returns DG_OK and touches nothing (every pointer may be NULL).
 *   Sizes.  d_offsets always receives the true sizes: d_offsets[i+1] -
 *     d_offsets[i] is the size of pair i's delta whether or not it was
 *     written, so d_offsets[N] is the out_cap with which every pair fits
 *     (at most dg_encode_plan_output_bound).
 *   Capacity.  A pair whose end d_offsets[i+1] passes out_cap gets
 *     DG_ERR_CAPACITY and writes nothing, not even its header; the pairs
 *     before it are complete.
 *   Containment.  No byte outside d_out[0 .. min(d_offsets[N], out_cap)) is
 *     written, and of d_offsets and d_status only entries [0, N] and [0, N).
 *   Status.  Every run sets every d_status[i] anew: no status, size or other
 *     state of an earlier run stays with the plan. */
int dg_encode_plan_run(dg_encode_plan_t *plan,
                       const uint8_t *d_ref_arena, const uint8_t *d_ver_arena,
                       uint8_t *d_out, uint64_t out_cap,
                       uint64_t *d_offsets, int32_t *d_status,
                       void *stream);
/* Optional per-stage timing with HIP events on the streams the kernels run on
 * (the CRC kernels run on a plan-owned side stream forked from / joined to
 * the run stream).  dg_encode_plan_set_timing(plan, slots) with slots > 0
 * makes every run record its events into one of `slots` event sets (a ring;
 * 0 disables) and resets the run count; dg_encode_plan_stage_times fills up to
 * `n` stage durations (ms), averaged over the last min(runs, slots) runs, and
 * their names ("crc64", "diff", "scan", "serialize+join", "total", "members";
 * "members" is the member kernel alone, inside "diff", 0 in plain chain mode).  Returns
 * the number of stages.  No host synchronisation happens until stage_times.
 * Correcting plans add "corr_build" and "corr_scan" (the R-index build and
 * the V scan), greedy plans "greedy_build" and "greedy_scan" (the seed index
 * of every R and the V scan).  dg_encode_plan_set_timing_mode(plan, DG_TIMING_DOMINANT)
 * records only the events around the dominant kernel(s) — the member kernel
 * ("members"), the correcting or greedy build and scan ("corr_build",
 * "corr_scan" or "greedy_build", "greedy_scan", and "diff") or the onepass
 * kernel ("diff") — and stage_times reports those
 * only: each timing event costs the run stream a few microseconds, so a
 * throughput measurement records as few as it needs.
 * dg_encode_plan_set_timing_every(plan, k), k >= 1: only every k-th run
 * (the first after set_timing, then every k-th) records its events; the
 * ring then holds the last `slots` recorded runs.  Resets the run count. */
#define DG_TIMING_ALL      0
#define DG_TIMING_DOMINANT 1
int dg_encode_plan_set_timing(dg_encode_plan_t *plan, int slots);
int dg_encode_plan_set_timing_mode(dg_encode_plan_t *plan, int mode);
int dg_encode_plan_set_timing_every(dg_encode_plan_t *plan, int every);
int dg_encode_plan_stage_times(dg_encode_plan_t *plan, float *ms,
                               const char **names, int n);
/* --verbose counters (correcting plans): d_stats = 8 u64 per pair in device
 * memory, zeroed by the caller (NULL = off, the default): seeds passing the
 * build's checkpoint test, slots stored, scan checkpoints, fingerprint
 * mismatches, byte mismatches, matches, the checkpoint class k, passing
 * seeds whose slot is inside the table (the dbg_* counters of
 * correcting.c:95-98).  dg_encode / dg_encode_batch with DG_OPT_VERBOSE set
 * print the reference's diagnostic lines to stderr from these and the delta
 * (onepass.c:64-69, 277-285; correcting.c:137-152, 200-214, 470-485). */
int dg_encode_plan_set_stats(dg_encode_plan_t *plan, uint64_t *d_stats);
/* How the plan runs (bit flags): DG_PLAN_MEMBERS = onepass through verified
 * diagonal members (DG_LIMIT_ONEPASS_MEMBERS). */
#define DG_PLAN_MEMBERS 1u
uint32_t dg_encode_plan_flags(const dg_encode_plan_t *plan);
/* The plan's runs so far by how they ran: in member mode, and as a plain plan
 * (every run of a plan without member mode; in automatic member mode, the
 * runs of a batch whose every pair the last completed member-mode run routed
 * to the plain chain, between member-mode probes every 16th run).  The output
 * bytes are the same either way.  Returns DG_OK or DG_ERR_INVALID_ARG. */
int dg_encode_plan_run_modes(const dg_encode_plan_t *plan, uint64_t *member_runs, uint64_t *plain_runs);
/* Per-pair command statistics of the last run (device pointers owned by the
 * plan, valid until the next run): number of COPY commands and delta size. */
const uint32_t *dg_encode_plan_copy_counts_device(const dg_encode_plan_t *plan);
void dg_encode_plan_destroy(dg_encode_plan_t *plan);

/* ── host-buffer convenience (end-to-end; includes PCIe transfers) ──────── */

/* One pair: the chain of src/c/main.c:257-292, R and V in host memory.
 * out->data is malloc'd; free with dg_buffer_free. */
int dg_encode(dg_context_t *ctx, dg_algorithm_t algo,
              const uint8_t *r, size_t r_len,
              const uint8_t *v, size_t v_len,
              const dg_diff_options_t *opts, dg_buffer_t *out);

/* N pairs in host memory: pinned staging -> device -> host. outs[i] is
 * malloc'd per pair; status[i] per pair (may be NULL). */
int dg_encode_batch(dg_context_t *ctx, dg_algorithm_t algo,
                    const uint8_t *const *r, const size_t *r_len,
                    const uint8_t *const *v, const size_t *v_len,
                    uint32_t n_pairs, const dg_diff_options_t *opts,
                    dg_buffer_t *outs, int32_t *status);

/* ── Pipelined host-to-host batch encode ──────────
 * The reference's encode reads R and V from host files and writes the delta
 * back (main.c:33-121, 249-292).  For n pairs in host arenas h_ref / h_ver,
 * laid out by pairs[] as for dg_encode_plan_create, this cuts the batch into
 * chunks of consecutive pairs of about chunk_bytes of input each (0: 256 MiB)
 * and keeps two chunks in flight on two streams: the H2D copy of chunk i+1
 * and the D2H copy of chunk i-1's exact delta bytes overlap the encode of
 * chunk i.  The deltas land in h_out (out_cap bytes) packed in pair order,
 * delta i at out_offsets[i] .. out_offsets[i+1] (host, n+1 entries); status[i]
 * per pair (host, may be NULL).  Arenas and h_out from dg_host_alloc (pinned)
 * are copied directly (keeping the arena's 16-byte phase); other host memory
 * goes through pinned staging that the context keeps between calls, which
 * places every pair's streams at 16-byte offsets on the device (so unaligned
 * pageable layouts still take the LDS-window kernels).  Device buffers and
 * plans are kept too: a chunk with the same layout, options and context
 * limits as the slot's last one reuses its plan.  With DG_OPT_INPLACE in
 * opts->flags every chunk's encode is followed on the same stream by its
 * in-place conversion (dg_inplace_plan_*, policy from DG_OPT_POLICY_CONSTANT)
 * and the converted deltas are what lands in h_out.
 * Returns DG_OK (per-pair failures in status), DG_ERR_CAPACITY when h_out is
 * too small (the pairs that did not fit get status DG_ERR_CAPACITY and
 * out_offsets equal to the bytes written so far), or the first failure when
 * status is NULL. */
int dg_encode_pipelined(dg_context_t *ctx, dg_algorithm_t algo,
                        const uint8_t *h_ref, const uint8_t *h_ver,
                        const dg_pair_t *pairs, uint32_t n_pairs,
                        const dg_diff_options_t *opts, uint64_t chunk_bytes,
                        uint8_t *h_out, uint64_t out_cap,
                        uint64_t *out_offsets, int32_t *status);

/* The same host-to-host encode sharded over several devices (one context
 * per device, e.g. the 8 MI355X of a node): contiguous pair
 * ranges balanced by sum(|R|+|V|), one host thread per context running
 * dg_encode_pipelined on its range into a private buffer (sized by the
 * range's output bound), then the ranges' deltas are packed into h_out in
 * pair order: when everything fits, h_out, out_offsets and status read
 * exactly as the one-device call leaves them.  Under a tight out_cap the
 * pairs are packed up to the first one that does not fit, and it and every
 * later pair get DG_ERR_CAPACITY (a pair the device failed keeps its own
 * status) with out_offsets at the bytes written (the one-device call stops
 * at a chunk boundary instead).  No bytes move between devices.  n_ctx == 1
 * is dg_encode_pipelined.  Returns as dg_encode_pipelined (the first failing
 * range's code when status is NULL; a range that failed as a whole returns
 * its code even when status is given).  UNVERIFIED on two or more physical
 * devices: the multi-device path has only run with several contexts on one
 * device (tests/test_gpu_pipelined.py); the caller's current device is
 * restored on return. */
int dg_encode_pipelined_multi(dg_context_t *const *ctxs, uint32_t n_ctx, dg_algorithm_t algo,
                              const uint8_t *h_ref, const uint8_t *h_ver,
                              const dg_pair_t *pairs, uint32_t n_pairs,
                              const dg_diff_options_t *opts, uint64_t chunk_bytes,
                              uint8_t *h_out, uint64_t out_cap,
                              uint64_t *out_offsets, int32_t *status);

/* Pinned (page-locked) host memory for the arenas and outputs above. */
int  dg_host_alloc(dg_context_t *ctx, uint64_t bytes, void **out);
void dg_host_free(void *p);

/* ── CRC-64/XZ (delta.h:294-322), computed on the device ──────────────── */

typedef struct {
	uint64_t off;   /* byte offset into the arena */
	uint64_t len;
} dg_span_t;

/* CRC of a host buffer (copied to the device).  out = 8 bytes big-endian. */
int dg_crc64_xz(dg_context_t *ctx, const uint8_t *data, size_t len,
                uint8_t out[DG_CRC_SIZE]);
/* CRC of N spans of one device arena; d_crc receives N u64 values (the CRC
 * register value, not byte-swapped). spans are host descriptors. */
int dg_crc64_xz_batch_device(dg_context_t *ctx, const uint8_t *d_arena,
                             const dg_span_t *spans, uint32_t n,
                             uint64_t *d_crc, void *stream);

/* ── decode + apply + CRC verify (encoding.c:111-178, apply.c:229-284,
 *    main.c:341-385) ────────────────────────────────────────────────────── */

/* Decode one delta against R (host buffers).  Returns DG_OK,
 * DG_ERR_MALFORMED, DG_ERR_SRC_CRC or DG_ERR_DST_CRC (the reference's exit
 * paths); ignore_hash skips both CRC checks (main.c:330-333).  On DG_OK and
 * on DG_ERR_DST_CRC, *out holds the decoded bytes (the reference writes the
 * output before its post-check fails, main.c:374-383): free it with
 * dg_buffer_free in both cases. */
int dg_decode(dg_context_t *ctx, const uint8_t *r, size_t r_len,
              const uint8_t *delta, size_t delta_len, int ignore_hash,
              dg_buffer_t *out);

/* Batched device decode: stream i is d_delta[delta_off[i] .. +delta_len[i])
 * applied to d_ref[ref spans i]; output written to d_out at out_off[i]
 * (capacity out_cap[i] >= version_size, and >= |R| for in-place deltas).
 * d_status[i] receives a dg_status_t. Descriptors are host arrays.  The
 * output bytes the descriptors name must not overlap the reference or delta
 * bytes they name (the in-place replay runs in the output buffer after R is
 * copied into it, and the source CRC is computed from d_ref after the
 * apply): an overlapping call returns DG_ERR_INVALID_ARG and writes nothing.
 * The output is written even when a stream's source CRC check fails. */
typedef struct {
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_len;
	uint64_t out_off, out_cap;
} dg_decode_desc_t;

int dg_decode_batch_device(dg_context_t *ctx, const uint8_t *d_ref,
                           const uint8_t *d_delta,
                           const dg_decode_desc_t *descs, uint32_t n,
                           int ignore_hash, uint8_t *d_out,
                           uint64_t *d_out_len, int32_t *d_status,
                           void *stream);

/* Plan form of the batched decode (C5): descriptors uploaded once;
 * dg_decode_plan_run is one kernel launch (no host synchronisation,
 * graph-capturable) that parses and applies every stream and then computes
 * the CRC-64/XZ of its reference and of its output (length from the delta
 * header) and checks both against the header.  Status precedence per
 * stream: DG_ERR_MALFORMED / DG_ERR_CAPACITY, then DG_ERR_SRC_CRC, then
 * DG_ERR_DST_CRC (main.c:335-385).  Arena base pointers d_ref and d_out must
 * be 16-byte aligned.  Timing as for the encode plan, with one stage,
 * "decode" (the kernel, CRC checks included). */
typedef struct dg_decode_plan dg_decode_plan_t;
int dg_decode_plan_create(dg_context_t *ctx, const dg_decode_desc_t *descs,
                          uint32_t n, int ignore_hash,
                          dg_decode_plan_t **out);
int dg_decode_plan_run(dg_decode_plan_t *plan, const uint8_t *d_ref,
                       const uint8_t *d_delta, uint8_t *d_out,
                       uint64_t *d_out_len, int32_t *d_status, void *stream);
int dg_decode_plan_set_timing(dg_decode_plan_t *plan, int slots);
int dg_decode_plan_set_timing_every(dg_decode_plan_t *plan, int every);
int dg_decode_plan_stage_times(dg_decode_plan_t *plan, float *ms,
                               const char **names, int n);
void dg_decode_plan_destroy(dg_decode_plan_t *plan);

/* ── delta inspection (host parse, src/c/main.c:402-425) ─────────────── */

typedef struct {
	int      inplace;
	uint64_t version_size;
	uint8_t  src_crc[DG_CRC_SIZE];
	uint8_t  dst_crc[DG_CRC_SIZE];
	uint64_t num_commands, num_copies, num_adds;
	uint64_t copy_bytes, add_bytes;
} dg_delta_info_t;

int dg_delta_info(const uint8_t *delta, size_t len, dg_delta_info_t *info);

/* ── command lists (delta.h:94-137, 280-284, 326-368) ───────────────────
 *
 * For callers that work between the algorithm and the container, as in
 * HOWTO.md:426-464 (delta_diff -> delta_place_commands -> delta_encode;
 * delta_decode -> delta_apply_placed).  One record type serves both the
 * algorithm's commands (delta_command_t: COPY offset = src, ADD data) and the
 * placed ones (delta_placed_command_t: + dst).  Lengths and offsets are in
 * bytes; ADD data point into storage owned by the list. */
#define DG_CMD_COPY 0   /* == CMD_COPY, PCMD_COPY */
#define DG_CMD_ADD  1   /* == CMD_ADD, PCMD_ADD */
typedef struct {
	uint32_t       tag;      /* DG_CMD_COPY or DG_CMD_ADD */
	uint64_t       src;      /* COPY: offset in R (0 for ADD) */
	uint64_t       dst;      /* offset in V */
	uint64_t       length;
	const uint8_t *data;     /* ADD: `length` literal bytes (NULL for COPY) */
} dg_placed_command_t;
typedef struct {
	dg_placed_command_t *data;
	size_t               len;
	void                *storage;   /* owns data and the ADD bytes */
} dg_commands_t;
void dg_commands_free(dg_commands_t *cmds);

/* delta_diff(algo, R, V, opts) followed by delta_place_commands (apply.c:
 * 136-164): the commands of the delta dg_encode produces, in algorithm order
 * with sequential dst (so dropping dst gives delta_diff's list).  Runs on the
 * GPU for all three algorithms (DG_OPT_SPLAY: greedy only, see above);
 * DG_OPT_INPLACE in opts->flags is ignored (in-place conversion is
 * dg_make_inplace on an encoded delta). */
int dg_diff(dg_context_t *ctx, dg_algorithm_t algo,
            const uint8_t *r, size_t r_len, const uint8_t *v, size_t v_len,
            const dg_diff_options_t *opts, dg_commands_t *out);
/* delta_decode (encoding.c:111-178): the placed commands of a delta in stream
 * order, and its header (hdr may be NULL; it receives dg_delta_info's
 * summary).  DG_ERR_MALFORMED where the reference exits with "not a delta
 * file" / "truncated ..." / "unknown command type".  Host only. */
int dg_delta_decode(const uint8_t *delta, size_t len, dg_commands_t *out,
                    dg_delta_info_t *hdr);
/* delta_encode (encoding.c:39-90): placed commands -> DLT\x03 bytes,
 * out->data malloc'd.  Offsets, lengths and version_size of 4 GiB or more
 * (which the format's u32 fields cannot hold) give DG_ERR_INVALID_ARG.  Host
 * only. */
int dg_encode_commands(const dg_placed_command_t *cmds, size_t n, int inplace,
                       uint64_t version_size, const uint8_t src_crc[DG_CRC_SIZE],
                       const uint8_t dst_crc[DG_CRC_SIZE], dg_buffer_t *out);

/* ── in-place conversion (src/c/inplace.c:272-736), one delta on the host ──
 *
 * Converts a standard delta against R into an in-place delta: the chain of
 * main.c `inplace` (main.c:427-480) = delta_decode -> delta_unplace_commands
 * -> delta_make_inplace(policy) -> delta_encode(inplace = true), byte for
 * byte.  A delta that is already in-place is returned unchanged
 * (stats->already_inplace = 1).  Pure host code: no context, no GPU.
 * Like the reference it does not take the dst fields as they are: it sorts
 * the commands by dst (stable) and places them one after the other itself, in
 * 64 bits.  So a stream whose dst fields are off by some bytes, or whose
 * lengths sum past 2^32 (every dst field then being the running sum mod 2^32),
 * is converted all the same: DG_OK, the output's dst fields being the new
 * places mod 2^32.  The device plan refuses both (DG_ERR_UNSUPPORTED, below).
 * dg_encode / dg_encode_batch with DG_OPT_INPLACE (policy from
 * dg_diff_options_t.flags bit DG_OPT_POLICY_CONSTANT) run this on their
 * output; dg_encode_pipelined with DG_OPT_INPLACE and dg_make_inplace_batch
 * convert on the device instead (dg_inplace_plan_*, below). */
#define DG_POLICY_LOCALMIN 0
#define DG_POLICY_CONSTANT 1
typedef struct {
	int      already_inplace;
	uint64_t num_copies, num_adds;
	uint64_t copy_bytes, add_bytes;
} dg_inplace_stats_t;

int dg_make_inplace(const uint8_t *r, size_t r_len, const uint8_t *delta,
                    size_t delta_len, int policy, dg_buffer_t *out,
                    dg_inplace_stats_t *stats);

/* ── in-place conversion of a batch on the device ──────────────────────────
 *
 * The same conversion, byte for byte, for N standard deltas in one device
 * arena against N references in another: one wave per delta orders the
 * copies (the CRWI digraph in interval-range form), the size scan
 * packs the outputs, one block per delta writes them.  A run is two kernels
 * and the scan on one stream: no allocation, no host synchronisation.
 *
 * The device converts deltas whose commands are placed sequentially (each
 * dst = the sum of the earlier lengths), which every encoder here and
 * delta_place_commands emit; any other stream gets DG_ERR_UNSUPPORTED (the
 * host function sorts such commands first).  Per-stream status: DG_OK,
 * DG_ERR_MALFORMED (bad magic, a field or payload past the stream's end, an
 * unknown command, a COPY reading past |R|), DG_ERR_UNSUPPORTED, or
 * DG_ERR_CAPACITY (the stream is longer than delta_cap or holds more commands
 * than its capacity allows, or its output ends past out_cap); a nonzero
 * incoming d_delta_status[i] is passed on.  A failed stream's output is
 * empty (for DG_ERR_CAPACITY from out_cap the offsets still count its size,
 * as dg_encode_plan_run's do) and its neighbours are untouched.  A delta that
 * is already in-place is copied through.
 *
 * Output: packed like the encode plan's, delta i at
 * d_out[d_out_offsets[i] .. d_out_offsets[i+1]), n + 1 offsets.  With
 * d_delta_offsets (n + 1 entries, as dg_encode_plan_run writes them) stream i
 * is d_delta[d_delta_offsets[i] .. d_delta_offsets[i+1]) and delta_cap only
 * bounds its length; with NULL it is exactly delta_cap bytes at delta_off.
 * So dg_encode_plan_run -> dg_inplace_plan_run chain on one stream with no
 * host step between them.
 *
 * Work memory is allocated at plan creation from each delta's capacity, about
 * 73 bytes per possible COPY ((delta_cap - 25) / 13 of them; a plan made from
 * an encode plan uses the encoder's record capacity) and 8 per possible ADD;
 * DG_ERR_NOMEM when it cannot be had.  Like the greedy encoder, a
 * pathological delta (neighbour ranges totalling O(n^2)) holds its wave for
 * as long as it takes while the rest of the batch proceeds.
 *
 * The kernels live in dg_inplace.hsaco beside libdeltagpu.so and are loaded
 * on first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the encode plan: "order", "scan", "emit", "total". */
typedef struct {
	uint64_t ref_off, ref_len;       /* R_i in the reference arena */
	uint64_t delta_off, delta_cap;   /* standard delta i: start, and most bytes it may have */
} dg_inplace_desc_t;
typedef struct dg_inplace_plan dg_inplace_plan_t;

int dg_inplace_plan_create(dg_context_t *ctx, const dg_inplace_desc_t *descs /* host */,
                           uint32_t n, int policy, dg_inplace_plan_t **out);
/* Geometry from an encode plan: pair i's R span, its worst-case delta size
 * and its copy count (the record capacity). */
int dg_inplace_plan_create_for(dg_context_t *ctx, const dg_encode_plan_t *enc,
                               int policy, dg_inplace_plan_t **out);
/* Upper bound of the packed output: per delta its capacity plus the version
 * bytes its COPYs can turn into ADD payload (for a plan made from
 * descriptors, max copies x |R| capped at 4 GiB: pass a smaller out_cap when
 * the version sizes are known). */
uint64_t dg_inplace_plan_output_bound(const dg_inplace_plan_t *plan);
int dg_inplace_plan_run(dg_inplace_plan_t *plan, const uint8_t *d_ref,
                        const uint8_t *d_delta, const uint64_t *d_delta_offsets,
                        const int32_t *d_delta_status, uint8_t *d_out,
                        uint64_t out_cap, uint64_t *d_out_offsets,
                        int32_t *d_status, void *stream);
int dg_inplace_plan_set_timing(dg_inplace_plan_t *plan, int slots);
int dg_inplace_plan_stage_times(dg_inplace_plan_t *plan, float *ms,
                                const char **names, int n);
void dg_inplace_plan_destroy(dg_inplace_plan_t *plan);

/* Host buffers in, host buffers out (outs[i] malloc'd, status[i] may be
 * NULL): the batch converted on the device; a stream the device reports
 * DG_ERR_UNSUPPORTED is converted by dg_make_inplace.  Returns DG_OK (per-
 * stream failures in status) or the first failure when status is NULL. */
int dg_make_inplace_batch(dg_context_t *ctx, const uint8_t *const *r, const size_t *r_len,
                          const uint8_t *const *delta, const size_t *delta_len,
                          uint32_t n, int policy, dg_buffer_t *outs, int32_t *status);

/* ── in-place update of a batch on the device: R becomes V in its own buffer ──
 *
 * The consuming side of in-place deltas (Burns et al.; inplace.c, apply.c:
 * 253-284): stream i's buffer, buf_cap bytes at buf_off of one device arena,
 * holds R_i in its first ref_len bytes; after the run it holds V_i in its first
 * version_size bytes.  No second arena and no copy of R: against
 * dg_decode_plan_run, which needs the reference arena and an output arena and
 * copies every R into the output first.
 *
 * All or nothing.  The buffer is the only copy of R, so a stream is validated
 * completely before its first byte is stored: the whole command chain is
 * parsed and every command's bounds are checked (encoding.c:111-178), and R's
 * CRC-64/XZ is checked against the header (main.c:341-356).  Per-stream
 * status, in this precedence (main.c:335-385):
 *   DG_ERR_MALFORMED    exactly the streams dg_decode_plan_run calls malformed:
 *                       magic, framing, an unknown command, a missing payload,
 *                       dst + len or a COPY's src + len past
 *                       bsz = max(ref_len, version_size);
 *   DG_ERR_CAPACITY     bsz > buf_cap (and, with d_delta_offsets, a stream
 *                       longer than delta_len);
 *   DG_ERR_UNSUPPORTED  a well-formed standard delta (header flag clear): its
 *                       COPYs read R while V overwrites it; convert it first
 *                       (dg_inplace_plan_*);
 *   DG_ERR_SRC_CRC      the buffer's first ref_len bytes are not the delta's R;
 *   DG_ERR_DST_CRC      the result does not match dst_crc;
 * a nonzero incoming d_delta_status[i] is passed on.  ignore_hash skips both
 * CRC checks.  On every status except DG_OK and DG_ERR_DST_CRC no byte of the
 * arena is changed and d_out_len[i] = 0.
 *
 * Result.  On DG_OK and DG_ERR_DST_CRC bytes [0, version_size) of the buffer
 * equal the reference's replay (apply.c:271-284: R, zeros up to bsz, then the
 * commands in stream order with memmove), so a delta that leaves part of a
 * grown tail uncovered leaves zeros there; d_out_len[i] = version_size.  Bytes
 * [version_size, ref_len) of a shrinking update are unspecified.  No byte at
 * or past bsz, and none outside the stream's own region, is written.
 *
 * Layout.  d_buf is 16-byte aligned; buf_off may be any value; regions may
 * touch but not overlap (DG_ERR_INVALID_ARG); a buf_cap, ref_len or delta_len
 * of 4 GiB or more is DG_ERR_TOO_LARGE; n == 0 is a valid empty plan.  The
 * delta bytes must not overlap the buffers: the stream is read again while the
 * buffer is written, and the library cannot check this for device offsets.
 * With d_delta_offsets (n + 1 entries, as dg_inplace_plan_run writes them)
 * stream i is d_delta[d_delta_offsets[i] .. d_delta_offsets[i+1]) and delta_len
 * only bounds its length; with NULL it is exactly delta_len bytes at delta_off.
 * So dg_encode_plan_run -> dg_inplace_plan_run -> dg_update_plan_run chain on
 * one stream with no host step.
 *
 * A run is one kernel on one stream: no allocation, no host synchronisation.
 * The plan owns, per stream, 40 bytes of descriptor and at most 64 KiB (about
 * delta_len / 4) in which the validating pass leaves every command's offset
 * for the applying pass; a stream of more commands than fit (some 30 000) is
 * parsed a second time instead.  DG_ERR_NOMEM when it cannot be had.
 * The kernel lives in dg_update.hsaco beside libdeltagpu.so and is loaded on
 * first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the decode plan: "update" (the kernel, validation and
 * both CRC checks included) and "total". */
typedef struct {
	uint64_t buf_off, buf_cap;      /* stream i's buffer in the arena; holds R_i in its first ref_len bytes */
	uint64_t ref_len;
	uint64_t delta_off, delta_len;  /* in-place delta i (with d_delta_offsets: delta_len only bounds it) */
} dg_update_desc_t;
typedef struct dg_update_plan dg_update_plan_t;

int dg_update_plan_create(dg_context_t *ctx, const dg_update_desc_t *descs /* host */, uint32_t n,
                          int ignore_hash, dg_update_plan_t **out);
int dg_update_plan_run(dg_update_plan_t *plan, uint8_t *d_buf, const uint8_t *d_delta,
                       const uint64_t *d_delta_offsets, const int32_t *d_delta_status,
                       uint64_t *d_out_len, int32_t *d_status, void *stream);
int dg_update_plan_set_timing(dg_update_plan_t *plan, int slots);
int dg_update_plan_stage_times(dg_update_plan_t *plan, float *ms, const char **names, int n);
void dg_update_plan_destroy(dg_update_plan_t *plan);

/* Host buffers: bufs[i] (buf_cap[i] bytes, R_i in the first ref_len[i]) is
 * overwritten with V_i, out_len[i] = version_size; a stream that fails (status[i],
 * may be NULL) keeps its bytes, except that DG_ERR_DST_CRC leaves the replay's
 * result.  Returns DG_OK (per-stream failures in status) or the first failure
 * when status is NULL. */
int dg_update_batch(dg_context_t *ctx, uint8_t *const *bufs, const size_t *ref_len, const size_t *buf_cap,
                    const uint8_t *const *delta, const size_t *delta_len, uint32_t n,
                    int ignore_hash, size_t *out_len, int32_t *status);

/* ── composition: delta(R -> V1) and delta(V1 -> V2) give delta(R -> V2) ──────
 *
 * A store keeps R, A = delta(R -> V1) and B = delta(V1 -> V2); a client that
 * still holds R needs one delta R -> V2.  Composition is a pure transform of
 * the two command streams: it needs none of R, V1 or V2.  Every byte of V2 is
 * a literal of B, a literal of A, or a byte of R, and the two command lists
 * say which.  (The reference has no such function; xdelta's `merge` is the
 * same step.)
 *
 * Inputs.  A and B are standard deltas (header flag clear), B against
 * V1: |V1| = A.version_size.  Both are sequentially placed exact covers: every
 * command's dst equals the sum of the earlier lengths and the lengths sum to
 * the stream's version_size, which every encoder here and
 * delta_place_commands emit.
 *
 * Provenance.  Walk B's commands in order.  An ADD contributes its literal
 * bytes.  A COPY(s, l) contributes, for each command j of A whose V1 interval
 * [d_j, d_j + len_j) meets [s, s + l), the overlap [x, y): if j is a COPY,
 * COPY(src_j + (x - d_j), y - x) from R; if j is an ADD, the literal slice
 * data_j[x - d_j .. y - d_j).  Zero-length commands contribute nothing.
 *
 * Normal form.  The pieces are concatenated and neighbours merged maximally:
 * consecutive literal pieces become one ADD; consecutive COPY pieces become
 * one COPY whenever the second starts in R where the first ends; wherever the
 * neighbours came from (inside one COPY of B, across commands of B, from two
 * commands of A).  No zero-length command is emitted, dst is sequential, the
 * header has flag byte 0, version_size = B.version_size, src_crc = A.src_crc,
 * dst_crc = B.dst_crc, and one END byte closes the stream.  The result is a
 * function of the byte-provenance map alone (for each position of V2: a
 * literal, or which offset of R), so compose(compose(A, B), C) ==
 * compose(A, compose(B, C)) byte for byte, and compose(A, I) with I the
 * one-COPY identity delta of V1 is A's own normal form.  The host function,
 * the device path and the tests' Python model produce it byte for byte; it is
 * an ordinary DLT\x03 standard delta that every decoder here and the
 * reference's `delta decode` decode to V2 with both CRC checks passing.
 *
 * Status, per pair.  The kind of defect decides, not its position in the
 * stream; first match wins:
 *   (incoming)          a nonzero d_a_status[i], then d_b_status[i], is passed on;
 *   DG_ERR_MALFORMED    what dg_inplace_plan_run calls malformed, in either
 *                       stream (magic, framing, an unknown command, a payload
 *                       past the end); a COPY of B with src + len >
 *                       A.version_size; a COPY of A with src + len > 2^32,
 *                       which no reference of this format satisfies;
 *   DG_ERR_CAPACITY     (device) a stream longer than its capacity, or more
 *                       commands than the plan's work memory holds;
 *   DG_ERR_UNSUPPORTED  either header has the in-place flag; placement is not
 *                       sequential; the lengths do not sum to version_size;
 *   DG_ERR_SRC_CRC      A.dst_crc != B.src_crc: B is not a delta against A's
 *                       output; ignore_hash skips this check;
 *   DG_ERR_TOO_LARGE    the composed delta would be 4 GiB or more;
 *   DG_ERR_CAPACITY     (device) the pair's output ends past out_cap.
 * The composer never sees R: a COPY of A that reads past |R| passes through,
 * and decode rejects C exactly as it would reject A.  A failed pair's output
 * is empty and its neighbours are untouched; for a pair that fails on out_cap
 * the offsets still count its size, as the encode and in-place plans' do.
 *
 * dg_compose is pure host code (no context, no GPU): linear in input plus
 * output, one binary search per COPY of B; *out is malloc'd.  Streams of
 * 4 GiB or more are DG_ERR_TOO_LARGE. */
int dg_compose(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
               int ignore_hash, dg_buffer_t *out);

/* ── composition of a batch on the device ──────────────────────────────────
 *
 * The same transform, byte for byte, for N pairs: streams A_i in one device
 * arena, B_i in another, C_i packed like the encode plan's output at
 * d_out[d_out_offsets[i] .. d_out_offsets[i+1]), n + 1 offsets.  One wave per
 * pair maps B's commands onto A's (tables over A's commands, two binary
 * searches per COPY of B, merges across commands by wave scans), the size scan
 * packs the outputs, one block per pair writes them.  A run is two kernels and
 * the scan on one stream: no allocation, no host synchronisation, graph-
 * capturable like its siblings.  So dg_encode_plan_run (twice) ->
 * dg_compose_plan_run -> dg_inplace_plan_run -> dg_update_plan_run take a
 * buffer from R to V2 on one stream with no host step.
 *
 * Offsets.  With d_a_offsets (n + 1 entries, as dg_encode_plan_run writes
 * them) stream A_i is d_a[d_a_offsets[i] .. d_a_offsets[i+1]) and a_cap only
 * bounds its length; with NULL it is exactly a_cap bytes at a_off.  Likewise
 * for B.  The d_a, d_b and d_out ranges must not overlap.
 *
 * Sizing.  There is no a-priori bound of the output: B may copy one range of
 * V1 many times, so the piece count can reach |A commands| x |B copies|.
 * d_out_offsets always receives the true sizes.  A run with d_out = NULL and
 * out_cap = 0 is the sizing run: every pair that would be DG_OK reports the
 * out_cap DG_ERR_CAPACITY.
 *
 * Work memory is allocated at plan creation from the capacities: (a_cap - 25)
 * / 9 possible commands of A and (b_cap - 25) / 9 of B (a plan made from two
 * encode plans uses the encoders' record capacities), 20 bytes per command of
 * either stream; DG_ERR_NOMEM when it cannot be had.  A capacity of 4 GiB or
 * more is DG_ERR_TOO_LARGE; n == 0 is a valid empty plan.  In the emit kernel
 * one lane walks the pieces of one command of B, so a COPY of B that spans
 * very many commands of A holds its lane for that long.
 *
 * The kernels live in dg_compose.hsaco beside libdeltagpu.so and are loaded
 * on first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the in-place plan: "map", "scan", "emit", "total". */
typedef struct {
	uint64_t a_off, a_cap;   /* delta(R -> V1) i: start, and most bytes it may have */
	uint64_t b_off, b_cap;   /* delta(V1 -> V2) i */
} dg_compose_desc_t;
typedef struct dg_compose_plan dg_compose_plan_t;

int dg_compose_plan_create(dg_context_t *ctx, const dg_compose_desc_t *descs /* host */,
                           uint32_t n, int ignore_hash, dg_compose_plan_t **out);
/* Capacities from two encode plans with equal pair counts: (R, V1) and
 * (V1, V2); pass dg_encode_plan_run's offsets and statuses to the run. */
int dg_compose_plan_create_for(dg_context_t *ctx, const dg_encode_plan_t *enc_a,
                               const dg_encode_plan_t *enc_b, int ignore_hash,
                               dg_compose_plan_t **out);
int dg_compose_plan_run(dg_compose_plan_t *plan,
                        const uint8_t *d_a, const uint64_t *d_a_offsets,
                        const int32_t *d_a_status,
                        const uint8_t *d_b, const uint64_t *d_b_offsets,
                        const int32_t *d_b_status,
                        uint8_t *d_out, uint64_t out_cap,
                        uint64_t *d_out_offsets, int32_t *d_status, void *stream);
int dg_compose_plan_set_timing(dg_compose_plan_t *plan, int slots);
int dg_compose_plan_stage_times(dg_compose_plan_t *plan, float *ms,
                                const char **names, int n);
void dg_compose_plan_destroy(dg_compose_plan_t *plan);

/* Host buffers in, host buffers out (outs[i] malloc'd, status[i] may be
 * NULL): the sizing run, then the real run.  Returns DG_OK (per-pair failures
 * in status) or the first failure when status is NULL. */
int dg_compose_batch(dg_context_t *ctx, const uint8_t *const *a, const size_t *a_len,
                     const uint8_t *const *b, const size_t *b_len, uint32_t n,
                     int ignore_hash, dg_buffer_t *outs, int32_t *status);

/* ── inversion: R and delta(R -> V) give delta(V -> R) ────────────────────────
 *
 * A store that keeps the newest version whole and older ones as backward
 * deltas encodes A = delta(R -> V) on a commit and then needs delta(V -> R) to
 * drop R.  A already holds everything the inverse can hold: every byte of R
 * that some COPY of A reads is in V at a known offset, and every other byte of
 * R has to be carried as a literal.  So the inverse is a pure transform of A's
 * command list plus the uncovered bytes of R: no V, no fingerprints, no
 * tables.  (The reference has no such function.)  With dg_compose it closes
 * the set: compose(invert(A), B) re-bases a chain without re-encoding.
 *
 * Inputs.  R of ref_len bytes, and A, a standard delta (header flag clear)
 * against R: a sequentially placed exact cover, as for dg_compose.
 *
 * Provenance of R.  A COPY(src, dst, len) of A with len > 0 covers position x
 * of R when src <= x < src + len.  If no COPY covers x, x is a literal with
 * the byte R[x].  Otherwise x's owner is, among the covering COPYs, the one
 * with the smallest src; among those the longest; among those the first in
 * the stream; and x comes from V at owner.dst + (x - owner.src).
 * Equivalently: sort the COPYs by (src ascending, len descending, stream
 * index ascending) and sweep with a running maximum `reach` of the ends seen
 * so far; COPY j owns [max(src_j, reach), src_j + len_j) when that interval is
 * not empty, and the bytes between reach and a later src_j, and between the
 * final reach and ref_len, are literals.  ADDs of A and zero-length commands
 * contribute nothing.
 *
 * Normal form.  That map, run-length encoded over x = 0 .. ref_len - 1:
 * consecutive literals are one ADD; consecutive V positions are one COPY
 * whenever the V offset also advances by one, whichever owners they came from
 * (two touching COPYs of A whose dst ranges also touch merge; a shadowed COPY
 * vanishes).  No zero-length command is emitted, dst is sequential, the
 * header is DLT\x03 with flag byte 0, version_size = ref_len, src_crc =
 * A.dst_crc, dst_crc = A.src_crc, and one END byte closes the stream.  The
 * host function, the device path and the tests' Python model produce it byte
 * for byte; every decoder here and the reference's `delta decode` decode it
 * against V to R with both CRC checks passing.
 *
 * Status, per delta.  The kind of defect decides, not its position in the
 * stream; first match wins:
 *   (incoming)          a nonzero d_delta_status[i] is passed on;
 *   DG_ERR_MALFORMED    magic, framing, an unknown command, a payload past the
 *                       end, or a COPY with src + len > ref_len;
 *   DG_ERR_CAPACITY     (device) a stream longer than its capacity, or more
 *                       COPYs than the plan's work memory holds;
 *   DG_ERR_UNSUPPORTED  the in-place flag is set; placement is not sequential;
 *                       the lengths do not sum to version_size;
 *   DG_ERR_TOO_LARGE    the inverse would be 4 GiB or more;
 *   DG_ERR_CAPACITY     (device) the delta's output ends past out_cap.
 * A failed delta's output is empty and its neighbours are untouched; for a
 * delta that fails on out_cap the offsets still count its size.
 *
 * R's CRC is not checked by the library: the inverse's dst_crc is A.src_crc,
 * so a wrong R shows as DG_ERR_DST_CRC when the inverse is decoded.  (`delta
 * invert` checks it unless --ignore-hash is given.)
 *
 * dg_invert is pure host code (no context, no GPU): linear in input plus
 * output apart from one sort of the COPYs; *out is malloc'd.  An R or a
 * stream of 4 GiB or more is DG_ERR_TOO_LARGE. */
int dg_invert(const uint8_t *r, size_t r_len, const uint8_t *a, size_t a_len,
              dg_buffer_t *out);

/* ── inversion of a batch on the device ────────────────────────────────────
 *
 * The same transform, byte for byte, for N deltas: the references in one
 * device arena, the streams in another (packed as the encode plan writes
 * them, or one per descriptor), the inverses packed at
 * d_out[d_out_offsets[i] .. d_out_offsets[i+1]), n + 1 offsets.  One wave per
 * delta parses the stream, puts its COPYs into key order (skipped when the
 * stream has them so already, as every encoder whose matches move forward in
 * both buffers emits them; else a radix sort by that wave) and sweeps them;
 * the size scan packs the outputs; one block per delta writes them.  A run is
 * two kernels and the scan on one stream: no allocation, no host
 * synchronisation, graph-capturable like its siblings.  So
 * dg_encode_plan_run -> dg_invert_plan_run turn (R, V) into delta(V -> R) on
 * one stream with no host step.
 *
 * Offsets.  With d_delta_offsets (n + 1 entries, as dg_encode_plan_run writes
 * them) stream i is d_delta[d_delta_offsets[i] .. d_delta_offsets[i+1]) and
 * delta_cap only bounds its length; with NULL it is exactly delta_cap bytes at
 * delta_off.  The d_ref, d_delta and d_out ranges must not overlap.
 *
 * Sizing.  With C possible COPYs the inverse has at most 2 C + 1 runs, so one
 * delta needs at most 25 + 13 C + 9 (C + 1) + ref_len + 1 bytes;
 * dg_invert_plan_output_bound is the sum over the batch.
 *
 * Work memory is allocated at plan creation from the capacities: (delta_cap -
 * 26) / 13 possible COPYs (a plan made from an encode plan uses the encoder's
 * record capacity), 64 bytes per possible COPY; DG_ERR_NOMEM when it cannot be
 * had.  A capacity or ref_len of 4 GiB or more is DG_ERR_TOO_LARGE; n == 0 is
 * a valid empty plan.  One wave sorts and sweeps one delta's COPYs, so a delta
 * with very many COPYs out of key order holds its wave for eight passes over
 * them.
 *
 * The kernels live in dg_invert.hsaco beside libdeltagpu.so and are loaded on
 * first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the in-place plan: "map", "scan", "emit", "total". */
typedef struct {
	uint64_t ref_off, ref_len;       /* R_i in d_ref */
	uint64_t delta_off, delta_cap;   /* delta(R -> V) i: start, and most bytes it may have */
} dg_invert_desc_t;
typedef struct dg_invert_plan dg_invert_plan_t;

int dg_invert_plan_create(dg_context_t *ctx, const dg_invert_desc_t *descs /* host */,
                          uint32_t n, dg_invert_plan_t **out);
/* Geometry from an encode plan: its R spans, worst-case delta sizes and record
 * capacities; pass dg_encode_plan_run's offsets and statuses to the run. */
int dg_invert_plan_create_for(dg_context_t *ctx, const dg_encode_plan_t *enc,
                              dg_invert_plan_t **out);
uint64_t dg_invert_plan_output_bound(const dg_invert_plan_t *plan);
int dg_invert_plan_run(dg_invert_plan_t *plan, const uint8_t *d_ref,
                       const uint8_t *d_delta, const uint64_t *d_delta_offsets,
                       const int32_t *d_delta_status,
                       uint8_t *d_out, uint64_t out_cap,
                       uint64_t *d_out_offsets, int32_t *d_status, void *stream);
int dg_invert_plan_set_timing(dg_invert_plan_t *plan, int slots);
int dg_invert_plan_stage_times(dg_invert_plan_t *plan, float *ms,
                               const char **names, int n);
void dg_invert_plan_destroy(dg_invert_plan_t *plan);

/* Host buffers in, host buffers out (outs[i] malloc'd, status may be NULL).
 * Returns DG_OK (per-delta failures in status) or the first failure when
 * status is NULL. */
int dg_invert_batch(dg_context_t *ctx, const uint8_t *const *r, const size_t *r_len,
                    const uint8_t *const *delta, const size_t *delta_len, uint32_t n,
                    dg_buffer_t *outs, int32_t *status);

/* ── one large pair: segments of V, windows of R, and the splice of their deltas ──
 *
 * The encoders give one wavefront to a pair, so one large pair would run on one
 * wave.  A large pair is instead cut into segments of V, each encoded against a
 * window of R as one dg_pair_t of an ordinary encode plan (thousands of waves),
 * and the k segment deltas are spliced into ONE standard DLT\x03 delta R -> V.
 * The splice is a pure transform of command streams, in the family of
 * composition and inversion: it needs none of R or V.  The result is a
 * different, documented encoder's output (a segment sees matches only inside
 * its window), a standard delta that every decoder accepts.  (The reference has
 * no such step.)
 *
 * Segmentation rule (dg_segment_pairs).  For a whole pair (r_off, r_len, v_off,
 * v_len), seg_bytes S > 0 and window_bytes W, both multiples of 16, the count
 * is k = max(1, ceil(v_len / S)); segment j is V[jS, min((j + 1) S, v_len)); its
 * window is R[a, max(a, b)) with lo = min(jS, r_len), a = lo - min(lo, W), b =
 * min(r_len, jS + S + W).  Pure arithmetic: with whole offsets that are multiples
 * of 16 every segment offset is one too, so the encode plan takes its LDS-window
 * kernels.  For n_groups whole pairs the segments are written group after group
 * and seg_first[g] (n_groups + 1 entries) is group g's first segment.  With segs
 * == NULL only seg_first is filled (the count).  DG_ERR_INVALID_ARG for S == 0
 * or an S or W that is no multiple of 16; DG_ERR_TOO_LARGE for an r_len or v_len
 * at or above 4 GiB - 1 MiB (the encode plan's limit) or more than 2^32 - 1
 * segments; DG_ERR_CAPACITY when segs_cap entries do not hold them.  Host only.
 *
 * Inputs of the splice, per group.  A group is one large pair: a span `whole` of
 * the two arenas and n_seg >= 1 consecutive segments seg[j], the very array given
 * to dg_encode_plan_create.  The segments' V spans tile [v_off, v_off + v_len)
 * exactly and in order; empty segments are allowed.  Every R window lies inside
 * [r_off, r_off + r_len); windows may overlap, repeat, leave gaps and be empty.
 * A_j is a standard, sequentially placed delta of seg[j] (as for dg_compose);
 * its version_size equals seg[j].v_len.
 *
 * Provenance.  Walk the segments in order and each A_j's commands in order.  An
 * ADD contributes its literal bytes; a COPY(src, len) contributes COPY(src +
 * seg[j].r_off - whole.r_off, len); zero-length commands contribute nothing.
 *
 * Normal form.  Composition's rule: consecutive literal pieces become one ADD;
 * consecutive COPY pieces become one COPY whenever the second starts in R where
 * the first ends; inside a segment's stream and across segment seams alike,
 * through any number of empty segments.  dst is sequential, no zero-length
 * command is emitted, one END byte closes the stream, the flag byte is 0 and
 * version_size = whole.v_len.  The result is a function of the byte-provenance
 * map of V alone: R == V cut into any number of segments whose windows contain
 * them splices to one COPY (25 + 13 + 1 = 39 bytes); a V unrelated to R to one
 * ADD of |V|; one segment whose window is all of R to compose(A, identity(V)),
 * A's own normal form.  The host function, the device path and the tests'
 * Python model produce it byte for byte.
 *
 * CRCs.  src_crc is the CRC-64/XZ of all of R: the windows need not cover R, so
 * the caller supplies it (device: one u64 per group as dg_crc64_xz_batch_device
 * writes it; host: 8 bytes, big-endian as in the header).  dst_crc is not
 * recomputed from V: it is combined from the segments' own header dst_crc
 * values, crc(X || Y) = crc(X) x^(8 |Y|) + crc(Y) in GF(2)[x] mod P.  The
 * weights x^(8 * bytes after the segment) are computed once per segment at plan
 * creation; the device multiplies once per segment and reduces with XOR.  The
 * spliced header costs no pass over V.
 *
 * Status, per group; first match wins:
 *   (incoming)          the first nonzero incoming segment status, in segment
 *                       order, is passed on;
 *   DG_ERR_MALFORMED    what the siblings call malformed, in any segment stream
 *                       (magic, framing, an unknown command, a payload past the
 *                       end); a COPY with src + len > seg[j].r_len: the splicer
 *                       knows the window, and rebased such a COPY would read
 *                       valid but wrong bytes of R;
 *   DG_ERR_CAPACITY     (device) a stream longer than its capacity;
 *   DG_ERR_UNSUPPORTED  an in-place flag; placement not sequential; lengths that
 *                       do not sum to version_size; version_size != seg[j].v_len;
 *   DG_ERR_TOO_LARGE    the spliced delta would be 4 GiB or more (host: also a
 *                       stream of 4 GiB or more);
 *   DG_ERR_CAPACITY     (device) the group's output ends past out_cap.
 * A failed group's output is empty and its neighbours are untouched; for a
 * group that fails on out_cap the offsets still count its size.
 *
 * Geometry errors (dg_splice, dg_splice_plan_create*): DG_ERR_INVALID_ARG for
 * segments that do not tile V in order, a window outside R, a group without a
 * segment or a seg_first that does not run from 0 to n_seg; DG_ERR_TOO_LARGE for
 * an r_len or v_len at or above 4 GiB - 1 MiB or a capacity of 4 GiB or more.
 *
 * dg_splice is pure host code (no context, no GPU), linear in its input; *out
 * is malloc'd.  seg_status may be NULL (every segment DG_OK). */
int dg_segment_pairs(const dg_pair_t *wholes, uint32_t n_groups, uint64_t seg_bytes,
                     uint64_t window_bytes, dg_pair_t *segs /* or NULL */, uint64_t segs_cap,
                     uint32_t *seg_first /* n_groups + 1 */);
int dg_splice(const dg_pair_t *whole, const dg_pair_t *segs, uint32_t n_seg,
              const uint8_t *const *deltas, const size_t *delta_len,
              const int32_t *seg_status /* or NULL */, const uint8_t src_crc[DG_CRC_SIZE],
              dg_buffer_t *out);

/* ── the splice of a batch of groups on the device ─────────────────────────
 *
 * The same transform, byte for byte.  Segment j's stream is
 * d_deltas[d_offsets[j] .. d_offsets[j + 1]) (n_seg + 1 entries, as
 * dg_encode_plan_run writes them; required) and its capacity only bounds its
 * length; d_seg_status (may be NULL) as dg_encode_plan_run writes it.  The
 * groups' deltas are packed like the encode plan's output, group g at
 * d_out[d_out_offsets[g] .. d_out_offsets[g + 1]), n_groups + 1 offsets.
 *
 * A run is three kernels and the library's size scan on one stream: no
 * allocation, no host synchronisation, graph-capturable like its siblings.
 *   map      one wave per segment parses and validates its stream and leaves a
 *            fixed-size summary: status, the bytes of its own normal form, its
 *            first run's kind / start in R / length, its last run's kind / end
 *            in R / length, whether it is one run, its weighted dst_crc;
 *   resolve  one wave per group walks the summaries 64 at a time with wave
 *            scans and a carry: every seam, every segment's place in the
 *            output, whether its first run continues its predecessor's, the
 *            whole length of a run that crosses seams; status, size, dst_crc;
 *   scan     the groups' sizes into d_out_offsets;
 *   emit     one wave per segment parses again and writes rebased commands and
 *            payloads inside its own resolved range; the first segment's block
 *            writes the header, the last one the END byte.
 * So dg_encode_plan_run(segments) -> dg_splice_plan_run is a large-pair encoder
 * on one stream with no host step, and -> dg_inplace_plan_run ->
 * dg_update_plan_run, dg_compose_plan_run, dg_invert_plan_run and
 * dg_read_plan_index follow as for any delta.
 *
 * Sizing.  d_out_offsets always receives the true sizes.  The splice of a group
 * is never longer than its segment deltas together plus one byte:
 * dg_splice_plan_output_bound is the sum of the capacities plus one byte per
 * group (a plan made from an encode plan uses the encoder's bounds; 0 for a
 * plan created without capacities).  A run with d_out = NULL and out_cap = 0 is
 * the sizing run, as for dg_compose_plan_run.
 *
 * Work memory is 56 + 16 bytes per segment, allocated at plan creation
 * (DG_ERR_NOMEM when it cannot be had); no per-command tables.  n_groups == 0
 * with n_seg == 0 is a valid empty plan.  One wave parses and writes one
 * segment's delta, so the emit stage's parallelism is the segment count.
 *
 * The kernels live in dg_splice.hsaco beside libdeltagpu.so and are loaded on
 * first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the in-place plan: "map", "resolve", "scan", "emit",
 * "total". */
typedef struct dg_splice_plan dg_splice_plan_t;

int dg_splice_plan_create(dg_context_t *ctx, const dg_pair_t *segs /* host */, uint32_t n_seg,
                          const dg_pair_t *wholes, const uint32_t *seg_first /* n_groups + 1 */,
                          uint32_t n_groups, const uint64_t *seg_caps /* n_seg, or NULL */,
                          dg_splice_plan_t **out);
/* Segments and capacities from the encode plan that encodes them; pass
 * dg_encode_plan_run's offsets and statuses to the run. */
int dg_splice_plan_create_for(dg_context_t *ctx, const dg_encode_plan_t *enc,
                              const dg_pair_t *wholes, const uint32_t *seg_first,
                              uint32_t n_groups, dg_splice_plan_t **out);
uint64_t dg_splice_plan_output_bound(const dg_splice_plan_t *plan);
int dg_splice_plan_run(dg_splice_plan_t *plan, const uint8_t *d_deltas,
                       const uint64_t *d_offsets, const int32_t *d_seg_status,
                       const uint64_t *d_src_crc, uint8_t *d_out, uint64_t out_cap,
                       uint64_t *d_out_offsets, int32_t *d_status, void *stream);
int dg_splice_plan_set_timing(dg_splice_plan_t *plan, int slots);
int dg_splice_plan_stage_times(dg_splice_plan_t *plan, float *ms, const char **names, int n);
void dg_splice_plan_destroy(dg_splice_plan_t *plan);

/* Host buffers in, host buffers out: deltas[j] / delta_len[j] / seg_status[j]
 * (may be NULL) per segment, src_crc 8 bytes per group, outs[g] malloc'd,
 * status[g] may be NULL.  Returns DG_OK (per-group failures in status) or the
 * first failure when status is NULL. */
int dg_splice_batch(dg_context_t *ctx, const dg_pair_t *wholes, uint32_t n_groups,
                    const dg_pair_t *segs, const uint32_t *seg_first,
                    const uint8_t *const *deltas, const size_t *delta_len,
                    const int32_t *seg_status, const uint8_t *src_crc,
                    dg_buffer_t *outs, int32_t *status);

/* One large pair in host memory: dg_segment_pairs, upload, R's CRC on the
 * device, the encode plan over the segments (every algorithm and option of
 * dg_encode_plan_create), the splice plan, download.  With DG_OPT_INPLACE the
 * spliced delta is converted on the host, as dg_encode's is.  out->data is
 * malloc'd.  Cost: with window_bytes > 0 every segment but the
 * first lies window_bytes off its pair's diagonal, which onepass encodes on one
 * wave per segment; with window_bytes == 0 the segments lie on their diagonals
 * and the splice's time per segment is what remains, so smaller segments
 * (256 KiB) serve a large onepass pair best. */
int dg_encode_large(dg_context_t *ctx, dg_algorithm_t algo,
                    const uint8_t *r, size_t r_len, const uint8_t *v, size_t v_len,
                    const dg_diff_options_t *opts, uint64_t seg_bytes, uint64_t window_bytes,
                    dg_buffer_t *out);

/* ── range reads: bytes [off, off + len) of a version kept as R and a delta ────
 *
 * What a version store does most: serve a read of part of a version without
 * rebuilding the version.  The reference has no such function; the contract
 * is its replay, sliced.  The result equals bytes [off, off + n) of what
 * delta_apply_placed (apply.c:229-249) produces: a zeroed buffer of
 * version_size bytes, then the commands in stream order, later writes over
 * earlier ones (so an uncovered gap reads as zeros).  pread semantics, in 64
 * bits: n = off >= version_size ? 0 : min(len, version_size - off).
 *
 * Standard deltas only.  Status, the first that applies:
 *   DG_ERR_TOO_LARGE    r_len or delta_len of 4 GiB or more (for a plan: at
 *                       create);
 *   DG_ERR_MALFORMED    shorter than the 25-byte header, or another magic;
 *   DG_ERR_UNSUPPORTED  the in-place flag is set: that replay reads the buffer
 *                       it rewrites, so a slice of it needs the whole replay;
 *   DG_ERR_MALFORMED    exactly what dg_decode_plan_run calls malformed:
 *                       framing, an unknown command, a payload past the end,
 *                       dst + len > version_size, a COPY's src + len > r_len
 *                       (anywhere in the stream, not only in the range).  A
 *                       missing END is accepted, as in decode.
 *
 * No CRC is checked.  dst_crc cannot be checked from a slice, and checking
 * src_crc would read all of R for every request.  A store checks R once when
 * it takes it in: dg_crc64_xz_batch_device over the references against
 * dg_delta_info's src_crc.
 *
 * dg_read is pure host code: no context, no GPU.  One walk over the stream,
 * which applies only the commands' intersections with the range; *out takes
 * n bytes (free with dg_buffer_free; data is non-NULL on DG_OK even for n = 0). */
int dg_read(const uint8_t *r, size_t r_len, const uint8_t *delta, size_t delta_len,
            uint64_t off, uint64_t len, dg_buffer_t *out);

/* ── range reads of a batch on the device ──────────────────────────────────
 *
 * Streams are fixed at create: stream i's reference is ref_len bytes at
 * ref_off of the reference arena, its delta delta_len bytes at delta_off of
 * the delta arena.  Requests are a device array given at run, any number of
 * them per stream.  R and the deltas are only read.
 *
 * Index.  dg_read_plan_index is one launch, one block per stream: it parses
 * and validates every stream once and leaves, in memory the plan owns, what
 * lets a read start near its range: per stream a 32-byte head (status,
 * version_size, whether the commands tile V in stream order) and 8 bytes per
 * 1024 bytes of stream, at most delta_len / 128 + 64 bytes per stream
 * (allocated at create; DG_ERR_NOMEM if that fails).  The layout is private.
 * d_delta_offsets (n + 1 entries) and d_delta_status mean what they mean for
 * dg_update_plan_run: with offsets, stream i is d_delta[d_delta_offsets[i] ..
 * d_delta_offsets[i+1]) and delta_len only bounds it (a longer stream is
 * DG_ERR_CAPACITY); a nonzero d_delta_status[i] is passed on and comes before
 * every status above.  So dg_encode_plan_run -> dg_read_plan_index ->
 * dg_read_plan_run chain on one stream with no host step.  Each stream's
 * status goes to d_stream_status[i] (may be NULL) and is kept by the plan; for
 * a standard stream it equals dg_decode_batch_device(ignore_hash = 1)'s.  The
 * index describes the delta bytes as they were: run it again whenever they
 * change.  A run before any index is DG_ERR_INVALID_ARG (dg_last_error says
 * so); a plan of no streams needs none.
 *
 * Run.  One launch, one block per request, n_req <= max_requests
 * (DG_ERR_INVALID_ARG otherwise); no allocation, no host synchronisation.
 * Request j's status goes to d_status[j]: DG_ERR_INVALID_ARG for stream >=
 * n_streams or reserved != 0, else its stream's status, else DG_OK with
 * d_out_len[j] = n and the slice in d_out[out_off .. out_off + n).  Bytes
 * [n, len) of the slot are not touched; on a failing status n = 0 and the
 * slot is not touched; nothing outside the slots is written for any status.
 * Slots that overlap are the caller's error (unspecified inside the overlap).
 * out_off may have any alignment; d_out must be 16-byte aligned.
 *
 * Cost.  A stream whose commands tile V in stream order (what every encoder,
 * dg_compose and dg_invert emit) is entered at the index entry before the
 * range and left after it: the work is proportional to the range.  Any other
 * valid stream (commands out of order, overlapping writes, gaps) is correct
 * but costs a parse of the whole stream per request.
 *
 * Containment.  Whatever the arenas hold, a stale index after the deltas
 * were overwritten included, a run reads only the streams' reference and
 * delta bytes (the delta in whole aligned 16-byte words that hold one of its
 * bytes, as decode does) and writes only inside the requests' slots: the read
 * kernel checks every COPY's src + len against ref_len and clips every store
 * itself.  Results under a stale index are otherwise unspecified.
 *
 * The kernels live in dg_read.hsaco beside libdeltagpu.so and are loaded on
 * first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the update plan, of runs: "read" (the kernel), "total". */
typedef struct {
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_len;  /* with d_delta_offsets: delta_len only bounds the stream */
} dg_read_stream_t;
typedef struct {
	uint32_t stream, off, len;
	uint32_t reserved;              /* 0 */
	uint64_t out_off;               /* the slot: d_out[out_off .. out_off + len) */
} dg_read_req_t;
typedef struct dg_read_plan dg_read_plan_t;

int dg_read_plan_create(dg_context_t *ctx, const dg_read_stream_t *streams /* host */, uint32_t n_streams,
                        uint32_t max_requests, dg_read_plan_t **out);
int dg_read_plan_index(dg_read_plan_t *plan, const uint8_t *d_delta,
                       const uint64_t *d_delta_offsets, const int32_t *d_delta_status,
                       int32_t *d_stream_status, void *stream);
int dg_read_plan_run(dg_read_plan_t *plan, const uint8_t *d_ref, const uint8_t *d_delta,
                     const dg_read_req_t *d_reqs, uint32_t n_req, uint8_t *d_out,
                     uint32_t *d_out_len, int32_t *d_status, void *stream);
int dg_read_plan_set_timing(dg_read_plan_t *plan, int slots);
int dg_read_plan_stage_times(dg_read_plan_t *plan, float *ms, const char **names, int n);
void dg_read_plan_destroy(dg_read_plan_t *plan);

/* Host buffers: request j (reqs[j].stream, .off, .len; out_off is ignored)
 * reads from refs[stream] and deltas[stream]; outs[j] takes the n bytes
 * (malloc'd; free with dg_buffer_free; left empty on a failing status).
 * Returns DG_OK (per-request failures in status) or the first failure when
 * status is NULL. */
int dg_read_batch(dg_context_t *ctx, const uint8_t *const *refs, const size_t *ref_len,
                  const uint8_t *const *deltas, const size_t *delta_len, uint32_t n_streams,
                  const dg_read_req_t *reqs /* host */, uint32_t n_req,
                  dg_buffer_t *outs, int32_t *status);

/* ── a chunked index: one stream parsed by many blocks ───────────────────────
 *
 * dg_read_plan_index gives every stream to one block, which suits a batch of
 * many streams.  One large delta (dg_encode_large's of a 1 GiB pair is about
 * 220 MB) is instead indexed by the whole GPU: every stream of the plan is cut
 * into chunks of chunk_bytes (a stream shorter than one chunk is one chunk),
 * and the pass is four launches on one stream ("A chunked index"):
 * per chunk, for EVERY offset of the chunk, where the chain that starts there
 * leaves the chunk; one walk over the chunks that picks the true chain; per
 * chunk the real validation from its true entry, which writes the index.
 *
 * dg_read_plan_chunk_index is called once per plan (a second call is
 * DG_ERR_INVALID_ARG).  chunk_bytes is a multiple of 4096, at least 4096, or 0
 * for DG_CHUNK_BYTES_DEFAULT; anything else is DG_ERR_INVALID_ARG.  It
 * allocates all work memory of the pass, so a pass allocates nothing:
 *     4 bytes per stream byte (of the plan's delta_len bounds)
 *   + 24 bytes per chunk (sum over streams of max(1, ceil(delta_len / chunk_bytes)))
 *   + 32 bytes and two table words (12 bytes) per stream;
 * DG_ERR_NOMEM when it cannot be had.  A stream bound above 4 GiB - 16 bytes is
 * DG_ERR_TOO_LARGE (the pass keeps stream offsets and two codes in a u32).  The
 * kernels live in dg_index.hsaco beside libdeltagpu.so and are loaded here;
 * DG_ERR_HIP with the path in dg_last_error when it is missing.
 *
 * dg_read_plan_index_chunked takes dg_read_plan_index's arguments with the same
 * meanings (offsets array, passed-on status, DG_ERR_CAPACITY for a stream longer
 * than the plan allows, d_stream_status) and leaves the plan in exactly the
 * state dg_read_plan_index would: every stream's head is identical (status,
 * version_size, the sequential flag, the entry count, where the stream was and
 * its length) and, for every stream whose status is 0, so is every entry.  A
 * failed stream's entries are unspecified in both passes.  dg_read_plan_run
 * does not know which pass ran.  Before dg_read_plan_chunk_index it is
 * DG_ERR_INVALID_ARG (dg_last_error says so).  Asynchronous on the caller's
 * stream, no host synchronisation, no allocation: it chains after
 * dg_encode_plan_run and dg_splice_plan_run as the one-block pass does.  The
 * grid is sized from the plan's delta_len bounds; with device-side offsets the
 * blocks past a stream's real length leave at once.  No block waits for
 * another inside a kernel.
 *
 * dg_read_plan_index_get copies stream stream_i's 32-byte head and, when its
 * status is 0, its entries (8 bytes each, the head's entry count of them) to
 * host memory, after synchronising the context's stream.  *bytes is set to the
 * bytes needed; a smaller cap is DG_ERR_CAPACITY.  DG_ERR_INVALID_ARG before
 * any index pass.  It exists so that two index passes can be compared, and for
 * diagnostics: the layout stays private.
 *
 * Stage timing of the chunked passes: dg_read_plan_index_set_timing, then
 * dg_read_plan_index_stage_times: "map", "resolve", "fill" (with the launch
 * that writes the heads), "total".  dg_read_plan_stage_times is unchanged. */
#define DG_CHUNK_BYTES_DEFAULT 65536u
int dg_read_plan_chunk_index(dg_read_plan_t *plan, uint32_t chunk_bytes);
int dg_read_plan_index_chunked(dg_read_plan_t *plan, const uint8_t *d_delta,
                               const uint64_t *d_delta_offsets, const int32_t *d_delta_status,
                               int32_t *d_stream_status, void *stream);
int dg_read_plan_index_get(dg_read_plan_t *plan, uint32_t stream_i,
                           void *host_dst, uint64_t cap, uint64_t *bytes);
int dg_read_plan_index_set_timing(dg_read_plan_t *plan, int slots);
int dg_read_plan_index_stage_times(dg_read_plan_t *plan, float *ms, const char **names, int n);

/* ── one delta decoded by the whole GPU ──────────────────────────────────────
 *
 * dg_tile_requests is host arithmetic (no GPU, no context): the read requests
 * of stream 0 that tile [0, version_size) in tiles of tile_bytes (0:
 * DG_TILE_BYTES_DEFAULT), slots contiguous (out_off == off), the last tile
 * short.  *n takes their number, ceil(version_size / tile_bytes) (0 for
 * version_size 0); a smaller cap is DG_ERR_CAPACITY and writes nothing else.
 *
 * dg_decode_large gives, for every input, the status and the output bytes that
 * dg_decode gives (the output on DG_ERR_DST_CRC and the malformed / source /
 * output precedence included).  Route: the header checks on the host; an
 * in-place delta, or an r_len or delta_len of 4 GiB or more, goes to dg_decode;
 * otherwise upload, a one-stream read plan, the chunked index (chunk_bytes as
 * above); a failing stream status is DG_ERR_MALFORMED; a valid stream that is
 * not sequential goes to dg_decode_batch_device on the bytes already uploaded
 * (the read kernel would replay the whole stream once per tile); a sequential
 * stream is read as dg_tile_requests tiles into one buffer, the CRCs of R and
 * of the output (dg_crc64_xz_batch_device) are compared with the header unless
 * ignore_hash, and the output is downloaded. */
#define DG_TILE_BYTES_DEFAULT 65536u
int dg_tile_requests(uint32_t version_size, uint32_t tile_bytes,
                     dg_read_req_t *reqs, uint32_t cap, uint32_t *n);
int dg_decode_large(dg_context_t *ctx, const uint8_t *r, size_t r_len,
                    const uint8_t *delta, size_t delta_len, int ignore_hash,
                    uint32_t chunk_bytes, uint32_t tile_bytes, dg_buffer_t *out);

/* ── lineage reads: byte ranges through chains of deltas ─────────────────────
 *
 * A store keeps one buffer whole and every other version as a delta on a base
 * that is usually itself a delta: backward deltas from the newest version
 * (dg_invert), or trees whose parents dg_sketch_match chose.  A lineage is a base
 * buffer R = V_0 and standard deltas d_1 .. d_k with V_j = apply(V_{j-1}, d_j).
 * A lineage read returns bytes [off, off + n) of V_k, with pread's rule in 64
 * bits: n = off >= |V_k| ? 0 : min(len, |V_k| - off).  That is exactly what k
 * replays (apply.c:229-249) and a slice give; no V_j is built.  No CRC is
 * checked, as for dg_read.
 *
 * Every delta of a lineage is sequential: its commands tile its version in
 * stream order (each starts where the one before it ends, the last ends at
 * version_size).  Every encoder, dg_compose, dg_invert and dg_splice emit such
 * streams.  A caller with another valid stream directly on a base uses
 * dg_read / dg_read_plan_run.
 *
 * Status of a read, the first that applies; the order is the same on the host
 * and on the device:
 *   1. DG_ERR_INVALID_ARG  (device) stream >= n_streams or reserved != 0;
 *                          (host) k > DG_LINEAGE_MAX_DEPTH, a NULL argument;
 *   2. walking from the requested delta towards its base, for each one:
 *      a. its index status: what dg_read_plan_index reports for it, with the
 *         size of the version below it as its ref_len (DG_ERR_MALFORMED,
 *         DG_ERR_UNSUPPORTED for an in-place delta, or a passed-on status).  So
 *         a COPY of d_j that leaves V_{j-1} is DG_ERR_MALFORMED;
 *      b. DG_ERR_UNSUPPORTED if it is valid but not sequential;
 *      c. (device) DG_ERR_INVALID_ARG if its ref_len is not its parent's
 *         version_size.  A parent whose own index status is not 0 has no
 *         version_size: that status, which is next in the order, is the result.
 *   3. DG_OK.
 *
 * dg_read_lineage is pure host code: no context, no GPU.  deltas[0] is the
 * delta on R, deltas[k - 1] the one whose version is read; k == 0 reads R
 * itself.  Level j's ref_len is version_size of d_{j-1}'s header; a d_{j-1}
 * without a readable header (shorter than 25 bytes, another magic) states none
 * and d_j's COPYs are then checked against 2^32 - 1 (the walk ends at d_{j-1}
 * with DG_ERR_MALFORMED unless d_j fails first).  DG_ERR_TOO_LARGE for an r_len
 * or delta_len of 4 GiB or more.  Work memory is the n output bytes, one frame
 * per level and 16 bytes per KiB of the deltas; time is a validating parse of
 * every delta plus, per level, the commands that meet the range. */
#define DG_LINEAGE_BASE 0xFFFFFFFFu
#define DG_LINEAGE_MAX_DEPTH 64u
int dg_read_lineage(const uint8_t *r, size_t r_len,
                    const uint8_t *const *deltas, const size_t *delta_len, uint32_t k,
                    uint64_t off, uint64_t len, dg_buffer_t *out);

/* ── lineage reads of a batch on the device ──────────────────────────────────
 *
 * The lineages of a batch are a forest over the streams of a read plan:
 * parent[i] is DG_LINEAGE_BASE or the index of another stream of the plan.
 *   parent[i] == DG_LINEAGE_BASE: stream i's reference is ref_len bytes at
 *      ref_off of the reference arena, as for dg_read_plan_run;
 *   otherwise: ref_off is ignored and ref_len is what the caller states to be
 *      the parent's version size; the index passes validate every COPY of the
 *      stream against it (status c above holds the caller to it).
 * At most DG_LINEAGE_MAX_DEPTH deltas lie between a stream and its base.
 *
 * dg_lineage_plan_create checks the forest on the host: a parent out of range,
 * a cycle, or a depth above DG_LINEAGE_MAX_DEPTH is DG_ERR_INVALID_ARG, and
 * dg_last_error says which stream.  The read plan must outlive the lineage
 * plan, which uses its stream table and its index memory and owns only the
 * parents; destroy the lineage plan first.  Streams are indexed by the read
 * plan's own passes, dg_read_plan_index or dg_read_plan_index_chunked, with
 * identical results; a run before either is DG_ERR_INVALID_ARG.
 *
 * Run.  One launch, one block per request; no allocation, no host
 * synchronisation; n_req <= max_requests (DG_ERR_INVALID_ARG otherwise).
 * Requests, slots and outputs are dg_read_plan_run's: d_status[j] as above,
 * d_out_len[j] = n and the slice in d_out[out_off .. out_off + n) on DG_OK;
 * bytes [n, len) of the slot are not touched; on a failing status n = 0 and
 * the slot is not touched; nothing outside the slots is written.  out_off may
 * have any alignment; d_out must be 16-byte aligned.
 *
 * Work memory is fixed: a request's block keeps a stack of
 * dg_lineage_work_items() work items in LDS, whatever the data (DESIGN.md,
 * "Lineage reads on the device").  No block waits for another.
 *
 * Cost.  A request parses, per level, the 4 KiB windows of that level's stream
 * that hold commands meeting the range, once per piece the level above cut the
 * range into: about depth x (n + windows touched) work.  Materialising every
 * level (k dg_decode_plan_runs) moves every version whole, and composing
 * (k - 1 dg_compose_plan_runs, an index pass, dg_read_plan_run) pays once for
 * any number of later reads.  Measured with 1 % edits per level and one read
 * per lineage of a whole batch (README.md): a 4 KiB lineage read is the
 * fastest route for 1 MiB versions at every depth up to 16 and for 64 KiB
 * versions up to depth 2; a 64 KiB read only up to depth 2 at 1 MiB; beyond
 * that, materialise.  The item count of a range grows with the square of the
 * depth (every level cuts the range at its own edits).
 *
 * Containment.  As for dg_read_plan_run: whatever the arenas hold, a stale
 * index included, a run reads only reference and delta bytes of the plan's
 * streams and writes only inside the requests' slots.  Under a stale index the
 * kernel re-checks that the commands it walks follow one another and cover the
 * range (a window of zero-length commands only covers nothing and is passed:
 * the walk moves on in the stream), every COPY's src + len <= ref_len, and the
 * depth; a violation ends
 * the request with DG_ERR_MALFORMED (bytes inside its slot are then
 * unspecified), so a request cannot fan out.
 *
 * The kernel lives in dg_lineage.hsaco beside libdeltagpu.so and is loaded at
 * create; DG_ERR_HIP with the path in dg_last_error when it is missing.  Stage
 * timing as for the read plan: "read" (the kernel), "total". */
typedef struct dg_lineage_plan dg_lineage_plan_t;
uint32_t dg_lineage_work_items(void);
int dg_lineage_plan_create(dg_read_plan_t *reads, const uint32_t *parent /* host, n_streams */,
                           uint32_t max_requests, dg_lineage_plan_t **out);
int dg_lineage_plan_run(dg_lineage_plan_t *plan, const uint8_t *d_ref, const uint8_t *d_delta,
                        const dg_read_req_t *d_reqs, uint32_t n_req, uint8_t *d_out,
                        uint32_t *d_out_len, int32_t *d_status, void *stream);
int dg_lineage_plan_set_timing(dg_lineage_plan_t *plan, int slots);
int dg_lineage_plan_stage_times(dg_lineage_plan_t *plan, float *ms, const char **names, int n);
void dg_lineage_plan_destroy(dg_lineage_plan_t *plan);

/* Host buffers, as dg_read_batch: refs[i] and ref_len[i] are read only for
 * streams whose parent is DG_LINEAGE_BASE; for the others ref_len comes from
 * the parent's header (2^32 - 1 when it has no readable header, as for
 * dg_read_lineage).  The forest is checked as at create. */
int dg_read_lineage_batch(dg_context_t *ctx, const uint8_t *const *refs, const size_t *ref_len,
                          const uint8_t *const *deltas, const size_t *delta_len,
                          const uint32_t *parent, uint32_t n_streams,
                          const dg_read_req_t *reqs /* host */, uint32_t n_req,
                          dg_buffer_t *outs, int32_t *status);

/* ── reference selection: resemblance sketches and base matching ─────────────
 *
 * Every entry point above starts from a pair: the caller knows which R a V is
 * encoded against.  A store that receives a new object has to choose that R
 * among the buffers it holds, and a poor choice costs more than any encoder
 * wins back: a delta against an unrelated buffer is |V| plus framing.  The
 * choice is resemblance detection by min-wise sketches (Broder) over the
 * fingerprints the encoders already compute, in the one-permutation form: one
 * hash per window, K bins, the minimum of each bin.  (The reference has no
 * such step.)  The result feeds dg_encode_plan_create: target t against
 * candidate best[t] is one dg_pair_t.
 *
 * Sketch.  Parameters: the seed length p, 1 <= p <= 64 (DG_SEED_LEN is the
 * default), and the bin count K, a power of two with 16 <= K <= 1024
 * (DG_SKETCH_BINS is the default).  For a buffer X of n bytes:
 *   features  fp_a = the Karp-Rabin fingerprint of X[a .. a + p) for every
 *             byte offset a = 0 .. n - p: Horner with base 263 mod 2^61 - 1
 *             (hash.c:28-38).  Every offset counts, so the feature set does
 *             not move when bytes are inserted in front;
 *   hash      h_a = mix(fp_a), the splitmix64 finaliser, mod 2^64:
 *               z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *               z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *               z ^= z >> 31
 *   bin       bin(h) = h >> (64 - log2 K);
 *   sketch    sketch[b] = the minimum h_a over the features with bin(h_a) = b;
 *             a bin no feature falls into holds DG_SKETCH_EMPTY; when n < p
 *             every bin does.
 * A sketch is K uint64_t in bin order (2 KiB at the default K) and a pure
 * function of (bytes, p, K).  The definition is frozen: stores persist
 * sketches.  The host function, the device path and the tests' Python model
 * produce it bit for bit.
 *
 * Score.  For two sketches A and B of the same (p, K):
 *   equal = #{b : A[b] == B[b] != DG_SKETCH_EMPTY}
 *   used  = #{b : A[b] != DG_SKETCH_EMPTY or B[b] != DG_SKETCH_EMPTY}
 * and equal / used estimates the Jaccard resemblance of the two fingerprint
 * sets.  Scores are compared as exact rationals by cross-multiplication (both
 * numbers are at most 1024); no floating point appears anywhere.
 *
 * Selection.  Target t of n_t (a window of a larger set: its index in that set
 * is target_base + t) against candidates c = 0 .. n_c - 1.  c is admissible
 *   DG_MATCH_ALL       always;
 *   DG_MATCH_NOT_SELF  when c != target_base + t;
 *   DG_MATCH_EARLIER   when c < target_base + t: one set matched against
 *                      itself this way has an acyclic base assignment;
 * and eligible when also equal_c >= min_equal (min_equal >= 1).  c beats c'
 * iff equal_c used_c' > equal_c' used_c, or the two products are equal and
 * c < c'.  The result is the eligible candidate that beats every other:
 * best, its equal and used, and reserved = 0; with nothing eligible best =
 * DG_MATCH_NONE and equal = used = 0.
 *
 * dg_sketch and dg_sketch_match are pure host code (no context, no GPU);
 * dg_sketch is linear in len.  A p, K or mode outside the above, or min_equal
 * == 0, is DG_ERR_INVALID_ARG; a len of 4 GiB or more is DG_ERR_TOO_LARGE. */
#define DG_SKETCH_BINS  256
#define DG_SKETCH_EMPTY 0xFFFFFFFFFFFFFFFFull
#define DG_MATCH_NONE   0xFFFFFFFFu
#define DG_MATCH_ALL      0
#define DG_MATCH_NOT_SELF 1
#define DG_MATCH_EARLIER  2
typedef struct {
	uint32_t best;       /* candidate index, or DG_MATCH_NONE */
	uint32_t equal, used;
	uint32_t reserved;   /* 0 */
} dg_match_t;

int dg_sketch(const uint8_t *data, size_t len, uint32_t p, uint32_t K,
              uint64_t *out /* K words */);
int dg_sketch_match(const uint64_t *targets /* n_t x K */, uint32_t n_t,
                    const uint64_t *cands /* n_c x K */, uint32_t n_c, uint32_t K,
                    int mode, uint32_t target_base, uint32_t min_equal,
                    dg_match_t *out /* n_t */);

/* ── sketches of a batch and base matching on the device ───────────────────
 *
 * The same words, bit for bit.  A sketch plan fixes N spans of one device
 * arena, p and K; dg_sketch_plan_run writes span i's sketch to
 * d_sketch[i K .. (i + 1) K).  Every span's windows are cut into chunks of
 * dg_sketch_plan_chunk_bytes consecutive window starts (one value per plan);
 * one block takes one chunk: it stages the chunk's bytes and the p - 1 after
 * them in LDS, every lane fingerprints consecutive windows by rolling, the
 * block keeps the K bins in LDS and folds its non-empty bins into d_sketch
 * with 64-bit unsigned-minimum atomics.  A minimum does not depend on the
 * order, so the result does not depend on the schedule.
 *
 * A run first sets all n K words to DG_SKETCH_EMPTY on the stream, so a plan
 * is run any number of times, on other bytes of the same layout each time, and
 * no run keeps a minimum of the runs before it.  It is a fill and one kernel
 * on one stream: no allocation, no host synchronisation.  d_arena is 16-byte
 * aligned; span offsets and lengths are arbitrary (a span of 4 GiB or more is
 * DG_ERR_TOO_LARGE); spans may overlap; n == 0 is a valid plan whose run
 * touches nothing.  No byte outside a span is read and no word outside the
 * n K outputs is written.
 *
 * dg_sketch_match_device is dg_sketch_match on device arrays: stateless, one
 * kernel launch on the stream.  A wave holds two target sketches in registers
 * (one from 512 bins up) and streams every candidate sketch past them (compare,
 * ballot, population count), so the cost is O(n_t n_c K) word comparisons;
 * d_out needs no alignment beyond a uint32_t's; candidate sketches for
 * thousands of buffers stay in the last-level cache.  n_t == 0 enqueues
 * nothing.
 *
 * The kernels live in dg_sketch.hsaco beside libdeltagpu.so and are loaded on
 * first use; DG_ERR_HIP with the path in dg_last_error when it is missing.
 * Stage timing as for the decode plan: "sketch" (the fill and the kernel) and
 * "total". */
typedef struct dg_sketch_plan dg_sketch_plan_t;

int dg_sketch_plan_create(dg_context_t *ctx, const dg_span_t *spans /* host */,
                          uint32_t n, uint32_t p, uint32_t K, dg_sketch_plan_t **out);
uint32_t dg_sketch_plan_chunk_bytes(const dg_sketch_plan_t *plan);
int dg_sketch_plan_run(dg_sketch_plan_t *plan, const uint8_t *d_arena,
                       uint64_t *d_sketch /* n x K */, void *stream);
int dg_sketch_plan_set_timing(dg_sketch_plan_t *plan, int slots);
int dg_sketch_plan_stage_times(dg_sketch_plan_t *plan, float *ms,
                               const char **names, int n);
void dg_sketch_plan_destroy(dg_sketch_plan_t *plan);

int dg_sketch_match_device(dg_context_t *ctx, const uint64_t *d_targets, uint32_t n_t,
                           const uint64_t *d_cands, uint32_t n_c, uint32_t K,
                           int mode, uint32_t target_base, uint32_t min_equal,
                           dg_match_t *d_out, void *stream);

/* Host buffers in, sketches out (out: n x K words of host memory), sketched on
 * the device in one batch; equal to dg_sketch buffer by buffer. */
int dg_sketch_batch(dg_context_t *ctx, const uint8_t *const *bufs, const size_t *lens,
                    uint32_t n, uint32_t p, uint32_t K, uint64_t *out);

/* ── synthetic batch generators (bench / test inputs, on the device) ─────
 * Workload definitions in DESIGN.md ("Synthetic inputs"); the oracle's
 * or_synth_* functions produce the same bytes on the CPU. */
int dg_synth_edit_pairs_device(dg_context_t *ctx, uint8_t *d_ref,
                               uint8_t *d_ver, uint32_t n_pairs,
                               uint64_t pair_len, uint64_t seed_base,
                               uint64_t n_edits, void *stream);
/* C4 transposition pairs (tests/gen_transpositions.py _gen_sizes/_gen_perm
 * with a per-pair splitmix64 seed seed_base + i): pair i has
 * num_blocks = 8 + (i mod 57) blocks of mean size target_len / num_blocks,
 * pct % of them permuted.  Pairs are packed at 16-byte aligned offsets,
 * written to pairs[n].  With d_ref == NULL only the layout is computed and
 * *ref_bytes / *ver_bytes receive the arena sizes to allocate. */
int dg_synth_transpose_pairs_device(dg_context_t *ctx, uint64_t seed_base,
                                    uint32_t n_pairs, uint64_t target_len,
                                    uint32_t pct, dg_pair_t *pairs,
                                    uint64_t *ref_bytes, uint64_t *ver_bytes,
                                    uint8_t *d_ref, uint8_t *d_ver,
                                    void *stream);
/* Shift pairs (a stated extra workload beside C3: edits that move the
 * diagonal): R_i = the splitmix64 stream of seed seed_base + i, pair_len
 * bytes; V_i = R_i with n_edits edits, one per equal stratum of R_i,
 * indel_pct % of them insertions or deletions of 1..8 bytes (half each), the
 * rest byte substitutions (oracle or_synth_shift).  Layout and the
 * d_ref == NULL protocol as for dg_synth_transpose_pairs_device. */
int dg_synth_shift_pairs_device(dg_context_t *ctx, uint64_t seed_base,
                                uint32_t n_pairs, uint64_t pair_len,
                                uint64_t n_edits, uint32_t indel_pct,
                                dg_pair_t *pairs, uint64_t *ref_bytes,
                                uint64_t *ver_bytes, uint8_t *d_ref,
                                uint8_t *d_ver, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DELTA_GPU_H */
