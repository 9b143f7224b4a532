// dg_device.h — the kernels' argument structs and launchers, shared by the
// kernels and the host code that enqueues them.  The constants and plain-data
// records both sides agree on are in dg_layout.h.
#pragma once
#include <stdint.h>

#include "../../include/delta_gpu.h"
#include "dg_layout.h"

namespace dg {


struct EncodeArgs {
	const uint8_t* ref;
	const uint8_t* ver;
	const PairDev* pairs;
	const PairPlanDev* pplan;
	uint32_t n_pairs;          // pairs [pair0, n_pairs) of the batch in this launch
	uint32_t pair0;
	uint32_t p;
	const uint64_t* powc;      // p constants: 263^(p-1-k) mod (2^61-1)
	uint32_t* rec;             // 3 x u32 per COPY record (v, r, len)
	uint32_t* n_rec;           // per pair
	uint64_t* dsize;           // per pair serialized delta size
	int32_t* status;           // per pair
	// Tier-C table pool (long epochs)
	unsigned long long* tables;   // n_tables x 2 x qmax entries
	uint64_t qmax;
	uint32_t n_tables;
	uint32_t* table_locks;
	uint32_t* table_tags;
	// fused serialisation (onepass16_kernel): packed output, offsets and the
	// per-pair look-back words; lookback == nullptr selects scan + serialise
	uint8_t* out;
	uint64_t out_cap;
	uint64_t* offsets;
	unsigned long long* lookback;
	// correcting
	uint32_t buf_cap;          // lookback buffer entries (correcting.c:14-62)
	uint32_t* ctab;            // R index: per pair q x u32 offsets (~0 = empty)
	uint32_t max_seeds;        // max over pairs of |R| - p + 1
	uint64_t* kcls;            // per pair: checkpoint class k (correcting.c:131-136), computed once
	const uint32_t* gpairs;    // the pairs whose R index is built in memory (q > the LDS capacity)
	uint32_t n_gpairs;
	// member mode (onepass16_kernel after the member kernels, dg_members.hip):
	// verified diagonal members are taken as they are; nullptr = plain chain
	const uint32_t* mem_s;     // per member slot (PairPlanDev::mem_base + chunk slots): epoch start
	const uint32_t* n_mem;     // per chunk (PairPlanDev::chunk_base + c): members starting in it
	const uint32_t* srec;      // per member slot: (x, COPY length, ADD head, verified)
	const uint32_t* csum;      // per chunk: verified prefix length, its delta bytes
	// the delta's pieces for member_serialize_kernel: per chunk (chunk_base +
	// c) the members taken in bulk (count, byte offset in the delta; zeroed by
	// the member kernel), and per pair (n_chunks + 2 entries from chunk_base +
	// 2 pair) the runs of records the chain wrote itself, then the trailing
	// ADD + END: uint4 (first record or kSegTail, count, byte offset, ADD start)
	uint32_t* cmap;
	uint32_t* seg;
	uint32_t* nseg;            // per pair: segments written
	// automatic member mode: pairs averaging fewer verified members per chunk
	// than this run the plain chain (its records as one segment); 0 = never
	uint32_t route_min;
	// ... and the pairs so routed, counted by the routed chain (scan_sizes_kernel
	// hands the count to the host and zeroes it; nullptr = not counted)
	uint32_t* route_cnt;
	// --verbose diagnostics (correcting; nullptr = off): per pair 8 u64 —
	// build seeds passing the checkpoint, slots stored, scan checkpoints, fp
	// mismatches, byte mismatches, matches, k, passing seeds whose slot is in
	// the table (correcting.c:95-98, 137-214, 470-485)
	uint64_t* stats;
	// correcting with every R index in LDS: R's CRC-64/XZ computed by the
	// build (nullptr = a separate CRC pass): out[2 pair] = CRC of R
	uint64_t* crc_out;
	const uint64_t* crc_tab;   // the context's CRC tables (CrcArgs::tables)
	const uint64_t* crc_k32;   // x^(8 * 32 * t), t = 0..1023
};

// greedy (dg_greedy.hip): the CSR seed index over every pair's R and the
// scan's outputs (records in the onepass layout, kRecWordsOnepass)
struct GreedyArgs {
	const uint8_t* ref;
	const uint8_t* ver;
	const PairDev* pairs;
	const PairPlanDev* pplan;
	uint32_t n_pairs;
	uint32_t p;
	uint32_t splay;            // ties among the longest: 0 = largest offset, 1 = smallest (DG_OPT_SPLAY)
	uint32_t max_seeds;        // max over pairs of |R| - p + 1
	uint32_t* heads;           // per pair f_size + 1 words from tab_base: bucket b = entries [h[b], h[b + 1])
	uint2* ent;                // per pair |R| - p + 1 entries from m: (offset, tag), grouped by bucket
	uint32_t* rec;
	uint32_t* n_rec;
	uint64_t* dsize;
	int32_t* status;
};

struct SpecArgs {
	const uint8_t* ref;
	const uint8_t* ver;
	const PairDev* pairs;
	const PairPlanDev* pplan;
	const uint2* chunks;       // per wave: (pair, chunk)
	uint32_t job0;             // wave w of the launch takes job job0 + w
	uint32_t* mem_s;           // per member slot: epoch start s_k
	uint32_t* n_mem;           // per chunk: members starting in it
	uint32_t* srec;            // per member slot: (x, COPY length, ADD head, verified)
	uint32_t* csum;            // per chunk: verified prefix length, its delta bytes
	uint32_t* cmap;            // per chunk: bulk (count, byte offset), zeroed here
};

// member-mode serialisation (dg_members.hip): one wave per (pair, chunk) job
// writes the pair's segments 2c, 2c + 1 (the last chunk's wave the rest)
struct MemSerArgs {
	const uint8_t* ver;
	const PairDev* pairs;
	const PairPlanDev* pplan;
	const uint2* chunks;
	uint32_t job0;             // the launch's jobs: [job0, job0 + n_jobs)
	const uint32_t* cmap;
	const uint32_t* seg;
	const uint32_t* nseg;
	const uint32_t* mem_s;
	const uint32_t* srec;
	const uint32_t* rec;       // kRecWordsOnepass words per record
	const uint64_t* offsets;   // n + 1
	uint8_t* out;
	uint64_t out_cap;
	int32_t* status;
	// sum |V| of the batch: a sparse batch (the scan's total delta bytes,
	// offsets[n_pairs], under half of it) runs the serialiser's whole grid
	uint64_t v_total;
	uint32_t n_pairs;
};

struct SerArgs {
	const uint8_t* ver;
	const PairDev* pairs;
	const PairPlanDev* pplan;
	const uint32_t* rec;
	uint32_t rec_words;        // 3 or 4 (kRecWords*)
	const uint32_t* n_rec;
	const uint64_t* crc;       // 2 per pair: R, V (final: the kernel writes header bytes 9..24)
	const uint64_t* offsets;   // n+1
	uint8_t* out;
	uint64_t out_cap;
	int32_t* status;
	uint32_t n_pairs;
};

struct CrcArgs {
	const uint8_t* arena[2];   // selected by CrcSpanDev::which
	const CrcSpanDev* spans;
	const CrcSegDev* segs;
	uint32_t n_segs;
	uint32_t n_spans;
	const uint64_t* tables;    // slice (8x256) + nibble tables: 6 levels, kseg, 16 pad inverses
	uint64_t* seg_crc;
	uint64_t* out;             // per span: CRC-64/XZ value
	const uint64_t* xinv;      // 16 constants x^(-8t) mod P
	uint64_t kseg;             // x^(8*kCrcSegBytes) mod P
	const uint32_t* prio_flag; // member plans: set once the member kernel is done (rows pass to priority 1)
};

struct dg_decode_desc_dev {   // == dg_decode_desc_t
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_len;
	uint64_t out_off, out_cap;
};

struct DecodeArgs {
	const uint8_t* ref;
	const uint8_t* delta;
	const dg_decode_desc_dev* descs;
	uint32_t n;
	uint8_t* out;
	uint64_t* out_len;
	int32_t* status;
	const uint64_t* tables;    // CRC tables (CrcArgs::tables); with crc_check
	uint32_t crc_check;        // 1: src/dst CRC-64/XZ computed and checked in-kernel (main.c:341-385)
};

// Measurement switches of the A/B builds (make ab / make variant, compiled
// with -DDG_AB_SWITCHES): getenv(name) there, always NULL in the product
// library, which therefore reads no environment variable that changes the
// work it does (dg_host.cpp).
const char* ab_env(const char* name);
// the context's slot for the pipelined host path's state, and its destructor
void** ctx_io(dg_context_t* ctx, void (*release)(void*));
uint64_t ctx_limits_gen(const dg_context_t* ctx);   // changes with every dg_context_set_limit
int ctx_device(const dg_context_t* ctx);            // the context's HIP device
// the plan's per-pair parameters (n_pairs records; for print_verbose, dg_plan.h)
const PairPlanDev* plan_pp(const dg_encode_plan_t* P);
// what dg_inplace_plan_create_for, dg_compose_plan_create_for and dg_invert_plan_create_for read of an encode plan
const dg_pair_t* plan_pairs(const dg_encode_plan_t* P);
dg_context_t* plan_ctx(const dg_encode_plan_t* P);
void plan_options(const dg_encode_plan_t* P, dg_algorithm_t* algo, dg_diff_options_t* opts);
// the context's slots for code objects loaded at run time, one per module
// (filled by load_kernels, dg_hostutil.h)
enum : int { kCtxModInplace = 0, kCtxModUpdate = 1, kCtxModCompose = 2, kCtxModInvert = 3, kCtxModSketch = 4, kCtxModRead = 5, kCtxModSplice = 6, kCtxModIndex = 7, kCtxModLineage = 8, kCtxModules = 9 };
void** ctx_module(dg_context_t* ctx, int slot, void (*release)(void*));
const uint64_t* ctx_crc_tables(const dg_context_t* ctx);     // the CRC tables on the device (CrcArgs::tables)
int ctx_fail(dg_context_t* ctx, int code, const char* msg);   // records dg_last_error, returns code

// launchers (dg_kernels.hip)
// (member plans: routed_after, when set, is waited for between the member
// chain's launch and the routed plain chain's)
hipError_t launch_onepass(const EncodeArgs& a, uint32_t p, bool aligned16, hipStream_t st,
                          hipEvent_t routed_after = nullptr);
bool onepass16_selected();   // false when DG_ONEPASS_GLOBAL=1 forces the HBM-direct kernel
hipError_t launch_members(const SpecArgs& a, uint32_t n_chunks, uint32_t n_cu, hipStream_t st);
hipError_t launch_member_serialize(const MemSerArgs& a, uint32_t n_chunks, uint32_t n_cu, hipStream_t st);
// ev_built, ev_fork (nullable): recorded after the R-index build, before the
// V scan (stage timing; the fork of V's CRC when the build computes R's)
hipError_t launch_correcting_clear(const EncodeArgs& a, hipStream_t st);
hipError_t launch_correcting(const EncodeArgs& a, uint32_t p, hipStream_t st, uint32_t lds_cap, uint64_t qmin,
                             hipEvent_t ev_built, hipEvent_t ev_fork);
// greedy: zero the heads (head_words in all), build every pair's index, record
// ev_built (nullable, stage timing), scan
hipError_t launch_greedy(const GreedyArgs& g, uint64_t head_words, hipStream_t st, hipEvent_t ev_built);
// (route_cnt / route_fb: the routed-pair count moved to a host-mapped word)
hipError_t launch_scan(const uint64_t* sz, uint64_t* off, uint32_t n, hipStream_t st,
                       uint32_t* route_cnt = nullptr, uint32_t* route_fb = nullptr);
hipError_t launch_serialize_wave(const SerArgs& s, hipStream_t st);   // wave per pair, header CRCs included
hipError_t launch_crc_patch(uint8_t* out, const uint64_t* offsets, const uint64_t* crc,
                            const int32_t* status, uint32_t n, hipStream_t st);
// pass: the row-interleaved pass on byte tables (16 KiB LDS per block) or on
// five-bit tables (3.25 KiB: beside the member kernel, which leaves little LDS)
enum : int { kCrcPassRows = 0, kCrcPassRows5 = 1 };
hipError_t launch_crc(const CrcArgs& a, hipStream_t st, uint32_t overlap_cap = 0, int pass = kCrcPassRows,
                      bool finalize = true);
hipError_t launch_crc_finalize(const CrcArgs& a, hipStream_t st);   // the per-span combine alone
// the CRC on 16-byte pieces (32 KiB of tables): for a pass that has the GPU to itself
hipError_t launch_crc_wide(const CrcArgs& a, uint32_t n_cu, hipStream_t st);
hipError_t launch_decode(const DecodeArgs& a, hipStream_t st);
hipError_t launch_synth(uint8_t* ref, uint8_t* ver, uint32_t n_pairs, uint64_t pair_len,
                        uint64_t seed_base, uint64_t n_edits, hipStream_t st);
hipError_t launch_synth_shift(uint8_t* ref, uint8_t* ver, const SynthSpan* spans, const uint64_t* v_off,
                              uint32_t n, uint64_t n_edits, uint32_t pct, hipStream_t st);
hipError_t launch_synth_transpose(uint8_t* ref, uint8_t* ver, const SynthSpan* spans, uint32_t n_spans,
                                  const SynthCopy* cmds, uint32_t n_cmds, hipStream_t st);

}  // namespace dg
