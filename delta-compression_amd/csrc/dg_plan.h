// dg_plan.h — the host arithmetic behind a context and an encode plan: the
// CRC constant tables, the table sizes and buffer geometry of a batch, and
// the --verbose report.  No HIP: dg_host.cpp allocates and uploads what these
// functions compute, and tests/test_plan_cpu.py runs them on the CPU.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_compose_dev.h"
#include "dg_inplace_dev.h"
#include "dg_invert_dev.h"
#include "dg_layout.h"
#include "dg_sketch_dev.h"
#include "dg_splice_dev.h"

namespace dg {

// ── number theory, GF(2)[x] mod P (reflected: bit 63 = x^0) ──
bool is_prime_u64(uint64_t n);
uint64_t next_prime(uint64_t n);              // src/c/hash.c:180-190
uint64_t gf2_mul(uint64_t a, uint64_t b);
uint64_t gf2_pow(uint64_t base, uint64_t e);  // base^e
uint64_t gf2_xpow(uint64_t n);                // x^n
uint64_t gf2_div_x(uint64_t z);               // z * x^-1

// Every CRC constant the kernels read (layout: the kCrc* offsets of dg_layout.h)
struct CrcTables {
	std::vector<uint64_t> tab;   // kCrcTabWords: slice-by-8, nibble, row and five-bit tables
	uint64_t xinv[16];           // x^(-8t)
	uint64_t k32[1024];          // x^(8 * 32 * t) (the correcting build's CRC)
	uint64_t kseg;               // x^(8 kCrcSegBytes)
};
void crc_tables_build(CrcTables& t);

// Segment layout for spans whose device address is 16-byte aligned at
// offset 0 of the arena (checked at run time): the padded domain is
// [align_down(off,16), align_up(off+len,16)).
// outs: where span i's CRC goes in CrcArgs::out (nullptr: at i)
void plan_crc_spans(const std::vector<dg_span_t>& spans, const std::vector<uint32_t>& which,
                    std::vector<CrcSpanDev>& sd, std::vector<CrcSegDev>& seg,
                    const std::vector<uint32_t>* outs = nullptr);

// What a plan's geometry depends on besides the batch and its options: the
// device, the context's limits and the A/B switches (the value of each
// variable, NULL when unset and always NULL in the product library)
struct PlanEnv {
	uint32_t n_cu = 256;
	int lds_bytes = 0;               // LDS per block (0: unknown, no R index in LDS)
	uint64_t table_pool_bytes = 0;   // DG_LIMIT_TABLE_POOL_BYTES (0 = automatic)
	uint64_t onepass_members = 0;    // DG_LIMIT_ONEPASS_MEMBERS (0 auto, 1 on, 2 off)
	bool onepass16 = true;           // onepass16_selected()
	const char* no_members = nullptr;   // DG_NO_MEMBERS
	const char* members = nullptr;      // DG_MEMBERS
	const char* corr_build = nullptr;   // DG_CORR_BUILD
	const char* fused = nullptr;        // DG_FUSED
	const char* route_min = nullptr;    // DG_ROUTE_MIN
};

struct EncodeGeometry {
	std::vector<PairPlanDev> pp;
	uint64_t out_bound = 0;
	uint64_t total_rec = 0;
	uint64_t qmax = 0, qmin = ~0ull;
	uint64_t ctab_entries = 0;     // correcting: sum of per-pair index sizes
	uint64_t greedy_heads = 0;     // greedy: sum of per-pair head words (buckets + 1), in d_ctab
	uint64_t greedy_entries = 0;   // greedy: (offset, tag) per seed of every R
	uint64_t max_seeds = 0;
	bool aligned16 = true;         // every pair offset a multiple of 16 (LDS-window kernel)
	uint64_t v_total = 0;          // sum |V| of the batch
	std::vector<uint64_t> powc;    // 263^(p-1-k) mod (2^61-1)
	uint32_t corr_lds_cap = 0;     // correcting: R indexes up to this many slots built in LDS (DG_CORR_BUILD=global: none)
	bool crc_fused = false;        // correcting: R's CRC computed by the LDS build, V's forked after it
	std::vector<uint32_t> gpairs;  // correcting: the pairs whose R index is built in memory
	std::vector<CrcSpanDev> spans;
	std::vector<CrcSegDev> segs;
	uint64_t table_bytes = 0;      // table-tier pool: bytes per table (2 x qmax u64)
	uint32_t n_tables = 0;
	bool fused = false;            // DG_FUSED=1: onepass16 serialises in-kernel (default: scan + serialise)
	// onepass member mode (dg_members.hip): wanted for this batch; the plan
	// clears it when the member arrays cannot be allocated
	bool members = false;
	uint32_t route_min = 0;        // member mode chosen automatically: route poorly verified pairs to the plain chain
	std::vector<uint32_t> jobs;    // members: (pair, chunk) per member-kernel wave
	uint64_t mem_slots = 0;        // members: member slots of the batch
	uint32_t n_chunks = 0;
};

// Validates the options and sizes everything a plan of `n` pairs needs.
// Returns DG_OK, or the status with its message in err.
int encode_geometry(dg_algorithm_t algo, const dg_diff_options_t& o, const dg_pair_t* pairs, uint32_t n,
                    const PlanEnv& env, EncodeGeometry& g, std::string& err);

// The most bytes an encoder writes for a version of v_len bytes with seed
// length p (>= 1): what an encode plan reserves per pair, and what a plan that
// reads an encoder's deltas takes as their capacity.
uint64_t pair_out_bound(dg_algorithm_t algo, uint64_t p, uint64_t v_len);

// ── the transform plans' sizing (dg_inplace_host.cpp, dg_compose_host.cpp, dg_invert_host.cpp) ──
// Each returns DG_OK with the device descriptors (work offsets assigned, 16-byte
// aligned regions of work_bytes(...) each) and the work memory's size, or
// DG_ERR_TOO_LARGE (a stream or reference of 4 GiB or more) with its message
// in err.  The _for variants size from encode plans.

// what they read of an encode plan of n pairs
struct EncodePlanView {
	const dg_pair_t* pairs;
	const PairPlanDev* pp;
	dg_algorithm_t algo;
	uint64_t p;
};

struct InplaceGeometry {
	std::vector<dgip::IpDesc> descs;
	uint64_t work = 0;    // bytes of work memory
	uint64_t bound = 0;   // dg_inplace_plan_output_bound: sum of capacity + the bytes COPYs can turn into ADD payload
};
int inplace_plan_geometry(const dg_inplace_desc_t* descs, uint32_t n, InplaceGeometry& g, std::string& err);
int inplace_plan_geometry_for(const EncodePlanView& e, uint32_t n, InplaceGeometry& g, std::string& err);

struct ComposeGeometry {
	std::vector<dgcp::CpDesc> descs;
	uint64_t work = 0;
};
// the most commands a stream of cap bytes holds (the END byte may be missing)
uint32_t compose_max_cmds(uint64_t cap);
int compose_plan_geometry(const dg_compose_desc_t* descs, uint32_t n, ComposeGeometry& g, std::string& err);
int compose_plan_geometry_for(const EncodePlanView& a, const EncodePlanView& b, uint32_t n, ComposeGeometry& g,
                              std::string& err);

struct InvertGeometry {
	std::vector<dgiv::IvDesc> descs;
	uint64_t work = 0;
	uint64_t bound = 0;   // dg_invert_plan_output_bound: sum of dgiv::out_bound
};
// the most COPYs a stream of cap bytes holds
uint32_t invert_max_copies(uint64_t cap);
int invert_plan_geometry(const dg_invert_desc_t* descs, uint32_t n, InvertGeometry& g, std::string& err);
int invert_plan_geometry_for(const EncodePlanView& e, uint32_t n, InvertGeometry& g, std::string& err);

// ── the splice plan (dg_splice_host.cpp) and the host splice (dg_splice.cpp) ──
struct SpliceGeometry {
	std::vector<dgsp::SpDesc> descs;     // per segment
	std::vector<dgsp::SpGroup> groups;
	uint64_t bound = 0;   // dg_splice_plan_output_bound: the capacities' sum + one byte per group; 0 without capacities
};
// Checks the groups (seg_first: n_groups + 1 ascending entries from 0 to n_seg,
// every group with a segment), that each group's segments tile its V span in
// order and that every window lies inside its R span (DG_ERR_INVALID_ARG); an
// r_len or v_len at or above 4 GiB - 1 MiB, the encode plan's limit, or a
// capacity of 4 GiB or more is DG_ERR_TOO_LARGE.  caps may be NULL: no bound.
// Fills the descriptors: rebase, window, place in V and the weight of the
// segment's dst_crc in the group's, x^(8 * bytes of V after it).
int splice_plan_geometry(const dg_pair_t* segs, uint32_t n_seg, const dg_pair_t* wholes, const uint32_t* seg_first,
                         uint32_t n_groups, const uint64_t* caps, SpliceGeometry& g, std::string& err);

// ── the sketch plan (dg_sketch_host.cpp) ──
struct SketchGeometry {
	std::vector<dgsk::SkItem> items;   // the grid: one block per (span, chunk), span by span
	std::vector<uint64_t> powc;        // 263^(p-1-k) mod (2^61-1); powc[0] is SkArgs::top
	uint32_t chunk_bytes = 0;          // window starts per chunk (dg_sketch_plan_chunk_bytes)
	uint32_t shift = 0;                // 64 - log2 K
};
// Validates p, K and the spans (DG_ERR_INVALID_ARG; DG_ERR_TOO_LARGE for a span
// of 4 GiB or more, or more chunks than a grid holds) and cuts every span's
// n - p + 1 windows into chunks of chunk_bytes window starts (0: the default,
// dgsk::kChunkBytes).  A chunk's windows are those starting in it; the last
// p - 1 of them read into the next chunk, none past the span.
int sketch_plan_geometry(const dg_span_t* spans, uint32_t n, uint32_t p, uint32_t K, uint32_t chunk_bytes,
                         SketchGeometry& g, std::string& err);

// dg_update_plan_create's descriptor checks: DG_OK, DG_ERR_TOO_LARGE (a buffer
// or a length of 4 GiB or more) or DG_ERR_INVALID_ARG (a region wrapping the
// address space, two buffer regions overlapping), with its message in err
int update_check_descs(const dg_update_desc_t* descs, uint32_t n, std::string& err);

// --verbose: the reference's diagnostic lines for one pair to stderr, from
// its parameters, its 8 device counters (copied to the host; may be NULL for
// onepass) and its delta
void print_verbose(dg_algorithm_t algo, const dg_diff_options_t& o, const dg_pair_t& d, const PairPlanDev& x,
                   const uint64_t* stats, const uint8_t* delta, size_t delta_len);

}  // namespace dg
