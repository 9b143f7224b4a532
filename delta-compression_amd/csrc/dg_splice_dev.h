// dg_splice_dev.h — what the splice kernels (dg_splice_dev.hip, built as the
// stand-alone code object lib/dg_splice.hsaco), the host code that launches
// them (dg_splice_host.cpp) and the plan's sizing (dg_plan.cpp) agree on.
//
// Work memory is per segment: one summary the map stage leaves for the resolve
// stage and one emit record the resolve stage leaves for the emit stage.  No
// per-command tables: the emit stage parses its stream again.
#pragma once
#include <stdint.h>

namespace dgsp {

// One segment, fixed at plan creation.
struct SpDesc {
	uint64_t cap;        // most bytes its delta may have
	uint64_t shift;      // x^(8 * bytes of V after this segment in its group) mod P: its dst_crc's weight
	uint32_t rebase;     // seg.r_off - whole.r_off: added to every COPY's src
	uint32_t r_len;      // the window's length: a COPY's src + len may not pass it
	uint32_t v_rel;      // seg.v_off - whole.v_off: where the segment starts in the group's version
	uint32_t v_len;
	uint32_t group;
	uint32_t pad;
};

// One group, fixed at plan creation.
struct SpGroup {
	uint32_t first, count;   // its segments: [first, first + count)
	uint32_t v_len;          // the whole pair's version size
	uint32_t pad;
};

constexpr uint32_t kOwnsRun = 1u;    // SpSum/SpRec flag bits
constexpr uint32_t kSingle = 2u;     // SpSum: the whole segment is one run
constexpr uint32_t kContinues = 4u;  // SpRec: the segment's first run continues its predecessor's: no header

// What the map stage leaves per segment.  Runs are the segment's own normal
// form: its non-empty commands with neighbours merged, COPY sources rebased.
struct SpSum {
	int32_t incoming;    // the nonzero status that came with the segment, else 0
	int32_t own;         // what the splicer found: 0, 8 malformed, 7 over capacity, 2 unsupported
	uint32_t runs;       // 0: the segment contributes nothing
	uint32_t flags;      // kSingle
	uint32_t first_kind, first_src, first_len;   // the first run: 1 COPY / 2 ADD, where it starts in R, its length
	uint32_t last_kind, last_end, last_len;      // the last run: its kind, where it ends in R, its length
	uint64_t body;       // bytes of the runs' headers and payloads, every run with its header
	uint64_t crc_term;   // dst_crc * shift mod P
};

// What the resolve stage leaves per segment.  Offsets are relative to the
// group's first command byte (output byte 25).
struct SpRec {
	uint32_t out, out_end;   // the segment's bytes
	uint32_t flags;          // kContinues; kOwnsRun: last_len is valid
	uint32_t last_len;       // the whole length of the run that begins as the segment's last run
};

struct SpRes {               // the resolve stage's result per group
	uint64_t dst_crc;
};

struct SpArgs {
	const uint8_t* deltas;
	const uint64_t* offsets;        // n_seg + 1: segment j's stream is deltas[offsets[j] .. offsets[j + 1])
	const int32_t* seg_status;      // or nullptr
	const uint64_t* src_crc;        // per group
	const SpDesc* descs;
	const SpGroup* groups;
	SpSum* sums;
	SpRec* recs;
	SpRes* res;
	uint64_t* sizes;                // per group
	int32_t* status;                // per group
	uint8_t* out;
	uint64_t out_cap;
	const uint64_t* out_offsets;    // n_groups + 1
	uint32_t n_seg;
	uint32_t n_groups;
};

}  // namespace dgsp
