// dg_invert_dev.h — what the inversion kernels (dg_invert_dev.hip, built as the
// stand-alone code object lib/dg_invert.hsaco) and the host code that launches
// them (dg_invert_host.cpp) agree on.
//
// Work memory is per delta, sized at plan creation: C possible COPYs
// ((delta_cap - 26) / 13; a plan made from an encode plan uses the encoder's
// record capacity).  Per possible COPY 64 bytes: two 16-byte records (the sort
// ping-pongs between two record buffers) and one 32-byte emit record; one more
// emit record closes the stream (the literals after the last COPY).  Only
// non-empty COPYs take entries.
#pragma once
#include <stdint.h>

namespace dgiv {

constexpr uint32_t kNoClose = 0xFFFFFFFFu;

struct IvDesc {
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_cap;
	uint64_t work_off;        // bytes into the plan's work memory
	uint32_t max_copies;      // C
	uint32_t pad;
};

// a non-empty COPY of the input: reads [src, src + len) of R, writes V at dst
struct IvRec {
	uint32_t src, len, dst, index;
};

// What the map stage leaves per COPY in key order for the emit stage: the
// literals of R before the COPY's owned interval and the interval itself.
// Offsets are relative to the delta's first command byte (output byte 25).
struct IvEmit {
	uint32_t gap_x;       // where the record's bytes of R start: the literals, then the owned interval
	uint32_t gap_len;     // literals (one ADD when > 0)
	uint32_t out;         // where the record's first output byte goes
	uint32_t vsrc;        // head: where the owned interval is in V
	uint32_t close_off;   // the COPY length field this record closes (the run open before it), or kNoClose
	uint32_t close_len;   // and that run's length
	uint32_t head;        // 1: the owned interval begins a COPY of the output
	uint32_t pad;
};

struct IvRes {               // the map stage's result for the emit stage
	uint64_t delta_off;      // where the stream starts in d_delta
	uint32_t n_emit;         // emit records (COPYs + 1)
	uint32_t pad;
};

struct IvArgs {
	const uint8_t* ref;
	const uint8_t* delta;
	const IvDesc* descs;
	const uint64_t* delta_offsets;   // n + 1, or nullptr: the descriptors are exact
	const int32_t* delta_status;     // or nullptr
	uint8_t* work;
	IvRes* res;
	uint64_t* sizes;
	int32_t* status;
	uint8_t* out;
	uint64_t out_cap;
	const uint64_t* out_offsets;
	uint32_t n;
};

inline uint64_t work_bytes(uint64_t max_copies) {
	return 2 * sizeof(IvRec) * max_copies + sizeof(IvEmit) * (max_copies + 1);
}

// the most bytes the inverse of a delta with at most max_copies COPYs against
// ref_len bytes has: header, 2 C + 1 runs, every byte of R a literal, END
inline uint64_t out_bound(uint64_t max_copies, uint64_t ref_len) {
	return 25 + 13 * max_copies + 9 * (max_copies + 1) + ref_len + 1;
}

}  // namespace dgiv
