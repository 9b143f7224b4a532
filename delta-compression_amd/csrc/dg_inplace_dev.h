// dg_inplace_dev.h — what the in-place conversion kernels (dg_inplace_dev.hip,
// built as the stand-alone code object lib/dg_inplace.hsaco) and the host code
// that launches them (dg_inplace_host.cpp) agree on.
//
// Work memory is per delta, sized at plan creation from the delta's capacity:
// at most C = (cap - 25) / 13 copies and A = (cap - 25) / 9 adds (a plan made
// from an encode plan uses the encoder's record capacity instead).  Per copy
// 18 u32 words (src, dst, len, range start, range end, in-degree, rank,
// by-rank, order; dg_inplace_core.h's nine) plus one flag byte and one bit of
// the spilled ready bitmap: 73.2 bytes.  Per add 8 bytes (stream offset,
// output offset).  The depth-n DFS stacks are among the nine core words.
//
// One wave converts one delta.  Like the greedy encoder, a pathological delta
// holds its wave for as long as it takes (its neighbour ranges can total
// O(n^2) indices, and Tarjan and the cycle search walk them serially); the
// rest of the batch proceeds.
#pragma once
#include <stdint.h>

namespace dgip {

constexpr uint32_t kCopyWords = 18;   // u32 arrays of C entries
constexpr uint32_t kAddWords = 2;     // u32 arrays of A entries

struct IpDesc {
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_cap;
	uint64_t work_off;        // bytes into the plan's work memory
	uint32_t max_copies, max_adds;
};

struct IpRes {                // the order stage's result for the emit stage
	uint64_t stream_off;      // where the stream starts in d_delta
	uint64_t add_bytes;       // the original ADDs as written: 9 + len each
	uint32_t stream_len;
	uint32_t n_copies, kept, victims, n_adds;
	uint32_t passthrough;     // already in-place: copied unchanged
};

struct IpArgs {
	const uint8_t* ref;
	const uint8_t* delta;
	const IpDesc* descs;
	const uint64_t* delta_offsets;   // n + 1, or nullptr: the descriptors are exact
	const int32_t* delta_status;     // or nullptr
	uint8_t* work;
	IpRes* res;
	uint64_t* sizes;
	int32_t* status;
	uint8_t* out;
	uint64_t out_cap;
	const uint64_t* out_offsets;
	uint32_t n;
	uint32_t policy;
};

inline uint64_t work_bytes(uint64_t max_copies, uint64_t max_adds) {
	const uint64_t b = 4 * (kCopyWords * max_copies + (max_copies + 31) / 32 + kAddWords * max_adds) + max_copies;
	return (b + 15) & ~15ull;
}

}  // namespace dgip
