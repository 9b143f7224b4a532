// dg_compose_dev.h — what the composition kernels (dg_compose_dev.hip, built
// as the stand-alone code object lib/dg_compose.hsaco) and the host code that
// launches them (dg_compose_host.cpp) agree on.
//
// Work memory is per pair, sized at plan creation: CA possible commands of A
// and CB of B ((cap - 25) / 9 each; a plan made from two encode plans uses the
// encoders' record capacities).  Per command of A five u32 words, 20 bytes:
// where it starts in V1, its R source or its payload's offset in stream A, the
// prefix count of run heads, the prefix count of ADD run heads, the prefix of
// ADD bytes (CA + 1 entries each: the last one closes the tiling).  Per
// command of B one 20-byte emit record.  Only non-empty commands take entries.
#pragma once
#include <stdint.h>

namespace dgcp {

constexpr uint32_t kAWords = 5;   // u32 arrays of CA + 1 entries
constexpr uint32_t kNoClose = 0xFFFFFFFFu;
constexpr uint32_t kHeadBit = 0x80000000u;

struct CpDesc {
	uint64_t a_off, a_cap;
	uint64_t b_off, b_cap;
	uint64_t work_off;        // bytes into the plan's work memory
	uint32_t max_a, max_b;    // CA, CB
};

// What the map stage leaves per non-empty command of B for the emit stage.
// Offsets are relative to the pair's first command byte (output byte 25).
struct CpRec {
	uint32_t pos;         // the command in stream B
	uint32_t out;         // where its first output byte goes
	uint32_t j0;          // COPY: its first command of A; kHeadBit: its first run begins a run of the output
	uint32_t close_off;   // the length field this command closes (the run open before it), or kNoClose
	uint32_t close_len;   // and that run's length
};

struct CpRes {                // the map stage's result for the emit stage
	uint64_t a_off, b_off;    // where the streams start in d_a and d_b
	uint32_t n_a, n_b;        // non-empty commands
	uint32_t close_off;       // the last run's length field (kNoClose: V2 is empty)
	uint32_t close_len;
};

struct CpArgs {
	const uint8_t* a;
	const uint8_t* b;
	const CpDesc* descs;
	const uint64_t* a_offsets;   // n + 1, or nullptr: the descriptors are exact
	const uint64_t* b_offsets;
	const int32_t* a_status;     // or nullptr
	const int32_t* b_status;
	uint8_t* work;
	CpRes* res;
	uint64_t* sizes;
	int32_t* status;
	uint8_t* out;
	uint64_t out_cap;
	const uint64_t* out_offsets;
	uint32_t n;
	uint32_t ignore_hash;
};

inline uint64_t work_bytes(uint64_t max_a, uint64_t max_b) {
	const uint64_t b = 4 * kAWords * (max_a + 1) + sizeof(CpRec) * max_b;
	return (b + 15) & ~15ull;
}

}  // namespace dgcp
