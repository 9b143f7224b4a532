// dg_update_dev.h — what the in-place update kernel (dg_update_dev.hip, built as
// the stand-alone code object lib/dg_update.hsaco) and the host code that
// launches it (dg_update_host.cpp) agree on.
#pragma once
#include <stdint.h>

namespace dgup {

constexpr uint32_t kUpBlock = 256;   // threads per stream (one block each)

struct UpDesc {   // == dg_update_desc_t
	uint64_t buf_off, buf_cap;
	uint64_t ref_len;
	uint64_t delta_off, delta_len;
};

struct UpArgs {
	uint8_t* buf;                    // the arena of the streams' buffers: R in, V out
	const uint8_t* delta;
	const UpDesc* descs;
	const uint64_t* delta_offsets;   // n + 1, or nullptr: the descriptors are exact
	const int32_t* delta_status;     // or nullptr
	uint64_t* out_len;
	int32_t* status;
	const uint64_t* tables;          // the context's CRC tables (CrcArgs::tables)
	uint32_t n;
	uint32_t crc_check;              // 0: ignore_hash
	// phase A's per-window command lists for phase B: stream i's part is
	// scratch[scratch_off[i] .. scratch_off[i + 1]) (16-byte aligned offsets)
	uint8_t* scratch;
	const uint64_t* scratch_off;
	unsigned long long* prof;        // kUpProfN sums (the profiling code object only; nullptr otherwise)
};

// phase cycles of the profiling build (make update_prof), summed over blocks
enum { UP_A_PARSE, UP_A_CRC, UP_B_ZERO, UP_B_PARSE, UP_B_APPLY, UP_C_CRC, UP_TOTAL, UP_BLOCKS, kUpProfN };

// Bytes that hold every window's record of a stream of at most delta_len
// bytes: 2 per command (the shortest is 9 bytes) and 32 per window (a window
// that is not the last consumes at least 4096 - 12 bytes), at most kUpScratchMax:
// a stream of more than some 30 000 commands has phase B parse again.
constexpr uint64_t kUpScratchMax = 64ull << 10;
inline uint64_t scratch_bytes(uint64_t delta_len) {
	const uint64_t b = 2 * (delta_len / 9 + 1) + 32 * (delta_len / 4000 + 2);
	return ((b < kUpScratchMax ? b : kUpScratchMax) + 15) & ~15ull;
}

}  // namespace dgup
