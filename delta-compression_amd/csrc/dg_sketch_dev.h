// dg_sketch_dev.h — what the resemblance kernels (dg_sketch_dev.hip, built as the
// stand-alone code object lib/dg_sketch.hsaco), the host code that launches
// them (dg_sketch_host.cpp), the plan geometry (dg_plan.cpp) and the host
// functions (dg_sketch.cpp) agree on.  The definition of a sketch, of a score
// and of the selection is in include/delta_gpu.h.
//
// A plan cuts every span's windows (a window = the p bytes at one offset) into
// chunks of chunk_bytes consecutive window starts; one block takes one chunk.
// A chunk's block reads the chunk's bytes and the p - 1 after them, never past
// the span.  Spans shorter than p have no chunk.
#pragma once
#include <stdint.h>

namespace dgsk {

constexpr uint64_t kEmpty = 0xFFFFFFFFFFFFFFFFull;   // DG_SKETCH_EMPTY
constexpr uint32_t kNone = 0xFFFFFFFFu;              // DG_MATCH_NONE
constexpr uint32_t kMaxSeed = 64, kMinBins = 16, kMaxBins = 1024;

// window starts per chunk: a multiple of 4 kSkBlock (every lane takes a
// multiple of four windows), one value per plan
#ifndef DG_SKETCH_CHUNK_BYTES
#define DG_SKETCH_CHUNK_BYTES 16384
#endif
constexpr uint32_t kChunkBytes = DG_SKETCH_CHUNK_BYTES;
constexpr uint32_t kSkBlock = 256;         // threads of a sketch block
constexpr uint32_t kMatchBlock = 256;      // threads of a match block: 4 waves
constexpr uint32_t kMatchTargets = 2;      // target sketches a wave holds in registers ...
// ... up to 256 bins; one from 512 bins up (8 and 16 words per lane per sketch)
inline constexpr uint32_t match_targets_per_wave(uint32_t K) { return K >= 512 ? 1 : kMatchTargets; }

struct SkSpan {            // == dg_span_t
	uint64_t off, len;
};

struct SkItem {            // one block's work: chunk `chunk` of span `span`
	uint32_t span, chunk;
};

// The staged bytes of a chunk in LDS: dword d of the image at word d + d / 16,
// so that lanes whose windows start 64 bytes apart read different banks.
// Image bytes: the chunk, p - 1 more, and up to 15 in front (the image starts
// at a 16-byte boundary of the arena) and behind (whole 16-byte pieces).
inline constexpr uint32_t image_words(uint32_t chunk_bytes) {
	const uint32_t dwords = (chunk_bytes + kMaxSeed - 1 + 15 + 15) / 16 * 4;
	return dwords + dwords / 16 + 1;
}
// dynamic LDS of a sketch block: K bins, the 256-entry roll table, the image
inline constexpr uint32_t sketch_lds_bytes(uint32_t K, uint32_t chunk_bytes) {
	return 8 * K + 8 * 256 + 4 * image_words(chunk_bytes);
}

struct SkArgs {
	const uint8_t* arena;
	const SkSpan* spans;
	const SkItem* items;
	uint64_t* out;            // n x K words; holds kEmpty everywhere when the kernel starts
	const uint64_t* powc;     // p constants 263^(p-1-k) mod (2^61-1)
	uint64_t top;             // 263^(p-1) mod (2^61-1)
	uint32_t p, K, shift;     // shift = 64 - log2 K
	uint32_t chunk_bytes;
};

struct MatchArgs {
	const uint64_t* targets;   // n_t x K
	const uint64_t* cands;     // n_c x K
	uint32_t* out;             // n_t x 4 words: dg_match_t
	uint32_t n_t, n_c, K;
	uint32_t mode, target_base, min_equal;
};

}  // namespace dgsk
