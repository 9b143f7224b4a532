// dg_index_dev.h — what the chunked index kernels (dg_index_dev.hip, built as
// the stand-alone code object lib/dg_index.hsaco) and the host code that
// launches them (dg_index_host.cpp) agree on.  The index they leave is the one
// dg_read_dev.h describes; this is their work memory.
#pragma once
#include <stdint.h>

#include "dg_read_dev.h"

namespace dgix {

constexpr uint32_t kIxWin = 4096;             // stream bytes per window of the map and fill kernels
constexpr uint32_t kIxChunkDefault = 65536;   // dg_read_plan_chunk_index(plan, 0): DG_CHUNK_BYTES_DEFAULT
// A stream's chunk k is stream bytes [k C, (k + 1) C).  exit[x], one u32 per
// stream byte: the stream offset of the first command at or after the end of
// x's chunk on the chain that starts at x (the stream's length when the chain
// runs off the stream's end), or one of two codes.  Offsets are at most the
// stream's length, which dg_read_plan_chunk_index keeps below the codes.
constexpr uint32_t kIxEnd = 0xFFFFFFFFu;      // the chain from x reaches END inside the chunk
constexpr uint32_t kIxBad = 0xFFFFFFFEu;      // ... or a malformed command (framing only)
constexpr uint64_t kIxMaxStream = 0xFFFFFFF0ull;   // longest stream a chunked plan takes

// per chunk: what resolve leaves for fill, and fill for finish
struct IxChunk {
	uint32_t stream;      // (host, at dg_read_plan_chunk_index) the chunk's stream
	uint32_t entry;       // resolve: the first command at or after the chunk's start on the true chain
	uint32_t live;        // resolve: on the chain before END, the stream's end or a malformed command
	uint32_t res;         // fill: kIxFailed | kIxAny | kIxBrk
	uint32_t first_dst;   // fill: dst of the chunk's first command
	uint32_t last_end;    // fill: dst + len of its last
};
constexpr uint32_t kIxFailed = 1;   // a command on the chain is malformed or out of bounds
constexpr uint32_t kIxAny = 2;      // a command starts in the chunk
constexpr uint32_t kIxBrk = 4;      // one of them does not start where the one before it ends

// per stream: the early statuses, taken once by resolve
struct IxStream {
	uint64_t doff;
	uint32_t dl, vsize;
	int32_t st;           // passed on, capacity, bad magic, in-place
	uint32_t walk_bad;    // the chain reaches a command with bad framing
	uint32_t pad[2];
};

struct IxArgs {
	const uint8_t* delta;
	const dgrd::RdStream* streams;
	const uint64_t* delta_offsets;   // n + 1, or nullptr
	const int32_t* delta_status;     // or nullptr
	int32_t* stream_status;          // or nullptr
	uint8_t* index;                  // the plan's index memory (dg_read_dev.h)
	const uint64_t* index_off;
	uint32_t* exit;
	const uint64_t* exit_off;        // n + 1: a stream's first exit word
	const uint32_t* chunk_base;      // n + 1: a stream's first chunk
	IxChunk* chunks;
	IxStream* sstate;
	uint32_t n, n_chunks, chunk_bytes;
};

}  // namespace dgix
