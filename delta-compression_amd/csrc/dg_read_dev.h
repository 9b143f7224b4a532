// dg_read_dev.h — what the range-read kernels (dg_read_dev.hip, built as the
// stand-alone code object lib/dg_read.hsaco) and the host code that launches
// them (dg_read_host.cpp) agree on; the chunked index pass (dg_index_dev.h)
// and the lineage reads (dg_lineage_dev.h) leave and read the same index.
// The device functions those three kernel files share are dg_read_walk_dev.h's.
#pragma once
#include <stdint.h>

namespace dgrd {

constexpr uint32_t kRdBlock = 256;     // threads per stream of the index kernel
// Threads per request of the read kernel: 256 (4 KiB parse windows) or 64 (one
// wave, 1 KiB windows).  dg_read_dev.hip builds the form DG_READ_BLOCK names,
// this one by default; the other is built as lib/dg_read_alt.hsaco for
// measurements only (make read_alt; scripts/read_rate.py).
constexpr uint32_t kRdReadBlock = 256;
constexpr uint32_t kRdStride = 1024;   // stream bytes per index entry

struct RdStream {   // == dg_read_stream_t
	uint64_t ref_off, ref_len;
	uint64_t delta_off, delta_len;
};

struct RdReq {   // == dg_read_req_t
	uint32_t stream, off, len, reserved;
	uint64_t out_off;
};

// A stream's index in the plan's memory: the head, then n_ent entries.
// Entry k names the first command that starts at or after stream offset
// kRdStride * k (its stream offset and its dst); entries past the last
// command hold (dl, ~0).  In a sequential stream the entries' dst never
// decrease, so a read binary-searches them.
struct RdHead {
	uint64_t doff;      // where the stream was when it was indexed
	uint32_t dl;        // and its length
	uint32_t vsize;
	int32_t status;
	uint32_t flags;     // kRdSeq
	uint32_t n_ent;     // dl / kRdStride + 1 (0 for a failed stream)
	uint32_t pad;
};
struct RdEnt {
	uint32_t spos, dst;
};
constexpr uint32_t kRdSeq = 1;   // every command starts where the one before it ends, the last ends at vsize

// bytes of the index of a stream of at most delta_len bytes, a multiple of 16:
// at most delta_len / 128 + 55
inline uint64_t index_bytes(uint64_t delta_len) {
	return (sizeof(RdHead) + sizeof(RdEnt) * (delta_len / kRdStride + 1) + 15) & ~15ull;
}

struct RdIndexArgs {
	const uint8_t* delta;
	const RdStream* streams;
	const uint64_t* delta_offsets;   // n + 1, or nullptr: the descriptors are exact
	const int32_t* delta_status;     // or nullptr
	int32_t* stream_status;          // or nullptr
	uint8_t* index;
	const uint64_t* index_off;       // n + 1 (16-byte aligned offsets)
	uint32_t n;
};

struct RdArgs {
	const uint8_t* ref;
	const uint8_t* delta;
	const RdStream* streams;
	const uint8_t* index;
	const uint64_t* index_off;
	const RdReq* reqs;
	uint8_t* out;
	uint32_t* out_len;
	int32_t* status;
	uint32_t n_streams;
	uint32_t n_req;
};

}  // namespace dgrd
