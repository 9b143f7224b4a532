// dg_lineage_dev.h — what the lineage-read kernel (dg_lineage_dev.hip, built as
// the stand-alone code object lib/dg_lineage.hsaco) and the host code that
// launches it (dg_lineage_host.cpp) agree on.  The streams, their indexes and
// the requests are the read plan's (dg_read_dev.h).
#pragma once
#include <stdint.h>

#include "dg_read_dev.h"

namespace dgln {

constexpr uint32_t kLnBlock = 256;          // threads per request: decode's 4 KiB window step
constexpr uint32_t kLnBase = 0xFFFFFFFFu;   // == DG_LINEAGE_BASE: the stream's reference is bytes of the arena
constexpr uint32_t kLnMaxDepth = 64;        // == DG_LINEAGE_MAX_DEPTH
// Work items of a request's stack (LDS), and as many staged children of one
// step.  Any value >= kLnMaxDepth + 2 makes progress ("Lineage reads
// on the device"); 256 keeps three blocks on a CU.
constexpr uint32_t kLnItems = 256;
constexpr uint32_t kLnRun = 128;            // items one parsed window serves at the most
constexpr uint32_t kLnDirect = 1024;        // pieces (ADD payloads, COPYs from R) staged before they are copied

struct LnArgs {
	const uint8_t* ref;
	const uint8_t* delta;
	const dgrd::RdStream* streams;
	const uint8_t* index;
	const uint64_t* index_off;
	const uint32_t* parent;   // n_streams: kLnBase or a stream (a forest of depth <= kLnMaxDepth: checked at create)
	const dgrd::RdReq* reqs;
	uint8_t* out;
	uint32_t* out_len;
	int32_t* status;
	uint32_t n_streams;
	uint32_t n_req;
};

}  // namespace dgln
