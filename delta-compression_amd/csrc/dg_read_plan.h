// dg_read_plan.h — what dg_read_host.cpp lets the chunked index pass
// (dg_index_host.cpp) and the lineage plan (dg_lineage_host.cpp) see of a read
// plan: its stream table, its index memory, and one slot for the chunked
// pass's own state; and what the read and lineage plans' runs and host-memory
// batch wrappers share.  Internal; host only.
#pragma once
#include <stdint.h>

#include <functional>

#include "../../include/delta_gpu.h"
#include "dg_read_dev.h"

namespace dg {

struct ReadPlanView {
	dg_context_t* ctx;
	uint32_t n;
	const dg_read_stream_t* streams;    // host copy of the descriptors (n)
	const uint64_t* index_off;          // host copy of the index offsets (n + 1)
	const dgrd::RdStream* d_streams;
	uint8_t* d_index;
	const uint64_t* d_index_off;
};
ReadPlanView read_plan_view(dg_read_plan_t* P);
// the plan's slot for the chunked pass's state, released with the plan
void** read_plan_ext(dg_read_plan_t* P, void (*release)(void*));
bool read_plan_indexed(const dg_read_plan_t* P);
void read_plan_set_indexed(dg_read_plan_t* P);   // an index pass has been enqueued: runs are allowed

// The arguments of dg_read_plan_run and dg_lineage_plan_run (label: "read
// plan", "lineage plan"): n_req <= max_req, and for a run with requests no
// null buffer (has_streams: d_ref and d_delta are needed) and a 16-byte
// aligned d_out.  DG_OK also for n_req == 0, which runs nothing.
int read_run_check(dg_context_t* ctx, const char* label, uint32_t n_req, uint32_t max_req, bool has_streams,
                   const void* d_ref, const void* d_delta, const void* d_reqs, const void* d_out, const void* d_out_len,
                   const void* d_status);

// dg_read_batch and dg_read_lineage_batch: the references packed 16 bytes
// apart in one arena, the deltas packed in another, every request's slot (no
// larger than its stream's version_size, header_vsize) 16 bytes apart in a
// third; a read plan over them, the upload, dg_read_plan_index, the caller's
// run, the download of the slots' used prefix, outs and status.  The caller
// has checked its arguments, emptied outs and returned for n_req == 0.
struct ReadBatchOps {
	// stream i's ref_len as its descriptor states it; *in_arena: its bytes are refs[i], packed into the arena
	std::function<uint64_t(uint32_t i, bool* in_arena)> ref_len;
	// what the run needs on top of the read plan, made before anything is uploaded (may be empty) ...
	std::function<int(dg_read_plan_t*)> open;
	// ... and released before the read plan is (may be empty)
	std::function<void()> close;
	// dg_read_plan_run or its like on the device arenas
	std::function<int(dg_read_plan_t*, const uint8_t* d_ref, const uint8_t* d_delta, const dg_read_req_t* d_reqs,
	                  uint32_t n_req, uint8_t* d_out, uint32_t* d_out_len, int32_t* d_status, void* stream)>
	    run;
};
int read_batch(dg_context_t* ctx, const uint8_t* const* refs, const uint8_t* const* deltas, const size_t* delta_len,
               uint32_t n_streams, const dg_read_req_t* reqs, uint32_t n_req, dg_buffer_t* outs, int32_t* status,
               const ReadBatchOps& ops);

}  // namespace dg
