// dg_read_plan.h — what dg_read_host.cpp lets the chunked index pass
// (dg_index_host.cpp) see of a read plan: its stream table, its index memory,
// and one slot for the pass's own state.  Internal; host only.
#pragma once
#include <stdint.h>

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

}  // namespace dg
