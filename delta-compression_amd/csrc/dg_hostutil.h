// dg_hostutil.h — what the host files that touch the device share (dg_host.cpp,
// dg_host_io.cpp and the transform plans' dg_inplace_host.cpp,
// dg_update_host.cpp, dg_compose_host.cpp, dg_invert_host.cpp, the sketch
// plan's dg_sketch_host.cpp, the read plan's dg_read_host.cpp and
// dg_index_host.cpp and the lineage plan's dg_lineage_host.cpp): device
// buffers, the stage-timing event ring, the loader of the code objects that
// are loaded at run time, the timed launch of a run that is one kernel
// (launch_timed: read, lineage), and the small pieces of the plans and of the
// host-memory batch wrappers, among them the version_size a wrapper sizes a
// stream's output from (header_vsize: in-place, read, lineage).
// Internal; needs HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_plan.h"

namespace dg {

struct DevBuf {
	void* p = nullptr;
	size_t n = 0;
	~DevBuf() { if (p) hipFree(p); }
	void release() {
		if (p) hipFree(p);
		p = nullptr;
		n = 0;
	}
	int alloc(size_t bytes) {
		if (p) { hipFree(p); p = nullptr; }
		n = bytes;
		if (bytes == 0) return 0;
		return hipMalloc(&p, bytes) == hipSuccess ? 0 : -1;
	}
	// as alloc, but never leaves p null: a kernel argument of the transform
	// plans is a valid address even for an empty batch
	int alloc_nonnull(size_t bytes) { return alloc(std::max<size_t>(bytes, 16)); }
	template <class T> T* as() const { return static_cast<T*>(p); }
};

// Stage timing of a plan: `slots` sets of `per_run` events, one set per
// timed run (a ring); ev holds ev_sets >= slots sets (never shrunk, only the
// ring is).  The caller has the plan's device current.
struct TimingRing {
	std::vector<hipEvent_t> ev;
	uint32_t per_run = 0;
	uint32_t slots = 0, runs = 0, ev_sets = 0;
	uint32_t every = 1, calls = 0;   // events on every `every`-th run (dg_*_plan_set_timing_every)
	bool timing = false;
	~TimingRing() {
		for (auto& e : ev)
			if (e) hipEventDestroy(e);
	}
	// false: an event could not be created (timing is then off)
	bool set(uint32_t n_slots, uint32_t events_per_run) {
		if (n_slots > ev_sets) {
			for (auto& e : ev) hipEventDestroy(e);
			ev.assign((size_t)events_per_run * n_slots, nullptr);
			per_run = events_per_run;
			ev_sets = slots = 0;
			for (auto& e : ev)
				// timing only: no system-scope fence when the event is recorded
				// (a cache writeback + invalidate per event slowed the timed
				// steps by 15 %: C2 0.335 -> 0.391 ms with two events per step)
				if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
					e = nullptr;
					timing = false;
					return false;
				}
			ev_sets = n_slots;
		}
		// the ring is exactly `slots` runs long, so stage_times averages the
		// last `slots` runs even after a longer ring was set before
		slots = n_slots;
		timing = n_slots > 0;
		runs = calls = 0;
		return true;
	}
	void set_every(uint32_t n) {
		every = n;
		calls = 0;
	}
	// the event set this run records, or nullptr (timing off, or not this run's turn)
	hipEvent_t* next() {
		if (!timing || calls++ % every != 0) return nullptr;
		return &ev[(size_t)per_run * (runs++ % slots)];
	}
	// recorded sets to average over, and set s of them
	uint32_t used() const { return slots ? std::min(runs, slots) : 0; }
	hipEvent_t* set_at(uint32_t s) { return &ev[(size_t)per_run * s]; }
	// A plan whose stages are the intervals between consecutive events, with
	// first-to-last as the final one (per_run values; stage_names has as many):
	// their means over the recorded sets, up to n of them, into ms and names
	// (either may be NULL).  Returns the count; 0 when nothing was recorded.
	int stage_times(const char* const* stage_names, float* ms, const char** names, int n) {
		const uint32_t sets = used();
		if (!sets || n < 1) return 0;
		std::vector<double> acc(per_run, 0.0);
		for (uint32_t s = 0; s < sets; ++s) {
			hipEvent_t* e = set_at(s);
			if (hipEventSynchronize(e[per_run - 1]) != hipSuccess) return 0;
			float t = 0;
			for (uint32_t k = 0; k + 1 < per_run; ++k) {
				hipEventElapsedTime(&t, e[k], e[k + 1]);
				acc[k] += t;
			}
			hipEventElapsedTime(&t, e[0], e[per_run - 1]);
			acc[per_run - 1] += t;
		}
		const int m = std::min<int>(n, (int)per_run);
		for (int k = 0; k < m; ++k) {
			if (ms) ms[k] = (float)(acc[k] / sets);
			if (names) names[k] = stage_names[k];
		}
		return m;
	}
};

// The kernels of a code object that is not part of the library's fat binary:
// `file` beside the library (found via dladdr), loaded into the context's slot
// (dg_device.h) on first use and unloaded with the context.  fns[k] is kernel
// names[k].  A failure is DG_ERR_HIP with "<label>: cannot load <path>: <hip
// error>" as the context's last error.  (dg_host.cpp)
int load_kernels(dg_context_t* ctx, int slot, const char* file, const char* label, const char* const* names,
                 int n_names, const hipFunction_t** fns);

// records "<what> failed: <hip error>" as the context's last error; returns DG_ERR_HIP
inline int hip_fail(dg_context_t* ctx, const char* what, hipError_t e) {
	const std::string msg = std::string(what) + " failed: " + hipGetErrorString(e);
	return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
}

// A run that is one kernel (read, lineage): the launch between the two events
// of the run's set (ev, or nullptr: not timed).  `name` is the kernel's, for
// the context's last error.
inline int launch_timed(dg_context_t* ctx, hipEvent_t* ev, hipFunction_t fn, const char* name, uint32_t grid,
                        uint32_t block, void* args, hipStream_t st) {
	void* params[] = {args};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, (std::string("launch of ") + name).c_str(), e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

// what the transform plans' sizing reads of an encode plan (dg_plan.h)
inline EncodePlanView encode_plan_view(const dg_encode_plan_t* enc) {
	dg_algorithm_t algo;
	dg_diff_options_t o;
	plan_options(enc, &algo, &o);
	return EncodePlanView{plan_pairs(enc), plan_pp(enc), algo, o.p};
}

// dg_*_plan_destroy of a plan with a ctx member: waits for the context's stream first
template <class Plan>
void plan_destroy(Plan* P) {
	if (!P) return;
	hipSetDevice(ctx_device(P->ctx));
	hipStreamSynchronize((hipStream_t)dg_context_stream(P->ctx));
	delete P;
}

// ── the host-memory batch wrappers ──

template <class F>
struct ScopeExit {
	F f;
	explicit ScopeExit(F g) : f(g) {}
	~ScopeExit() { f(); }
	ScopeExit(const ScopeExit&) = delete;
	ScopeExit& operator=(const ScopeExit&) = delete;
};

// version_size as the delta's header states it (bytes 5..8, big-endian), or
// `otherwise` where d does not begin with a header: what a wrapper sizes a
// stream's output from before the device has judged the stream
inline uint64_t header_vsize(const uint8_t* d, size_t dl, uint64_t otherwise = 0) {
	if (dl < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4) != 0) return otherwise;
	return ((uint64_t)d[5] << 24) | ((uint64_t)d[6] << 16) | ((uint64_t)d[7] << 8) | d[8];
}

// out takes a malloc'ed copy of len bytes at src (one byte allocated when len == 0); false: out of memory
inline bool buffer_copy(dg_buffer_t* out, const uint8_t* src, uint64_t len) {
	out->data = (uint8_t*)malloc(len ? len : 1);
	if (!out->data) return false;
	memcpy(out->data, src, len);
	out->len = len;
	return true;
}

// stream i ended with status s: reported per stream where the caller gave an
// array, and the first failure otherwise
struct BatchStatus {
	int32_t* status;
	int first_bad = DG_OK;
	void set(uint32_t i, int s) {
		if (status) status[i] = s;
		if (s && !first_bad) first_bad = s;
	}
	int result() const { return status ? DG_OK : first_bad; }
};

}  // namespace dg
