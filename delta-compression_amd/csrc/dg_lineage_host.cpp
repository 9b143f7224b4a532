// dg_lineage_host.cpp — host side of the lineage reads (dg_lineage_plan_*,
// dg_read_lineage_batch; include/delta_gpu.h).
//
// The kernel is the stand-alone code object dg_lineage.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel: a run is one launch,
// one block per request.  The streams, their indexes and the index passes are
// the read plan's (dg_read_plan.h); this plan adds the forest over them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_hostutil.h"
#include "dg_lineage_dev.h"
#include "dg_read_plan.h"

using namespace dg;
using namespace dgrd;
using namespace dgln;

static_assert(kLnBase == DG_LINEAGE_BASE && kLnMaxDepth == DG_LINEAGE_MAX_DEPTH, "the header states both");
static_assert(kLnItems >= DG_LINEAGE_MAX_DEPTH, "a request's stack makes progress at every allowed depth");

static const char* const kLnKernels[] = {"dg_lineage_read_kernel"};

constexpr int kLnEvents = 2;   // the kernel's start and end

struct dg_lineage_plan {
	dg_context_t* ctx = nullptr;
	dg_read_plan_t* reads = nullptr;
	const hipFunction_t* fn = nullptr;   // kLnKernels
	uint32_t n = 0, max_req = 0;
	DevBuf d_parent;
	TimingRing ring;   // kLnEvents events per run
};

namespace {

// the forest: every parent in range, no cycle, at most DG_LINEAGE_MAX_DEPTH deltas down to a base
int check_forest(dg_context_t* ctx, const uint32_t* parent, uint32_t n) {
	char msg[160];
	std::vector<uint32_t> depth(n, 0);   // 0: not known yet
	std::vector<uint32_t> trail;
	for (uint32_t i = 0; i < n; ++i)
		if (parent[i] != DG_LINEAGE_BASE && parent[i] >= n) {
			snprintf(msg, sizeof msg, "lineage plan: stream %u: parent %u is not a stream of the read plan", i, parent[i]);
			return ctx_fail(ctx, DG_ERR_INVALID_ARG, msg);
		}
	for (uint32_t i = 0; i < n; ++i) {
		trail.clear();
		uint32_t s = i;
		while (s != DG_LINEAGE_BASE && !depth[s]) {
			if (trail.size() > n) break;
			trail.push_back(s);
			s = parent[s];
		}
		if (trail.size() > n || (s != DG_LINEAGE_BASE && std::find(trail.begin(), trail.end(), s) != trail.end())) {
			snprintf(msg, sizeof msg, "lineage plan: stream %u: its parents form a cycle", i);
			return ctx_fail(ctx, DG_ERR_INVALID_ARG, msg);
		}
		uint32_t below = s == DG_LINEAGE_BASE ? 0u : depth[s];
		for (size_t k = trail.size(); k-- > 0;) depth[trail[k]] = ++below;
		if (depth[i] > DG_LINEAGE_MAX_DEPTH) {
			snprintf(msg, sizeof msg, "lineage plan: stream %u: %u deltas down to its base, more than %u", i, depth[i],
			         (unsigned)DG_LINEAGE_MAX_DEPTH);
			return ctx_fail(ctx, DG_ERR_INVALID_ARG, msg);
		}
	}
	return DG_OK;
}

}  // namespace

extern "C" {

uint32_t dg_lineage_work_items(void) { return kLnItems; }

int dg_lineage_plan_create(dg_read_plan_t* reads, const uint32_t* parent, uint32_t max_requests, dg_lineage_plan_t** out) {
	if (!reads || !out) return DG_ERR_INVALID_ARG;
	*out = nullptr;
	const ReadPlanView v = read_plan_view(reads);
	dg_context_t* ctx = v.ctx;
	if (v.n && !parent) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "lineage plan: null parent array");
	int rc = check_forest(ctx, parent, v.n);
	if (rc) return rc;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	const hipFunction_t* fn = nullptr;
	rc = load_kernels(ctx, kCtxModLineage, "dg_lineage.hsaco", "lineage read kernel", kLnKernels, 1, &fn);
	if (rc) return rc;
	auto* P = new (std::nothrow) dg_lineage_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->reads = reads;
	P->fn = fn;
	P->n = v.n;
	P->max_req = max_requests;
	if (P->d_parent.alloc_nonnull(4ull * v.n)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "lineage plan: device allocation failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (v.n) e = hipMemcpyAsync(P->d_parent.p, parent, 4ull * v.n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "lineage plan: upload of the parents failed");
	}
	*out = P;
	return DG_OK;
}

int dg_lineage_plan_set_timing(dg_lineage_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kLnEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// "read": the kernel; "total": the run, which is that one launch
int dg_lineage_plan_stage_times(dg_lineage_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kLnEvents] = {"read", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_lineage_plan_run(dg_lineage_plan_t* P, const uint8_t* d_ref, const uint8_t* d_delta, const dg_read_req_t* d_reqs,
                        uint32_t n_req, uint8_t* d_out, uint32_t* d_out_len, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (!read_plan_indexed(P->reads)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "lineage plan: no index pass of the read plan has run");
	const int rc = read_run_check(ctx, "lineage plan", n_req, P->max_req, P->n != 0, d_ref, d_delta, d_reqs, d_out, d_out_len, d_status);
	if (rc || n_req == 0) return rc;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	const ReadPlanView v = read_plan_view(P->reads);
	LnArgs a{};
	a.ref = d_ref;
	a.delta = d_delta;
	a.streams = v.d_streams;
	a.index = v.d_index;
	a.index_off = v.d_index_off;
	a.parent = P->d_parent.as<uint32_t>();
	a.reqs = reinterpret_cast<const RdReq*>(d_reqs);
	a.out = d_out;
	a.out_len = d_out_len;
	a.status = d_status;
	a.n_streams = P->n;
	a.n_req = n_req;
	return launch_timed(ctx, P->ring.next(), P->fn[0], "dg_lineage_read_kernel", n_req, kLnBlock, &a, st);
}

void dg_lineage_plan_destroy(dg_lineage_plan_t* P) { plan_destroy(P); }

int dg_read_lineage_batch(dg_context_t* ctx, const uint8_t* const* refs, const size_t* ref_len, const uint8_t* const* deltas,
                          const size_t* delta_len, const uint32_t* parent, uint32_t n_streams, const dg_read_req_t* reqs,
                          uint32_t n_req, dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n_streams && (!refs || !ref_len || !deltas || !delta_len || !parent)) || (n_req && (!reqs || !outs)))
		return DG_ERR_INVALID_ARG;
	for (uint32_t j = 0; j < n_req; ++j) outs[j] = dg_buffer_t{nullptr, 0};
	if (n_req == 0) return DG_OK;
	const int rc = check_forest(ctx, parent, n_streams);   // before anything is allocated
	if (rc) return rc;
	dg_lineage_plan_t* lin = nullptr;
	ReadBatchOps ops;
	// a stream on the base reads refs[i]; any other the version of its parent's delta, whose header states its
	// size (a parent without a readable header states none: its own status ends the request)
	ops.ref_len = [&](uint32_t i, bool* in_arena) {
		*in_arena = parent[i] == DG_LINEAGE_BASE;
		return *in_arena ? (uint64_t)ref_len[i] : header_vsize(deltas[parent[i]], delta_len[parent[i]], 0xFFFFFFFFull);
	};
	ops.open = [&](dg_read_plan_t* plan) { return dg_lineage_plan_create(plan, parent, n_req, &lin); };
	ops.close = [&] { dg_lineage_plan_destroy(lin); };
	ops.run = [&](dg_read_plan_t*, const uint8_t* d_ref, const uint8_t* d_delta, const dg_read_req_t* d_reqs, uint32_t n,
	              uint8_t* d_out, uint32_t* d_out_len, int32_t* d_status, void* stream) {
		return dg_lineage_plan_run(lin, d_ref, d_delta, d_reqs, n, d_out, d_out_len, d_status, stream);
	};
	return read_batch(ctx, refs, deltas, delta_len, n_streams, reqs, n_req, outs, status, ops);
}

}  // extern "C"
