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

uint64_t header_vsize(const uint8_t* d, size_t dl, uint64_t otherwise) {
	if (dl < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4) != 0) return otherwise;
	return ((uint64_t)d[5] << 24) | ((uint64_t)d[6] << 16) | ((uint64_t)d[7] << 8) | d[8];
}

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
	if (n_req > P->max_req) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "lineage plan: more requests than max_requests");
	if (n_req == 0) return DG_OK;
	if (!d_reqs || !d_out || !d_out_len || !d_status || (P->n && (!d_ref || !d_delta)))
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if ((uintptr_t)d_out & 15) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the output arena must be 16-byte aligned");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	const ReadPlanView v = read_plan_view(P->reads);
	hipEvent_t* ev = P->ring.next();
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
	void* params[] = {&a};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[0], n_req, 1, 1, kLnBlock, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_lineage_read_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

void dg_lineage_plan_destroy(dg_lineage_plan_t* P) { plan_destroy(P); }

int dg_read_lineage_batch(dg_context_t* ctx, const uint8_t* const* refs, const size_t* ref_len, const uint8_t* const* deltas,
                          const size_t* delta_len, const uint32_t* parent, uint32_t n_streams, const dg_read_req_t* reqs,
                          uint32_t n_req, dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n_streams && (!refs || !ref_len || !deltas || !delta_len || !parent)) || (n_req && (!reqs || !outs)))
		return DG_ERR_INVALID_ARG;
	for (uint32_t j = 0; j < n_req; ++j) outs[j] = dg_buffer_t{nullptr, 0};
	if (n_req == 0) return DG_OK;
	int rc = check_forest(ctx, parent, n_streams);
	if (rc) return rc;
	// the bases' references packed 16 bytes apart in one arena, the deltas packed
	// in another, every request's slot 16 bytes apart in a third
	std::vector<dg_read_stream_t> sv(n_streams);
	uint64_t rt = 0, dt = 0, ot = 0;
	for (uint32_t i = 0; i < n_streams; ++i) {
		const bool on_base = parent[i] == DG_LINEAGE_BASE;
		if ((on_base && ref_len[i] && !refs[i]) || (delta_len[i] && !deltas[i])) return DG_ERR_INVALID_ARG;
		// a parent without a readable header states no size: its own status ends the request
		const uint64_t rl = on_base ? ref_len[i] : header_vsize(deltas[parent[i]], delta_len[parent[i]], 0xFFFFFFFFull);
		sv[i] = dg_read_stream_t{on_base ? rt : 0, rl, dt, delta_len[i]};
		if (on_base) rt = (rt + rl + 15) & ~15ull;
		dt += delta_len[i];
	}
	std::vector<dg_read_req_t> rv(reqs, reqs + n_req);
	for (uint32_t j = 0; j < n_req; ++j) {
		rv[j].out_off = ot;
		// a slot no larger than the stream's version (its header says)
		const uint64_t vs = rv[j].stream < n_streams ? header_vsize(deltas[rv[j].stream], delta_len[rv[j].stream], 0) : 0;
		ot = (ot + std::min<uint64_t>(rv[j].len, vs) + 15) & ~15ull;
	}
	dg_read_plan_t* plan = nullptr;
	rc = dg_read_plan_create(ctx, sv.data(), n_streams, n_req, &plan);
	if (rc) return rc;
	dg_lineage_plan_t* lin = nullptr;
	ScopeExit guard([&] {
		dg_lineage_plan_destroy(lin);
		dg_read_plan_destroy(plan);
	});
	if ((rc = dg_lineage_plan_create(plan, parent, n_req, &lin)) != DG_OK) return rc;
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_ref, d_delta, d_req, d_out, d_len, d_st;
	std::vector<uint8_t> h_ref, h_delta, h_out;
	std::vector<uint32_t> lens(n_req);
	std::vector<int32_t> stv(n_req);
	try {
		h_ref.resize(rt);
		h_delta.resize(dt);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t i = 0; i < n_streams; ++i) {
		if (parent[i] == DG_LINEAGE_BASE && ref_len[i]) memcpy(h_ref.data() + sv[i].ref_off, refs[i], ref_len[i]);
		if (delta_len[i]) memcpy(h_delta.data() + sv[i].delta_off, deltas[i], delta_len[i]);
	}
	if (d_ref.alloc_nonnull(rt) || d_delta.alloc_nonnull(dt) || d_req.alloc_nonnull(sizeof(RdReq) * n_req) ||
	    d_out.alloc_nonnull(ot) || d_len.alloc_nonnull(4ull * n_req) || d_st.alloc_nonnull(4ull * n_req)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((rt && hipMemcpyAsync(d_ref.p, h_ref.data(), rt, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (dt && hipMemcpyAsync(d_delta.p, h_delta.data(), dt, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemcpyAsync(d_req.p, rv.data(), sizeof(RdReq) * n_req, hipMemcpyHostToDevice, st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	if ((rc = dg_read_plan_index(plan, d_delta.as<uint8_t>(), nullptr, nullptr, nullptr, st)) != DG_OK) return rc;
	rc = dg_lineage_plan_run(lin, d_ref.as<uint8_t>(), d_delta.as<uint8_t>(), d_req.as<dg_read_req_t>(), n_req,
	                         d_out.as<uint8_t>(), d_len.as<uint32_t>(), d_st.as<int32_t>(), st);
	if (rc) return rc;
	if (hipMemcpyAsync(lens.data(), d_len.p, 4ull * n_req, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(stv.data(), d_st.p, 4ull * n_req, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	// the slots' used parts end at the last request that has bytes
	uint64_t used = 0;
	for (uint32_t j = 0; j < n_req; ++j)
		if (!stv[j] && lens[j]) used = rv[j].out_off + lens[j];
	try {
		h_out.resize(used);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	if (used && (hipMemcpyAsync(h_out.data(), d_out.p, used, hipMemcpyDeviceToHost, st) != hipSuccess ||
	             hipStreamSynchronize(st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	BatchStatus bs{status};
	for (uint32_t j = 0; j < n_req; ++j) {
		const uint32_t nb = stv[j] ? 0u : lens[j];
		const uint8_t none = 0;
		if (!stv[j] && !buffer_copy(&outs[j], nb ? h_out.data() + rv[j].out_off : &none, nb)) {
			for (uint32_t k = 0; k < j; ++k) dg_buffer_free(&outs[k]);
			return DG_ERR_NOMEM;
		}
		bs.set(j, stv[j]);
	}
	return bs.result();
}

}  // extern "C"
