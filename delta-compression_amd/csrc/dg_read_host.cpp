// dg_read_host.cpp — host side of the range reads (dg_read_plan_*,
// dg_read_batch; include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_read.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  An index is one
// launch, one block per stream; a run is one launch, one block per request.
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
#include "dg_plan.h"
#include "dg_read_dev.h"
#include "dg_read_plan.h"

using namespace dg;
using namespace dgrd;

static_assert(sizeof(RdStream) == sizeof(dg_read_stream_t), "RdStream is dg_read_stream_t");
static_assert(sizeof(RdReq) == sizeof(dg_read_req_t), "RdReq is dg_read_req_t");

static const char* const kRdKernels[] = {"dg_read_index_kernel", "dg_read_kernel"};

constexpr int kRdEvents = 2;   // the read kernel's start and end

struct dg_read_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kRdKernels
	uint32_t n = 0, max_req = 0;
	uint32_t block = kRdReadBlock;       // threads per request of the loaded read kernel
	bool indexed = false;
	DevBuf d_streams;
	DevBuf d_index, d_index_off;   // the streams' indexes (dg_read_dev.h)
	TimingRing ring;               // kRdEvents events per run
	std::vector<dg_read_stream_t> streams;   // host copies, for the chunked index pass (dg_index_host.cpp)
	std::vector<uint64_t> ioff;
	void* ext = nullptr;           // that pass's state (read_plan_ext)
	void (*ext_free)(void*) = nullptr;
	~dg_read_plan() {
		if (ext && ext_free) ext_free(ext);
	}
};

ReadPlanView dg::read_plan_view(dg_read_plan_t* P) {
	return ReadPlanView{P->ctx, P->n, P->streams.data(), P->ioff.data(), P->d_streams.as<RdStream>(),
	                    P->d_index.as<uint8_t>(), P->d_index_off.as<uint64_t>()};
}
void** dg::read_plan_ext(dg_read_plan_t* P, void (*release)(void*)) {
	P->ext_free = release;
	return &P->ext;
}
bool dg::read_plan_indexed(const dg_read_plan_t* P) { return P->indexed; }
void dg::read_plan_set_indexed(dg_read_plan_t* P) { P->indexed = true; }

extern "C" {

int dg_read_plan_create(dg_context_t* ctx, const dg_read_stream_t* streams, uint32_t n, uint32_t max_requests,
                        dg_read_plan_t** out) {
	if (!ctx || !out || (n && !streams)) return DG_ERR_INVALID_ARG;
	*out = nullptr;
	char msg[160];
	for (uint32_t i = 0; i < n; ++i) {
		const dg_read_stream_t& s = streams[i];
		if (s.ref_len >= (1ull << 32) || s.delta_len >= (1ull << 32)) {
			snprintf(msg, sizeof msg, "read plan: stream %u: a length of 4 GiB or more does not fit the u32 format", i);
			return ctx_fail(ctx, DG_ERR_TOO_LARGE, msg);
		}
		if (s.ref_off + s.ref_len < s.ref_off || s.delta_off + s.delta_len < s.delta_off) {
			snprintf(msg, sizeof msg, "read plan: stream %u: a region wraps the address space", i);
			return ctx_fail(ctx, DG_ERR_INVALID_ARG, msg);
		}
	}
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	// (A/B builds: DG_READ_HSACO names another code object beside the library, the
	// read kernel's other block shape, and DG_READ_BLOCK its threads per request;
	// always NULL in the product library)
	const char* file = ab_env("DG_READ_HSACO");
	const char* blk = file ? ab_env("DG_READ_BLOCK") : nullptr;
	const hipFunction_t* fn = nullptr;
	int rc = load_kernels(ctx, kCtxModRead, file ? file : "dg_read.hsaco", "read kernels", kRdKernels, 2, &fn);
	if (rc) return rc;
	auto* P = new (std::nothrow) dg_read_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->fn = fn;
	P->n = n;
	P->max_req = max_requests;
	if (blk) P->block = atoi(blk) == 64 ? 64u : 256u;
	P->indexed = n == 0;   // nothing to index
	std::vector<uint64_t> ioff((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) ioff[i + 1] = ioff[i] + index_bytes(streams[i].delta_len);
	if (P->d_streams.alloc_nonnull(sizeof(RdStream) * std::max<uint64_t>(n, 1)) || P->d_index.alloc_nonnull(ioff[n]) ||
	    P->d_index_off.alloc_nonnull(8ull * (n + 1))) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "read plan: device allocation failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_streams.p, streams, sizeof(RdStream) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(P->d_index_off.p, ioff.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "read plan: descriptor upload failed");
	}
	P->streams.assign(streams, streams + n);
	P->ioff = std::move(ioff);
	*out = P;
	return DG_OK;
}

int dg_read_plan_set_timing(dg_read_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kRdEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// "read": the read kernel; "total": the run, which is that one launch
int dg_read_plan_stage_times(dg_read_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kRdEvents] = {"read", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_read_plan_index(dg_read_plan_t* P, const uint8_t* d_delta, const uint64_t* d_delta_offsets,
                       const int32_t* d_delta_status, int32_t* d_stream_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (P->n == 0) return DG_OK;
	if (!d_delta) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	RdIndexArgs a{};
	a.delta = d_delta;
	a.streams = P->d_streams.as<RdStream>();
	a.delta_offsets = d_delta_offsets;
	a.delta_status = d_delta_status;
	a.stream_status = d_stream_status;
	a.index = P->d_index.as<uint8_t>();
	a.index_off = P->d_index_off.as<uint64_t>();
	a.n = P->n;
	void* params[] = {&a};
	hipError_t e;
	if ((e = hipModuleLaunchKernel(P->fn[0], P->n, 1, 1, kRdBlock, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_read_index_kernel", e);
	P->indexed = true;
	return DG_OK;
}

int dg_read_plan_run(dg_read_plan_t* P, const uint8_t* d_ref, const uint8_t* d_delta, const dg_read_req_t* d_reqs,
                     uint32_t n_req, uint8_t* d_out, uint32_t* d_out_len, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (!P->indexed) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: dg_read_plan_index has not run");
	const int rc = read_run_check(ctx, "read plan", n_req, P->max_req, P->n != 0, d_ref, d_delta, d_reqs, d_out, d_out_len, d_status);
	if (rc || n_req == 0) return rc;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	RdArgs a{};
	a.ref = d_ref;
	a.delta = d_delta;
	a.streams = P->d_streams.as<RdStream>();
	a.index = P->d_index.as<uint8_t>();
	a.index_off = P->d_index_off.as<uint64_t>();
	a.reqs = reinterpret_cast<const RdReq*>(d_reqs);
	a.out = d_out;
	a.out_len = d_out_len;
	a.status = d_status;
	a.n_streams = P->n;
	a.n_req = n_req;
	return launch_timed(ctx, P->ring.next(), P->fn[1], "dg_read_kernel", n_req, P->block, &a, st);
}

void dg_read_plan_destroy(dg_read_plan_t* P) { plan_destroy(P); }

int dg_read_batch(dg_context_t* ctx, const uint8_t* const* refs, const size_t* ref_len, const uint8_t* const* deltas,
                  const size_t* delta_len, uint32_t n_streams, const dg_read_req_t* reqs, uint32_t n_req,
                  dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n_streams && (!refs || !ref_len || !deltas || !delta_len)) || (n_req && (!reqs || !outs)))
		return DG_ERR_INVALID_ARG;
	for (uint32_t j = 0; j < n_req; ++j) outs[j] = dg_buffer_t{nullptr, 0};
	if (n_req == 0) return DG_OK;
	ReadBatchOps ops;
	ops.ref_len = [&](uint32_t i, bool* in_arena) {
		*in_arena = true;
		return (uint64_t)ref_len[i];
	};
	ops.run = dg_read_plan_run;
	return read_batch(ctx, refs, deltas, delta_len, n_streams, reqs, n_req, outs, status, ops);
}

}  // extern "C"

int dg::read_run_check(dg_context_t* ctx, const char* label, uint32_t n_req, uint32_t max_req, bool has_streams,
                       const void* d_ref, const void* d_delta, const void* d_reqs, const void* d_out,
                       const void* d_out_len, const void* d_status) {
	if (n_req > max_req)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, (std::string(label) + ": more requests than max_requests").c_str());
	if (n_req == 0) return DG_OK;
	if (!d_reqs || !d_out || !d_out_len || !d_status || (has_streams && (!d_ref || !d_delta)))
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if ((uintptr_t)d_out & 15) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the output arena must be 16-byte aligned");
	return DG_OK;
}

int dg::read_batch(dg_context_t* ctx, const uint8_t* const* refs, const uint8_t* const* deltas, const size_t* delta_len,
                   uint32_t n_streams, const dg_read_req_t* reqs, uint32_t n_req, dg_buffer_t* outs, int32_t* status,
                   const ReadBatchOps& ops) {
	std::vector<dg_read_stream_t> sv(n_streams);
	std::vector<uint64_t> packed(n_streams);   // bytes of refs[i] in the arena
	uint64_t rt = 0, dt = 0, ot = 0;
	for (uint32_t i = 0; i < n_streams; ++i) {
		bool in_arena = false;
		const uint64_t rl = ops.ref_len(i, &in_arena);
		packed[i] = in_arena ? rl : 0;
		if ((packed[i] && !refs[i]) || (delta_len[i] && !deltas[i])) return DG_ERR_INVALID_ARG;
		sv[i] = dg_read_stream_t{in_arena ? rt : 0, rl, dt, delta_len[i]};
		rt = (rt + packed[i] + 15) & ~15ull;
		dt += delta_len[i];
	}
	std::vector<dg_read_req_t> rv(reqs, reqs + n_req);
	for (uint32_t j = 0; j < n_req; ++j) {
		rv[j].out_off = ot;
		// a slot no larger than the stream's version (its header says; the kernel
		// stores min(len, version_size - off) bytes at the most)
		const uint32_t s = rv[j].stream;
		const uint64_t vs = s < n_streams ? header_vsize(deltas[s], delta_len[s]) : 0;
		ot = (ot + std::min<uint64_t>(rv[j].len, vs) + 15) & ~15ull;
	}
	dg_read_plan_t* plan = nullptr;
	int rc = dg_read_plan_create(ctx, sv.data(), n_streams, n_req, &plan);
	if (rc) return rc;
	ScopeExit guard([&] {
		if (ops.close) ops.close();
		dg_read_plan_destroy(plan);
	});
	if (ops.open && (rc = ops.open(plan)) != DG_OK) return rc;
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
		if (packed[i]) memcpy(h_ref.data() + sv[i].ref_off, refs[i], packed[i]);
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
	rc = dg_read_plan_index(plan, d_delta.as<uint8_t>(), nullptr, nullptr, nullptr, st);
	if (rc) return rc;
	rc = ops.run(plan, d_ref.as<uint8_t>(), d_delta.as<uint8_t>(), d_req.as<dg_read_req_t>(), n_req, d_out.as<uint8_t>(),
	             d_len.as<uint32_t>(), d_st.as<int32_t>(), st);
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
