// dg_sketch_host.cpp — host side of the device sketches and base matching
// (dg_sketch_plan_*, dg_sketch_match_device, dg_sketch_batch; include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_sketch.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  A plan run is a fill of
// the output with DG_SKETCH_EMPTY and the sketch kernel on one stream.  The
// work list of a plan is sketch_plan_geometry (dg_plan.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_hostutil.h"
#include "dg_plan.h"
#include "dg_sketch_dev.h"

using namespace dg;
using namespace dgsk;

static const char* const kSkKernels[] = {"dg_sketch_kernel", "dg_sketch_match_kernel"};
enum { kSkSketch = 0, kSkMatch = 1, kSkKernelCount = 2 };

constexpr int kSkEvents = 2;   // before the fill, after the kernel

struct dg_sketch_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kSkKernels
	uint32_t n = 0, n_items = 0;
	uint32_t p = 0, K = 0, shift = 0, chunk_bytes = 0;
	uint64_t top = 0;
	DevBuf d_spans, d_items, d_powc;
	TimingRing ring;   // kSkEvents events per run
};

namespace {

int load(dg_context_t* ctx, const hipFunction_t** fn) {
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	return load_kernels(ctx, kCtxModSketch, "dg_sketch.hsaco", "sketch kernels", kSkKernels, kSkKernelCount, fn);
}

}  // namespace

extern "C" {

int dg_sketch_plan_create(dg_context_t* ctx, const dg_span_t* spans, uint32_t n, uint32_t p, uint32_t K,
                          dg_sketch_plan_t** out) {
	if (!ctx || !out || (n && !spans)) return DG_ERR_INVALID_ARG;
	*out = nullptr;
	const hipFunction_t* fn = nullptr;
	int rc = load(ctx, &fn);
	if (rc) return rc;
	SketchGeometry g;
	std::string err;
	if ((rc = sketch_plan_geometry(spans, n, p, K, 0, g, err)) != DG_OK) return ctx_fail(ctx, rc, err.c_str());
	auto* P = new (std::nothrow) dg_sketch_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->fn = fn;
	P->n = n;
	P->n_items = (uint32_t)g.items.size();
	P->p = p;
	P->K = K;
	P->shift = g.shift;
	P->chunk_bytes = g.chunk_bytes;
	P->top = g.powc[0];
	static_assert(sizeof(SkSpan) == sizeof(dg_span_t), "the spans are uploaded as they are");
	if (P->d_spans.alloc_nonnull(sizeof(SkSpan) * n) || P->d_items.alloc_nonnull(sizeof(SkItem) * g.items.size()) ||
	    P->d_powc.alloc_nonnull(8ull * p)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "sketch plan: device allocation of the work list failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipMemcpyAsync(P->d_powc.p, g.powc.data(), 8ull * p, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && n) e = hipMemcpyAsync(P->d_spans.p, spans, sizeof(SkSpan) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && P->n_items)
		e = hipMemcpyAsync(P->d_items.p, g.items.data(), sizeof(SkItem) * g.items.size(), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "sketch plan: work list upload failed");
	}
	*out = P;
	return DG_OK;
}

uint32_t dg_sketch_plan_chunk_bytes(const dg_sketch_plan_t* P) { return P ? P->chunk_bytes : 0; }

int dg_sketch_plan_set_timing(dg_sketch_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kSkEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

int dg_sketch_plan_stage_times(dg_sketch_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kSkEvents] = {"sketch", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_sketch_plan_run(dg_sketch_plan_t* P, const uint8_t* d_arena, uint64_t* d_sketch, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (P->n == 0) return DG_OK;
	if (!d_sketch || (P->n_items && !d_arena)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if ((uintptr_t)d_arena & 15) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the arena is not 16-byte aligned");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	hipEvent_t* ev = P->ring.next();
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	// every bin empty: the kernel only lowers words
	if ((e = hipMemsetAsync(d_sketch, 0xFF, 8ull * P->n * P->K, st)) != hipSuccess) return hip_fail(ctx, "hipMemsetAsync", e);
	if (P->n_items) {
		SkArgs a{};
		a.arena = d_arena;
		a.spans = P->d_spans.as<SkSpan>();
		a.items = P->d_items.as<SkItem>();
		a.out = d_sketch;
		a.powc = P->d_powc.as<uint64_t>();
		a.top = P->top;
		a.p = P->p;
		a.K = P->K;
		a.shift = P->shift;
		a.chunk_bytes = P->chunk_bytes;
		void* params[] = {&a};
		if ((e = hipModuleLaunchKernel(P->fn[kSkSketch], P->n_items, 1, 1, kSkBlock, 1, 1,
		                               sketch_lds_bytes(P->K, P->chunk_bytes), st, params, nullptr)) != hipSuccess)
			return hip_fail(ctx, "launch of dg_sketch_kernel", e);
	}
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

void dg_sketch_plan_destroy(dg_sketch_plan_t* P) { plan_destroy(P); }

int dg_sketch_match_device(dg_context_t* ctx, const uint64_t* d_targets, uint32_t n_t, const uint64_t* d_cands, uint32_t n_c,
                           uint32_t K, int mode, uint32_t target_base, uint32_t min_equal, dg_match_t* d_out, void* stream) {
	if (!ctx) return DG_ERR_INVALID_ARG;
	if (K < kMinBins || K > kMaxBins || (K & (K - 1)) || min_equal == 0 ||
	    (mode != DG_MATCH_ALL && mode != DG_MATCH_NOT_SELF && mode != DG_MATCH_EARLIER))
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "sketch match: bad bin count, mode or min_equal");
	if (n_t == 0) return DG_OK;
	if (!d_targets || !d_out || (n_c && !d_cands)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	const hipFunction_t* fn = nullptr;
	int rc = load(ctx, &fn);
	if (rc) return rc;
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	MatchArgs a{};
	a.targets = d_targets;
	a.cands = d_cands;
	a.out = reinterpret_cast<uint32_t*>(d_out);
	a.n_t = n_t;
	a.n_c = n_c;
	a.K = K;
	a.mode = (uint32_t)mode;
	a.target_base = target_base;
	a.min_equal = min_equal;
	void* params[] = {&a};
	const uint32_t per_block = match_targets_per_wave(K) * (kMatchBlock / 64);
	const uint32_t blocks = (uint32_t)(((uint64_t)n_t + per_block - 1) / per_block);
	hipError_t e = hipModuleLaunchKernel(fn[kSkMatch], blocks, 1, 1, kMatchBlock, 1, 1, 0, st, params, nullptr);
	return e == hipSuccess ? DG_OK : hip_fail(ctx, "launch of dg_sketch_match_kernel", e);
}

int dg_sketch_batch(dg_context_t* ctx, const uint8_t* const* bufs, const size_t* lens, uint32_t n, uint32_t p, uint32_t K,
                    uint64_t* out) {
	if (!ctx || (n && (!bufs || !lens || !out))) return DG_ERR_INVALID_ARG;
	std::vector<dg_span_t> spans(n);
	uint64_t total = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if (lens[i] && !bufs[i]) return DG_ERR_INVALID_ARG;
		spans[i] = dg_span_t{total, lens[i]};
		total += lens[i];
	}
	dg_sketch_plan_t* plan = nullptr;
	int rc = dg_sketch_plan_create(ctx, spans.data(), n, p, K, &plan);
	if (rc) return rc;
	ScopeExit guard([&] { dg_sketch_plan_destroy(plan); });
	if (n == 0) return DG_OK;
	std::vector<uint8_t> h_in;
	try {
		h_in.resize(total);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t i = 0; i < n; ++i)
		if (lens[i]) memcpy(h_in.data() + spans[i].off, bufs[i], lens[i]);
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_in, d_out;
	const uint64_t out_bytes = 8ull * n * K;
	if (d_in.alloc_nonnull(total) || d_out.alloc_nonnull(out_bytes)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if (total && hipMemcpyAsync(d_in.p, h_in.data(), total, hipMemcpyHostToDevice, st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	if ((rc = dg_sketch_plan_run(plan, d_in.as<uint8_t>(), d_out.as<uint64_t>(), st)) != DG_OK) return rc;
	if (hipMemcpyAsync(out, d_out.p, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	return DG_OK;
}

}  // extern "C"
