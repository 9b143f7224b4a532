// dg_compose_host.cpp — host side of the device composition
// (dg_compose_plan_*, dg_compose_batch; include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_compose.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  A run is map kernel ->
// the library's size scan -> emit kernel on one stream.  The sizing of a plan
// is compose_plan_geometry (dg_plan.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_compose_dev.h"
#include "dg_device.h"
#include "dg_hostutil.h"
#include "dg_plan.h"

using namespace dg;
using namespace dgcp;

static const char* const kCpKernels[] = {"dg_compose_map_kernel", "dg_compose_emit_kernel"};
enum { kCpMap = 0, kCpEmit = 1, kCpKernelCount = 2 };

constexpr int kCpEvents = 4;   // before the map kernel, after it, after the scan, after the emit kernel

struct dg_compose_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kCpKernels
	uint32_t n = 0;
	int ignore_hash = 0;
	DevBuf d_desc, d_work, d_res, d_sizes;
	TimingRing ring;   // kCpEvents events per run
};

namespace {

// g, grc, gerr: what compose_plan_geometry{,_for} returned
int plan_make(dg_context_t* ctx, const ComposeGeometry& g, int grc, const std::string& gerr, int ignore_hash,
              dg_compose_plan_t** out) {
	*out = nullptr;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	const hipFunction_t* fn = nullptr;
	int rc = load_kernels(ctx, kCtxModCompose, "dg_compose.hsaco", "composition kernels", kCpKernels, kCpKernelCount, &fn);
	if (rc) return rc;
	if (grc) return ctx_fail(ctx, grc, gerr.c_str());
	auto* P = new (std::nothrow) dg_compose_plan_t();
	if (!P) return DG_ERR_NOMEM;
	const uint32_t n = (uint32_t)g.descs.size();
	P->ctx = ctx;
	P->fn = fn;
	P->n = n;
	P->ignore_hash = ignore_hash ? 1 : 0;
	const uint64_t nn = std::max<uint32_t>(n, 1);
	if (P->d_desc.alloc_nonnull(sizeof(CpDesc) * nn) || P->d_work.alloc_nonnull(g.work) ||
	    P->d_res.alloc_nonnull(sizeof(CpRes) * nn) || P->d_sizes.alloc_nonnull(8 * nn)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "compose plan: device allocation of the work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, g.descs.data(), sizeof(CpDesc) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "compose plan: descriptor upload failed");
	}
	*out = P;
	return DG_OK;
}

}  // namespace

extern "C" {

int dg_compose_plan_create(dg_context_t* ctx, const dg_compose_desc_t* descs, uint32_t n, int ignore_hash,
                           dg_compose_plan_t** out) {
	if (!ctx || !out || (n && !descs)) return DG_ERR_INVALID_ARG;
	ComposeGeometry g;
	std::string err;
	const int grc = compose_plan_geometry(descs, n, g, err);
	return plan_make(ctx, g, grc, err, ignore_hash, out);
}

int dg_compose_plan_create_for(dg_context_t* ctx, const dg_encode_plan_t* enc_a, const dg_encode_plan_t* enc_b,
                               int ignore_hash, dg_compose_plan_t** out) {
	if (!ctx || !enc_a || !enc_b || !out) return DG_ERR_INVALID_ARG;
	if (plan_ctx(enc_a) != ctx || plan_ctx(enc_b) != ctx)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "an encode plan belongs to another context");
	const uint32_t n = dg_encode_plan_num_pairs(enc_a);
	if (dg_encode_plan_num_pairs(enc_b) != n)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "compose plan: the encode plans differ in their pair counts");
	ComposeGeometry g;
	std::string err;
	const int grc = compose_plan_geometry_for(encode_plan_view(enc_a), encode_plan_view(enc_b), n, g, err);
	return plan_make(ctx, g, grc, err, ignore_hash, out);
}

int dg_compose_plan_set_timing(dg_compose_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kCpEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

int dg_compose_plan_stage_times(dg_compose_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kCpEvents] = {"map", "scan", "emit", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_compose_plan_run(dg_compose_plan_t* P, const uint8_t* d_a, const uint64_t* d_a_offsets, const int32_t* d_a_status,
                        const uint8_t* d_b, const uint64_t* d_b_offsets, const int32_t* d_b_status, uint8_t* d_out,
                        uint64_t out_cap, uint64_t* d_out_offsets, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (!d_out_offsets) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	if (P->n == 0) {
		return hipMemsetAsync(d_out_offsets, 0, 8, st) == hipSuccess ? DG_OK : ctx_fail(ctx, DG_ERR_HIP, "hipMemsetAsync failed");
	}
	// (d_out may be NULL with out_cap == 0: the sizing run)
	if (!d_a || !d_b || !d_status || (!d_out && out_cap)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipEvent_t* ev = P->ring.next();
	CpArgs a{};
	a.a = d_a;
	a.b = d_b;
	a.descs = P->d_desc.as<CpDesc>();
	a.a_offsets = d_a_offsets;
	a.b_offsets = d_b_offsets;
	a.a_status = d_a_status;
	a.b_status = d_b_status;
	a.work = P->d_work.as<uint8_t>();
	a.res = P->d_res.as<CpRes>();
	a.sizes = P->d_sizes.as<uint64_t>();
	a.status = d_status;
	a.out = d_out;
	a.out_cap = out_cap;
	a.out_offsets = d_out_offsets;
	a.n = P->n;
	a.ignore_hash = (uint32_t)P->ignore_hash;
	void* params[] = {&a};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kCpMap], P->n, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_compose_map_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = launch_scan(P->d_sizes.as<uint64_t>(), d_out_offsets, P->n, st)) != hipSuccess)
		return hip_fail(ctx, "launch of the size scan", e);
	if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kCpEmit], P->n, 1, 1, 256, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_compose_emit_kernel", e);
	if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

void dg_compose_plan_destroy(dg_compose_plan_t* P) { plan_destroy(P); }

int dg_compose_batch(dg_context_t* ctx, const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b,
                     const size_t* b_len, uint32_t n, int ignore_hash, dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n && (!a || !a_len || !b || !b_len || !outs))) return DG_ERR_INVALID_ARG;
	for (uint32_t i = 0; i < n; ++i) outs[i].data = nullptr, outs[i].len = 0;
	if (n == 0) return DG_OK;
	std::vector<dg_compose_desc_t> descs(n);
	uint64_t at = 0, bt = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if ((a_len[i] && !a[i]) || (b_len[i] && !b[i])) return DG_ERR_INVALID_ARG;
		descs[i] = dg_compose_desc_t{at, a_len[i], bt, b_len[i]};
		at += a_len[i];
		bt += b_len[i];
	}
	dg_compose_plan_t* plan = nullptr;
	int rc = dg_compose_plan_create(ctx, descs.data(), n, ignore_hash, &plan);
	if (rc) return rc;
	ScopeExit guard([&] { dg_compose_plan_destroy(plan); });
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_a, d_b, d_out, d_off, d_st;
	std::vector<uint8_t> h_in, h_out;
	std::vector<uint64_t> off((size_t)n + 1);
	std::vector<int32_t> stv(n);
	try {
		h_in.resize(at + bt);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t i = 0; i < n; ++i) {
		if (a_len[i]) memcpy(h_in.data() + descs[i].a_off, a[i], a_len[i]);
		if (b_len[i]) memcpy(h_in.data() + at + descs[i].b_off, b[i], b_len[i]);
	}
	if (d_a.alloc_nonnull(at) || d_b.alloc_nonnull(bt) || d_off.alloc_nonnull(8ull * (n + 1)) || d_st.alloc_nonnull(4ull * n)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((at && hipMemcpyAsync(d_a.p, h_in.data(), at, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (bt && hipMemcpyAsync(d_b.p, h_in.data() + at, bt, hipMemcpyHostToDevice, st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	// the sizing run: there is no a-priori bound of the output
	rc = dg_compose_plan_run(plan, d_a.as<uint8_t>(), nullptr, nullptr, d_b.as<uint8_t>(), nullptr, nullptr, nullptr, 0,
	                         d_off.as<uint64_t>(), d_st.as<int32_t>(), st);
	if (rc) return rc;
	if (hipMemcpyAsync(off.data(), d_off.p, 8ull * (n + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	const uint64_t total = off[n];
	if (d_out.alloc_nonnull(total)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	rc = dg_compose_plan_run(plan, d_a.as<uint8_t>(), nullptr, nullptr, d_b.as<uint8_t>(), nullptr, nullptr, d_out.as<uint8_t>(),
	                         total, d_off.as<uint64_t>(), d_st.as<int32_t>(), st);
	if (rc) return rc;
	try {
		h_out.resize(total);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	if (hipMemcpyAsync(off.data(), d_off.p, 8ull * (n + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(stv.data(), d_st.p, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    (total && hipMemcpyAsync(h_out.data(), d_out.p, total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	BatchStatus bs{status};
	for (uint32_t i = 0; i < n; ++i) {
		const int32_t s = stv[i];
		if (s == DG_OK && !buffer_copy(&outs[i], h_out.data() + off[i], off[i + 1] - off[i])) return DG_ERR_NOMEM;
		bs.set(i, s);
	}
	return bs.result();
}

}  // extern "C"
