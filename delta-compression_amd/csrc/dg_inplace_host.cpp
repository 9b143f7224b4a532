// dg_inplace_host.cpp — host side of the device in-place conversion
// (dg_inplace_plan_*, dg_make_inplace_batch; include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_inplace.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  A run is order kernel
// -> the library's size scan -> emit kernel on one stream.  The sizing of a
// plan is inplace_plan_geometry (dg_plan.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_hostutil.h"
#include "dg_inplace_dev.h"
#include "dg_plan.h"

using namespace dg;
using namespace dgip;

static const char* const kIpKernels[] = {"dg_inplace_order_kernel", "dg_inplace_emit_kernel"};
enum { kIpOrder = 0, kIpEmit = 1, kIpKernelCount = 2 };

constexpr int kIpEvents = 4;   // before the order kernel, after it, after the scan, after the emit kernel

struct dg_inplace_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kIpKernels
	uint32_t n = 0;
	int policy = DG_POLICY_LOCALMIN;
	uint64_t bound = 0;
	DevBuf d_desc, d_work, d_res, d_sizes;
	TimingRing ring;   // kIpEvents events per run
};

namespace {

// g, grc, gerr: what inplace_plan_geometry{,_for} returned
int plan_make(dg_context_t* ctx, const InplaceGeometry& g, int grc, const std::string& gerr, int policy,
              dg_inplace_plan_t** out) {
	*out = nullptr;
	if (policy != DG_POLICY_LOCALMIN && policy != DG_POLICY_CONSTANT)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "unknown in-place policy");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	const hipFunction_t* fn = nullptr;
	int rc = load_kernels(ctx, kCtxModInplace, "dg_inplace.hsaco", "in-place kernels", kIpKernels, kIpKernelCount, &fn);
	if (rc) return rc;
	if (grc) return ctx_fail(ctx, grc, gerr.c_str());
	auto* P = new (std::nothrow) dg_inplace_plan_t();
	if (!P) return DG_ERR_NOMEM;
	const uint32_t n = (uint32_t)g.descs.size();
	P->ctx = ctx;
	P->fn = fn;
	P->n = n;
	P->policy = policy;
	P->bound = g.bound;
	const uint64_t nn = std::max<uint32_t>(n, 1);
	if (P->d_desc.alloc_nonnull(sizeof(IpDesc) * nn) || P->d_work.alloc_nonnull(g.work) ||
	    P->d_res.alloc_nonnull(sizeof(IpRes) * nn) || P->d_sizes.alloc_nonnull(8 * nn)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "in-place plan: device allocation of the work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, g.descs.data(), sizeof(IpDesc) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "in-place plan: descriptor upload failed");
	}
	*out = P;
	return DG_OK;
}

}  // namespace

extern "C" {

int dg_inplace_plan_create(dg_context_t* ctx, const dg_inplace_desc_t* descs, uint32_t n, int policy,
                           dg_inplace_plan_t** out) {
	if (!ctx || !out || (n && !descs)) return DG_ERR_INVALID_ARG;
	InplaceGeometry g;
	std::string err;
	const int grc = inplace_plan_geometry(descs, n, g, err);
	return plan_make(ctx, g, grc, err, policy, out);
}

int dg_inplace_plan_create_for(dg_context_t* ctx, const dg_encode_plan_t* enc, int policy, dg_inplace_plan_t** out) {
	if (!ctx || !enc || !out) return DG_ERR_INVALID_ARG;
	if (plan_ctx(enc) != ctx) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the encode plan belongs to another context");
	InplaceGeometry g;
	std::string err;
	const int grc = inplace_plan_geometry_for(encode_plan_view(enc), dg_encode_plan_num_pairs(enc), g, err);
	return plan_make(ctx, g, grc, err, policy, out);
}

uint64_t dg_inplace_plan_output_bound(const dg_inplace_plan_t* P) { return P ? P->bound : 0; }

int dg_inplace_plan_set_timing(dg_inplace_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kIpEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

int dg_inplace_plan_stage_times(dg_inplace_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kIpEvents] = {"order", "scan", "emit", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_inplace_plan_run(dg_inplace_plan_t* P, const uint8_t* d_ref, const uint8_t* d_delta,
                        const uint64_t* d_delta_offsets, const int32_t* d_delta_status, uint8_t* d_out,
                        uint64_t out_cap, uint64_t* d_out_offsets, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (!d_out_offsets) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	if (P->n == 0) {
		return hipMemsetAsync(d_out_offsets, 0, 8, st) == hipSuccess ? DG_OK : ctx_fail(ctx, DG_ERR_HIP, "hipMemsetAsync failed");
	}
	if (!d_ref || !d_delta || !d_out || !d_status) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipEvent_t* ev = P->ring.next();
	IpArgs a{};
	a.ref = d_ref;
	a.delta = d_delta;
	a.descs = P->d_desc.as<IpDesc>();
	a.delta_offsets = d_delta_offsets;
	a.delta_status = d_delta_status;
	a.work = P->d_work.as<uint8_t>();
	a.res = P->d_res.as<IpRes>();
	a.sizes = P->d_sizes.as<uint64_t>();
	a.status = d_status;
	a.out = d_out;
	a.out_cap = out_cap;
	a.out_offsets = d_out_offsets;
	a.n = P->n;
	a.policy = (uint32_t)P->policy;
	void* params[] = {&a};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kIpOrder], P->n, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_inplace_order_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = launch_scan(P->d_sizes.as<uint64_t>(), d_out_offsets, P->n, st)) != hipSuccess)
		return hip_fail(ctx, "launch of the size scan", e);
	if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kIpEmit], P->n, 1, 1, 256, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_inplace_emit_kernel", e);
	if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

void dg_inplace_plan_destroy(dg_inplace_plan_t* P) { plan_destroy(P); }

int dg_make_inplace_batch(dg_context_t* ctx, const uint8_t* const* r, const size_t* r_len, const uint8_t* const* delta,
                          const size_t* delta_len, uint32_t n, int policy, dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n && (!r || !r_len || !delta || !delta_len || !outs))) return DG_ERR_INVALID_ARG;
	for (uint32_t i = 0; i < n; ++i) outs[i].data = nullptr, outs[i].len = 0;
	if (n == 0) return DG_OK;
	std::vector<dg_inplace_desc_t> descs(n);
	uint64_t rt = 0, dt = 0, out_cap = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if ((r_len[i] && !r[i]) || (delta_len[i] && !delta[i])) return DG_ERR_INVALID_ARG;
		descs[i] = dg_inplace_desc_t{rt, r_len[i], dt, delta_len[i]};
		rt += r_len[i];
		dt += delta_len[i];
		// an in-place delta is at most the stream plus its version bytes as ADD payload
		out_cap += delta_len[i] + header_vsize(delta[i], delta_len[i]);
	}
	dg_inplace_plan_t* plan = nullptr;
	int rc = dg_inplace_plan_create(ctx, descs.data(), n, policy, &plan);
	if (rc) return rc;
	ScopeExit guard([&] { dg_inplace_plan_destroy(plan); });
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_ref, d_delta, d_out, d_off, d_st;
	std::vector<uint8_t> h_in, h_out;
	std::vector<uint64_t> off((size_t)n + 1);
	std::vector<int32_t> stv(n);
	try {
		h_in.resize(rt + dt);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t i = 0; i < n; ++i) {
		if (r_len[i]) memcpy(h_in.data() + descs[i].ref_off, r[i], r_len[i]);
		if (delta_len[i]) memcpy(h_in.data() + rt + descs[i].delta_off, delta[i], delta_len[i]);
	}
	if (d_ref.alloc_nonnull(rt) || d_delta.alloc_nonnull(dt) || d_out.alloc_nonnull(out_cap) ||
	    d_off.alloc_nonnull(8ull * (n + 1)) || d_st.alloc_nonnull(4ull * n)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((rt && hipMemcpyAsync(d_ref.p, h_in.data(), rt, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (dt && hipMemcpyAsync(d_delta.p, h_in.data() + rt, dt, hipMemcpyHostToDevice, st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	rc = dg_inplace_plan_run(plan, d_ref.as<uint8_t>(), d_delta.as<uint8_t>(), nullptr, nullptr, d_out.as<uint8_t>(), out_cap,
	                         d_off.as<uint64_t>(), d_st.as<int32_t>(), st);
	if (rc) return rc;
	if (hipMemcpyAsync(off.data(), d_off.p, 8ull * (n + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(stv.data(), d_st.p, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	const uint64_t total = std::min<uint64_t>(off[n], out_cap);
	try {
		h_out.resize(total);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	if (total && (hipMemcpyAsync(h_out.data(), d_out.p, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
	              hipStreamSynchronize(st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	BatchStatus bs{status};
	for (uint32_t i = 0; i < n; ++i) {
		int32_t s = stv[i];
		// not placed sequentially (the host sorts), past 32-bit offsets, or a
		// header whose version size understates the commands': the host converts
		if (s == DG_ERR_UNSUPPORTED || s == DG_ERR_CAPACITY)
			s = dg_make_inplace(r[i], r_len[i], delta[i], delta_len[i], policy, &outs[i], nullptr);
		else if (s == DG_OK && !buffer_copy(&outs[i], h_out.data() + off[i], off[i + 1] - off[i]))
			return DG_ERR_NOMEM;
		bs.set(i, s);
	}
	return bs.result();
}

}  // extern "C"
