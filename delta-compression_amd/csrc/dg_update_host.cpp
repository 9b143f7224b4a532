// dg_update_host.cpp — host side of the in-place update (dg_update_plan_*,
// dg_update_batch; include/delta_gpu.h).
//
// The kernel is the stand-alone code object dg_update.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  A run is that one
// launch.
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
#include "dg_plan.h"
#include "dg_update_dev.h"

using namespace dg;
using namespace dgup;

static_assert(sizeof(UpDesc) == sizeof(dg_update_desc_t), "UpDesc is dg_update_desc_t");

static const char* const kUpKernels[] = {"dg_update_kernel"};

constexpr int kUpEvents = 2;   // the kernel's start and end

struct dg_update_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kUpKernels
	uint32_t n = 0;
	int ignore_hash = 0;
	DevBuf d_desc;
	DevBuf d_scratch, d_scratch_off;   // phase A's command lists for phase B (dg_update_dev.h)
	DevBuf d_prof;   // A/B builds: the profiling code object's phase cycles
	TimingRing ring;   // kUpEvents events per run
};

extern "C" {

int dg_update_plan_create(dg_context_t* ctx, const dg_update_desc_t* descs, uint32_t n, int ignore_hash,
                          dg_update_plan_t** out) {
	if (!ctx || !out || (n && !descs)) return DG_ERR_INVALID_ARG;
	*out = nullptr;
	std::string err;
	int rc = update_check_descs(descs, n, err);
	if (rc) return ctx_fail(ctx, rc, err.c_str());
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	// (A/B builds: DG_UPDATE_HSACO names another code object beside the library,
	// the profiling one; always NULL in the product library)
	const char* file = ab_env("DG_UPDATE_HSACO");
	const hipFunction_t* fn = nullptr;
	rc = load_kernels(ctx, kCtxModUpdate, file ? file : "dg_update.hsaco", "update kernel", kUpKernels, 1, &fn);
	if (rc) return rc;
	auto* P = new (std::nothrow) dg_update_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->fn = fn;
	P->n = n;
	P->ignore_hash = ignore_hash;
	std::vector<uint64_t> soff((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) soff[i + 1] = soff[i] + scratch_bytes(descs[i].delta_len);
	if (P->d_desc.alloc_nonnull(sizeof(UpDesc) * std::max<uint64_t>(n, 1)) || P->d_scratch.alloc_nonnull(soff[n]) ||
	    P->d_scratch_off.alloc_nonnull(8ull * (n + 1))) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "update plan: device allocation failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, descs, sizeof(UpDesc) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(P->d_scratch_off.p, soff.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "update plan: descriptor upload failed");
	}
	*out = P;
	return DG_OK;
}

int dg_update_plan_set_timing(dg_update_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kUpEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// "update": the kernel (validation, apply and both CRC checks); "total": the
// run, which is that one launch
int dg_update_plan_stage_times(dg_update_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kUpEvents] = {"update", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_update_plan_run(dg_update_plan_t* P, uint8_t* d_buf, const uint8_t* d_delta, const uint64_t* d_delta_offsets,
                       const int32_t* d_delta_status, uint64_t* d_out_len, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (P->n == 0) return DG_OK;
	if (!d_buf || !d_delta || !d_out_len || !d_status) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if ((uintptr_t)d_buf & 15) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the buffer arena must be 16-byte aligned");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	hipEvent_t* ev = P->ring.next();
	UpArgs a{};
	a.buf = d_buf;
	a.delta = d_delta;
	a.descs = P->d_desc.as<UpDesc>();
	a.delta_offsets = d_delta_offsets;
	a.delta_status = d_delta_status;
	a.out_len = d_out_len;
	a.status = d_status;
	a.tables = ctx_crc_tables(ctx);
	a.n = P->n;
	a.crc_check = P->ignore_hash ? 0u : 1u;
	a.scratch = P->d_scratch.as<uint8_t>();
	a.scratch_off = P->d_scratch_off.as<uint64_t>();
	a.prof = P->d_prof.as<unsigned long long>();
	void* params[] = {&a};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[0], P->n, 1, 1, kUpBlock, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_update_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

#ifdef DG_AB_SWITCHES
// measurement builds only: zero (out == NULL) or read the phase cycle sums
int dg_update_plan_prof(dg_update_plan_t* P, unsigned long long* out, int n) {
	if (!P) return -1;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->d_prof.p && (P->d_prof.alloc(8 * kUpProfN) || hipMemset(P->d_prof.p, 0, 8 * kUpProfN) != hipSuccess)) return -1;
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	if (!out) return hipMemset(P->d_prof.p, 0, 8 * kUpProfN) == hipSuccess ? 0 : -1;
	if (n > kUpProfN) n = kUpProfN;
	return hipMemcpy(out, P->d_prof.p, 8 * n, hipMemcpyDeviceToHost) == hipSuccess ? n : -1;
}
#endif

void dg_update_plan_destroy(dg_update_plan_t* P) { plan_destroy(P); }

int dg_update_batch(dg_context_t* ctx, uint8_t* const* bufs, const size_t* ref_len, const size_t* buf_cap,
                    const uint8_t* const* delta, const size_t* delta_len, uint32_t n, int ignore_hash, size_t* out_len,
                    int32_t* status) {
	if (!ctx || (n && (!bufs || !ref_len || !buf_cap || !delta || !delta_len))) return DG_ERR_INVALID_ARG;
	if (n == 0) return DG_OK;
	// the buffers packed 16 bytes apart in one arena (R_i only is uploaded),
	// the deltas packed in another
	std::vector<dg_update_desc_t> descs(n);
	uint64_t bt = 0, dt = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if ((buf_cap[i] && !bufs[i]) || (delta_len[i] && !delta[i]) || ref_len[i] > buf_cap[i]) return DG_ERR_INVALID_ARG;
		descs[i] = dg_update_desc_t{bt, buf_cap[i], ref_len[i], dt, delta_len[i]};
		bt = (bt + buf_cap[i] + 15) & ~15ull;
		dt += delta_len[i];
	}
	dg_update_plan_t* plan = nullptr;
	int rc = dg_update_plan_create(ctx, descs.data(), n, ignore_hash, &plan);
	if (rc) return rc;
	ScopeExit guard([&] { dg_update_plan_destroy(plan); });
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_buf, d_delta, d_len, d_st;
	std::vector<uint8_t> h_delta;
	std::vector<uint64_t> lens(n);
	std::vector<int32_t> stv(n);
	try {
		h_delta.resize(dt);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t i = 0; i < n; ++i)
		if (delta_len[i]) memcpy(h_delta.data() + descs[i].delta_off, delta[i], delta_len[i]);
	if (d_buf.alloc_nonnull(bt) || d_delta.alloc_nonnull(dt) || d_len.alloc_nonnull(8ull * n) || d_st.alloc_nonnull(4ull * n)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	for (uint32_t i = 0; i < n; ++i)
		if (ref_len[i] && hipMemcpyAsync(d_buf.as<uint8_t>() + descs[i].buf_off, bufs[i], ref_len[i], hipMemcpyHostToDevice,
		                                 st) != hipSuccess)
			return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	if (dt && hipMemcpyAsync(d_delta.p, h_delta.data(), dt, hipMemcpyHostToDevice, st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	rc = dg_update_plan_run(plan, d_buf.as<uint8_t>(), d_delta.as<uint8_t>(), nullptr, nullptr, d_len.as<uint64_t>(),
	                        d_st.as<int32_t>(), st);
	if (rc) return rc;
	if (hipMemcpyAsync(lens.data(), d_len.p, 8ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(stv.data(), d_st.p, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	BatchStatus bs{status};
	for (uint32_t i = 0; i < n; ++i) {
		const int32_t s = stv[i];
		const bool written = s == DG_OK || s == DG_ERR_DST_CRC;
		if (written && lens[i] &&
		    hipMemcpyAsync(bufs[i], d_buf.as<uint8_t>() + descs[i].buf_off, lens[i], hipMemcpyDeviceToHost, st) != hipSuccess)
			return ctx_fail(ctx, DG_ERR_HIP, "download failed");
		if (out_len) out_len[i] = written ? (size_t)lens[i] : 0;
		bs.set(i, s);
	}
	if (hipStreamSynchronize(st) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	return bs.result();
}

}  // extern "C"
