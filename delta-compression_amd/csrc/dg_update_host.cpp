// dg_update_host.cpp — host side of the in-place update (dg_update_plan_*,
// dg_update_batch; include/delta_gpu.h).
//
// The kernel is not part of libdeltagpu.so's fat binary: it is the stand-alone
// code object dg_update.hsaco beside the library, loaded once per context on
// first use (hipModuleLoad) and launched with hipModuleLaunchKernel.  A run is
// that one launch.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_plan.h"
#include "dg_update_dev.h"

using namespace dg;
using namespace dgup;

static_assert(sizeof(UpDesc) == sizeof(dg_update_desc_t), "UpDesc is dg_update_desc_t");

namespace {

struct UpModule {
	hipModule_t mod = nullptr;
	hipFunction_t update = nullptr;
};

void module_release(void* p) {
	auto* m = static_cast<UpModule*>(p);
	if (m->mod) hipModuleUnload(m->mod);
	delete m;
}

// dg_update.hsaco in the directory this library was loaded from
std::string module_path() {
	Dl_info info{};
	if (!dladdr(reinterpret_cast<const void*>(&module_release), &info) || !info.dli_fname) return "dg_update.hsaco";
	std::string p = info.dli_fname;
	const size_t slash = p.rfind('/');
	p = slash == std::string::npos ? std::string() : p.substr(0, slash + 1);
	// (A/B builds: DG_UPDATE_HSACO names another code object in that directory,
	// the profiling one; always NULL in the product library)
	const char* name = ab_env("DG_UPDATE_HSACO");
	return p + (name ? name : "dg_update.hsaco");
}

int module_get(dg_context_t* ctx, UpModule** out) {
	void** slot = ctx_module(ctx, kCtxModUpdate, module_release);
	if (!*slot) {
		auto* m = new (std::nothrow) UpModule();
		if (!m) return DG_ERR_NOMEM;
		const std::string path = module_path();
		hipError_t e = hipModuleLoad(&m->mod, path.c_str());
		if (e == hipSuccess) e = hipModuleGetFunction(&m->update, m->mod, "dg_update_kernel");
		if (e != hipSuccess) {
			(void)hipGetLastError();
			const std::string msg = "update kernel: cannot load " + path + ": " + hipGetErrorString(e);
			module_release(m);
			return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
		}
		*slot = m;
	}
	*out = static_cast<UpModule*>(*slot);
	return DG_OK;
}

struct Buf {
	void* p = nullptr;
	~Buf() { if (p) hipFree(p); }
	bool alloc(uint64_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
	template <class T> T* as() const { return static_cast<T*>(p); }
};

constexpr int kUpEvents = 2;   // the kernel's start and end

}  // namespace

struct dg_update_plan {
	dg_context_t* ctx = nullptr;
	UpModule* mod = nullptr;
	uint32_t n = 0;
	int ignore_hash = 0;
	Buf d_desc;
	Buf d_scratch, d_scratch_off;   // phase A's command lists for phase B (dg_update_dev.h)
	Buf d_prof;   // A/B builds: the profiling code object's phase cycles
	// stage timing: a ring of `slots` event sets
	std::vector<hipEvent_t> ev;
	uint32_t slots = 0, runs = 0;
	~dg_update_plan() {
		for (hipEvent_t e : ev)
			if (e) hipEventDestroy(e);
	}
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
	UpModule* mod = nullptr;
	rc = module_get(ctx, &mod);
	if (rc) return rc;
	auto* P = new (std::nothrow) dg_update_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->mod = mod;
	P->n = n;
	P->ignore_hash = ignore_hash;
	std::vector<uint64_t> soff((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) soff[i + 1] = soff[i] + scratch_bytes(descs[i].delta_len);
	if (!P->d_desc.alloc(sizeof(UpDesc) * std::max<uint64_t>(n, 1)) || !P->d_scratch.alloc(soff[n]) ||
	    !P->d_scratch_off.alloc(8ull * (n + 1))) {
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
	if ((size_t)slots * kUpEvents > P->ev.size()) {
		const size_t have = P->ev.size();
		P->ev.resize((size_t)slots * kUpEvents, nullptr);
		for (size_t k = have; k < P->ev.size(); ++k)
			if (hipEventCreateWithFlags(&P->ev[k], hipEventDisableSystemFence) != hipSuccess) {
				P->ev[k] = nullptr;
				P->slots = 0;
				return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
			}
	}
	P->slots = (uint32_t)slots;
	P->runs = 0;
	return DG_OK;
}

// "update": the kernel (validation, apply and both CRC checks); "total": the
// run, which is that one launch
int dg_update_plan_stage_times(dg_update_plan_t* P, float* ms, const char** names, int n) {
	static const char* kNames[] = {"update", "total"};
	const uint32_t used = P && P->slots ? std::min(P->runs, P->slots) : 0;
	if (!used || n < 1) return 0;
	double acc = 0;
	for (uint32_t s = 0; s < used; ++s) {
		hipEvent_t* e = &P->ev[(size_t)kUpEvents * s];
		if (hipEventSynchronize(e[1]) != hipSuccess) return 0;
		float t = 0;
		hipEventElapsedTime(&t, e[0], e[1]);
		acc += t;
	}
	const int m = std::min(n, 2);
	for (int k = 0; k < m; ++k) {
		if (ms) ms[k] = (float)(acc / used);
		if (names) names[k] = kNames[k];
	}
	return m;
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
	hipEvent_t* ev = P->slots ? &P->ev[(size_t)kUpEvents * (P->runs++ % P->slots)] : nullptr;
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
	auto fail = [&](const char* what, hipError_t e) {
		const std::string msg = std::string(what) + " failed: " + hipGetErrorString(e);
		return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
	};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->mod->update, P->n, 1, 1, kUpBlock, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return fail("launch of dg_update_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return fail("hipEventRecord", e);
	return DG_OK;
}

#ifdef DG_AB_SWITCHES
// measurement builds only: zero (out == NULL) or read the phase cycle sums
int dg_update_plan_prof(dg_update_plan_t* P, unsigned long long* out, int n) {
	if (!P) return -1;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->d_prof.p && (!P->d_prof.alloc(8 * kUpProfN) || hipMemset(P->d_prof.p, 0, 8 * kUpProfN) != hipSuccess)) return -1;
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	if (!out) return hipMemset(P->d_prof.p, 0, 8 * kUpProfN) == hipSuccess ? 0 : -1;
	if (n > kUpProfN) n = kUpProfN;
	return hipMemcpy(out, P->d_prof.p, 8 * n, hipMemcpyDeviceToHost) == hipSuccess ? n : -1;
}
#endif

void dg_update_plan_destroy(dg_update_plan_t* P) {
	if (!P) return;
	hipSetDevice(ctx_device(P->ctx));
	hipStreamSynchronize((hipStream_t)dg_context_stream(P->ctx));
	delete P;
}

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
	struct Guard {
		dg_update_plan_t* p;
		~Guard() { dg_update_plan_destroy(p); }
	} guard{plan};
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	Buf d_buf, d_delta, d_len, d_st;
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
	if (!d_buf.alloc(bt) || !d_delta.alloc(dt) || !d_len.alloc(8ull * n) || !d_st.alloc(4ull * n)) {
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
	int first_bad = DG_OK;
	for (uint32_t i = 0; i < n; ++i) {
		const int32_t s = stv[i];
		const bool written = s == DG_OK || s == DG_ERR_DST_CRC;
		if (written && lens[i] &&
		    hipMemcpyAsync(bufs[i], d_buf.as<uint8_t>() + descs[i].buf_off, lens[i], hipMemcpyDeviceToHost, st) != hipSuccess)
			return ctx_fail(ctx, DG_ERR_HIP, "download failed");
		if (out_len) out_len[i] = written ? (size_t)lens[i] : 0;
		if (status) status[i] = s;
		if (s && !first_bad) first_bad = s;
	}
	if (hipStreamSynchronize(st) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	return status ? DG_OK : first_bad;
}

}  // extern "C"
