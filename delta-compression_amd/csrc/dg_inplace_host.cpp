// dg_inplace_host.cpp — host side of the device in-place conversion
// (dg_inplace_plan_*, dg_make_inplace_batch; include/delta_gpu.h).
//
// The kernels are not part of libdeltagpu.so's fat binary: they are the
// stand-alone code object dg_inplace.hsaco beside the library, loaded once per
// context on first use (hipModuleLoad) and launched with
// hipModuleLaunchKernel.  A run is order kernel -> the library's size scan ->
// emit kernel on one stream.
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
#include "dg_inplace_dev.h"

using namespace dg;
using namespace dgip;

namespace {

struct IpModule {
	hipModule_t mod = nullptr;
	hipFunction_t order = nullptr, emit = nullptr;
};

void module_release(void* p) {
	auto* m = static_cast<IpModule*>(p);
	if (m->mod) hipModuleUnload(m->mod);
	delete m;
}

// dg_inplace.hsaco in the directory this library was loaded from
std::string module_path() {
	Dl_info info{};
	if (!dladdr(reinterpret_cast<const void*>(&module_release), &info) || !info.dli_fname) return "dg_inplace.hsaco";
	std::string p = info.dli_fname;
	const size_t slash = p.rfind('/');
	p = slash == std::string::npos ? std::string() : p.substr(0, slash + 1);
	return p + "dg_inplace.hsaco";
}

int module_get(dg_context_t* ctx, IpModule** out) {
	void** slot = ctx_inplace(ctx, module_release);
	if (!*slot) {
		auto* m = new (std::nothrow) IpModule();
		if (!m) return DG_ERR_NOMEM;
		const std::string path = module_path();
		hipError_t e = hipModuleLoad(&m->mod, path.c_str());
		if (e == hipSuccess) e = hipModuleGetFunction(&m->order, m->mod, "dg_inplace_order_kernel");
		if (e == hipSuccess) e = hipModuleGetFunction(&m->emit, m->mod, "dg_inplace_emit_kernel");
		if (e != hipSuccess) {
			(void)hipGetLastError();
			const std::string msg = "in-place kernels: cannot load " + path + ": " + hipGetErrorString(e);
			module_release(m);
			return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
		}
		*slot = m;
	}
	*out = static_cast<IpModule*>(*slot);
	return DG_OK;
}

struct Buf {
	void* p = nullptr;
	~Buf() { if (p) hipFree(p); }
	bool alloc(uint64_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
	template <class T> T* as() const { return static_cast<T*>(p); }
};

constexpr int kIpEvents = 4;   // before the order kernel, after it, after the scan, after the emit kernel

}  // namespace

struct dg_inplace_plan {
	dg_context_t* ctx = nullptr;
	IpModule* mod = nullptr;
	uint32_t n = 0;
	int policy = DG_POLICY_LOCALMIN;
	uint64_t bound = 0;
	Buf d_desc, d_work, d_res, d_sizes;
	// stage timing: a ring of `slots` event sets
	std::vector<hipEvent_t> ev;
	uint32_t slots = 0, runs = 0;
	~dg_inplace_plan() {
		for (hipEvent_t e : ev)
			if (e) hipEventDestroy(e);
	}
};

namespace {

// descs with work_off, max_copies and max_adds filled; extra[i]: the version
// bytes delta i's COPYs can turn into ADD payload
int plan_make(dg_context_t* ctx, std::vector<IpDesc>& descs, const std::vector<uint64_t>& extra, int policy,
              dg_inplace_plan_t** out) {
	*out = nullptr;
	if (policy != DG_POLICY_LOCALMIN && policy != DG_POLICY_CONSTANT)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "unknown in-place policy");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	IpModule* mod = nullptr;
	int rc = module_get(ctx, &mod);
	if (rc) return rc;
	const uint32_t n = (uint32_t)descs.size();
	uint64_t work = 0, bound = 0;
	for (uint32_t i = 0; i < n; ++i) {
		IpDesc& d = descs[i];
		if (d.ref_len >= (1ull << 32) || d.delta_cap >= (1ull << 32))
			return ctx_fail(ctx, DG_ERR_TOO_LARGE, "in-place plan: a stream of 4 GiB or more does not fit the u32 format");
		d.work_off = work;
		work += work_bytes(d.max_copies, d.max_adds);
		bound += d.delta_cap + extra[i];
	}
	auto* P = new (std::nothrow) dg_inplace_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->mod = mod;
	P->n = n;
	P->policy = policy;
	P->bound = bound;
	const uint64_t nn = std::max<uint32_t>(n, 1);
	if (!P->d_desc.alloc(sizeof(IpDesc) * nn) || !P->d_work.alloc(work) || !P->d_res.alloc(sizeof(IpRes) * nn) ||
	    !P->d_sizes.alloc(8 * nn)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "in-place plan: device allocation of the work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, descs.data(), sizeof(IpDesc) * n, hipMemcpyHostToDevice, st);
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
	std::vector<IpDesc> d(n);
	std::vector<uint64_t> extra(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t cap = descs[i].delta_cap;
		// (the END byte may be missing: encoding.c:111-178 stops at the stream's end too)
		const uint64_t body = cap > 25 ? cap - 25 : 0;
		d[i] = IpDesc{descs[i].ref_off, descs[i].ref_len, descs[i].delta_off, cap, 0, (uint32_t)std::min<uint64_t>(body / 13, 0xFFFFFFFFull),
		              (uint32_t)std::min<uint64_t>(body / 9, 0xFFFFFFFFull)};
		extra[i] = std::min<uint64_t>((body / 13) * descs[i].ref_len, 1ull << 32);
	}
	return plan_make(ctx, d, extra, policy, out);
}

int dg_inplace_plan_create_for(dg_context_t* ctx, const dg_encode_plan_t* enc, int policy, dg_inplace_plan_t** out) {
	if (!ctx || !enc || !out) return DG_ERR_INVALID_ARG;
	if (plan_ctx(enc) != ctx) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the encode plan belongs to another context");
	const uint32_t n = dg_encode_plan_num_pairs(enc);
	const dg_pair_t* pairs = plan_pairs(enc);
	const PairPlanDev* pp = plan_pp(enc);
	dg_algorithm_t algo;
	dg_diff_options_t o;
	plan_options(enc, &algo, &o);
	const uint64_t p = o.p;
	std::vector<IpDesc> d(n);
	std::vector<uint64_t> extra(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t vl = pairs[i].v_len;
		// the encode plan's per-pair output bound (dg_plan.cpp)
		const uint64_t cap = algo == DG_ALGO_CORRECTING ? 57 + vl + 22 * (vl / p) : 35 + vl + (vl / p) * (p < 22 ? 22 - p : 0);
		// the encoders alternate COPY and ADD: at most one ADD before each COPY and one at the end
		d[i] = IpDesc{pairs[i].r_off, pairs[i].r_len, 0, cap, 0, pp[i].rec_cap, pp[i].rec_cap + 1};
		extra[i] = vl;
	}
	return plan_make(ctx, d, extra, policy, out);
}

uint64_t dg_inplace_plan_output_bound(const dg_inplace_plan_t* P) { return P ? P->bound : 0; }

int dg_inplace_plan_set_timing(dg_inplace_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if ((size_t)slots * kIpEvents > P->ev.size()) {
		const size_t have = P->ev.size();
		P->ev.resize((size_t)slots * kIpEvents, nullptr);
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

int dg_inplace_plan_stage_times(dg_inplace_plan_t* P, float* ms, const char** names, int n) {
	static const char* kNames[] = {"order", "scan", "emit", "total"};
	const uint32_t used = P && P->slots ? std::min(P->runs, P->slots) : 0;
	if (!used || n < 1) return 0;
	double acc[4] = {0, 0, 0, 0};
	for (uint32_t s = 0; s < used; ++s) {
		hipEvent_t* e = &P->ev[(size_t)kIpEvents * s];
		if (hipEventSynchronize(e[3]) != hipSuccess) return 0;
		float t = 0;
		for (int k = 0; k < 3; ++k) {
			hipEventElapsedTime(&t, e[k], e[k + 1]);
			acc[k] += t;
		}
		hipEventElapsedTime(&t, e[0], e[3]);
		acc[3] += t;
	}
	const int m = std::min(n, 4);
	for (int k = 0; k < m; ++k) {
		if (ms) ms[k] = (float)(acc[k] / used);
		if (names) names[k] = kNames[k];
	}
	return m;
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
	hipEvent_t* ev = P->slots ? &P->ev[(size_t)kIpEvents * (P->runs++ % P->slots)] : nullptr;
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
	auto fail = [&](const char* what, hipError_t e) {
		const std::string msg = std::string(what) + " failed: " + hipGetErrorString(e);
		return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
	};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->mod->order, P->n, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return fail("launch of dg_inplace_order_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = launch_scan(P->d_sizes.as<uint64_t>(), d_out_offsets, P->n, st)) != hipSuccess)
		return fail("launch of the size scan", e);
	if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->mod->emit, P->n, 1, 1, 256, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return fail("launch of dg_inplace_emit_kernel", e);
	if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return fail("hipEventRecord", e);
	return DG_OK;
}

void dg_inplace_plan_destroy(dg_inplace_plan_t* P) {
	if (!P) return;
	hipSetDevice(ctx_device(P->ctx));
	hipStreamSynchronize((hipStream_t)dg_context_stream(P->ctx));
	delete P;
}

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
		// an in-place delta is at most the stream plus its version bytes
		// (header bytes 5..8) as ADD payload
		uint64_t vs = 0;
		if (delta_len[i] >= DG_HEADER_SIZE)
			vs = ((uint64_t)delta[i][5] << 24) | ((uint64_t)delta[i][6] << 16) | ((uint64_t)delta[i][7] << 8) | delta[i][8];
		out_cap += delta_len[i] + vs;
	}
	dg_inplace_plan_t* plan = nullptr;
	int rc = dg_inplace_plan_create(ctx, descs.data(), n, policy, &plan);
	if (rc) return rc;
	struct Guard {
		dg_inplace_plan_t* p;
		~Guard() { dg_inplace_plan_destroy(p); }
	} guard{plan};
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	Buf d_ref, d_delta, d_out, d_off, d_st;
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
	if (!d_ref.alloc(rt) || !d_delta.alloc(dt) || !d_out.alloc(out_cap) || !d_off.alloc(8ull * (n + 1)) || !d_st.alloc(4ull * n)) {
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
	int first_bad = DG_OK;
	for (uint32_t i = 0; i < n; ++i) {
		int32_t s = stv[i];
		// not placed sequentially (the host sorts), past 32-bit offsets, or a
		// header whose version size understates the commands': the host converts
		if (s == DG_ERR_UNSUPPORTED || s == DG_ERR_CAPACITY) {
			s = dg_make_inplace(r[i], r_len[i], delta[i], delta_len[i], policy, &outs[i], nullptr);
		} else if (s == DG_OK) {
			const uint64_t len = off[i + 1] - off[i];
			outs[i].data = (uint8_t*)malloc(len ? len : 1);
			if (!outs[i].data) return DG_ERR_NOMEM;
			memcpy(outs[i].data, h_out.data() + off[i], len);
			outs[i].len = len;
		}
		if (status) status[i] = s;
		if (s && !first_bad) first_bad = s;
	}
	return status ? DG_OK : first_bad;
}

}  // extern "C"
