// dg_compose_host.cpp — host side of the device composition
// (dg_compose_plan_*, dg_compose_batch; include/delta_gpu.h).
//
// The kernels are not part of libdeltagpu.so's fat binary: they are the
// stand-alone code object dg_compose.hsaco beside the library, loaded once per
// context on first use (hipModuleLoad) and launched with
// hipModuleLaunchKernel.  A run is map kernel -> the library's size scan ->
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
#include "dg_compose_dev.h"
#include "dg_device.h"

using namespace dg;
using namespace dgcp;

namespace {

struct CpModule {
	hipModule_t mod = nullptr;
	hipFunction_t map = nullptr, emit = nullptr;
};

void module_release(void* p) {
	auto* m = static_cast<CpModule*>(p);
	if (m->mod) hipModuleUnload(m->mod);
	delete m;
}

// dg_compose.hsaco in the directory this library was loaded from
std::string module_path() {
	Dl_info info{};
	if (!dladdr(reinterpret_cast<const void*>(&module_release), &info) || !info.dli_fname) return "dg_compose.hsaco";
	std::string p = info.dli_fname;
	const size_t slash = p.rfind('/');
	p = slash == std::string::npos ? std::string() : p.substr(0, slash + 1);
	return p + "dg_compose.hsaco";
}

int module_get(dg_context_t* ctx, CpModule** out) {
	void** slot = ctx_module(ctx, kCtxModCompose, module_release);
	if (!*slot) {
		auto* m = new (std::nothrow) CpModule();
		if (!m) return DG_ERR_NOMEM;
		const std::string path = module_path();
		hipError_t e = hipModuleLoad(&m->mod, path.c_str());
		if (e == hipSuccess) e = hipModuleGetFunction(&m->map, m->mod, "dg_compose_map_kernel");
		if (e == hipSuccess) e = hipModuleGetFunction(&m->emit, m->mod, "dg_compose_emit_kernel");
		if (e != hipSuccess) {
			(void)hipGetLastError();
			const std::string msg = "composition kernels: cannot load " + path + ": " + hipGetErrorString(e);
			module_release(m);
			return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
		}
		*slot = m;
	}
	*out = static_cast<CpModule*>(*slot);
	return DG_OK;
}

struct Buf {
	void* p = nullptr;
	~Buf() { if (p) hipFree(p); }
	bool alloc(uint64_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
	template <class T> T* as() const { return static_cast<T*>(p); }
};

constexpr int kCpEvents = 4;   // before the map kernel, after it, after the scan, after the emit kernel

}  // namespace

struct dg_compose_plan {
	dg_context_t* ctx = nullptr;
	CpModule* mod = nullptr;
	uint32_t n = 0;
	int ignore_hash = 0;
	Buf d_desc, d_work, d_res, d_sizes;
	// stage timing: a ring of `slots` event sets
	std::vector<hipEvent_t> ev;
	uint32_t slots = 0, runs = 0;
	~dg_compose_plan() {
		for (hipEvent_t e : ev)
			if (e) hipEventDestroy(e);
	}
};


namespace {

// descs with a_cap, b_cap, max_a and max_b filled; work_off is set here
int plan_make(dg_context_t* ctx, std::vector<CpDesc>& descs, int ignore_hash, dg_compose_plan_t** out) {
	*out = nullptr;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	CpModule* mod = nullptr;
	int rc = module_get(ctx, &mod);
	if (rc) return rc;
	const uint32_t n = (uint32_t)descs.size();
	uint64_t work = 0;
	for (uint32_t i = 0; i < n; ++i) {
		CpDesc& d = descs[i];
		if (d.a_cap >= (1ull << 32) || d.b_cap >= (1ull << 32))
			return ctx_fail(ctx, DG_ERR_TOO_LARGE, "compose plan: a stream of 4 GiB or more does not fit the u32 format");
		d.work_off = work;
		work += work_bytes(d.max_a, d.max_b);
	}
	auto* P = new (std::nothrow) dg_compose_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->mod = mod;
	P->n = n;
	P->ignore_hash = ignore_hash ? 1 : 0;
	const uint64_t nn = std::max<uint32_t>(n, 1);
	if (!P->d_desc.alloc(sizeof(CpDesc) * nn) || !P->d_work.alloc(work) || !P->d_res.alloc(sizeof(CpRes) * nn) ||
	    !P->d_sizes.alloc(8 * nn)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "compose plan: device allocation of the work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, descs.data(), sizeof(CpDesc) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "compose plan: descriptor upload failed");
	}
	*out = P;
	return DG_OK;
}

// the most commands a stream of cap bytes holds (the END byte may be missing)
uint32_t max_cmds(uint64_t cap) { return (uint32_t)std::min<uint64_t>(cap > 25 ? (cap - 25) / 9 : 0, 0xFFFFFFFEull); }

// pair i's worst-case delta size and command count in an encode plan
void enc_geometry(const dg_encode_plan_t* enc, uint32_t i, uint64_t* cap, uint32_t* cmds) {
	dg_algorithm_t algo;
	dg_diff_options_t o;
	plan_options(enc, &algo, &o);
	const uint64_t p = o.p, vl = plan_pairs(enc)[i].v_len;
	// the encode plan's per-pair output bound (dg_plan.cpp)
	*cap = algo == DG_ALGO_CORRECTING ? 57 + vl + 22 * (vl / p) : 35 + vl + (vl / p) * (p < 22 ? 22 - p : 0);
	// the encoders alternate COPY and ADD: at most one ADD before each COPY and one at the end
	*cmds = (uint32_t)std::min<uint64_t>(2ull * plan_pp(enc)[i].rec_cap + 1, max_cmds(*cap));
}

}  // namespace

extern "C" {

int dg_compose_plan_create(dg_context_t* ctx, const dg_compose_desc_t* descs, uint32_t n, int ignore_hash,
                           dg_compose_plan_t** out) {
	if (!ctx || !out || (n && !descs)) return DG_ERR_INVALID_ARG;
	std::vector<CpDesc> d(n);
	for (uint32_t i = 0; i < n; ++i)
		d[i] = CpDesc{descs[i].a_off, descs[i].a_cap, descs[i].b_off, descs[i].b_cap, 0, max_cmds(descs[i].a_cap),
		              max_cmds(descs[i].b_cap)};
	return plan_make(ctx, d, ignore_hash, out);
}

int dg_compose_plan_create_for(dg_context_t* ctx, const dg_encode_plan_t* enc_a, const dg_encode_plan_t* enc_b,
                               int ignore_hash, dg_compose_plan_t** out) {
	if (!ctx || !enc_a || !enc_b || !out) return DG_ERR_INVALID_ARG;
	if (plan_ctx(enc_a) != ctx || plan_ctx(enc_b) != ctx)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "an encode plan belongs to another context");
	const uint32_t n = dg_encode_plan_num_pairs(enc_a);
	if (dg_encode_plan_num_pairs(enc_b) != n)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "compose plan: the encode plans differ in their pair counts");
	std::vector<CpDesc> d(n);
	for (uint32_t i = 0; i < n; ++i) {
		d[i] = CpDesc{};
		enc_geometry(enc_a, i, &d[i].a_cap, &d[i].max_a);
		enc_geometry(enc_b, i, &d[i].b_cap, &d[i].max_b);
	}
	return plan_make(ctx, d, ignore_hash, out);
}

int dg_compose_plan_set_timing(dg_compose_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if ((size_t)slots * kCpEvents > P->ev.size()) {
		const size_t have = P->ev.size();
		P->ev.resize((size_t)slots * kCpEvents, nullptr);
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

int dg_compose_plan_stage_times(dg_compose_plan_t* P, float* ms, const char** names, int n) {
	static const char* kNames[] = {"map", "scan", "emit", "total"};
	const uint32_t used = P && P->slots ? std::min(P->runs, P->slots) : 0;
	if (!used || n < 1) return 0;
	double acc[4] = {0, 0, 0, 0};
	for (uint32_t s = 0; s < used; ++s) {
		hipEvent_t* e = &P->ev[(size_t)kCpEvents * s];
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
	hipEvent_t* ev = P->slots ? &P->ev[(size_t)kCpEvents * (P->runs++ % P->slots)] : nullptr;
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
	auto fail = [&](const char* what, hipError_t e) {
		const std::string msg = std::string(what) + " failed: " + hipGetErrorString(e);
		return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
	};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->mod->map, P->n, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return fail("launch of dg_compose_map_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = launch_scan(P->d_sizes.as<uint64_t>(), d_out_offsets, P->n, st)) != hipSuccess)
		return fail("launch of the size scan", e);
	if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return fail("hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->mod->emit, P->n, 1, 1, 256, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return fail("launch of dg_compose_emit_kernel", e);
	if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return fail("hipEventRecord", e);
	return DG_OK;
}

void dg_compose_plan_destroy(dg_compose_plan_t* P) {
	if (!P) return;
	hipSetDevice(ctx_device(P->ctx));
	hipStreamSynchronize((hipStream_t)dg_context_stream(P->ctx));
	delete P;
}

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
	struct Guard {
		dg_compose_plan_t* p;
		~Guard() { dg_compose_plan_destroy(p); }
	} guard{plan};
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	Buf d_a, d_b, d_out, d_off, d_st;
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
	if (!d_a.alloc(at) || !d_b.alloc(bt) || !d_off.alloc(8ull * (n + 1)) || !d_st.alloc(4ull * n)) {
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
	if (!d_out.alloc(total)) {
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
	int first_bad = DG_OK;
	for (uint32_t i = 0; i < n; ++i) {
		const int32_t s = stv[i];
		if (s == DG_OK) {
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
