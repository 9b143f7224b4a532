// dg_host.cpp — host side of libdeltagpu.so: the C ABI of include/delta_gpu.h.
//
// Thin by design: it validates the arguments, allocates and uploads what
// dg_plan.cpp computed (the CRC constant tables of a context; the table sizes
// and buffer geometry of a batch), and enqueues the kernels of the .hip files
// on the run stream and one side stream.  The host-memory entry points are in
// dg_host_io.cpp.  There is no CPU compute fallback: without a GPU every
// entry point fails with DG_ERR_NO_DEVICE.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_device.h"
#include "dg_hostutil.h"
#include "dg_plan.h"

using namespace dg;

// ───────────────────────────── context ────────────────────────────────────

struct dg_context {
	int device = -1;
	hipStream_t stream = nullptr;
	uint64_t* d_crc_tables = nullptr;   // slice(8x256) + levels(6x256)
	uint64_t* d_xinv = nullptr;         // 16
	uint64_t* d_k32 = nullptr;          // x^(8 * 32 * t), t = 0..1023 (the correcting build's CRC)
	uint64_t kseg = 0;
	uint32_t n_cu = 256;                // compute units (grid caps)
	int lds_bytes = 0;                  // LDS a block may use (0: not known)
	uint64_t table_pool_bytes = 0;      // DG_LIMIT_TABLE_POOL_BYTES (0 = automatic)
	uint64_t onepass_members = 0;       // DG_LIMIT_ONEPASS_MEMBERS (0 auto, 1 on, 2 off)
	uint64_t limits_gen = 0;            // bumped by every dg_context_set_limit (cached plans key on it)
	std::string err;
	// scratch reused by the host-buffer entry points
	void* pin = nullptr;
	size_t pin_cap = 0;
	void* io = nullptr;                 // dg_encode_pipelined's slots (dg_host_io.cpp)
	void (*io_free)(void*) = nullptr;
	// code objects loaded at run time: the in-place conversion module
	// (dg_inplace_host.cpp), the in-place update module (dg_update_host.cpp),
	// the composition module (dg_compose_host.cpp), the inversion module
	// (dg_invert_host.cpp), the sketch module (dg_sketch_host.cpp)
	void* module[kCtxModules] = {};
	void (*module_free[kCtxModules])(void*) = {};
};

uint64_t dg::ctx_limits_gen(const dg_context_t* ctx) { return ctx->limits_gen; }
int dg::ctx_device(const dg_context_t* ctx) { return ctx->device; }

void** dg::ctx_io(dg_context_t* ctx, void (*release)(void*)) {
	ctx->io_free = release;
	return &ctx->io;
}

void** dg::ctx_module(dg_context_t* ctx, int slot, void (*release)(void*)) {
	ctx->module_free[slot] = release;
	return &ctx->module[slot];
}

const uint64_t* dg::ctx_crc_tables(const dg_context_t* ctx) { return ctx->d_crc_tables; }

int dg::ctx_fail(dg_context_t* ctx, int code, const char* msg) {
	if (ctx) ctx->err = msg;
	return code;
}

static int set_err(dg_context_t* ctx, int code, const char* fmt, ...) {
	if (ctx) {
		char buf[512];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		ctx->err = buf;
	}
	return code;
}

#define HIPCHK(ctx, expr)                                                                   \
	do {                                                                                    \
		hipError_t e_ = (expr);                                                             \
		if (e_ != hipSuccess)                                                               \
			return set_err((ctx), DG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

extern "C" {

int dg_abi_version(void) { return DG_ABI_VERSION; }

void dg_diff_options_default(dg_diff_options_t* o) {
	o->p = DG_SEED_LEN;
	o->q = DG_TABLE_SIZE;
	o->buf_cap = DG_BUF_CAP;
	o->max_table = DG_MAX_TABLE_SIZE;
	o->flags = 0;
}


const char* dg_status_string(int s) {
	switch (s) {
	case DG_OK: return "ok";
	case DG_ERR_INVALID_ARG: return "invalid argument";
	case DG_ERR_UNSUPPORTED: return "unsupported option";
	case DG_ERR_TOO_LARGE: return "input too large for the u32 delta format";
	case DG_ERR_NO_DEVICE: return "no HIP device";
	case DG_ERR_HIP: return "HIP runtime error";
	case DG_ERR_NOMEM: return "out of memory";
	case DG_ERR_CAPACITY: return "output buffer too small";
	case DG_ERR_MALFORMED: return "malformed delta";
	case DG_ERR_SRC_CRC: return "source file does not match delta";
	case DG_ERR_DST_CRC: return "output integrity check failed";
	case DG_ERR_TABLE_POOL: return "onepass work-table pool exhausted";
	case DG_ERR_INTERNAL: return "internal invariant failed on the device (library bug)";
	default: return "unknown status";
	}
}

const char* dg_last_error(const dg_context_t* ctx) { return ctx ? ctx->err.c_str() : ""; }

int dg_context_create(int device, dg_context_t** out) {
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DG_ERR_NO_DEVICE;
	dg_context_t* ctx = new (std::nothrow) dg_context_t();
	if (!ctx) return DG_ERR_NOMEM;
	if (device < 0) {
		if (hipGetDevice(&device) != hipSuccess) device = 0;
	}
	if (device >= n) { delete ctx; return DG_ERR_NO_DEVICE; }
	ctx->device = device;
	if (hipSetDevice(device) != hipSuccess) { delete ctx; return DG_ERR_HIP; }
	if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return DG_ERR_HIP; }
	{
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
			ctx->n_cu = (uint32_t)cus;
		if (hipDeviceGetAttribute(&ctx->lds_bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess)
			ctx->lds_bytes = 0;
	}

	CrcTables t;
	crc_tables_build(t);
	ctx->kseg = t.kseg;
	if (hipMalloc(&ctx->d_crc_tables, t.tab.size() * 8) != hipSuccess ||
	    hipMalloc(&ctx->d_xinv, sizeof t.xinv) != hipSuccess ||
	    hipMalloc(&ctx->d_k32, sizeof t.k32) != hipSuccess ||
	    hipMemcpy(ctx->d_crc_tables, t.tab.data(), t.tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(ctx->d_xinv, t.xinv, sizeof t.xinv, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(ctx->d_k32, t.k32, sizeof t.k32, hipMemcpyHostToDevice) != hipSuccess) {
		dg_context_destroy(ctx);
		return DG_ERR_HIP;
	}
	*out = ctx;
	return DG_OK;
}

void dg_context_destroy(dg_context_t* ctx) {
	if (!ctx) return;
	hipSetDevice(ctx->device);
	if (ctx->stream) hipStreamSynchronize(ctx->stream);
	hipFree(ctx->d_crc_tables);
	hipFree(ctx->d_xinv);
	hipFree(ctx->d_k32);
	if (ctx->pin) hipHostFree(ctx->pin);
	if (ctx->io && ctx->io_free) ctx->io_free(ctx->io);
	for (int k = 0; k < kCtxModules; ++k)
		if (ctx->module[k] && ctx->module_free[k]) ctx->module_free[k](ctx->module[k]);
	if (ctx->stream) hipStreamDestroy(ctx->stream);
	delete ctx;
}

void* dg_context_stream(dg_context_t* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int dg_context_set_limit(dg_context_t* ctx, int limit, uint64_t value) {
	if (!ctx) return DG_ERR_INVALID_ARG;
	switch (limit) {
	case DG_LIMIT_TABLE_POOL_BYTES:
		ctx->table_pool_bytes = value;
		++ctx->limits_gen;
		return DG_OK;
	case DG_LIMIT_ONEPASS_MEMBERS:
		if (value > 2) return set_err(ctx, DG_ERR_INVALID_ARG, "onepass members mode %llu", (unsigned long long)value);
		ctx->onepass_members = value;
		++ctx->limits_gen;
		return DG_OK;
	default: return set_err(ctx, DG_ERR_INVALID_ARG, "unknown limit %d", limit);
	}
}

}  // extern "C"

const char* dg::ab_env(const char* name) {
#ifdef DG_AB_SWITCHES
	return getenv(name);
#else
	(void)name;
	return nullptr;
#endif
}

// ───────────────────── code objects loaded at run time ────────────────────

namespace {

struct CodeObject {
	hipModule_t mod = nullptr;
	std::vector<hipFunction_t> fn;
};

void code_object_release(void* p) {
	auto* m = static_cast<CodeObject*>(p);
	if (m->mod) hipModuleUnload(m->mod);
	delete m;
}

// `file` in the directory this library was loaded from
std::string beside_library(const char* file) {
	Dl_info info{};
	if (!dladdr(reinterpret_cast<const void*>(&code_object_release), &info) || !info.dli_fname) return file;
	std::string p = info.dli_fname;
	const size_t slash = p.rfind('/');
	p = slash == std::string::npos ? std::string() : p.substr(0, slash + 1);
	return p + file;
}

}  // namespace

int dg::load_kernels(dg_context_t* ctx, int slot, const char* file, const char* label, const char* const* names,
                     int n_names, const hipFunction_t** fns) {
	void** held = ctx_module(ctx, slot, code_object_release);
	if (!*held) {
		auto* m = new (std::nothrow) CodeObject();
		if (!m) return DG_ERR_NOMEM;
		m->fn.assign(n_names, nullptr);
		const std::string path = beside_library(file);
		hipError_t e = hipModuleLoad(&m->mod, path.c_str());
		for (int k = 0; k < n_names && e == hipSuccess; ++k) e = hipModuleGetFunction(&m->fn[k], m->mod, names[k]);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			const std::string msg = std::string(label) + ": cannot load " + path + ": " + hipGetErrorString(e);
			code_object_release(m);
			return ctx_fail(ctx, DG_ERR_HIP, msg.c_str());
		}
		*held = m;
	}
	*fns = static_cast<CodeObject*>(*held)->fn.data();
	return DG_OK;
}

// ───────────────────────────── device buffers ─────────────────────────────

namespace {

// one u32 of mapped, coherent host memory the device writes (h: host address,
// d: its device address)
struct HostWord {
	uint32_t* h = nullptr;
	uint32_t* d = nullptr;
	~HostWord() { release(); }
	void release() {
		if (h) hipHostFree(h);
		h = d = nullptr;
	}
	int alloc() {
		release();
		if (hipHostMalloc((void**)&h, 4, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
			h = nullptr;
			return -1;
		}
		*h = 0;
		if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess) {
			release();
			return -1;
		}
		return 0;
	}
	uint32_t read() const { return __atomic_load_n(h, __ATOMIC_RELAXED); }
};

}  // namespace

// ───────────────────────────── encode plan ────────────────────────────────

struct dg_encode_plan {
	dg_context_t* ctx = nullptr;
	dg_algorithm_t algo = DG_ALGO_ONEPASS;
	dg_diff_options_t opts{};
	uint32_t n = 0;
	EncodeGeometry g;   // sizes and layout (dg_plan.h); g.members: member mode in use
	std::vector<dg_pair_t> pairs;   // the batch layout (dg_inplace_plan_create_for)
	// device buffers
	DevBuf d_pairs, d_pplan, d_powc, d_rec, d_nrec, d_dsize, d_crc_spans_r, d_crc_segs,
	    d_seg_crc, d_crc, d_tables, d_locks, d_tags, d_ctab, d_lookback, d_kcls, d_gpairs, d_prio_flag,
	    d_gent;   // greedy: (offset, tag) per seed of every R
	// onepass member mode (dg_members.hip): member arrays share the record
	// slots' indexing; the verification work queue
	DevBuf d_mem_s, d_srec, d_nmem, d_chunks, d_csum, d_cmap, d_seg, d_nseg;
	// fork/join of the CRC kernels onto a side stream
	hipStream_t side = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	bool serial_crc = false;   // DG_SERIAL_CRC=1: CRC on the run stream, before the differencing (A/B bound)
	bool skip_crc = false;     // DG_SKIP_CRC=1: no CRC kernels, wrong header CRCs (A/B bound only)
	// automatic member mode: the routed-pair count of the last completed run
	// (written by scan_sizes_kernel into mapped host memory) decides whether the
	// routed chain waits for the CRC pass (see the run)
	DevBuf d_route_cnt;
	HostWord route_fb;
	uint32_t plain_streak = 0;   // runs since the last member-mode probe (dg_encode_plan_run)
	uint64_t member_runs = 0, plain_runs = 0;   // dg_encode_plan_run_modes
	uint64_t* stats = nullptr; // dg_encode_plan_set_stats: --verbose counters (device, 8 per pair)
	int timing_mode = DG_TIMING_ALL;
	TimingRing ring;           // kTimingEvents events per run
};

const PairPlanDev* dg::plan_pp(const dg_encode_plan_t* P) { return P->g.pp.data(); }
const dg_pair_t* dg::plan_pairs(const dg_encode_plan_t* P) { return P->pairs.data(); }
dg_context_t* dg::plan_ctx(const dg_encode_plan_t* P) { return P->ctx; }
void dg::plan_options(const dg_encode_plan_t* P, dg_algorithm_t* algo, dg_diff_options_t* opts) {
	*algo = P->algo;
	*opts = P->opts;
}

static const char* kStageNames[] = {"crc64", "diff", "scan", "serialize+join", "total", "members", "corr_build", "corr_scan"};
static const char* kGreedyStageNames[] = {"greedy_build", "greedy_scan"};   // stages 6, 7 of a greedy plan

extern "C" {

#ifndef DG_CRC_PRIO_FLAG   // A/B: member plans raise the rows pass to priority 1 after the member kernel
#define DG_CRC_PRIO_FLAG 0
#endif
constexpr bool kCrcPrioFlag = DG_CRC_PRIO_FLAG != 0;

// geometry -> allocations -> uploads -> side stream and events; on failure the
// caller destroys the half-built plan
static int plan_fill(dg_encode_plan_t* P, const dg_pair_t* pairs) {
	dg_context_t* ctx = P->ctx;
	const dg_algorithm_t algo = P->algo;
	const uint32_t n = P->n;
	EncodeGeometry& g = P->g;
	PlanEnv env;
	env.n_cu = ctx->n_cu;
	env.lds_bytes = ctx->lds_bytes;
	env.table_pool_bytes = ctx->table_pool_bytes;
	env.onepass_members = ctx->onepass_members;
	env.onepass16 = onepass16_selected();
	env.no_members = ab_env("DG_NO_MEMBERS");
	env.members = ab_env("DG_MEMBERS");
	env.corr_build = ab_env("DG_CORR_BUILD");
	env.fused = ab_env("DG_FUSED");
	env.route_min = ab_env("DG_ROUTE_MIN");
	std::string err;
	const int rc = encode_geometry(algo, P->opts, pairs, n, env, g, err);
	if (rc != DG_OK) {
		if (!err.empty()) ctx->err = err;
		return rc;
	}
	hipSetDevice(ctx->device);

	const uint32_t n1 = std::max<uint32_t>(n, 1);
	const size_t p = P->opts.p;
	int bad = 0;
	bad |= P->d_pairs.alloc(sizeof(PairDev) * n1);
	bad |= P->d_pplan.alloc(sizeof(PairPlanDev) * n1);
	bad |= P->d_powc.alloc(8 * p);
	bad |= P->d_rec.alloc(4ull * (algo != DG_ALGO_CORRECTING ? kRecWordsOnepass : kRecWordsCorrecting) *
	                      std::max<uint64_t>(g.total_rec, 1));
	bad |= P->d_nrec.alloc(4ull * n1);
	bad |= P->d_dsize.alloc(8ull * n1);
	bad |= P->d_crc_spans_r.alloc(sizeof(CrcSpanDev) * std::max<size_t>(g.spans.size(), 1));
	bad |= P->d_crc_segs.alloc(sizeof(CrcSegDev) * std::max<size_t>(g.segs.size(), 1));
	bad |= P->d_seg_crc.alloc(8 * std::max<size_t>(g.segs.size(), 1));
	bad |= P->d_crc.alloc(16ull * n1);   // per pair: CRC of R, of V
	bad |= P->d_tables.alloc(g.table_bytes * g.n_tables);
	bad |= P->d_locks.alloc(4ull * g.n_tables);
	bad |= P->d_tags.alloc(4ull * g.n_tables);
	if (algo == DG_ALGO_CORRECTING) {
		bad |= P->d_gpairs.alloc(4ull * std::max<size_t>(g.gpairs.size(), 1));
		if (!bad && !g.gpairs.empty() &&
		    hipMemcpy(P->d_gpairs.p, g.gpairs.data(), 4 * g.gpairs.size(), hipMemcpyHostToDevice) != hipSuccess)
			bad = 1;
		bad |= P->d_ctab.alloc(4ull * std::max<uint64_t>(g.ctab_entries, 1));
		bad |= P->d_kcls.alloc(8ull * n1);
	}
	if (g.fused) bad |= P->d_lookback.alloc(8ull * n1);
	if (algo == DG_ALGO_GREEDY) {
		bad |= P->d_ctab.alloc(4ull * std::max<uint64_t>(g.greedy_heads, 1));
		bad |= P->d_gent.alloc(8ull * std::max<uint64_t>(g.greedy_entries, 1));
	}
	if (g.members) {
		const uint32_t nc1 = std::max<uint32_t>(g.n_chunks, 1);
		int mbad = 0;
		mbad |= P->d_mem_s.alloc(4ull * std::max<uint64_t>(g.mem_slots, 1));
		mbad |= P->d_srec.alloc(16ull * std::max<uint64_t>(g.mem_slots, 1));
		mbad |= P->d_nmem.alloc(4ull * nc1);
		mbad |= P->d_chunks.alloc(8ull * nc1);
		mbad |= P->d_csum.alloc(8ull * nc1);
		mbad |= P->d_cmap.alloc(8ull * nc1);
		mbad |= P->d_seg.alloc(16ull * ((uint64_t)g.n_chunks + 2ull * n));
		mbad |= P->d_nseg.alloc(4ull * n1);
		mbad |= P->d_prio_flag.alloc(4);
		if (g.route_min) {
			mbad |= P->d_route_cnt.alloc(4);
			mbad |= P->route_fb.alloc();
			if (!mbad && hipMemset(P->d_route_cnt.p, 0, 4) != hipSuccess) mbad = 1;
		}
		if (!mbad && !g.jobs.empty() &&
		    hipMemcpy(P->d_chunks.p, g.jobs.data(), 4 * g.jobs.size(), hipMemcpyHostToDevice) != hipSuccess)
			mbad = 1;
		if (mbad && ctx->onepass_members != 1) {
			// automatic mode: member mode is an optimisation, so a batch that
			// fits with the plain chain still gets a plan
			(void)hipGetLastError();
			for (DevBuf* b : {&P->d_mem_s, &P->d_srec, &P->d_nmem, &P->d_chunks, &P->d_csum, &P->d_cmap,
			                  &P->d_seg, &P->d_nseg, &P->d_prio_flag, &P->d_route_cnt})
				b->release();
			P->route_fb.release();
			g.members = false;
			g.n_chunks = 0;
			mbad = 0;
		}
		bad |= mbad;
	}
	if (bad) return set_err(ctx, DG_ERR_NOMEM, "device allocation failed");
	hipStream_t st = ctx->stream;
	hipError_t e = hipSuccess;
	if (n) {
		e = hipMemcpyAsync(P->d_pairs.p, pairs, sizeof(PairDev) * n, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(P->d_pplan.p, g.pp.data(), sizeof(PairPlanDev) * n, hipMemcpyHostToDevice, st);
		if (e == hipSuccess) e = hipMemcpyAsync(P->d_crc_spans_r.p, g.spans.data(), sizeof(CrcSpanDev) * g.spans.size(), hipMemcpyHostToDevice, st);
		if (e == hipSuccess && !g.segs.empty()) e = hipMemcpyAsync(P->d_crc_segs.p, g.segs.data(), sizeof(CrcSegDev) * g.segs.size(), hipMemcpyHostToDevice, st);
	}
	if (e == hipSuccess) e = hipMemcpyAsync(P->d_powc.p, g.powc.data(), 8 * p, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemsetAsync(P->d_tables.p, 0, P->d_tables.n, st);
	if (e == hipSuccess) e = hipMemsetAsync(P->d_locks.p, 0, P->d_locks.n, st);
	if (e == hipSuccess) e = hipMemsetAsync(P->d_tags.p, 0, P->d_tags.n, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return set_err(ctx, DG_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e));
	const char* sc = ab_env("DG_SERIAL_CRC");
	P->serial_crc = sc && sc[0] == '1';
	const char* sk = ab_env("DG_SKIP_CRC");
	P->skip_crc = sk && sk[0] == '1';

	if (!P->serial_crc) {
		e = hipStreamCreateWithFlags(&P->side, hipStreamNonBlocking);
		// stream-to-stream ordering on one device: a device-scope release (the
		// default system-scope one writes back and invalidates the caches)
		if (e == hipSuccess) e = hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming | hipEventReleaseToDevice);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming | hipEventReleaseToDevice);
		if (e != hipSuccess) return set_err(ctx, DG_ERR_HIP, "side stream creation failed: %s", hipGetErrorString(e));
	}
	return DG_OK;
}

int dg_encode_plan_create(dg_context_t* ctx, dg_algorithm_t algo, const dg_pair_t* pairs,
                          uint32_t n, const dg_diff_options_t* opts, dg_encode_plan_t** out) {
	*out = nullptr;
	if (!ctx) return DG_ERR_INVALID_ARG;
	dg_encode_plan_t* P = new (std::nothrow) dg_encode_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->algo = algo;
	if (opts) P->opts = *opts; else dg_diff_options_default(&P->opts);
	P->n = n;
	if (n && pairs) P->pairs.assign(pairs, pairs + n);
	const int rc = plan_fill(P, pairs);
	if (rc != DG_OK) {
		dg_encode_plan_destroy(P);
		return rc;
	}
	*out = P;
	return DG_OK;
}

uint64_t dg_encode_plan_output_bound(const dg_encode_plan_t* P) { return P ? P->g.out_bound : 0; }
uint32_t dg_encode_plan_num_pairs(const dg_encode_plan_t* P) { return P ? P->n : 0; }
uint32_t dg_encode_plan_flags(const dg_encode_plan_t* P) { return P && P->g.members ? DG_PLAN_MEMBERS : 0u; }
int dg_encode_plan_run_modes(const dg_encode_plan_t* P, uint64_t* member_runs, uint64_t* plain_runs) {
	if (!P || !member_runs || !plain_runs) return DG_ERR_INVALID_ARG;
	*member_runs = P->member_runs;
	*plain_runs = P->plain_runs;
	return DG_OK;
}

int dg_encode_plan_set_stats(dg_encode_plan_t* P, uint64_t* d_stats) {
	if (!P) return DG_ERR_INVALID_ARG;
	P->stats = d_stats;
	return DG_OK;
}
#ifdef DG_AB_SWITCHES
// A/B and profiling builds only: the member kernel's outputs of the last run
// (device pointers; scripts/member_debug.py)
int dg_encode_plan_member_debug(const dg_encode_plan_t* P, void** mem_s, void** srec, void** n_mem,
                                void** csum, uint32_t* n_chunks) {
	if (!P || !P->g.members) return -1;
	*mem_s = P->d_mem_s.p;
	*srec = P->d_srec.p;
	*n_mem = P->d_nmem.p;
	*csum = P->d_csum.p;
	*n_chunks = P->g.n_chunks;
	return 0;
}
#endif
uint64_t dg_encode_plan_table_size(const dg_encode_plan_t* P, uint32_t i) {
	return (P && i < P->n) ? P->g.pp[i].q : 0;
}
const uint32_t* dg_encode_plan_copy_counts_device(const dg_encode_plan_t* P) {
	return P ? P->d_nrec.as<uint32_t>() : nullptr;
}

constexpr int kTimingEvents = 8;
constexpr uint32_t kTimingAll = (1u << kTimingEvents) - 1u;
// the events a run records: all, or around the dominant kernel(s) only —
// the member kernel (2, 6), the correcting build and scan (2, 7, 3), the
// plain onepass kernel (2, 3); member plans also 3 (the chains after the
// member kernel: the routed plain chain dominates on data off diagonal 0)
static uint32_t timing_mask(const dg_encode_plan_t* P) {
	if (P->timing_mode != DG_TIMING_DOMINANT) return kTimingAll;
	if (P->g.members) return (1u << 2) | (1u << 6) | (1u << 3);   // the member kernel, then the chains
	if (P->algo != DG_ALGO_ONEPASS) return (1u << 2) | (1u << 7) | (1u << 3);   // build, scan
	return (1u << 2) | (1u << 3);
}

int dg_encode_plan_set_timing(dg_encode_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(P->ctx->device);
	if (!P->ring.set((uint32_t)slots, kTimingEvents)) return set_err(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// Per-run events: 0/1 around the CRC kernels (side stream), 2/3 around the
// differencing kernel(s), 4 after the scan, 5 after serialisation + the CRC
// join + the header CRCs (member plans: crc_patch_kernel; DG_FUSED=1: the join
// falls before 4), 6 after the member kernel (member mode; else with 2), 7
// after the correcting R-index build (before the V scan; onepass: with 3).  Stages
// corr_build (2..7) and corr_scan (7..3) are reported for correcting plans only
// (greedy plans: the same two intervals as greedy_build and greedy_scan).
// Returns the mean over the runs recorded since set_timing (at most `slots`).
int dg_encode_plan_stage_times(dg_encode_plan_t* P, float* ms, const char** names, int n) {
	const uint32_t used = P ? P->ring.used() : 0;
	if (!used) return 0;
	const int pairs[8][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {2, 5}, {2, 6}, {2, 7}, {7, 3}};
	const uint32_t mask = timing_mask(P);
	int sel[8], ns = 0;   // the stages whose two events were recorded
	for (int k = 0; k < 8; ++k) {
		if (k >= 6 && P->algo == DG_ALGO_ONEPASS) continue;
		if (k == 5 && P->g.members == false && mask != kTimingAll) continue;
		if ((mask >> pairs[k][0] & 1) && (mask >> pairs[k][1] & 1)) sel[ns++] = k;
	}
	const int last = (mask >> 5) & 1 ? 5 : (P->g.members && !(mask >> 3 & 1) ? 6 : 3);
	double acc[8] = {};
	for (uint32_t s = 0; s < used; ++s) {
		hipEvent_t* e = P->ring.set_at(s);
		if (hipEventSynchronize(e[last]) != hipSuccess) return 0;
		for (int i = 0; i < ns; ++i) {
			float t = 0;
			hipEventElapsedTime(&t, e[pairs[sel[i]][0]], e[pairs[sel[i]][1]]);
			acc[i] += t;
		}
	}
	int i = 0;
	for (; i < ns && i < n; ++i) {
		if (ms) ms[i] = (float)(acc[i] / used);
		if (names) names[i] = sel[i] >= 6 && P->algo == DG_ALGO_GREEDY ? kGreedyStageNames[sel[i] - 6] : kStageNames[sel[i]];
	}
	return i;
}

int dg_encode_plan_set_timing_mode(dg_encode_plan_t* P, int mode) {
	if (!P || (mode != DG_TIMING_ALL && mode != DG_TIMING_DOMINANT)) return DG_ERR_INVALID_ARG;
	P->timing_mode = mode;
	return DG_OK;
}

int dg_encode_plan_set_timing_every(dg_encode_plan_t* P, int every) {
	if (!P || every < 1) return DG_ERR_INVALID_ARG;
	P->ring.set_every((uint32_t)every);
	return DG_OK;
}

static MemSerArgs mem_ser_args(const dg_encode_plan_t* P, const uint8_t* d_ver, uint8_t* d_out, uint64_t out_cap,
                               const uint64_t* d_offsets, int32_t* d_status) {
	MemSerArgs m{};
	m.ver = d_ver;
	m.pairs = P->d_pairs.as<PairDev>();
	m.pplan = P->d_pplan.as<PairPlanDev>();
	m.chunks = P->d_chunks.as<uint2>();
	m.cmap = P->d_cmap.as<uint32_t>();
	m.seg = P->d_seg.as<uint32_t>();
	m.nseg = P->d_nseg.as<uint32_t>();
	m.mem_s = P->d_mem_s.as<uint32_t>();
	m.srec = P->d_srec.as<uint32_t>();
	m.rec = P->d_rec.as<uint32_t>();
	m.offsets = d_offsets;
	m.out = d_out;
	m.out_cap = out_cap;
	m.status = d_status;
	m.v_total = P->g.v_total;
	m.n_pairs = P->n;
	return m;
}

// automatic member mode over a batch the member kernel gains nothing on: one
// run in this many runs in member mode (the others as a plain plan)
constexpr uint32_t kProbeEvery = 16;

// onepass: the plain chain; or (mem) the member kernel, ev_members (nullable,
// stage timing), then the member chain and, for the pairs it routes, the plain
// chain (after routed_after, when set)
static int enqueue_onepass(dg_encode_plan_t* P, EncodeArgs a, bool mem, hipEvent_t ev_members,
                           hipEvent_t routed_after, hipStream_t st) {
	dg_context_t* ctx = P->ctx;
	if (!mem) {
		HIPCHK(ctx, launch_onepass(a, a.p, P->g.aligned16, st));
		return DG_OK;
	}
	SpecArgs m{};
	m.ref = a.ref;
	m.ver = a.ver;
	m.pairs = a.pairs;
	m.pplan = a.pplan;
	m.chunks = P->d_chunks.as<uint2>();
	m.mem_s = P->d_mem_s.as<uint32_t>();
	m.n_mem = P->d_nmem.as<uint32_t>();
	m.srec = P->d_srec.as<uint32_t>();
	m.csum = P->d_csum.as<uint32_t>();
	m.cmap = P->d_cmap.as<uint32_t>();
	a.csum = m.csum;
	a.cmap = m.cmap;
	a.seg = P->d_seg.as<uint32_t>();
	a.nseg = P->d_nseg.as<uint32_t>();
	a.route_min = P->g.route_min;
	a.mem_s = m.mem_s;
	a.n_mem = m.n_mem;
	a.srec = m.srec;
	HIPCHK(ctx, launch_members(m, P->g.n_chunks, ctx->n_cu, st));
	if (kCrcPrioFlag) HIPCHK(ctx, hipMemsetD32Async(P->d_prio_flag.p, 1, 1, st));   // the rows pass to priority 1
	if (ev_members) HIPCHK(ctx, hipEventRecord(ev_members, st));
	if (P->g.route_min) a.route_cnt = P->d_route_cnt.as<uint32_t>();
	HIPCHK(ctx, launch_onepass(a, a.p, P->g.aligned16, st, routed_after));
	return DG_OK;
}

// greedy: zeroed bucket counts, the seed index of every R, then the V scan
static int enqueue_greedy(dg_encode_plan_t* P, const EncodeArgs& a, hipEvent_t ev_built, hipStream_t st) {
	GreedyArgs g{};
	g.ref = a.ref;
	g.ver = a.ver;
	g.pairs = a.pairs;
	g.pplan = a.pplan;
	g.n_pairs = P->n;
	g.p = a.p;
	g.splay = (uint32_t)((P->opts.flags >> DG_OPT_SPLAY) & 1);
	g.max_seeds = (uint32_t)P->g.max_seeds;
	g.heads = P->d_ctab.as<uint32_t>();
	g.ent = P->d_gent.as<uint2>();
	g.rec = a.rec;
	g.n_rec = a.n_rec;
	g.dsize = a.dsize;
	g.status = a.status;
	HIPCHK(P->ctx, launch_greedy(g, P->g.greedy_heads, st, ev_built));
	return DG_OK;
}

// correcting: fresh R indexes (~0 = empty slot), then build + scan; ev_fork
// (nullable) is recorded after the build, where V's CRC forks
static int enqueue_correcting(dg_encode_plan_t* P, EncodeArgs a, hipEvent_t ev_built, hipEvent_t ev_fork,
                              hipStream_t st) {
	dg_context_t* ctx = P->ctx;
	a.buf_cap = (uint32_t)P->opts.buf_cap;
	a.stats = P->stats;
	a.ctab = P->d_ctab.as<uint32_t>();
	a.kcls = P->d_kcls.as<uint64_t>();
	a.max_seeds = (uint32_t)P->g.max_seeds;
	// the LDS build writes every slot of every index; the global
	// build only fills, so its tables start empty (~0)
	a.gpairs = P->d_gpairs.as<uint32_t>();
	a.n_gpairs = (uint32_t)P->g.gpairs.size();
	HIPCHK(ctx, launch_correcting_clear(a, st));
	if (P->g.crc_fused) {
		a.crc_out = P->d_crc.as<uint64_t>();
		a.crc_tab = ctx->d_crc_tables;
		a.crc_k32 = ctx->d_k32;
	}
	HIPCHK(ctx, launch_correcting(a, a.p, st, P->g.corr_lds_cap, P->g.qmin, ev_built, ev_fork));
	return DG_OK;
}

// The run's stream graph:
//   hints (from the last completed run) -> fork the side stream ->
//   {differencing on the run stream, CRC pass on the side stream}, in one of
//   two enqueue orders; or, for a fused correcting plan, differencing -> fork
//   after the R-index build -> V's CRC beside the V scan ->
//   scan of the delta sizes -> serialise (plain or member) with the join.
// (DG_FUSED=1, A/B: join and header patch right after the differencing.)
int dg_encode_plan_run(dg_encode_plan_t* P, const uint8_t* d_ref, const uint8_t* d_ver,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* d_offsets, int32_t* d_status,
                       void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (P->n == 0) return DG_OK;
	if (!d_ref || !d_ver || !d_out || !d_offsets || !d_status)
		return set_err(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (((uintptr_t)d_ref & 15) || ((uintptr_t)d_ver & 15))
		return set_err(ctx, DG_ERR_INVALID_ARG, "arena base pointers must be 16-byte aligned");
	hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;

	// The CRC-64/XZ of every R (even spans) and V (odd spans) shares nothing
	// with the differencing kernel until the serialiser, so it runs on a
	// forked side stream.  (DG_SERIAL_CRC=1, an A/B bound: on the run stream,
	// before the differencing.)
	const bool serial = P->serial_crc;
	hipStream_t cs = serial ? st : P->side;
	hipEvent_t* const cur = P->ring.next();   // this run's events (nullptr: it records none)
	// event k: every stage event, or (DG_TIMING_DOMINANT) only the ones
	// around the dominant kernel(s) (each extra timing event costs the run
	// stream a few microseconds); nullptr = not recorded
	auto ev = [&](int k) -> hipEvent_t { return cur && (timing_mask(P) & (1u << k)) ? cur[k] : nullptr; };
	auto rec = [&](int k, hipStream_t s) -> hipError_t {
		hipEvent_t e = ev(k);
		return e ? hipEventRecord(e, s) : hipSuccess;
	};

	// ── hints (the run's bytes do not depend on them) ──
	// Automatic member mode: a batch whose every pair the last completed
	// member-mode run of this plan routed to the plain chain (shift and
	// transposition pairs, c3s / c4o) runs as a plain plan, the member kernel
	// and its serialiser skipped, except every kProbeEvery-th run, which
	// refreshes the count.
	bool mem = P->g.members;
	if (mem && P->g.route_min && P->route_fb.read() >= P->n) {
		if (++P->plain_streak < kProbeEvery) mem = false;
		else P->plain_streak = 0;
	}
	++(mem ? P->member_runs : P->plain_runs);
	// member plans: the per-span combine (crc_finalize) waits on the run
	// stream for the chains.  Enqueued right after the row pass, its waves
	// queue behind the chains' full grid and slowed the routed chain of c3s
	// by 13 % (40.9 vs 36.2 ms, profiles/r05_experiments.md).
	const bool late_fin = mem && !serial;
	// automatic member mode: when the last completed run of this plan routed
	// more pairs to the plain chain than one round of chains fills (16 per
	// CU), the routed chain's grid waits for the CRC pass to end.  Dispatched
	// beside the pass's resident blocks, the chains land unevenly over the
	// SIMDs and the second round's last pairs trail: c3s 39.1 -> 35.7 ms
	// (profiles/r06_experiments.md).  Batches that route fewer pairs keep the
	// pass beside the member chain, whose shadow it is at c6.
	const bool chain_join = mem && !serial && !P->skip_crc && P->g.route_min && P->route_fb.read() > 16u * ctx->n_cu;

	CrcArgs c{};
	c.arena[0] = d_ref;
	c.arena[1] = d_ver;
	c.spans = P->d_crc_spans_r.as<CrcSpanDev>();
	c.segs = P->d_crc_segs.as<CrcSegDev>();
	c.n_segs = (uint32_t)P->g.segs.size();
	c.n_spans = (uint32_t)P->g.spans.size();
	c.tables = ctx->d_crc_tables;
	c.seg_crc = P->d_seg_crc.as<uint64_t>();
	c.out = P->d_crc.as<uint64_t>();
	c.xinv = ctx->d_xinv;
	c.kseg = ctx->kseg;
	c.prio_flag = kCrcPrioFlag && mem ? P->d_prio_flag.as<uint32_t>() : nullptr;
	// the CRC pass on cs, then (side stream) the event the run stream joins on
	auto run_crc = [&]() -> int {
		HIPCHK(ctx, rec(0, cs));
		if (!P->skip_crc) {   // (DG_SKIP_CRC=1, an A/B bound: no CRC kernels, wrong header CRCs)
			// beside the differencing: 2 blocks per CU per round of differencing
			// waves (16 per CU), so the CRC neither crowds one round out nor
			// trails a multi-round batch (C2: 4096 pairs -> 512 blocks)
			// (correcting plans: V's CRC runs beside the latency-bound V scan
			// with its whole grid; capped at 2 blocks per CU it took 0.97 ms
			// there instead of 0.71: C4 731 -> 813 GiB/s)
			const uint32_t rounds = (P->n + 16u * ctx->n_cu - 1) / (16u * ctx->n_cu);
			const uint32_t cap = serial || P->g.crc_fused ? 0u : 2u * ctx->n_cu * std::max(rounds, 1u);
			// (member plans: the five-bit row pass, 3.25 KiB of LDS: the byte-table
			// pass's 16 KiB blocks find no room beside the member kernel and trail
			// it; the member waves run at a higher issue priority, so the pass
			// takes the VALU slots they leave: C3 +3 %, c6 +10 % over round 4's
			// lane-contiguous pass, profiles/r05_experiments.md)
			HIPCHK(ctx, launch_crc(c, cs, cap, mem ? kCrcPassRows5 : kCrcPassRows, !late_fin));
		}
		HIPCHK(ctx, rec(1, cs));
		if (!serial) HIPCHK(ctx, hipEventRecord(P->ev_join, cs));
		return DG_OK;
	};
	// differencing -> COPY records + per-pair delta sizes
	auto run_diff = [&]() -> int {
		HIPCHK(ctx, rec(2, st));
		if (!mem) HIPCHK(ctx, rec(6, st));
		EncodeArgs a{};
		a.ref = d_ref;
		a.ver = d_ver;
		a.pairs = P->d_pairs.as<PairDev>();
		a.pplan = P->d_pplan.as<PairPlanDev>();
		a.n_pairs = P->n;
		a.p = (uint32_t)P->opts.p;
		a.powc = P->d_powc.as<uint64_t>();
		a.rec = P->d_rec.as<uint32_t>();
		a.n_rec = P->d_nrec.as<uint32_t>();
		a.dsize = P->d_dsize.as<uint64_t>();
		a.status = d_status;
		a.tables = P->d_tables.as<unsigned long long>();
		a.qmax = P->g.qmax;
		a.n_tables = P->g.n_tables;
		a.table_locks = P->d_locks.as<uint32_t>();
		a.table_tags = P->d_tags.as<uint32_t>();
		if (P->g.fused) {   // (DG_FUSED=1, A/B: the onepass waves place and serialise their deltas)
			a.out = d_out;
			a.out_cap = out_cap;
			a.offsets = d_offsets;
			a.lookback = P->d_lookback.as<unsigned long long>();
			HIPCHK(ctx, hipMemsetAsync(P->d_lookback.p, 0, 8ull * P->n, st));
		}
		int rc;
		if (P->algo == DG_ALGO_ONEPASS)
			rc = enqueue_onepass(P, a, mem, ev(6), chain_join ? P->ev_join : nullptr, st);
		else if (P->algo == DG_ALGO_GREEDY)
			rc = enqueue_greedy(P, a, ev(7), st);
		else
			rc = enqueue_correcting(P, a, ev(7), P->g.crc_fused && !serial ? P->ev_fork : nullptr, st);
		if (rc != DG_OK) return rc;
		if (P->algo == DG_ALGO_ONEPASS) HIPCHK(ctx, rec(7, st));
		HIPCHK(ctx, rec(3, st));
		return DG_OK;
	};

	// ── {differencing, CRC} ──
	int rc;
	if (serial) {
		if ((rc = run_crc()) != DG_OK) return rc;
		if ((rc = run_diff()) != DG_OK) return rc;
	} else if (P->g.crc_fused) {
		// the build writes R's CRC; V's CRC forks after the build (ev_fork,
		// recorded by launch_correcting) and runs beside the V scan
		if ((rc = run_diff()) != DG_OK) return rc;
		HIPCHK(ctx, hipStreamWaitEvent(cs, P->ev_fork, 0));
		if ((rc = run_crc()) != DG_OK) return rc;
	} else {
		if (kCrcPrioFlag && mem) HIPCHK(ctx, hipMemsetD32Async(P->d_prio_flag.p, 0, 1, st));
		HIPCHK(ctx, hipEventRecord(P->ev_fork, st));
		HIPCHK(ctx, hipStreamWaitEvent(cs, P->ev_fork, 0));
		if (chain_join) {   // the routed chain waits for the CRC pass (ev_join)
			if ((rc = run_crc()) != DG_OK) return rc;
			if ((rc = run_diff()) != DG_OK) return rc;
		} else {
			// the differencing kernel first, so its (long, latency-bound) waves
			// are resident before the CRC waves fill the issue slots they leave
			if ((rc = run_diff()) != DG_OK) return rc;
			if ((rc = run_crc()) != DG_OK) return rc;
		}
	}

	if (P->g.fused) {
		// (DG_FUSED=1, A/B) the differencing kernel placed and serialised every
		// delta; only the header CRCs remain, once the CRC stream has joined
		if (!serial) HIPCHK(ctx, hipStreamWaitEvent(st, P->ev_join, 0));
		HIPCHK(ctx, rec(4, st));
		HIPCHK(ctx, launch_crc_patch(d_out, d_offsets, P->d_crc.as<uint64_t>(), d_status, P->n, st));
		HIPCHK(ctx, rec(5, st));
		return DG_OK;
	}

	// ── exclusive scan of the delta sizes -> packed offsets ──
	HIPCHK(ctx, launch_scan(P->d_dsize.as<uint64_t>(), d_offsets, P->n, st,
	                        mem && P->g.route_min ? P->d_route_cnt.as<uint32_t>() : nullptr, P->route_fb.d));
	HIPCHK(ctx, rec(4, st));

	// ── serialise + join ──
	if (mem) {
		// the chains' segment lists, one wave per chunk: everything but the
		// header CRCs (the CRC stream may still be running beside the chains),
		// then the join, the CRC's combine and the header patch
		const MemSerArgs m = mem_ser_args(P, d_ver, d_out, out_cap, d_offsets, d_status);
		HIPCHK(ctx, launch_member_serialize(m, P->g.n_chunks, ctx->n_cu, st));
		if (!serial) HIPCHK(ctx, hipStreamWaitEvent(st, P->ev_join, 0));
		if (late_fin && !P->skip_crc) HIPCHK(ctx, launch_crc_finalize(c, st));
		HIPCHK(ctx, launch_crc_patch(d_out, d_offsets, P->d_crc.as<uint64_t>(), d_status, P->n, st));
	} else {
		// the CRC pass (beside the differencing) has normally finished by
		// now: join it first and let the serialiser write the header CRCs
		// (a crc_patch_kernel after it is one dependent launch, ~12 us at C2, more)
		if (!serial) HIPCHK(ctx, hipStreamWaitEvent(st, P->ev_join, 0));
		SerArgs s{};
		s.ver = d_ver;
		s.pairs = P->d_pairs.as<PairDev>();
		s.pplan = P->d_pplan.as<PairPlanDev>();
		s.rec = P->d_rec.as<uint32_t>();
		s.rec_words = P->algo != DG_ALGO_CORRECTING ? kRecWordsOnepass : kRecWordsCorrecting;
		s.n_rec = P->d_nrec.as<uint32_t>();
		s.crc = P->d_crc.as<uint64_t>();
		s.offsets = d_offsets;
		s.out = d_out;
		s.out_cap = out_cap;
		s.status = d_status;
		s.n_pairs = P->n;
		HIPCHK(ctx, launch_serialize_wave(s, st));
	}
	HIPCHK(ctx, rec(5, st));
	return DG_OK;
}

void dg_encode_plan_destroy(dg_encode_plan_t* P) {
	if (!P) return;
	hipSetDevice(P->ctx->device);
	hipStreamSynchronize(P->ctx->stream);
	if (P->side) hipStreamSynchronize(P->side);
	if (P->ev_fork) hipEventDestroy(P->ev_fork);
	if (P->ev_join) hipEventDestroy(P->ev_join);
	if (P->side) hipStreamDestroy(P->side);
	delete P;
}

}  // extern "C"

// ───────────────────────────── CRC batch (utility) ────────────────────────

extern "C" int dg_crc64_xz_batch_device(dg_context_t* ctx, const uint8_t* d_arena,
                                        const dg_span_t* spans, uint32_t n, uint64_t* d_crc,
                                        void* stream) {
	if (!ctx || (n && (!d_arena || !spans || !d_crc))) return DG_ERR_INVALID_ARG;
	if ((uintptr_t)d_arena & 15)
		return set_err(ctx, DG_ERR_INVALID_ARG, "arena base pointer must be 16-byte aligned");
	if (n == 0) return DG_OK;
	hipSetDevice(ctx->device);
	hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
	std::vector<dg_span_t> sp(spans, spans + n);
	std::vector<uint32_t> which(n, 0);
	std::vector<CrcSpanDev> sd;
	std::vector<CrcSegDev> seg;
	plan_crc_spans(sp, which, sd, seg);
	DevBuf d_sd, d_seg, d_segc;
	if (d_sd.alloc(sizeof(CrcSpanDev) * sd.size()) || d_seg.alloc(sizeof(CrcSegDev) * std::max<size_t>(seg.size(), 1)) ||
	    d_segc.alloc(8 * std::max<size_t>(seg.size(), 1)))
		return set_err(ctx, DG_ERR_NOMEM, "device allocation failed");
	HIPCHK(ctx, hipMemcpyAsync(d_sd.p, sd.data(), sizeof(CrcSpanDev) * sd.size(), hipMemcpyHostToDevice, st));
	if (!seg.empty())
		HIPCHK(ctx, hipMemcpyAsync(d_seg.p, seg.data(), sizeof(CrcSegDev) * seg.size(), hipMemcpyHostToDevice, st));
	CrcArgs a{};
	a.arena[0] = a.arena[1] = d_arena;
	a.spans = d_sd.as<CrcSpanDev>();
	a.segs = d_seg.as<CrcSegDev>();
	a.n_segs = (uint32_t)seg.size();
	a.n_spans = n;
	a.tables = ctx->d_crc_tables;
	a.seg_crc = d_segc.as<uint64_t>();
	a.out = d_crc;
	a.xinv = ctx->d_xinv;
	a.kseg = ctx->kseg;
	HIPCHK(ctx, launch_crc_wide(a, ctx->n_cu, st));   // alone on the device: the wide pass
	HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries die here
	return DG_OK;
}

// ───────────────────────────── decode plan ────────────────────────────────

struct dg_decode_plan {
	dg_context_t* ctx = nullptr;
	uint32_t n = 0;
	int ignore_hash = 0;
	DevBuf d_desc;   // the decode kernel computes and checks both CRCs itself
	// byte extents the streams touch in each arena (run rejects overlaps),
	// and the intervals themselves, sorted and merged per arena (the exact
	// check when the extents of the arenas overlap)
	uint64_t ref_end = 0, delta_end = 0, out_end = 0;
	std::vector<std::pair<uint64_t, uint64_t>> iv_ref, iv_delta, iv_out;
	TimingRing ring;   // kDecEvents events per run
};

namespace {
constexpr int kDecEvents = 2;   // decode_kernel's start and end
}  // namespace

extern "C" {

int dg_decode_plan_create(dg_context_t* ctx, const dg_decode_desc_t* descs, uint32_t n,
                          int ignore_hash, dg_decode_plan_t** out) {
	if (!ctx || !out || (n && !descs)) return DG_ERR_INVALID_ARG;
	*out = nullptr;
	for (uint32_t i = 0; i < n; ++i)
		if (descs[i].ref_len >= (1ull << 32) || descs[i].out_cap >= (1ull << 32) + (1ull << 31))
			return set_err(ctx, DG_ERR_TOO_LARGE, "stream %u exceeds the u32 format", i);
	hipSetDevice(ctx->device);
	auto* P = new (std::nothrow) dg_decode_plan_t();
	if (!P) return DG_ERR_NOMEM;
	P->ctx = ctx;
	P->n = n;
	P->ignore_hash = ignore_hash;
	for (uint32_t i = 0; i < n; ++i) {
		P->ref_end = std::max(P->ref_end, descs[i].ref_off + descs[i].ref_len);
		P->delta_end = std::max(P->delta_end, descs[i].delta_off + descs[i].delta_len);
		P->out_end = std::max(P->out_end, descs[i].out_off + descs[i].out_cap);
		if (descs[i].ref_len) P->iv_ref.push_back({descs[i].ref_off, descs[i].ref_off + descs[i].ref_len});
		if (descs[i].delta_len) P->iv_delta.push_back({descs[i].delta_off, descs[i].delta_off + descs[i].delta_len});
		if (descs[i].out_cap) P->iv_out.push_back({descs[i].out_off, descs[i].out_off + descs[i].out_cap});
	}
	for (auto* iv : {&P->iv_ref, &P->iv_delta, &P->iv_out}) {
		std::sort(iv->begin(), iv->end());
		size_t k = 0;
		for (const auto& x : *iv) {
			if (k && x.first <= (*iv)[k - 1].second) (*iv)[k - 1].second = std::max((*iv)[k - 1].second, x.second);
			else (*iv)[k++] = x;
		}
		iv->resize(k);
	}
	const size_t nn = std::max<size_t>(n, 1);
	if (P->d_desc.alloc(sizeof(dg_decode_desc_t) * nn)) {
		dg_decode_plan_destroy(P);
		return set_err(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	hipStream_t st = ctx->stream;
	hipError_t e = hipSuccess;
	if (n) e = hipMemcpyAsync(P->d_desc.p, descs, sizeof(dg_decode_desc_t) * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		dg_decode_plan_destroy(P);
		return set_err(ctx, DG_ERR_HIP, "decode plan setup failed: %s", hipGetErrorString(e));
	}
	*out = P;
	return DG_OK;
}

int dg_decode_plan_set_timing(dg_decode_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(P->ctx->device);
	if (!P->ring.set((uint32_t)slots, kDecEvents)) return set_err(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// one stage, "decode": the kernel parses, applies and checks both CRCs
int dg_decode_plan_stage_times(dg_decode_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[] = {"decode", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, std::min(n, 1)) : 0;
}

int dg_decode_plan_set_timing_every(dg_decode_plan_t* P, int every) {
	if (!P || every < 1) return DG_ERR_INVALID_ARG;
	P->ring.set_every((uint32_t)every);
	return DG_OK;
}

int dg_decode_plan_run(dg_decode_plan_t* P, const uint8_t* d_ref, const uint8_t* d_delta,
                       uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (P->n == 0) return DG_OK;
	if (!d_ref || !d_delta || !d_out || !d_out_len || !d_status)
		return set_err(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (((uintptr_t)d_ref & 15) || ((uintptr_t)d_out & 15))
		return set_err(ctx, DG_ERR_INVALID_ARG, "arena base pointers must be 16-byte aligned");
	{
		// the kernel writes the output image before it reads R for the source
		// CRC, and reads the delta while it writes: an output arena that
		// overlaps the reference or delta bytes of the batch is rejected
		auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
			const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
			return na && nb && x < y + nb && y < x + na;
		};
		// the exact test (only when the extents overlap): the merged output
		// intervals against the merged reference / delta intervals, one sweep
		auto named_overlap = [&](const void* b, const std::vector<std::pair<uint64_t, uint64_t>>& ivb) {
			const uintptr_t xo = (uintptr_t)d_out, xb = (uintptr_t)b;
			size_t i = 0, j = 0;
			while (i < P->iv_out.size() && j < ivb.size()) {
				const uintptr_t a0 = xo + P->iv_out[i].first, a1 = xo + P->iv_out[i].second;
				const uintptr_t b0 = xb + ivb[j].first, b1 = xb + ivb[j].second;
				if (a0 < b1 && b0 < a1) return true;
				if (a1 <= b1) ++i;
				else ++j;
			}
			return false;
		};
		if ((overlap(d_out, P->out_end, d_ref, P->ref_end) && named_overlap(d_ref, P->iv_ref)) ||
		    (overlap(d_out, P->out_end, d_delta, P->delta_end) && named_overlap(d_delta, P->iv_delta)))
			return set_err(ctx, DG_ERR_INVALID_ARG, "the output bytes overlap the reference or delta bytes");
	}
	hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
	hipEvent_t* const ev = P->ring.next();
	const bool check = !P->ignore_hash;
	// parse + apply (encoding.c:111-178, apply.c:229-284), then the CRC-64/XZ
	// of R and of the output, checked against the header in the same kernel
	// (main.c:341-356, :376-385); --ignore-hash skips the CRCs.  Two events
	// around the one launch (each event costs the stream ~3.5 us: the three
	// empty stages the round-4 layout also recorded cost C5 ~8 %)
	if (ev) HIPCHK(ctx, hipEventRecord(ev[0], st));
	DecodeArgs a{};
	a.ref = d_ref;
	a.delta = d_delta;
	a.descs = P->d_desc.as<dg_decode_desc_dev>();
	a.n = P->n;
	a.out = d_out;
	a.out_len = d_out_len;
	a.status = d_status;
	a.tables = ctx->d_crc_tables;
	a.crc_check = check ? 1u : 0u;
	HIPCHK(ctx, launch_decode(a, st));
	if (ev) HIPCHK(ctx, hipEventRecord(ev[1], st));
	return DG_OK;
}

void dg_decode_plan_destroy(dg_decode_plan_t* P) { plan_destroy(P); }

}  // extern "C"
