// dg_splice_host.cpp — host side of the device splice (dg_splice_plan_*,
// dg_splice_batch) and the large-pair encoder built on it (dg_encode_large;
// include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_splice.hsaco (load_kernels,
// dg_hostutil.h), launched with hipModuleLaunchKernel.  A run is map kernel ->
// resolve kernel -> the library's size scan -> emit kernel on one stream.  The
// sizing of a plan is splice_plan_geometry (dg_plan.cpp).
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
#include "dg_splice_dev.h"

using namespace dg;
using namespace dgsp;

static const char* const kSpKernels[] = {"dg_splice_map_kernel", "dg_splice_resolve_kernel", "dg_splice_emit_kernel"};
enum { kSpMap = 0, kSpResolve = 1, kSpEmit = 2, kSpKernelCount = 3 };

constexpr int kSpEvents = 5;   // before the map kernel, after it, after the resolve kernel, after the scan, after the emit kernel

struct dg_splice_plan {
	dg_context_t* ctx = nullptr;
	const hipFunction_t* fn = nullptr;   // kSpKernels
	uint32_t n_seg = 0, n_groups = 0;
	uint64_t bound = 0;
	DevBuf d_desc, d_groups, d_sums, d_recs, d_res, d_sizes;
	TimingRing ring;   // kSpEvents events per run
};

namespace {

// g, grc, gerr: what splice_plan_geometry returned
int plan_make(dg_context_t* ctx, const SpliceGeometry& g, int grc, const std::string& gerr, dg_splice_plan_t** out) {
	*out = nullptr;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	const hipFunction_t* fn = nullptr;
	int rc = load_kernels(ctx, kCtxModSplice, "dg_splice.hsaco", "splice kernels", kSpKernels, kSpKernelCount, &fn);
	if (rc) return rc;
	if (grc) return ctx_fail(ctx, grc, gerr.c_str());
	auto* P = new (std::nothrow) dg_splice_plan_t();
	if (!P) return DG_ERR_NOMEM;
	const uint32_t ns = (uint32_t)g.descs.size(), ng = (uint32_t)g.groups.size();
	P->ctx = ctx;
	P->fn = fn;
	P->n_seg = ns;
	P->n_groups = ng;
	P->bound = g.bound;
	const uint64_t s1 = std::max<uint32_t>(ns, 1), g1 = std::max<uint32_t>(ng, 1);
	if (P->d_desc.alloc_nonnull(sizeof(SpDesc) * s1) || P->d_groups.alloc_nonnull(sizeof(SpGroup) * g1) ||
	    P->d_sums.alloc_nonnull(sizeof(SpSum) * s1) || P->d_recs.alloc_nonnull(sizeof(SpRec) * s1) ||
	    P->d_res.alloc_nonnull(sizeof(SpRes) * g1) || P->d_sizes.alloc_nonnull(8 * g1)) {
		(void)hipGetLastError();
		delete P;
		return ctx_fail(ctx, DG_ERR_NOMEM, "splice plan: device allocation of the work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipSuccess;
	if (ns) e = hipMemcpyAsync(P->d_desc.p, g.descs.data(), sizeof(SpDesc) * ns, hipMemcpyHostToDevice, st);
	if (e == hipSuccess && ng) e = hipMemcpyAsync(P->d_groups.p, g.groups.data(), sizeof(SpGroup) * ng, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete P;
		return ctx_fail(ctx, DG_ERR_HIP, "splice plan: descriptor upload failed");
	}
	*out = P;
	return DG_OK;
}

}  // namespace

extern "C" {

int dg_splice_plan_create(dg_context_t* ctx, const dg_pair_t* segs, uint32_t n_seg, const dg_pair_t* wholes,
                          const uint32_t* seg_first, uint32_t n_groups, const uint64_t* seg_caps, dg_splice_plan_t** out) {
	if (!ctx || !out || !seg_first || (n_seg && !segs) || (n_groups && !wholes)) return DG_ERR_INVALID_ARG;
	SpliceGeometry g;
	std::string err;
	const int grc = splice_plan_geometry(segs, n_seg, wholes, seg_first, n_groups, seg_caps, g, err);
	return plan_make(ctx, g, grc, err, out);
}

int dg_splice_plan_create_for(dg_context_t* ctx, const dg_encode_plan_t* enc, const dg_pair_t* wholes,
                              const uint32_t* seg_first, uint32_t n_groups, dg_splice_plan_t** out) {
	if (!ctx || !enc || !out || !seg_first || (n_groups && !wholes)) return DG_ERR_INVALID_ARG;
	if (plan_ctx(enc) != ctx) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "the encode plan belongs to another context");
	const EncodePlanView e = encode_plan_view(enc);
	const uint32_t n = dg_encode_plan_num_pairs(enc);
	std::vector<uint64_t> caps(n);
	for (uint32_t j = 0; j < n; ++j) caps[j] = pair_out_bound(e.algo, e.p, e.pairs[j].v_len);
	SpliceGeometry g;
	std::string err;
	const int grc = splice_plan_geometry(e.pairs, n, wholes, seg_first, n_groups, caps.data(), g, err);
	return plan_make(ctx, g, grc, err, out);
}

uint64_t dg_splice_plan_output_bound(const dg_splice_plan_t* P) { return P ? P->bound : 0; }

int dg_splice_plan_set_timing(dg_splice_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	hipSetDevice(ctx_device(P->ctx));
	if (!P->ring.set((uint32_t)slots, kSpEvents)) return ctx_fail(P->ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

int dg_splice_plan_stage_times(dg_splice_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kSpEvents] = {"map", "resolve", "scan", "emit", "total"};
	return P ? P->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_splice_plan_run(dg_splice_plan_t* P, const uint8_t* d_deltas, const uint64_t* d_offsets, const int32_t* d_seg_status,
                       const uint64_t* d_src_crc, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets,
                       int32_t* d_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	dg_context_t* ctx = P->ctx;
	if (!d_out_offsets) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	if (P->n_groups == 0) {
		return hipMemsetAsync(d_out_offsets, 0, 8, st) == hipSuccess ? DG_OK : ctx_fail(ctx, DG_ERR_HIP, "hipMemsetAsync failed");
	}
	// (d_out may be NULL with out_cap == 0: the sizing run)
	if (!d_deltas || !d_offsets || !d_src_crc || !d_status || (!d_out && out_cap))
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipEvent_t* ev = P->ring.next();
	SpArgs a{};
	a.deltas = d_deltas;
	a.offsets = d_offsets;
	a.seg_status = d_seg_status;
	a.src_crc = d_src_crc;
	a.descs = P->d_desc.as<SpDesc>();
	a.groups = P->d_groups.as<SpGroup>();
	a.sums = P->d_sums.as<SpSum>();
	a.recs = P->d_recs.as<SpRec>();
	a.res = P->d_res.as<SpRes>();
	a.sizes = P->d_sizes.as<uint64_t>();
	a.status = d_status;
	a.out = d_out;
	a.out_cap = out_cap;
	a.out_offsets = d_out_offsets;
	a.n_seg = P->n_seg;
	a.n_groups = P->n_groups;
	void* params[] = {&a};
	hipError_t e;
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kSpMap], P->n_seg, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_splice_map_kernel", e);
	if (ev && (e = hipEventRecord(ev[1], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kSpResolve], P->n_groups, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_splice_resolve_kernel", e);
	if (ev && (e = hipEventRecord(ev[2], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = launch_scan(P->d_sizes.as<uint64_t>(), d_out_offsets, P->n_groups, st)) != hipSuccess)
		return hip_fail(ctx, "launch of the size scan", e);
	if (ev && (e = hipEventRecord(ev[3], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	if ((e = hipModuleLaunchKernel(P->fn[kSpEmit], P->n_seg, 1, 1, 64, 1, 1, 0, st, params, nullptr)) != hipSuccess)
		return hip_fail(ctx, "launch of dg_splice_emit_kernel", e);
	if (ev && (e = hipEventRecord(ev[4], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	return DG_OK;
}

void dg_splice_plan_destroy(dg_splice_plan_t* P) { plan_destroy(P); }

int dg_splice_batch(dg_context_t* ctx, const dg_pair_t* wholes, uint32_t n_groups, const dg_pair_t* segs,
                    const uint32_t* seg_first, const uint8_t* const* deltas, const size_t* delta_len,
                    const int32_t* seg_status, const uint8_t* src_crc, dg_buffer_t* outs, int32_t* status) {
	if (!ctx || (n_groups && (!wholes || !segs || !seg_first || !deltas || !delta_len || !src_crc || !outs)))
		return DG_ERR_INVALID_ARG;
	for (uint32_t i = 0; i < n_groups; ++i) outs[i].data = nullptr, outs[i].len = 0;
	if (n_groups == 0) return DG_OK;
	const uint32_t ns = seg_first[n_groups];
	std::vector<uint64_t> off((size_t)ns + 1), caps(ns), crc(n_groups), goff((size_t)n_groups + 1);
	uint64_t dt = 0;
	for (uint32_t j = 0; j < ns; ++j) {
		if (delta_len[j] && !deltas[j]) return DG_ERR_INVALID_ARG;
		off[j] = dt;
		caps[j] = delta_len[j];
		dt += delta_len[j];
	}
	off[ns] = dt;
	for (uint32_t i = 0; i < n_groups; ++i) {
		uint64_t c = 0;
		for (int k = 0; k < 8; ++k) c = (c << 8) | src_crc[8ull * i + k];
		crc[i] = c;
	}
	dg_splice_plan_t* plan = nullptr;
	int rc = dg_splice_plan_create(ctx, segs, ns, wholes, seg_first, n_groups, caps.data(), &plan);
	if (rc) return rc;
	ScopeExit guard([&] { dg_splice_plan_destroy(plan); });
	const uint64_t out_cap = dg_splice_plan_output_bound(plan);
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	DevBuf d_delta, d_off, d_sst, d_crc, d_out, d_goff, d_st;
	std::vector<uint8_t> h_in, h_out;
	std::vector<int32_t> stv(n_groups);
	try {
		h_in.resize(dt);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	for (uint32_t j = 0; j < ns; ++j)
		if (delta_len[j]) memcpy(h_in.data() + off[j], deltas[j], delta_len[j]);
	if (d_delta.alloc_nonnull(dt) || d_off.alloc_nonnull(8ull * (ns + 1)) || d_sst.alloc_nonnull(4ull * ns) ||
	    d_crc.alloc_nonnull(8ull * n_groups) || d_out.alloc_nonnull(out_cap) || d_goff.alloc_nonnull(8ull * (n_groups + 1)) ||
	    d_st.alloc_nonnull(4ull * n_groups)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((dt && hipMemcpyAsync(d_delta.p, h_in.data(), dt, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemcpyAsync(d_off.p, off.data(), 8ull * (ns + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
	    (seg_status && ns && hipMemcpyAsync(d_sst.p, seg_status, 4ull * ns, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemcpyAsync(d_crc.p, crc.data(), 8ull * n_groups, hipMemcpyHostToDevice, st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	rc = dg_splice_plan_run(plan, d_delta.as<uint8_t>(), d_off.as<uint64_t>(), seg_status ? d_sst.as<int32_t>() : nullptr,
	                        d_crc.as<uint64_t>(), d_out.as<uint8_t>(), out_cap, d_goff.as<uint64_t>(), d_st.as<int32_t>(), st);
	if (rc) return rc;
	if (hipMemcpyAsync(goff.data(), d_goff.p, 8ull * (n_groups + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(stv.data(), d_st.p, 4ull * n_groups, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	const uint64_t total = std::min<uint64_t>(goff[n_groups], out_cap);
	try {
		h_out.resize(total);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	if (total && (hipMemcpyAsync(h_out.data(), d_out.p, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
	              hipStreamSynchronize(st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	BatchStatus bs{status};
	for (uint32_t i = 0; i < n_groups; ++i) {
		const int32_t s = stv[i];
		if (s == DG_OK && !buffer_copy(&outs[i], h_out.data() + goff[i], goff[i + 1] - goff[i])) return DG_ERR_NOMEM;
		bs.set(i, s);
	}
	return bs.result();
}

int dg_encode_large(dg_context_t* ctx, dg_algorithm_t algo, const uint8_t* r, size_t r_len, const uint8_t* v, size_t v_len,
                    const dg_diff_options_t* opts, uint64_t seg_bytes, uint64_t window_bytes, dg_buffer_t* out) {
	if (!ctx || !out || (r_len && !r) || (v_len && !v)) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	dg_diff_options_t o;
	if (opts) o = *opts;
	else dg_diff_options_default(&o);
	// DG_OPT_INPLACE: the spliced delta is converted on the host, as dg_encode's is
	const bool inplace = (o.flags >> DG_OPT_INPLACE) & 1;
	const int policy = ((o.flags >> DG_OPT_POLICY_CONSTANT) & 1) ? DG_POLICY_CONSTANT : DG_POLICY_LOCALMIN;
	o.flags &= ~((1ull << DG_OPT_INPLACE) | (1ull << DG_OPT_POLICY_CONSTANT) | (1ull << DG_OPT_VERBOSE));
	const dg_pair_t whole{0, r_len, 0, v_len};
	uint32_t first[2] = {0, 0};
	int rc = dg_segment_pairs(&whole, 1, seg_bytes, window_bytes, nullptr, 0, first);
	if (rc) return ctx_fail(ctx, rc, "dg_encode_large: segment and window sizes are multiples of 16, the pair below 4 GiB - 1 MiB");
	std::vector<dg_pair_t> segs(first[1]);
	if ((rc = dg_segment_pairs(&whole, 1, seg_bytes, window_bytes, segs.data(), segs.size(), first)) != DG_OK) return rc;
	const uint32_t ns = first[1];
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	dg_encode_plan_t* enc = nullptr;
	dg_splice_plan_t* sp = nullptr;
	ScopeExit guard([&] {
		dg_splice_plan_destroy(sp);
		dg_encode_plan_destroy(enc);
	});
	if ((rc = dg_encode_plan_create(ctx, algo, segs.data(), ns, &o, &enc)) != DG_OK) return rc;
	if ((rc = dg_splice_plan_create_for(ctx, enc, &whole, first, 1, &sp)) != DG_OK) return rc;
	const uint64_t enc_cap = dg_encode_plan_output_bound(enc), out_cap = dg_splice_plan_output_bound(sp);
	DevBuf d_ref, d_ver, d_seg, d_soff, d_sst, d_crc, d_out, d_goff, d_st;
	if (d_ref.alloc_nonnull(r_len) || d_ver.alloc_nonnull(v_len) || d_seg.alloc_nonnull(enc_cap) ||
	    d_soff.alloc_nonnull(8ull * (ns + 1)) || d_sst.alloc_nonnull(4ull * ns) || d_crc.alloc_nonnull(8) ||
	    d_out.alloc_nonnull(out_cap) || d_goff.alloc_nonnull(16) || d_st.alloc_nonnull(4)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((r_len && hipMemcpyAsync(d_ref.p, r, r_len, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (v_len && hipMemcpyAsync(d_ver.p, v, v_len, hipMemcpyHostToDevice, st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	const dg_span_t all_r{0, r_len};
	if ((rc = dg_crc64_xz_batch_device(ctx, d_ref.as<uint8_t>(), &all_r, 1, d_crc.as<uint64_t>(), st)) != DG_OK) return rc;
	if ((rc = dg_encode_plan_run(enc, d_ref.as<uint8_t>(), d_ver.as<uint8_t>(), d_seg.as<uint8_t>(), enc_cap,
	                             d_soff.as<uint64_t>(), d_sst.as<int32_t>(), st)) != DG_OK)
		return rc;
	if ((rc = dg_splice_plan_run(sp, d_seg.as<uint8_t>(), d_soff.as<uint64_t>(), d_sst.as<int32_t>(), d_crc.as<uint64_t>(),
	                             d_out.as<uint8_t>(), out_cap, d_goff.as<uint64_t>(), d_st.as<int32_t>(), st)) != DG_OK)
		return rc;
	uint64_t goff[2] = {0, 0};
	int32_t gst = 0;
	if (hipMemcpyAsync(goff, d_goff.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipMemcpyAsync(&gst, d_st.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	if (gst) return ctx_fail(ctx, gst, "dg_encode_large: the pair's splice failed");
	const uint64_t n = goff[1] - goff[0];
	uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
	if (!buf) return DG_ERR_NOMEM;
	if (hipMemcpyAsync(buf, d_out.as<uint8_t>() + goff[0], n, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) {
		free(buf);
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	}
	if (inplace) {
		dg_buffer_t ip{nullptr, 0};
		rc = dg_make_inplace(r, r_len, buf, n, policy, &ip, nullptr);
		free(buf);
		if (rc) return rc;
		*out = ip;
		return DG_OK;
	}
	out->data = buf;
	out->len = n;
	return DG_OK;
}

}  // extern "C"
