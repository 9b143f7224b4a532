// dg_index_host.cpp — host side of the read plan's chunked index pass
// (dg_read_plan_chunk_index, dg_read_plan_index_chunked, dg_read_plan_index_get)
// and of the decode built on it (dg_tile_requests, dg_decode_large;
// include/delta_gpu.h).
//
// The kernels are the stand-alone code object dg_index.hsaco (load_kernels,
// dg_hostutil.h).  A pass is four launches on one stream: map (a block per
// chunk), resolve (a wave per stream), fill (a block per chunk), finish (a
// wave per stream).  The plan's index memory and stream table are
// dg_read_host.cpp's (dg_read_plan.h).
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
#include "dg_index_dev.h"
#include "dg_read_plan.h"

using namespace dg;
using namespace dgrd;
using namespace dgix;

static const char* const kIxKernels[] = {"dg_index_map_kernel", "dg_index_resolve_kernel", "dg_index_fill_kernel",
                                         "dg_index_finish_kernel"};
enum { kIxMap = 0, kIxResolve = 1, kIxFill = 2, kIxFinish = 3, kIxKernelCount = 4 };

static_assert(kIxChunkDefault == DG_CHUNK_BYTES_DEFAULT, "the header states the default");

constexpr int kIxEvents = 4;   // before map, after map, after resolve, after fill and finish

namespace {

struct IxState {
	const hipFunction_t* fn = nullptr;   // kIxKernels
	uint32_t chunk_bytes = 0, n_chunks = 0;
	DevBuf d_exit, d_exit_off, d_chunk_base, d_chunks, d_sstate;
	TimingRing ring;
};

void ix_release(void* p) { delete static_cast<IxState*>(p); }

IxState* ix_state(dg_read_plan_t* P) { return static_cast<IxState*>(*read_plan_ext(P, ix_release)); }

uint64_t rd_be64(const uint8_t* p) {
	uint64_t v = 0;
	for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
	return v;
}

}  // namespace

extern "C" {

int dg_read_plan_chunk_index(dg_read_plan_t* P, uint32_t chunk_bytes) {
	if (!P) return DG_ERR_INVALID_ARG;
	const ReadPlanView v = read_plan_view(P);
	dg_context_t* ctx = v.ctx;
	if (ix_state(P)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: dg_read_plan_chunk_index is called once per plan");
	if (chunk_bytes == 0) chunk_bytes = kIxChunkDefault;
	if (chunk_bytes < kIxWin || chunk_bytes % kIxWin)
		return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: chunk_bytes is a multiple of 4096, or 0 for the default");
	std::vector<uint64_t> xoff((size_t)v.n + 1, 0);
	std::vector<uint32_t> cbase((size_t)v.n + 1, 0);
	uint64_t nch = 0;
	char msg[160];
	for (uint32_t i = 0; i < v.n; ++i) {
		const uint64_t dl = v.streams[i].delta_len;
		if (dl > kIxMaxStream) {
			snprintf(msg, sizeof msg, "read plan: stream %u: the chunked index takes streams of at most 4 GiB - 16 bytes", i);
			return ctx_fail(ctx, DG_ERR_TOO_LARGE, msg);
		}
		xoff[i + 1] = xoff[i] + dl;
		nch += std::max<uint64_t>(1, (dl + chunk_bytes - 1) / chunk_bytes);
		if (nch > 0x7FFFFFFFull) return ctx_fail(ctx, DG_ERR_TOO_LARGE, "read plan: more chunks than one launch takes");
		cbase[i + 1] = (uint32_t)nch;
	}
	std::vector<IxChunk> chunks((size_t)nch);
	for (uint32_t i = 0; i < v.n; ++i)
		for (uint32_t g = cbase[i]; g < cbase[i + 1]; ++g) chunks[g] = IxChunk{i, 0, 0, 0, 0, 0};
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	const hipFunction_t* fn = nullptr;
	int rc = load_kernels(ctx, kCtxModIndex, "dg_index.hsaco", "chunked index kernels", kIxKernels, kIxKernelCount, &fn);
	if (rc) return rc;
	auto* S = new (std::nothrow) IxState();
	if (!S) return DG_ERR_NOMEM;
	S->fn = fn;
	S->chunk_bytes = chunk_bytes;
	S->n_chunks = (uint32_t)nch;
	if (S->d_exit.alloc_nonnull(4 * xoff[v.n]) || S->d_exit_off.alloc_nonnull(8ull * (v.n + 1)) ||
	    S->d_chunk_base.alloc_nonnull(4ull * (v.n + 1)) || S->d_chunks.alloc_nonnull(sizeof(IxChunk) * nch) ||
	    S->d_sstate.alloc_nonnull(sizeof(IxStream) * (uint64_t)v.n)) {
		(void)hipGetLastError();
		delete S;
		return ctx_fail(ctx, DG_ERR_NOMEM, "read plan: device allocation of the chunked index's work memory failed");
	}
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	hipError_t e = hipMemcpyAsync(S->d_exit_off.p, xoff.data(), 8ull * (v.n + 1), hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(S->d_chunk_base.p, cbase.data(), 4ull * (v.n + 1), hipMemcpyHostToDevice, st);
	if (e == hipSuccess && nch) e = hipMemcpyAsync(S->d_chunks.p, chunks.data(), sizeof(IxChunk) * nch, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) {
		delete S;
		return ctx_fail(ctx, DG_ERR_HIP, "read plan: upload of the chunk table failed");
	}
	*read_plan_ext(P, ix_release) = S;
	return DG_OK;
}

int dg_read_plan_index_chunked(dg_read_plan_t* P, const uint8_t* d_delta, const uint64_t* d_delta_offsets,
                               const int32_t* d_delta_status, int32_t* d_stream_status, void* stream) {
	if (!P) return DG_ERR_INVALID_ARG;
	const ReadPlanView v = read_plan_view(P);
	dg_context_t* ctx = v.ctx;
	IxState* S = ix_state(P);
	if (!S) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: dg_read_plan_chunk_index has not run");
	if (v.n == 0) return DG_OK;
	if (!d_delta) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "null device buffer");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)dg_context_stream(ctx);
	IxArgs a{};
	a.delta = d_delta;
	a.streams = v.d_streams;
	a.delta_offsets = d_delta_offsets;
	a.delta_status = d_delta_status;
	a.stream_status = d_stream_status;
	a.index = v.d_index;
	a.index_off = v.d_index_off;
	a.exit = S->d_exit.as<uint32_t>();
	a.exit_off = S->d_exit_off.as<uint64_t>();
	a.chunk_base = S->d_chunk_base.as<uint32_t>();
	a.chunks = S->d_chunks.as<IxChunk>();
	a.sstate = S->d_sstate.as<IxStream>();
	a.n = v.n;
	a.n_chunks = S->n_chunks;
	a.chunk_bytes = S->chunk_bytes;
	void* params[] = {&a};
	hipEvent_t* ev = S->ring.next();
	hipError_t e;
	static const struct {
		int k;
		bool per_chunk;
		uint32_t block;
		int event_after;   // or 0
	} kStages[] = {{kIxMap, true, kRdBlock, 1}, {kIxResolve, false, 64, 2}, {kIxFill, true, kRdBlock, 0}, {kIxFinish, false, 64, 3}};
	if (ev && (e = hipEventRecord(ev[0], st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
	for (const auto& sg : kStages) {
		const uint32_t grid = sg.per_chunk ? S->n_chunks : v.n;
		if ((e = hipModuleLaunchKernel(S->fn[sg.k], grid, 1, 1, sg.block, 1, 1, 0, st, params, nullptr)) != hipSuccess)
			return hip_fail(ctx, (std::string("launch of ") + kIxKernels[sg.k]).c_str(), e);
		if (ev && sg.event_after && (e = hipEventRecord(ev[sg.event_after], st)) != hipSuccess)
			return hip_fail(ctx, "hipEventRecord", e);
	}
	read_plan_set_indexed(P);
	return DG_OK;
}

int dg_read_plan_index_set_timing(dg_read_plan_t* P, int slots) {
	if (!P || slots < 0) return DG_ERR_INVALID_ARG;
	const ReadPlanView v = read_plan_view(P);
	IxState* S = ix_state(P);
	if (!S) return ctx_fail(v.ctx, DG_ERR_INVALID_ARG, "read plan: dg_read_plan_chunk_index has not run");
	hipSetDevice(ctx_device(v.ctx));
	if (!S->ring.set((uint32_t)slots, kIxEvents)) return ctx_fail(v.ctx, DG_ERR_HIP, "hipEventCreate failed");
	return DG_OK;
}

// "map", "resolve", "fill" (with the finish launch), "total"
int dg_read_plan_index_stage_times(dg_read_plan_t* P, float* ms, const char** names, int n) {
	static const char* const kNames[kIxEvents] = {"map", "resolve", "fill", "total"};
	IxState* S = P ? ix_state(P) : nullptr;
	return S ? S->ring.stage_times(kNames, ms, names, n) : 0;
}

int dg_read_plan_index_get(dg_read_plan_t* P, uint32_t stream_i, void* host_dst, uint64_t cap, uint64_t* bytes) {
	if (!P || !bytes) return DG_ERR_INVALID_ARG;
	*bytes = 0;
	const ReadPlanView v = read_plan_view(P);
	dg_context_t* ctx = v.ctx;
	if (stream_i >= v.n) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: no such stream");
	if (!read_plan_indexed(P)) return ctx_fail(ctx, DG_ERR_INVALID_ARG, "read plan: no index pass has run");
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	const uint8_t* src = v.d_index + v.index_off[stream_i];
	RdHead h;
	if (hipStreamSynchronize(st) != hipSuccess ||
	    hipMemcpyAsync(&h, src, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "read plan: download of the index failed");
	const uint64_t room = (v.index_off[stream_i + 1] - v.index_off[stream_i] - sizeof(RdHead)) / sizeof(RdEnt);
	const uint64_t n_ent = h.status ? 0 : std::min<uint64_t>(h.n_ent, room);   // a failed stream's entries are unspecified
	*bytes = sizeof(RdHead) + sizeof(RdEnt) * n_ent;
	if (cap < *bytes || !host_dst) return ctx_fail(ctx, DG_ERR_CAPACITY, "read plan: the index of the stream needs more room");
	memcpy(host_dst, &h, sizeof h);
	if (n_ent && (hipMemcpyAsync((uint8_t*)host_dst + sizeof h, src + sizeof h, sizeof(RdEnt) * n_ent, hipMemcpyDeviceToHost,
	                             st) != hipSuccess ||
	              hipStreamSynchronize(st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "read plan: download of the index failed");
	return DG_OK;
}

int dg_tile_requests(uint32_t version_size, uint32_t tile_bytes, dg_read_req_t* reqs, uint32_t cap, uint32_t* n) {
	if (!n) return DG_ERR_INVALID_ARG;
	if (tile_bytes == 0) tile_bytes = DG_TILE_BYTES_DEFAULT;
	const uint64_t need = ((uint64_t)version_size + tile_bytes - 1) / tile_bytes;
	*n = (uint32_t)need;
	if (need > cap) return DG_ERR_CAPACITY;
	if (need && !reqs) return DG_ERR_INVALID_ARG;
	for (uint64_t t = 0; t < need; ++t) {
		const uint64_t off = t * tile_bytes;
		reqs[t] = dg_read_req_t{0, (uint32_t)off, (uint32_t)std::min<uint64_t>(tile_bytes, version_size - off), 0, off};
	}
	return DG_OK;
}

int dg_decode_large(dg_context_t* ctx, const uint8_t* r, size_t r_len, const uint8_t* delta, size_t delta_len,
                    int ignore_hash, uint32_t chunk_bytes, uint32_t tile_bytes, dg_buffer_t* out) {
	if (!ctx || !out || (r_len && !r) || (delta_len && !delta)) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	if (delta_len < DG_HEADER_SIZE || memcmp(delta, "DLT\x03", 4) != 0) return DG_ERR_MALFORMED;
	// the in-place replay reads the buffer it rewrites; 4 GiB or more does not fit the read plan
	if ((delta[4] & 1) || r_len >= (1ull << 32) || delta_len > kIxMaxStream)
		return dg_decode(ctx, r, r_len, delta, delta_len, ignore_hash, out);
	const uint32_t vsize = (uint32_t)(rd_be64(delta + 5) >> 32);
	uint32_t n_req = 0;
	(void)dg_tile_requests(vsize, tile_bytes, nullptr, 0, &n_req);   // the count
	std::vector<dg_read_req_t> reqs;
	try {
		reqs.resize(n_req);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	int rc = dg_tile_requests(vsize, tile_bytes, reqs.data(), n_req, &n_req);
	if (rc) return rc;
	if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return ctx_fail(ctx, DG_ERR_HIP, "hipSetDevice failed");
	hipStream_t st = (hipStream_t)dg_context_stream(ctx);
	const dg_read_stream_t sd{0, r_len, 0, delta_len};
	dg_read_plan_t* plan = nullptr;
	if ((rc = dg_read_plan_create(ctx, &sd, 1, std::max<uint32_t>(n_req, 1), &plan)) != DG_OK) return rc;
	ScopeExit guard([&] { dg_read_plan_destroy(plan); });
	if ((rc = dg_read_plan_chunk_index(plan, chunk_bytes)) != DG_OK) return rc;
	const uint64_t cap = std::max<uint64_t>(vsize, r_len);   // (what dg_decode gives the one-block decode)
	DevBuf d_r, d_d, d_o, d_req, d_len, d_st, d_crc, d_olen;
	if (d_r.alloc_nonnull(r_len) || d_d.alloc_nonnull(delta_len) || d_o.alloc_nonnull(cap) ||
	    d_req.alloc_nonnull(sizeof(dg_read_req_t) * n_req) || d_len.alloc_nonnull(4ull * n_req) ||
	    d_st.alloc_nonnull(4ull * n_req) || d_crc.alloc_nonnull(16) || d_olen.alloc_nonnull(8)) {
		(void)hipGetLastError();
		return ctx_fail(ctx, DG_ERR_NOMEM, "device allocation failed");
	}
	if ((r_len && hipMemcpyAsync(d_r.p, r, r_len, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemcpyAsync(d_d.p, delta, delta_len, hipMemcpyHostToDevice, st) != hipSuccess ||
	    (n_req && hipMemcpyAsync(d_req.p, reqs.data(), sizeof(dg_read_req_t) * n_req, hipMemcpyHostToDevice, st) != hipSuccess))
		return ctx_fail(ctx, DG_ERR_HIP, "upload failed");
	if ((rc = dg_read_plan_index_chunked(plan, d_d.as<uint8_t>(), nullptr, nullptr, nullptr, st)) != DG_OK) return rc;
	// the stream's head (the first 32 bytes of its index): its status, and whether its commands tile V in order
	RdHead h;
	if (hipMemcpyAsync(&h, read_plan_view(plan).d_index, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess)
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	if (h.status) return DG_ERR_MALFORMED;
	int32_t s = DG_OK;
	if (!(h.flags & kRdSeq)) {
		// commands out of order, overlapping or with gaps: the read kernel would
		// replay the whole stream once per tile, so the one-block decode takes it
		const dg_decode_desc_t desc{0, r_len, 0, delta_len, 0, cap};
		rc = dg_decode_batch_device(ctx, d_r.as<uint8_t>(), d_d.as<uint8_t>(), &desc, 1, ignore_hash, d_o.as<uint8_t>(),
		                            d_olen.as<uint64_t>(), d_st.as<int32_t>(), st);
		if (rc) return rc;
		if (hipMemcpyAsync(&s, d_st.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
			return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	} else {
		if ((rc = dg_read_plan_run(plan, d_r.as<uint8_t>(), d_d.as<uint8_t>(), d_req.as<dg_read_req_t>(), n_req,
		                           d_o.as<uint8_t>(), d_len.as<uint32_t>(), d_st.as<int32_t>(), st)) != DG_OK)
			return rc;
		uint64_t crc[2] = {0, 0};
		if (!ignore_hash) {
			const dg_span_t all_r{0, r_len}, all_v{0, vsize};
			if ((rc = dg_crc64_xz_batch_device(ctx, d_r.as<uint8_t>(), &all_r, 1, d_crc.as<uint64_t>(), st)) != DG_OK) return rc;
			if ((rc = dg_crc64_xz_batch_device(ctx, d_o.as<uint8_t>(), &all_v, 1, d_crc.as<uint64_t>() + 1, st)) != DG_OK)
				return rc;
		}
		std::vector<int32_t> stv(n_req);
		if ((n_req && hipMemcpyAsync(stv.data(), d_st.p, 4ull * n_req, hipMemcpyDeviceToHost, st) != hipSuccess) ||
		    (!ignore_hash && hipMemcpyAsync(crc, d_crc.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess) ||
		    hipStreamSynchronize(st) != hipSuccess)
			return ctx_fail(ctx, DG_ERR_HIP, "download failed");
		for (uint32_t j = 0; j < n_req; ++j)
			if (stv[j]) return ctx_fail(ctx, DG_ERR_INTERNAL, "dg_decode_large: a tile of an indexed stream was refused");
		if (!ignore_hash) {
			if (crc[0] != rd_be64(delta + 9)) s = DG_ERR_SRC_CRC;
			else if (crc[1] != rd_be64(delta + 17)) s = DG_ERR_DST_CRC;
		}
	}
	// a failed output CRC still hands back the output, as dg_decode does
	if (s && s != DG_ERR_DST_CRC) return s;
	uint8_t* buf = (uint8_t*)malloc(vsize ? vsize : 1);
	if (!buf) return DG_ERR_NOMEM;
	if (vsize && (hipMemcpyAsync(buf, d_o.p, vsize, hipMemcpyDeviceToHost, st) != hipSuccess ||
	              hipStreamSynchronize(st) != hipSuccess)) {
		free(buf);
		return ctx_fail(ctx, DG_ERR_HIP, "download failed");
	}
	out->data = buf;
	out->len = vsize;
	return s;
}

}  // extern "C"
