// dg_index_dev.hip — the chunked index pass of the read plan
// (dg_read_plan_index_chunked), built as the stand-alone gfx950 code object
// lib/dg_index.hsaco.  It leaves the index dg_read_index_kernel
// (dg_read_dev.hip) leaves, with one stream parsed by many blocks.
//
// A stream cannot be entered in the middle on trust: an ADD payload may hold
// bytes that look like commands.  So every offset is treated as a possible
// entry.  Per chunk of the stream (dg_index_dev.h):
//
//   dg_index_map_kernel      one 256-thread block per chunk, the windows of the
//      chunk from last to first: for every offset x of the window the offset of
//      the next command IF a command started at x (dg_parse_chain.h's N1, here
//      judged against the stream's end only: the window is loaded with the
//      bytes after it, so a header that straddles a window or chunk edge is
//      decoded whole), composed by pointer doubling in LDS until every offset
//      has left the window; exit[x] is then the window exit when that is at or
//      past the chunk's end, else the exit already stored for that later offset
//      of the same chunk.  Only framing is judged.
//   dg_index_resolve_kernel  one wave per stream walks the chunks: the entry of
//      chunk 0 is 25, the entry of chunk k + 1 is exit[entry of k]; a chunk the
//      chain jumps over (inside a long payload) inherits the entry.  One
//      dependent load per chunk.
//   dg_index_fill_kernel     one block per chunk: the walk dg_read_index_kernel
//      runs (rd_index_walk, dg_read_walk_dev.h), from the chunk's true entry:
//      the real window step (dec_window, dg_decode_dev.h, bounds checks
//      included) until a command at or after the chunk's end has been seen;
//      the block writes exactly the index entries whose stride offsets lie in
//      its chunk and leaves what the sequential flag needs of the commands that
//      start in the chunk.
//   dg_index_finish_kernel   one wave per stream: status, the sequential flag
//      from chaining the chunk records, the head.
//
// The stages are separate launches on one stream; kernel boundaries are the
// only hand-off between blocks.  The one in-kernel hand-off is inside a block:
// the map kernel reads exit words its own earlier windows stored, behind
// block_sync_global.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_decode_dev.h"
#include "dg_index_dev.h"
#include "dg_read_dev.h"
#include "dg_read_walk_dev.h"

using namespace dg;
using namespace dgrd;
using namespace dgix;

namespace {

static_assert(kIxWin == kDecWin, "the map kernel's windows are the window step's");
static_assert(kIxWin % kRdStride == 0, "strides do not straddle chunks");
// doubling rounds until a window's longest chain (a command is 9 bytes or more) has left it
constexpr uint32_t kIxRounds = 9;
static_assert((1u << kIxRounds) >= kIxWin / 9 + 1, "2^rounds commands cover a window");
constexpr uint16_t kMEnd = 0xFFFE, kMBad = 0xFFFD, kMSpecial = 0xFFFD;   // codes of the LDS map (window offsets are < 4096)

struct IxEarly {
	uint64_t doff, dl;
	uint32_t vsize;
	int32_t st;
};

// the statuses dg_read_index_kernel takes before it parses, in its order
__device__ __forceinline__ IxEarly ix_early(const IxArgs& a, uint32_t i) {
	const RdStream sd = a.streams[i];
	IxEarly e{sd.delta_off, sd.delta_len, 0, a.delta_status ? a.delta_status[i] : 0};
	if (!e.st && a.delta_offsets) {
		e.doff = a.delta_offsets[i];
		e.dl = a.delta_offsets[i + 1] - e.doff;
		if (e.dl > sd.delta_len) e.st = 7;   // longer than the plan allowed for
	}
	const uint8_t* D = a.delta + e.doff;
	if (!e.st && bad_magic(D, e.dl)) e.st = 8;
	if (!e.st && (D[4] & 1)) e.st = 2;
	if (!e.st) e.vsize = be32(D + 5);
	return e;
}

// the chunk of block g: its stream and its number in the stream
__device__ __forceinline__ void ix_chunk_of(const IxArgs& a, uint32_t g, uint32_t& i, uint32_t& k) {
	i = a.chunks[g].stream;
	k = g - a.chunk_base[i];
}

}  // namespace

extern "C" __global__ __launch_bounds__(kRdBlock) void dg_index_map_kernel(IxArgs a) {
	const uint32_t g = blockIdx.x;
	if (g >= a.n_chunks) return;
	uint32_t i, k;
	ix_chunk_of(a, g, i, k);
	const IxEarly e = ix_early(a, i);
	const uint64_t c0 = (uint64_t)k * a.chunk_bytes;
	if (e.st || c0 >= e.dl) return;   // (blocks past the real length leave at once)
	const uint32_t tid = threadIdx.x;
	__shared__ __attribute__((aligned(16))) uint8_t win[kIxWin + 32];
	__shared__ __attribute__((aligned(16))) uint16_t MA[kIxWin];
	__shared__ __attribute__((aligned(16))) uint16_t MB[kIxWin];
	__shared__ uint32_t far[kIxWin];   // where the command at x ends, when that is outside the window

	const uint8_t* D = a.delta + e.doff;
	const uint64_t dl = e.dl;
	const uint64_t c1 = min(c0 + a.chunk_bytes, dl);
	uint32_t* X = a.exit + a.exit_off[i];
	const uint32_t nwin = (uint32_t)((c1 - c0 + kIxWin - 1) / kIxWin);
	for (uint32_t j = nwin; j-- > 0;) {
		const uint64_t ws = c0 + (uint64_t)j * kIxWin;
		const uint32_t avail = (uint32_t)min((uint64_t)kIxWin, dl - ws);
		const uint8_t* w = win + dec_load_window(win, D, dl, ws);
		__syncthreads();
		// N1 with the window's last command as a fixed point: M[x] = x when the
		// command at x ends at or past the window's end (far[x] says where)
		{
			const uint32_t x0 = 16 * tid;
			constexpr uint32_t bb = (uint32_t)kMBad | ((uint32_t)kMBad << 16);
			uint4* dst = reinterpret_cast<uint4*>(MA + x0);
			dst[0] = make_uint4(bb, bb, bb, bb);
			dst[1] = make_uint4(bb, bb, bb, bb);
			uint32_t d[4];
			win16(w + x0, d);
			uint32_t cand = 0;
#pragma unroll
			for (uint32_t q = 0; q < 16; ++q) cand |= (((d[q >> 2] >> (8 * (q & 3))) & 0xFFu) <= 2u ? 1u : 0u) << q;
			const uint32_t lim = avail > x0 ? umin32(avail - x0, 16u) : 0u;
			cand &= (1u << lim) - 1u;
			for (; cand; cand &= cand - 1) {
				const uint32_t x = x0 + (uint32_t)__builtin_ctz(cand);
				const uint32_t t = w[x];
				uint32_t nx = kMEnd;
				if (t != 0) {
					const uint32_t hdr = t == 1 ? 13u : 9u;
					nx = kMBad;
					if (ws + x + hdr <= dl) {   // (the only cut header is one that crosses the stream's end)
						const uint64_t len = t == 1 ? 0 : be32(w + x + 5);
						const uint64_t end = (uint64_t)x + hdr + len;
						if (ws + end <= dl) {
							if (end >= avail) {
								nx = x;
								far[x] = (uint32_t)(ws + end);
							} else {
								nx = (uint32_t)end;
							}
						}
					}
				}
				MA[x] = (uint16_t)nx;
			}
		}
		__syncthreads();
		uint16_t *src = MA, *dstM = MB;
		for (uint32_t r = 0; r < kIxRounds; ++r) {
			const uint32_t x0 = 16 * tid;
			const uint4* sp = reinterpret_cast<const uint4*>(src + x0);
			const uint4 va = sp[0], vb = sp[1];
			const uint32_t in[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
			uint32_t o[8];
#pragma unroll
			for (uint32_t q = 0; q < 8; ++q) {
				const uint32_t y0 = in[q] & 0xFFFFu, y1 = in[q] >> 16;
				const uint32_t z0 = y0 >= kMSpecial ? y0 : src[y0];
				const uint32_t z1 = y1 >= kMSpecial ? y1 : src[y1];
				o[q] = z0 | (z1 << 16);
			}
			uint4* dp = reinterpret_cast<uint4*>(dstM + x0);
			dp[0] = make_uint4(o[0], o[1], o[2], o[3]);
			dp[1] = make_uint4(o[4], o[5], o[6], o[7]);
			__syncthreads();
			uint16_t* t = src;
			src = dstM;
			dstM = t;
		}
		// src[x]: END, malformed, or the window's last command on the chain from x
		for (uint32_t x = tid; x < avail; x += kRdBlock) {
			const uint32_t m = src[x];
			uint32_t out;
			if (m == kMEnd) out = kIxEnd;
			else if (m == kMBad) out = kIxBad;
			else {
				const uint32_t t = far[m];   // <= dl
				out = t >= c1 ? t : X[t];    // a later window of this chunk: stored by this block
			}
			X[ws + x] = out;
		}
		block_sync_global();   // the stores before the next window's loads of them; the LDS is the next window's
	}
}

extern "C" __global__ __launch_bounds__(64) void dg_index_resolve_kernel(IxArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t lane = lane_id();
	const IxEarly e = ix_early(a, i);
	const uint32_t g0 = a.chunk_base[i], nch = a.chunk_base[i + 1] - g0;
	const uint32_t* X = a.exit + a.exit_off[i];
	const uint64_t dl = e.dl;
	uint64_t cur = 25;
	uint32_t mode = e.st ? 1u : 0u;   // 0: on the chain, 1: ended, 2: malformed
	if (!mode && cur >= dl) mode = 1;
	for (uint32_t k = 0; k < nch; ++k) {
		const uint64_t c0 = (uint64_t)k * a.chunk_bytes, cend = c0 + a.chunk_bytes;
		const bool live = !mode && c0 < dl;
		if (lane == 0) {
			a.chunks[g0 + k].entry = (uint32_t)(live ? cur : dl);
			a.chunks[g0 + k].live = live ? 1u : 0u;
		}
		if (live && cur < cend) {   // (else the chain jumps over the chunk: the next one inherits cur)
			const uint32_t nx = uni(X[cur]);
			if (nx == kIxEnd) mode = 1;
			else if (nx == kIxBad) mode = 2;
			else {
				cur = nx;
				if (cur >= dl) mode = 1;   // a missing END is end of input
			}
		}
	}
	if (lane == 0) {
		IxStream s{};
		s.doff = e.doff;
		s.dl = (uint32_t)e.dl;
		s.vsize = e.vsize;
		s.st = e.st;
		s.walk_bad = mode == 2 ? 1u : 0u;
		a.sstate[i] = s;
	}
}

extern "C" __global__ __launch_bounds__(kRdBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void dg_index_fill_kernel(
    IxArgs a) {
	const uint32_t g = blockIdx.x;
	if (g >= a.n_chunks) return;
	uint32_t i, k;
	ix_chunk_of(a, g, i, k);
	const IxStream s = a.sstate[i];
	const uint64_t c0 = (uint64_t)k * a.chunk_bytes, cend = c0 + a.chunk_bytes;
	const uint64_t dl = s.dl;
	if (s.st || c0 >= dl) return;
	__shared__ DecLdsMem M;
	__shared__ RdTileLds T;
	const DecLds L = dec_lds(M);

	const uint8_t* D = a.delta + s.doff;
	RdEnt* E = reinterpret_cast<RdEnt*>(a.index + a.index_off[i] + sizeof(RdHead));
	const uint64_t ref_len = a.streams[i].ref_len;
	// the chunk's strides: [klo, khi]; the stream's last chunk takes the one at the stream's end too
	const uint32_t n_ent = (uint32_t)(dl / kRdStride) + 1u;
	const uint32_t klo = (uint32_t)(c0 / kRdStride);
	const uint32_t khi = cend >= dl ? n_ent - 1u : (uint32_t)(cend / kRdStride) - 1u;
	const IxChunk ck = a.chunks[g];

	// from the chunk's true entry (a chunk that is not live has no command: only its strides are filled)
	const RdWalk r = rd_index_walk(L, T, D, dl, s.vsize, ref_len, E, ck.live ? ck.entry : dl, cend, klo, khi);
	if (threadIdx.x == 0) {
		a.chunks[g].res = (r.failed ? kIxFailed : 0u) | (r.t.any ? kIxAny : 0u) | (r.t.brk ? kIxBrk : 0u);
		a.chunks[g].first_dst = r.t.first;
		a.chunks[g].last_end = r.t.end;
	}
}

extern "C" __global__ __launch_bounds__(64) void dg_index_finish_kernel(IxArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t lane = lane_id();
	const IxStream s = a.sstate[i];
	const uint32_t g0 = a.chunk_base[i], nch = a.chunk_base[i + 1] - g0;
	int32_t st = s.st;
	bool seq = true;
	uint32_t run_end = 0;
	if (!st) {
		bool failed = s.walk_bad != 0;
		for (uint32_t b0 = 0; b0 < nch; b0 += 64) {   // (every lane takes part)
			const uint32_t c = b0 + lane;
			IxChunk ck{};
			if (c < nch) ck = a.chunks[g0 + c];
			const uint32_t res = ck.live ? ck.res : 0u;   // chunks after END are not looked at
			if (__ballot(res & kIxFailed)) failed = true;
			const bool any = res & kIxAny;
			const uint32_t p = prev_set(any, lane);
			const uint32_t before = shfl32(ck.last_end, p ? p - 1 : 0);
			const uint32_t pe = p ? before : run_end;
			if (__ballot(any && ((res & kIxBrk) || ck.first_dst != pe))) seq = false;
			const uint32_t ls = last_set(any);
			if (ls) run_end = rdlane(ck.last_end, ls - 1);
		}
		if (failed) st = 8;
	}
	if (lane == 0) {
		RdHead h;
		h.doff = s.doff;
		h.dl = st ? 0u : s.dl;
		h.vsize = s.vsize;
		h.status = st;
		h.flags = (!st && seq && run_end == s.vsize) ? kRdSeq : 0u;
		h.n_ent = s.st ? 0u : s.dl / kRdStride + 1u;
		h.pad = 0;
		*reinterpret_cast<RdHead*>(a.index + a.index_off[i]) = h;
		if (a.stream_status) a.stream_status[i] = st;
	}
}
