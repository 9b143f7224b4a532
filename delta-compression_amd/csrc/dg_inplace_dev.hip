// dg_inplace_dev.hip — in-place conversion of a batch of standard deltas on
// the device (src/c/inplace.c:272-736, Burns, Long & Stockmeyer, IEEE TKDE
// 2003), byte for byte what dg_make_inplace (dg_inplace.cpp) produces.
//
// Built on its own as lib/dg_inplace.hsaco and loaded by dg_inplace_host.cpp.
// Two kernels, with the library's size scan between them:
//
//   dg_inplace_order_kernel   one wave per delta.  Parses the DLT\x03 stream
//     through a 1 KiB LDS window (the command chain by pointer doubling,
//     dg_parse_chain.h; all lanes decode the headers), checks every field, and
//     fills the copy table
//     (src, dst, len) and the add table.  A standard delta's commands are in
//     destination order, so the CRWI neighbours of copy i are the index range
//     [a_i, b_i) minus i (dg_inplace_core.h): two binary searches per copy,
//     one copy per lane; in-degrees from a difference array and a wave scan;
//     the copies ranked once by (length, index) with a wave radix sort, the
//     ready set a bitmap in rank order, a pop a find-first-set across lanes,
//     a retire one neighbour per lane.  A stall runs dg_inplace_core.h's
//     policy on lane 0 (Tarjan lazily, at the first stall).  A delta without
//     any edge takes the rank order directly.
//   dg_inplace_emit_kernel    one 256-thread block per delta writes the
//     header (flag byte 1), the kept copies in Kahn order, the original ADDs
//     in command order (copied from the stream), the victims in conversion
//     order (payload from R) and the end byte.
//
// No byte outside [0, len) of a stream or of R is read: every multi-byte
// load is issued only where it fits, the rest byte by byte.
#include <hip/hip_runtime.h>

#include "dg_devutil.h"
#include "dg_inplace_core.h"
#include "dg_inplace_dev.h"
#include "dg_parse_chain.h"
#include "dg_stream_dev.h"

using namespace dg;
using namespace dgip;

namespace {

constexpr uint32_t kLdsWords = 2048;       // dst column cache; radix counters; small graph / ready bitmap
constexpr uint32_t kSmallGraph = 128;      // copies up to which the Kahn loop and the stall code run out of LDS

struct WorkPtrs {
	uint32_t *src, *dst, *len, *a, *b, *indeg, *rank, *byrank, *order;
	Work core;
	uint32_t* bitmap;    // ready bitmap when it does not fit LDS
	uint32_t *add_off, *add_out;
};

__device__ __forceinline__ WorkPtrs work_ptrs(uint8_t* base, uint32_t C, uint32_t A) {
	WorkPtrs p;
	uint32_t* w = reinterpret_cast<uint32_t*>(base);
	p.src = w; w += C;
	p.dst = w; w += C;
	p.len = w; w += C;
	p.a = w; w += C;
	p.b = w; w += C;
	p.indeg = w; w += C;
	p.rank = w; w += C;
	p.byrank = w; w += C;
	p.order = w; w += C;
	p.core.idx = w; w += C;
	p.core.low = w; w += C;
	p.core.tstk = w; w += C;
	p.core.callv = w; w += C;
	p.core.calln = w; w += C;
	p.core.scc = w; w += C;
	p.core.cverts = w; w += C;
	p.core.cstart = w; w += C;
	p.core.active = w; w += C;
	p.bitmap = w; w += (C + 31) / 32;
	p.add_off = w; w += A;
	p.add_out = w; w += A;
	p.core.flag = reinterpret_cast<uint8_t*>(w);
	return p;
}

// Stable wave radix sort of the copies by (length, index): rank[v] and
// by_rank[r].  Keys ping-pong between (kA, vA) and (kB, vB); cnt: 256 LDS words.
__device__ void rank_sort(uint32_t n, const uint32_t* len, uint32_t* kA, uint32_t* vA, uint32_t* kB, uint32_t* vB,
                          uint32_t* rank, uint32_t* byrank, uint32_t* cnt) {
	const uint32_t lane = lane_id();
	uint32_t mx = 0;
	for (uint32_t i = lane; i < n; i += 64) mx = umax32(mx, len[i]);
	mx = rdlane(wave_incl_max(mx), 63);
	const uint32_t passes = mx >= (1u << 24) ? 4 : (mx >= (1u << 16) ? 3 : (mx >= (1u << 8) ? 2 : 1));
	const uint32_t* ks = len;
	const uint32_t* vs = nullptr;   // pass 0: the index itself
	uint32_t *kd = kA, *vd = vA;
	for (uint32_t p = 0; p < passes; ++p) {
		const uint32_t sh = 8 * p;
		for (uint32_t k = lane; k < 256; k += 64) cnt[k] = 0;
		wave_sync();
		for (uint32_t i = lane; i < n; i += 64) atomicAdd(&cnt[(ks[i] >> sh) & 255u], 1u);
		wave_sync();
		{
			const uint32_t c0 = cnt[4 * lane], c1 = cnt[4 * lane + 1], c2 = cnt[4 * lane + 2], c3 = cnt[4 * lane + 3];
			const uint32_t s = c0 + c1 + c2 + c3;
			const uint32_t ex = wave_incl_scan(s) - s;
			wave_sync();
			cnt[4 * lane] = ex;
			cnt[4 * lane + 1] = ex + c0;
			cnt[4 * lane + 2] = ex + c0 + c1;
			cnt[4 * lane + 3] = ex + c0 + c1 + c2;
		}
		wave_sync();
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t i = base + lane;
			const bool act = i < n;
			const uint32_t k = act ? ks[i] : 0u;
			const uint32_t v = act ? (vs ? vs[i] : i) : 0u;
			const uint32_t d = (k >> sh) & 255u;
			uint64_t peers = __ballot(act);
#pragma unroll
			for (uint32_t bit = 0; bit < 8; ++bit) {
				const bool one = (d >> bit) & 1u;
				const uint64_t m = __ballot(act && one);
				peers &= one ? m : ~m;
			}
			uint32_t pos = 0;
			if (act) pos = cnt[d] + (uint32_t)__builtin_popcountll(peers & (mask_le(lane) >> 1));
			wave_sync();
			if (act && lane == ffs64(peers)) cnt[d] += (uint32_t)__builtin_popcountll(peers);
			wave_sync();
			if (act) {
				kd[pos] = k;
				vd[pos] = v;
			}
		}
		wave_sync();
		ks = kd;
		vs = vd;
		kd = kd == kA ? kB : kA;
		vd = vd == vA ? vB : vA;
	}
	for (uint32_t r = lane; r < n; r += 64) {
		const uint32_t v = vs[r];
		byrank[r] = v;
		rank[v] = r;
	}
	wave_sync();
}

// Kahn's order by smallest (length, index): the ready set is the bitmap bm in
// rank order, a pop a find-first-set across lanes, a retire one neighbour per
// lane; a stall is broken by dg_inplace_core.h's policy on lane 0.  kw: the
// arrays the loop touches (LDS or work memory; inlined per call site so that
// each keeps its address space).  order: kept copies from the front, victims
// from the back.
__device__ __forceinline__ void kahn_loop(uint32_t n, const WorkPtrs& kw, uint32_t* bm, uint32_t* order, int policy,
                                          uint32_t* kept_out, uint32_t* nv_out) {
	const uint32_t lane = lane_id();
	const uint32_t nw = (n + 31) / 32;
	uint32_t kept = 0, nv = 0;
	for (uint32_t k = lane; k < nw; k += 64) bm[k] = 0;
	wave_sync();
	for (uint32_t k = lane; k < n; k += 64)
		if (kw.indeg[k] == 0) {
			const uint32_t r = kw.rank[k];
			atomicOr(&bm[r >> 5], 1u << (r & 31u));
		}
	wave_sync();
	const uint32_t wpl = (nw + 63) / 64;
	const Graph g{n, kw.len, kw.a, kw.b};
	Stall s;
	s.policy = policy;
	while (kept + nv < n) {
		uint32_t cand = kNone;
		for (uint32_t k = 0; k < wpl; ++k) {
			const uint32_t wi = lane * wpl + k;
			if (wi < nw && cand == kNone) {
				const uint32_t x = bm[wi];
				if (x) cand = 32 * wi + (uint32_t)__builtin_ctz(x);
			}
		}
		const uint64_t m = __ballot(cand != kNone);
		uint32_t v;
		if (m) {
			const uint32_t r = rdlane(cand, ffs64(m));
			v = kw.byrank[r];
			if (lane == 0) {
				bm[r >> 5] &= ~(1u << (r & 31u));
				order[kept] = v;
			}
			++kept;
		} else {
			uint32_t vv = 0;
			if (lane == 0) vv = next_victim(g, kw.core, s);
			v = uni(vv);
			if (lane == 0) order[n - 1 - nv] = v;
			++nv;
		}
		if (lane == 0) mark_done(kw.core, s, v);
		wave_sync();
		const uint32_t av = kw.a[v], bv = kw.b[v];
		for (uint32_t x0 = av; x0 < bv; x0 += 64) {
			const uint32_t x = x0 + lane;
			if (x < bv && x != v && !(kw.core.flag[x] & kDone)) {
				const uint32_t d = kw.indeg[x] - 1;
				kw.indeg[x] = d;
				if (d == 0) {
					const uint32_t r = kw.rank[x];
					atomicOr(&bm[r >> 5], 1u << (r & 31u));
				}
			}
		}
		wave_sync();
	}
	*kept_out = kept;
	*nv_out = nv;
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void dg_inplace_order_kernel(IpArgs a) {
	// the parser's arrays first; then the dst column cache, the radix counters,
	// and a small graph or the ready bitmap (kLdsWords of it)
	constexpr uint32_t kLdsAlloc = kLdsWords > (kChainLdsBytes + 3) / 4 ? kLdsWords : (kChainLdsBytes + 3) / 4;
	__shared__ __attribute__((aligned(16))) uint32_t lds[kLdsAlloc];
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t lane = lane_id();
	const IpDesc dd = a.descs[i];
	IpRes res{};
	auto finish = [&](int32_t st, uint64_t size) {
		if (lane == 0) {
			a.status[i] = st;
			a.sizes[i] = st ? 0 : size;
			a.res[i] = res;
		}
	};
	if (a.delta_status && a.delta_status[i] != 0) return finish(a.delta_status[i], 0);
	const uint64_t s_off = a.delta_offsets ? a.delta_offsets[i] : dd.delta_off;
	const uint64_t s_len = a.delta_offsets ? a.delta_offsets[i + 1] - s_off : dd.delta_cap;
	if (s_len > dd.delta_cap || s_len >= (1ull << 32)) return finish(7, 0);
	const uint8_t* D = a.delta + s_off;
	const uint32_t dl = (uint32_t)s_len;
	res.stream_off = s_off;
	res.stream_len = dl;
	if (bad_magic(D, dl)) return finish(8, 0);
	if (D[4] & 1) {   // already in-place: unchanged
		res.passthrough = 1;
		return finish(0, dl);
	}
	const uint64_t rl = dd.ref_len;
	const uint32_t C = dd.max_copies, A = dd.max_adds;
	const WorkPtrs w = work_ptrs(a.work + dd.work_off, C, A);

	// ── parse: the command chain by pointer doubling (dg_parse_chain.h), then
	//    64 headers at a time ──
	const ChainLds cl = chain_lds(lds);
	const uint8_t* win = cl.win;
	const uint16_t* cmds = cl.cmds;
	uint32_t pos = 25, ncopy = 0, nadd = 0;
	uint64_t wpos = 0, add_len = 0;
	bool bad = false, unsup = false, full = false, ended = false;
	while (!ended && !bad) {
		if (pos >= dl) break;   // the stream ends without an END byte (encoding.c:111-178 allows it)
		const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, D, dl, pos), pos, dl);
		const uint32_t cnt = cw.cnt;
		for (uint32_t b0 = 0; b0 < cnt; b0 += 64) {
			const bool mine = b0 + lane < cnt;
			// (decode_hdr of dg_stream_dev.h, written out: calling it here changes
			// the instructions the compiler emits for this kernel)
			uint32_t cx = 0, kind = 0, c_src = 0, c_dst = 0, c_len = 0;
			if (mine) {
				cx = cmds[b0 + lane];
				kind = win[cx];
				if (kind == 1) {
					c_src = be32(win + cx + 1);
					c_dst = be32(win + cx + 5);
					c_len = be32(win + cx + 9);
				} else {
					c_dst = be32(win + cx + 1);
					c_len = be32(win + cx + 5);
				}
			}
			const bool is_copy = mine && kind == 1, is_add = mine && kind == 2;
			uint64_t tot_len, tot_add;
			const uint64_t pre_len = wave_excl_scan64(c_len, &tot_len);
			const uint64_t pre_add = wave_excl_scan64(is_add ? c_len : 0u, &tot_add);
			const uint32_t inc_c = wave_incl_scan(is_copy ? 1u : 0u), inc_a = wave_incl_scan(is_add ? 1u : 0u);
			const uint32_t ci = ncopy + inc_c - (is_copy ? 1u : 0u), ai = nadd + inc_a - (is_add ? 1u : 0u);
			// commands placed sequentially: dst = the sum of the earlier lengths
			if (__ballot(mine && (uint64_t)c_dst != wpos + pre_len)) unsup = true;
			// the victims read R
			if (__ballot(is_copy && (uint64_t)c_src + c_len > rl)) bad = true;
			if (ncopy + rdlane(inc_c, 63) > C || nadd + rdlane(inc_a, 63) > A) full = true;
			if (!unsup && !bad && !full) {
				if (is_copy) {
					w.src[ci] = c_src;
					w.dst[ci] = c_dst;
					w.len[ci] = c_len;
				}
				if (is_add) {
					w.add_off[ai] = pos + cx;
					w.add_out[ai] = (uint32_t)(add_len + pre_add + 9ull * (ai));
				}
			}
			ncopy += rdlane(inc_c, 63);
			nadd += rdlane(inc_a, 63);
			wpos += tot_len;
			add_len += tot_add;
		}
		if (cw.term == kChBad) bad = true;
		if (cw.term == kChEnd) ended = true;
		pos = cw.next_pos;
		wave_sync();   // the window is rewritten next
	}
	if (bad) return finish(8, 0);
	if (unsup) return finish(2, 0);
	if (full) return finish(7, 0);
	const uint32_t n = ncopy;
	res.n_copies = n;
	res.n_adds = nadd;
	res.add_bytes = add_len + 9ull * nadd;
	if (res.add_bytes >= (1ull << 32)) return finish(2, 0);   // 32-bit output offsets: left to the host

	uint32_t kept = 0, nv = 0;
	if (n) {
		// ── CRWI ranges and in-degrees ──
		const uint32_t* dcol = w.dst;
		if (n <= kLdsWords) {
			for (uint32_t k = lane; k < n; k += 64) lds[k] = w.dst[k];
			dcol = lds;
		}
		for (uint32_t k = lane; k < n; k += 64) {
			w.indeg[k] = 0;
			w.core.flag[k] = 0;
		}
		wave_sync();
		for (uint32_t k = lane; k < n; k += 64) {
			uint32_t ra, rb;
			range_of(k, n, w.src[k], w.len[k], dcol, w.len, &ra, &rb);
			w.a[k] = ra;
			w.b[k] = rb;
			if (ra < rb) {
				atomicAdd(&w.indeg[ra], 1u);
				if (rb < n) atomicAdd(&w.indeg[rb], 0xFFFFFFFFu);
			}
		}
		wave_sync();
		uint32_t carry = 0;
		bool edges = false;
		for (uint32_t b0 = 0; b0 < n; b0 += 64) {
			const uint32_t k = b0 + lane;
			const bool act = k < n;
			const uint32_t x = act ? w.indeg[k] : 0u;
			const uint32_t incl = wave_incl_scan(x) + carry;
			uint32_t deg = 0;
			if (act) {
				deg = incl - ((w.a[k] <= k && k < w.b[k]) ? 1u : 0u);
				w.indeg[k] = deg;
			}
			if (__ballot(deg != 0)) edges = true;
			carry = rdlane(incl, 63);
		}
		wave_sync();
		// ── rank by (length, index) ──
		rank_sort(n, w.len, w.core.idx, w.core.low, w.core.tstk, w.core.callv, w.rank, w.byrank, lds);
		if (!edges) {
			// no copy reads what another writes: the rank order is Kahn's
			for (uint32_t r = lane; r < n; r += 64) w.order[r] = w.byrank[r];
			kept = n;
		} else {
			// ── Kahn by (length, index), stalls broken by the policy ──
			const uint32_t nw = (n + 31) / 32;
			if (n <= kSmallGraph) {
				// a small graph runs out of LDS: a pop, a retire and every DFS
				// step of a stall are then LDS round trips
				WorkPtrs kw = w;
				uint32_t* q = lds;
				auto take = [&](const uint32_t* from) {
					uint32_t* d = q;
					q += n;
					if (from)
						for (uint32_t k = lane; k < n; k += 64) d[k] = from[k];
					return d;
				};
				kw.len = take(w.len);
				kw.a = take(w.a);
				kw.b = take(w.b);
				kw.indeg = take(w.indeg);
				kw.rank = take(w.rank);
				kw.byrank = take(w.byrank);
				kw.core.idx = take(nullptr);
				kw.core.low = take(nullptr);
				kw.core.tstk = take(nullptr);
				kw.core.callv = take(nullptr);
				kw.core.calln = take(nullptr);
				kw.core.scc = take(nullptr);
				kw.core.cverts = take(nullptr);
				kw.core.cstart = take(nullptr);
				kw.core.active = take(nullptr);
				uint32_t* bm = q;
				q += nw;
				kw.core.flag = reinterpret_cast<uint8_t*>(q);
				static_assert(15 * kSmallGraph + (kSmallGraph + 31) / 32 + (kSmallGraph + 3) / 4 <= kLdsWords, "small graph fits LDS");
				for (uint32_t k = lane; k < n; k += 64) kw.core.flag[k] = 0;
				kahn_loop(n, kw, bm, w.order, (int)a.policy, &kept, &nv);
			} else if (nw <= kLdsWords) {
				kahn_loop(n, w, lds, w.order, (int)a.policy, &kept, &nv);
			} else {
				kahn_loop(n, w, w.bitmap, w.order, (int)a.policy, &kept, &nv);
			}
		}
	}
	// ── the victims' output offsets (in the in-degree column, now free) and the size ──
	uint64_t vict_bytes = 0;
	for (uint32_t b0 = 0; b0 < nv; b0 += 64) {
		const uint32_t k = b0 + lane;
		const uint32_t l = k < nv ? w.len[w.order[n - 1 - k]] : 0u;
		uint64_t tot;
		const uint64_t pre = wave_excl_scan64(l, &tot);
		if (k < nv) w.indeg[k] = (uint32_t)(vict_bytes + pre + 9ull * k);
		vict_bytes += tot;
	}
	vict_bytes += 9ull * nv;
	if (vict_bytes >= (1ull << 32)) return finish(2, 0);
	res.kept = kept;
	res.victims = nv;
	finish(0, 25 + 13ull * kept + res.add_bytes + vict_bytes + 1);
}

extern "C" __global__ __launch_bounds__(256) void dg_inplace_emit_kernel(IpArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	if (a.status[i] != 0) return;
	const uint64_t base = a.out_offsets[i], end = a.out_offsets[i + 1];
	if (end > a.out_cap) {
		if (tid == 0) a.status[i] = 7;
		return;
	}
	const IpRes res = a.res[i];
	const uint8_t* D = a.delta + res.stream_off;
	uint8_t* O = a.out + base;
	if (res.passthrough) {
		// (64-bit: a stream may be up to 2^32 - 1 bytes, and a 32-bit counter would wrap above 2^32 - 16384)
		for (uint64_t c = wave * 4096u; c < res.stream_len; c += 4 * 4096u)
			wave_copy(O + c, D + c, umin32(4096u, (uint32_t)(res.stream_len - c)), lane);
		return;
	}
	const IpDesc dd = a.descs[i];
	const uint8_t* R = a.ref + dd.ref_off;
	const WorkPtrs w = work_ptrs(a.work + dd.work_off, dd.max_copies, dd.max_adds);
	const uint32_t n = res.n_copies, kept = res.kept, nv = res.victims, nadd = res.n_adds;
	// header: flag byte 1, version size and both CRCs as they are
	if (tid < 25) O[tid] = tid == 4 ? (uint8_t)1 : D[tid];
	if (tid == 0) O[end - base - 1] = 0;
	// the kept copies in Kahn order
	for (uint32_t k = tid; k < kept; k += 256) {
		const uint32_t v = w.order[k];
		uint8_t* p = O + 25 + 13ull * k;
		p[0] = 1;
		put_be32(p + 1, w.src[v]);
		put_be32(p + 5, w.dst[v]);
		put_be32(p + 9, w.len[v]);
	}
	// the original ADDs, whole commands from the stream; then the victims
	uint8_t* OA = O + 25 + 13ull * kept;
	uint8_t* OV = OA + res.add_bytes;
	for (uint32_t c = 64 * wave; c < nadd + nv; c += 256) {
		const uint32_t k = c + lane;
		const uint8_t* sp = D;
		uint8_t* dp = O;
		uint32_t nb = 0;
		if (k < nadd) {
			const uint32_t so = w.add_off[k];
			sp = D + so;
			dp = OA + w.add_out[k];
			nb = 9 + be32(D + so + 5);
		} else if (k < nadd + nv) {
			const uint32_t kk = k - nadd, v = w.order[n - 1 - kk];
			dp = OV + w.indeg[kk];
			dp[0] = 2;
			put_be32(dp + 1, w.dst[v]);
			put_be32(dp + 5, w.len[v]);
			dp += 9;
			sp = R + w.src[v];
			nb = w.len[v];
		}
		if (nb <= kSmallCopy)
			for (uint32_t t = 0; t < nb; ++t) dp[t] = sp[t];
		for (uint64_t m = __ballot(nb > kSmallCopy); m; m &= m - 1) {
			const uint32_t f = ffs64(m);
			const uint8_t* s2 = reinterpret_cast<const uint8_t*>(uni64((uint64_t)(uintptr_t)__shfl((unsigned long long)(uintptr_t)sp, (int)f, 64)));
			uint8_t* d2 = reinterpret_cast<uint8_t*>(uni64((uint64_t)(uintptr_t)__shfl((unsigned long long)(uintptr_t)dp, (int)f, 64)));
			wave_copy(d2, s2, rdlane(nb, f), lane);
		}
	}
}
