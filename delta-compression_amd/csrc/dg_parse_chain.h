// dg_parse_chain.h — the command chain of a DLT\x03 stream, one wave, by
// pointer doubling (the scheme of decode_kernel's parser, dg_kernels.hip, cut
// to one wave and a 1 KiB window; decode_kernel keeps its own four-wave copy).
//
// Parsing (encoding.c:111-178) is a chain x -> x + |cmd(x)| through the
// stream.  Per window of the stream, staged in LDS:
//   1. every lane computes, for each of the 16 window offsets it owns, the
//      offset of the next command IF a command started there (N1), or a code:
//      END, malformed, header cut by the window, next command past the window;
//   2. N2 = N1.N1, N4, N8, N16 by pointer doubling (codes propagate; N16
//      takes N4's place once N8 is built);
//   3. one uniform walk takes 16 commands per step through N16, then at most
//      one N8 step and single steps near the window end; the nodes in between
//      are expanded in parallel.
// So a window of ~90 commands costs ~15 dependent LDS reads instead of ~180.
//
// Only bytes [pos, min(pos + kChainWin, len)) of the stream are read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_devutil.h"

namespace dg {

constexpr uint32_t kChainWin = 1024;       // stream bytes per window
constexpr uint32_t kChainMaxCmds = 128;    // >= kChainWin / 9 (the shortest command), a multiple of 16
constexpr uint16_t kChEnd = 0xFFFE;        // END at x
constexpr uint16_t kChBad = 0xFFFD;        // malformed at x
constexpr uint16_t kChCut = 0xFFFF;        // header not complete in the window: restart at x
constexpr uint16_t kChFar = 0xFFFC;        // complete command at x, next one at/after the window end
constexpr uint16_t kChSpecial = 0xFFFC;    // codes are >= this
static_assert(kChainWin == 16 * 64, "16 window offsets per lane");

// LDS of one wave's parser, carved from a 16-byte aligned block
constexpr uint32_t kChainLdsBytes = 4 * 2 * kChainWin + (kChainWin + 32) + 2 * kChainMaxCmds + 2 * (kChainMaxCmds / 16 + 2) + 12;
struct ChainLds {
	uint16_t *N1, *N2, *N4, *N8;   // kChainWin each
	uint8_t* win;                  // kChainWin + 32, 16-byte aligned
	uint16_t* cmds;                // kChainMaxCmds: window offsets of the commands found
	uint16_t* jumps;               // kChainMaxCmds / 16 + 2
};
__device__ __forceinline__ ChainLds chain_lds(void* base) {
	ChainLds l;
	l.N1 = static_cast<uint16_t*>(base);
	l.N2 = l.N1 + kChainWin;
	l.N4 = l.N2 + kChainWin;
	l.N8 = l.N4 + kChainWin;
	l.win = reinterpret_cast<uint8_t*>(l.N8 + kChainWin);
	l.cmds = reinterpret_cast<uint16_t*>(l.win + kChainWin + 32);
	l.jumps = l.cmds + kChainMaxCmds;
	return l;
}

struct ChainWindow {
	uint32_t cnt;        // commands found: l.cmds[0 .. cnt), window offsets in stream order
	uint32_t term;       // kChEnd: the stream ends here; kChBad: malformed; else more follows
	uint32_t next_pos;   // where the next window starts
};

// orders LDS between the lanes of the wave
__device__ __forceinline__ void chain_sync() {
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

// One window of stream D (dl bytes, pos < dl) from offset pos.  Uniform call
// by a whole wave that owns l; l.win[x] = D[pos + x] afterwards.
__device__ __forceinline__ ChainWindow chain_window(const uint8_t* D, uint32_t dl, uint32_t pos, const ChainLds& l) {
	typedef uint32_t u32_u __attribute__((aligned(1)));
	const uint32_t lane = lane_id();
	const uint32_t avail = umin32(kChainWin, dl - pos);
	// ── 1. window -> LDS (unaligned dwords that fit, then the last bytes) ──
	{
		uint32_t* w32 = reinterpret_cast<uint32_t*>(l.win);
		for (uint32_t k = lane; 4 * k + 4 <= avail; k += 64) w32[k] = *reinterpret_cast<const u32_u*>(D + pos + 4 * k);
		if (lane < (avail & 3u)) l.win[(avail & ~3u) + lane] = D[pos + (avail & ~3u) + lane];
	}
	chain_sync();
	const uint8_t* w = l.win;
	// ── 2. N1: lane owns offsets [16 lane, 16 lane + 16): all default to
	//    malformed, and only offsets whose byte is a command type (0, 1, 2)
	//    inside the stream are decoded ──
	{
		const uint32_t x0 = 16 * lane;
		constexpr uint32_t bb = (uint32_t)kChBad | ((uint32_t)kChBad << 16);
		uint4* dst = reinterpret_cast<uint4*>(l.N1 + x0);
		dst[0] = make_uint4(bb, bb, bb, bb);
		dst[1] = make_uint4(bb, bb, bb, bb);
		const uint4 dv = reinterpret_cast<const uint4*>(w)[lane];
		const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w};
		uint32_t cand = 0;
#pragma unroll
		for (uint32_t k = 0; k < 16; ++k) cand |= (((d[k >> 2] >> (8 * (k & 3))) & 0xFFu) <= 2u ? 1u : 0u) << k;
		const uint32_t lim = avail > x0 ? umin32(avail - x0, 16u) : 0u;
		cand &= (1u << lim) - 1u;
		for (; cand; cand &= cand - 1) {
			const uint32_t x = x0 + (uint32_t)__builtin_ctz(cand);
			const uint32_t t = w[x];
			uint32_t nx = kChEnd;
			if (t != 0) {
				const uint32_t hdr = t == 1 ? 13u : 9u;
				if (x + hdr > avail) {
					nx = (uint64_t)pos + x + hdr > dl ? kChBad : kChCut;
				} else {
					const uint64_t len = t == 1 ? 0u
					                            : ((uint32_t)w[x + 5] << 24) | ((uint32_t)w[x + 6] << 16) |
					                                  ((uint32_t)w[x + 7] << 8) | w[x + 8];
					const uint64_t end = (uint64_t)x + hdr + len;
					if (pos + end > dl) nx = kChBad;
					else nx = end >= avail ? kChFar : (uint32_t)end;
				}
			}
			l.N1[x] = (uint16_t)nx;
		}
	}
	chain_sync();
	// ── 3. pointer doubling (16 offsets per lane: two 16-byte reads, 16
	//    independent gathers, two 16-byte stores) ──
	auto dbl = [&](const uint16_t* src, uint16_t* dstN) {
		const uint32_t x0 = 16 * lane;
		const uint4* sp = reinterpret_cast<const uint4*>(src + x0);
		const uint4 a = sp[0], b = sp[1];
		const uint32_t in[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
		uint32_t o[8];
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t y0 = in[k] & 0xFFFFu, y1 = in[k] >> 16;
			const uint32_t z0 = y0 >= kChSpecial ? y0 : src[y0];
			const uint32_t z1 = y1 >= kChSpecial ? y1 : src[y1];
			o[k] = z0 | (z1 << 16);
		}
		uint4* dp = reinterpret_cast<uint4*>(dstN + x0);
		dp[0] = make_uint4(o[0], o[1], o[2], o[3]);
		dp[1] = make_uint4(o[4], o[5], o[6], o[7]);
	};
	uint16_t* N16 = l.N4;   // (N4 is dead once N8 is built)
	dbl(l.N1, l.N2);
	chain_sync();
	dbl(l.N2, l.N4);
	chain_sync();
	dbl(l.N4, l.N8);
	chain_sync();
	dbl(l.N8, N16);
	chain_sync();
	// ── 4. the walk (uniform): 16 commands per N16 step, at most one N8 step,
	//    then single steps ──
	uint32_t x = 0, nj = 0, n8 = 0, term = 0;
	while (true) {
		const uint32_t y = uni(N16[x]);
		if (y >= kChSpecial || 16 * (nj + 1) > kChainMaxCmds) break;
		if (lane == 0) l.jumps[nj] = (uint16_t)x;
		++nj;
		x = y;
	}
	uint32_t cnt = 16 * nj;
	{
		const uint32_t y = uni(l.N8[x]);
		if (y < kChSpecial && cnt + 8 <= kChainMaxCmds) {
			if (lane == 0) l.jumps[nj] = (uint16_t)x;
			n8 = 1;
			cnt += 8;
			x = y;
		}
	}
	while (true) {   // single steps from x (at most 7 commands + the terminal)
		const uint32_t y = uni(l.N1[x]);
		if (y == kChEnd || y == kChBad || y == kChCut) { term = y; break; }
		if (cnt >= kChainMaxCmds) { term = kChCut; break; }   // restart the window at x
		if (lane == 0) l.cmds[cnt] = (uint16_t)x;
		++cnt;
		if (y == kChFar) { term = kChFar; break; }
		x = y;
	}
	chain_sync();
	// expand the jumps: 8 nodes from each base (e, N1 e, N2 e, ..., N1 N2 N2 N2 e);
	// a 16-command jump has bases e and N8 e
	for (uint32_t k = lane; k < 2 * nj + n8; k += 64) {
		const uint32_t j = k >> 1;
		const uint32_t e0 = j < nj ? ((k & 1) ? l.N8[l.jumps[j]] : l.jumps[j]) : l.jumps[nj];
		const uint32_t e2 = l.N2[e0];
		const uint32_t e4 = l.N2[e2];
		const uint32_t e6 = l.N2[e4];
		uint16_t* c = l.cmds + (j < nj ? 16 * j + 8 * (k & 1) : 16 * nj);
		c[0] = (uint16_t)e0;
		c[1] = l.N1[e0];
		c[2] = (uint16_t)e2;
		c[3] = l.N1[e2];
		c[4] = (uint16_t)e4;
		c[5] = l.N1[e4];
		c[6] = (uint16_t)e6;
		c[7] = l.N1[e6];
	}
	chain_sync();
	ChainWindow r;
	r.cnt = cnt;
	r.term = term;
	r.next_pos = pos + x;   // kChCut: restart at x
	if (term == kChFar) {
		const uint32_t t = w[x];
		const uint32_t len = ((uint32_t)w[x + 5] << 24) | ((uint32_t)w[x + 6] << 16) | ((uint32_t)w[x + 7] << 8) | w[x + 8];
		r.next_pos = pos + x + (t == 1 ? 13u : 9u + len);
	}
	return r;
}

}  // namespace dg
