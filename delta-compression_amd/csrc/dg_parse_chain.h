// dg_parse_chain.h — the command chain of a DLT\x03 stream by pointer
// doubling: the one parser of every kernel that reads a stream.  A block of T
// threads parses a window of 16 T stream bytes: T = 64 for the one-wave
// kernels (in-place, compose, invert: 1 KiB), T = 256 for decode and update
// (4 KiB).
//
// Parsing (encoding.c:111-178) is a chain x -> x + |cmd(x)| through the
// stream.  Per window of the stream, staged in LDS:
//   1. every thread computes, for each of the 16 window offsets it owns, the
//      offset of the next command IF a command started there (N1), or a code:
//      END, malformed, header cut by the window, next command past the window;
//   2. N2 = N1.N1, N4, N8, N16 by pointer doubling (codes propagate; N16
//      takes N4's place once N8 is built);
//   3. one uniform walk takes 16 commands per step through N16, then at most
//      one N8 step and single steps near the window end; the nodes in between
//      are expanded in parallel.
// So a 4 KiB window of ~300 commands costs ~25 dependent LDS reads instead of
// ~300 serial header decodes (1 KiB, ~90 commands: ~15 instead of ~180).
//
// The window is put into LDS by the caller's loader: chain_load_wave below
// for the one-wave kernels, dec_load_window (dg_decode_dev.h) for decode and
// update.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_devutil.h"
#include "dg_stream_dev.h"

namespace dg {

template <uint32_t T>
constexpr uint32_t kChainWin = 16 * T;       // stream bytes per window: 16 window offsets per thread
template <uint32_t T>
constexpr uint32_t kChainMaxCmds = 2 * T;    // commands per window, a multiple of 16
constexpr uint16_t kChEnd = 0xFFFE;          // END at x
constexpr uint16_t kChBad = 0xFFFD;          // malformed at x
constexpr uint16_t kChCut = 0xFFFF;          // header not complete in the window: restart at x
constexpr uint16_t kChFar = 0xFFFC;          // complete command at x, next one at/after the window end
constexpr uint16_t kChSpecial = 0xFFFC;      // codes are >= this

// The parser's LDS.  N1..N8 hold kChainWin entries each and are 16-byte
// aligned; win is where the loaders put the window.
struct ChainLds {
	uint16_t *N1, *N2, *N4, *N8;
	uint8_t* win;      // kChainWin + 32, 16-byte aligned
	uint16_t* cmds;    // kChainMaxCmds: window offsets of the commands found
	uint16_t* jumps;   // kChainMaxCmds / 16 + 2: 16-command jumps, then the one 8-command jump
	uint32_t* sh;      // T = 256 only: [0..3] and [6], the walk's result for the other waves
};

template <typename P>   // P: the caller's type of a stream offset, uint32_t or uint64_t
struct ChainWindow {
	uint32_t cnt;    // commands found: l.cmds[0 .. cnt), window offsets in stream order
	uint32_t term;   // kChEnd: the stream ends here; kChBad: malformed; else more follows
	P next_pos;      // where the next window starts (<= dl)
};

// profiling hook of the parser and of decode's window step (dg_decode_dev.h):
// empty in the product
struct ChainNoProf {
	__device__ __forceinline__ void start() {}
	__device__ __forceinline__ void lap(uint32_t) {}     // the time since start() or the last lap goes to a phase
	__device__ __forceinline__ void chain(uint32_t) {}   // lap of the parser's phase k: window wait, N1, doubling, walk, expand
	__device__ __forceinline__ void count(uint32_t) {}
};

// orders LDS between the threads of the block
template <uint32_t T>
__device__ __forceinline__ void chain_barrier() {
	if constexpr (T == 64) wave_sync();
	else __syncthreads();
}

// 16 window bytes at any offset as five aligned dwords and four funnel
// shifts (an unaligned ds_read_b128 stalls the LDS pipe on gfx950,
// profiles/r05_member_census.md; decode_kernel 0.1115 -> 0.1088 ms at C5);
// the window has 32 bytes of slack.
__device__ __forceinline__ void win16(const uint8_t* p, uint32_t (&h)[4]) {
	// (the LDS address, whose alignment the compiler may know: the one-wave
	// kernels' aligned reads then cost one 16-byte load and no shift)
	const uint32_t mis = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint8_t*)p & 3u;
	const uint32_t* d = reinterpret_cast<const uint32_t*>(p - mis);
	const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], sh = 8u * mis;
	h[0] = __builtin_amdgcn_alignbit(d1, d0, sh);
	h[1] = __builtin_amdgcn_alignbit(d2, d1, sh);
	h[2] = __builtin_amdgcn_alignbit(d3, d2, sh);
	h[3] = __builtin_amdgcn_alignbit(d4, d3, sh);
}

// One window of a stream of dl bytes from offset pos < dl, a command boundary.
// w points at the window's first stream byte in LDS (inside l.win, 16 bytes of
// slack after any offset), avail = min(kChainWin, dl - pos) bytes of it are the
// stream's.  Uniform call by a block of T threads that owns l; begins with a
// barrier (the loader's stores) and ends with one (l.cmds complete).
template <uint32_t T, typename P, class Prof = ChainNoProf>
__device__ __forceinline__ ChainWindow<P> chain_window(const ChainLds& l, const uint8_t* w, uint32_t avail, P pos, P dl,
                                                       Prof&& pf = Prof()) {
	static_assert(T == 64 || T == 256, "one wave or four");
	constexpr uint32_t kWin = kChainWin<T>, kMaxCmds = kChainMaxCmds<T>;
	static_assert(kWin == 16 * T, "16 window offsets per thread");
	static_assert(kMaxCmds >= kWin / 9 && kMaxCmds % 16 == 0, "the shortest command is 9 bytes");
	const uint32_t tid = threadIdx.x, lane = lane_id();
	chain_barrier<T>();
	pf.chain(0);
	// ── 1. N1: the thread owns offsets [16 tid, 16 tid + 16): all default to
	//    malformed (two 16-byte stores), and only offsets whose byte is a
	//    command type (0, 1, 2: ~1.3 of 16 in a command stream) inside the
	//    stream are decoded ──
	{
		const uint32_t x0 = 16 * tid;
		constexpr uint32_t bb = (uint32_t)kChBad | ((uint32_t)kChBad << 16);
		uint4* dst = reinterpret_cast<uint4*>(l.N1 + x0);
		dst[0] = make_uint4(bb, bb, bb, bb);
		dst[1] = make_uint4(bb, bb, bb, bb);
		uint32_t d[4];
		win16(w + x0, d);
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
					uint32_t lw = 0;
					__builtin_memcpy(&lw, w + x + 5, 4);
					const uint64_t len = t == 1 ? 0 : __builtin_bswap32(lw);
					const uint64_t end = (uint64_t)x + hdr + len;
					if (pos + end > dl) nx = kChBad;
					else nx = end >= avail ? kChFar : (uint32_t)end;
				}
			}
			l.N1[x] = (uint16_t)nx;
		}
	}
	chain_barrier<T>();
	pf.chain(1);
	// ── 2. pointer doubling (16 offsets per thread: two 16-byte reads, 16
	//    independent gathers, two 16-byte stores) ──
	auto dbl = [&](const uint16_t* src, uint16_t* dstN) {
		const uint32_t x0 = 16 * tid;
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
	chain_barrier<T>();
	dbl(l.N2, l.N4);
	chain_barrier<T>();
	dbl(l.N4, l.N8);
	chain_barrier<T>();
	dbl(l.N8, N16);
	chain_barrier<T>();
	pf.chain(2);
	// ── 3. the walk (one wave, uniform): 16 commands per N16 step, at most one
	//    N8 step, then single steps ──
	struct Walk {
		uint32_t cnt, nj, x, term, n8;
	};
	auto walk = [&]() {
		uint32_t x = 0, nj = 0, n8 = 0, term = 0;
		while (true) {
			const uint32_t y = uni(N16[x]);
			if (y >= kChSpecial || 16 * (nj + 1) > kMaxCmds) break;
			if (lane == 0) l.jumps[nj] = (uint16_t)x;
			++nj;
			x = y;
		}
		uint32_t cnt = 16 * nj;
		{
			const uint32_t y = uni(l.N8[x]);
			if (y < kChSpecial && cnt + 8 <= kMaxCmds) {
				if (lane == 0) l.jumps[nj] = (uint16_t)x;
				n8 = 1;
				cnt += 8;
				x = y;
			}
		}
		while (true) {   // single steps from x (at most 7 commands + the terminal)
			const uint32_t y = uni(l.N1[x]);
			if (y == kChEnd || y == kChBad || y == kChCut) { term = y; break; }
			if (cnt >= kMaxCmds) { term = kChCut; break; }   // restart the window at x
			if (lane == 0) l.cmds[cnt] = (uint16_t)x;
			++cnt;
			if (y == kChFar) { term = kChFar; break; }
			x = y;
		}
		return Walk{cnt, nj, x, term, n8};
	};
	Walk k;
	if constexpr (T == 64) {
		k = walk();
		chain_barrier<T>();
	} else {   // wave 0 walks; the others take its result from LDS
		if (tid < 64) {
			k = walk();
			if (lane == 0) {
				l.sh[0] = k.cnt;
				l.sh[1] = k.nj;
				l.sh[2] = k.x;
				l.sh[3] = k.term;
				l.sh[6] = k.n8;
			}
		}
		chain_barrier<T>();
		k = Walk{l.sh[0], l.sh[1], l.sh[2], l.sh[3], l.sh[6]};
	}
	pf.chain(3);
	// expand the jumps: 8 nodes from each base (e, N1 e, N2 e, ..., N1 N2 N2 N2 e);
	// a 16-command jump has bases e and N8 e
	for (uint32_t q = tid; q < 2 * k.nj + k.n8; q += T) {
		const uint32_t j = q >> 1;
		const uint32_t e0 = j < k.nj ? ((q & 1) ? l.N8[l.jumps[j]] : l.jumps[j]) : l.jumps[k.nj];
		const uint32_t e2 = l.N2[e0];
		const uint32_t e4 = l.N2[e2];
		const uint32_t e6 = l.N2[e4];
		uint16_t* c = l.cmds + (j < k.nj ? 16 * j + 8 * (q & 1) : 16 * k.nj);
		c[0] = (uint16_t)e0;
		c[1] = l.N1[e0];
		c[2] = (uint16_t)e2;
		c[3] = l.N1[e2];
		c[4] = (uint16_t)e4;
		c[5] = l.N1[e4];
		c[6] = (uint16_t)e6;
		c[7] = l.N1[e6];
	}
	chain_barrier<T>();   // cmds complete; N2..N8 dead
	pf.chain(4);
	ChainWindow<P> r;
	r.cnt = k.cnt;
	r.term = k.term;
	r.next_pos = pos + k.x;   // kChCut: restart at x
	if (k.term == kChFar) r.next_pos = pos + k.x + (w[k.x] == 1 ? 13u : 9u + be32(w + k.x + 5));
	return r;
}

// ── the one-wave kernels' window ──

// LDS of one wave's parser, carved from a 16-byte aligned block
constexpr uint32_t kChainLdsBytes =
    4 * 2 * kChainWin<64> + (kChainWin<64> + 32) + 2 * kChainMaxCmds<64> + 2 * (kChainMaxCmds<64> / 16 + 2) + 12;
__device__ __forceinline__ ChainLds chain_lds(void* base) {
	constexpr uint32_t kWin = kChainWin<64>;
	ChainLds l;
	l.N1 = static_cast<uint16_t*>(base);
	l.N2 = l.N1 + kWin;
	l.N4 = l.N2 + kWin;
	l.N8 = l.N4 + kWin;
	l.win = reinterpret_cast<uint8_t*>(l.N8 + kWin);
	l.cmds = reinterpret_cast<uint16_t*>(l.win + kWin + 32);
	l.jumps = l.cmds + kChainMaxCmds<64>;
	l.sh = nullptr;
	return l;
}

// The window of stream D (dl bytes) at pos < dl to win, win[x] = D[pos + x]:
// unaligned dwords that fit, then the last bytes, so only bytes
// [pos, min(pos + kChainWin<64>, dl)) of the stream are read.  Returns avail.
__device__ __forceinline__ uint32_t chain_load_wave(uint8_t* win, const uint8_t* D, uint32_t dl, uint32_t pos) {
	const uint32_t lane = lane_id();
	const uint32_t avail = umin32(kChainWin<64>, dl - pos);
	uint32_t* w32 = reinterpret_cast<uint32_t*>(win);
	for (uint32_t k = lane; 4 * k + 4 <= avail; k += 64) w32[k] = *reinterpret_cast<const u32_u*>(D + pos + 4 * k);
	if (lane < (avail & 3u)) win[(avail & ~3u) + lane] = D[pos + (avail & ~3u) + lane];
	return avail;
}

}  // namespace dg
