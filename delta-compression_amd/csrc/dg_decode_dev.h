// dg_decode_dev.h — the decode side's device functions: the LDS layout of a
// four-wave block, the window step (load, the command chain of
// dg_parse_chain.h, the bounds and order checks), the flat and grouped apply,
// and the in-kernel CRC segment helpers.  Used by decode_kernel
// (dg_kernels.hip) and the in-place update kernel (dg_update_dev.hip, the
// stand-alone code object lib/dg_update.hsaco).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_device.h"
#include "dg_devutil.h"
#include "dg_crc.h"
#include "dg_parse_chain.h"

namespace dg {

// wave-wide memmove of len bytes (src and dst may overlap)
__device__ void wave_memmove(uint8_t* dst, const uint8_t* src, uint64_t len) {
	const uint32_t lane = lane_id();
	if (len == 0 || dst == src) return;
	const bool backward = dst > src && dst < src + len;
	const uint64_t chunk = 64 * 4;
	const uint64_t nch = (len + chunk - 1) / chunk;
	for (uint64_t c = 0; c < nch; ++c) {
		const uint64_t cc = backward ? nch - 1 - c : c;
		const uint64_t base = cc * chunk + 4ull * lane;
		uint8_t b[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) b[k] = base + k < len ? src[base + k] : 0;
		// every lane's loads of this chunk complete before any store
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__builtin_amdgcn_wave_barrier();
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if (base + k < len) dst[base + k] = b[k];
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__builtin_amdgcn_wave_barrier();
	}
}

__device__ __forceinline__ bool overlap(uint64_t a, uint64_t al, uint64_t b, uint64_t bl) {
	return al && bl && a < b + bl && b < a + al;
}

// profiling build only (make prof): per-phase decode cycles.  DP_LOAD..DP_EXP
// are the parser's phases (ChainNoProf::chain) in its order.
enum { DP_FILL, DP_LOAD, DP_N1, DP_DBL, DP_WALK, DP_EXP, DP_HDR, DP_COPY, DP_WAIT, DP_WINDOWS, DP_BATCHES, DP_TOTAL,
       DP_ORDERED, DP_C_CMD, DP_C_FLAT, DP_C_BAR, DP_CRC_SYNC, DP_CRC_SEG, DP_CRC_TAIL, kDecProfN };
#ifdef DG_ONEPASS_PROF
__device__ unsigned long long g_decode_prof[kDecProfN];
#define DPROF_T(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define DPROF_ADD(i, t0) (dprof[(i)] += __builtin_amdgcn_s_memtime() - (t0))
#define DPROF_INC(i) (dprof[(i)] += 1)
struct DecProf {   // the window step's hook: laps into the kernel's dprof
	uint64_t* d;
	uint64_t t;
	__device__ __forceinline__ void start() { t = __builtin_amdgcn_s_memtime(); }
	__device__ __forceinline__ void lap(uint32_t i) {
		const uint64_t now = __builtin_amdgcn_s_memtime();
		d[i] += now - t;
		t = now;
	}
	__device__ __forceinline__ void chain(uint32_t k) { lap(DP_LOAD + k); }
	__device__ __forceinline__ void count(uint32_t i) { d[i] += 1; }
};
#define DPROF_HOOK DecProf{dprof, 0}
extern "C" int dg_decode_prof_read(unsigned long long* out, int n) {
	if (n > kDecProfN) n = kDecProfN;
	return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_decode_prof), 8 * n) == hipSuccess ? n : -1;
}
extern "C" int dg_decode_prof_reset(void) {
	unsigned long long z[kDecProfN] = {};
	return hipMemcpyToSymbol(HIP_SYMBOL(g_decode_prof), z, sizeof z) == hipSuccess ? 0 : -1;
}
#else
#define DPROF_T(v) ((void)0)
#define DPROF_ADD(i, t0) ((void)0)
#define DPROF_INC(i) ((void)0)
#define DPROF_HOOK ChainNoProf{}
#endif

// ── decode: one 256-thread block (4 waves) per delta stream ──
//
// Per window (4 KiB of the stream, up to 512 commands): all four waves build
// N1..N8; wave 0 walks; all expand (chain_window<256>, dg_parse_chain.h).  The
// window's commands are then applied 64 per wave at a time, all four waves
// at once, when the window is provably order-free: destinations increasing
// and disjoint in stream order and no in-place COPY that moves (src == dst
// in-place copies are no-ops).  Any other window is applied by wave 0 alone,
// batch by batch, with the conflict check and the strict memmove replay.
// The block barrier between windows also orders every store of one window
// before the next window's reads and writes.
constexpr uint32_t kDecBlock = 256;
constexpr uint32_t kDecWin = kChainWin<kDecBlock>;           // bytes of the command stream per window
constexpr uint32_t kDecMaxCmds = kChainMaxCmds<kDecBlock>;   // commands per window
constexpr uint32_t kDecCrcSeg = 16384;                // in-kernel CRC: 16 KiB segments
static_assert(4 * kDecCrcSeg == kCrcSegBytes, "the Horner step (4 segments) is x^(8 kCrcSegBytes)");

// A block barrier that also orders global memory between the block's waves:
// every wave's stores are acknowledged (vmcnt counts stores on gfx9) before
// any wave passes, and the CU's L1 is invalidated after, so loads of bytes
// another wave of the block just wrote see them.  A plain __syncthreads
// orders LDS only (its workgroup-scope fence waits for no global store), and
// agent-scope fences would write back the XCD's L2 (~6x slower decode).
__device__ __forceinline__ void block_sync_global() {
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	asm volatile("buffer_inv sc0" ::: "memory");
}
constexpr uint32_t kDecWaves = kDecBlock / 64;

struct DecCmd {
	bool mine;
	uint32_t kind;
	uint64_t src, dst, len;
};

// big-endian u32 at byte 1 + 4i of a 16-byte header image h[4] (i = 0, 1, 2)
__device__ __forceinline__ uint32_t hdr_be32(const uint32_t (&h)[4], int i) {
	return __builtin_bswap32(__builtin_amdgcn_alignbyte(h[i + 1], h[i], 1));
}

// The window holds >= 16 bytes past any command offset (win has 32 bytes of
// slack), so a header is one 16-byte read.
template <typename WP>
__device__ __forceinline__ DecCmd dec_cmd(WP w, const uint16_t* cmds, uint32_t b, uint32_t cnt, uint64_t pos) {
	DecCmd c{false, 0, 0, 0, 0};
	const uint32_t lane = lane_id();
	c.mine = b + lane < cnt;
	if (c.mine) {
		const uint32_t cx = cmds[b + lane];
		uint32_t h[4];
		win16(w + cx, h);
		c.kind = h[0] & 0xFFu;
		if (c.kind == 1) {
			c.src = hdr_be32(h, 0);
			c.dst = hdr_be32(h, 1);
			c.len = hdr_be32(h, 2);
		} else {
			c.src = pos + cx + 9;   // payload offset in the stream
			c.dst = hdr_be32(h, 0);
			c.len = hdr_be32(h, 1);
		}
	}
	return c;
}

// A command's last, partial 16-byte chunk (1 <= rem < 16 bytes).  Every load
// is issued before any store, so the chunk costs one memory round trip: the
// dwords at offsets 0, 4, 8, 12 clamped to rem - 4 (the last one overlaps the
// one before it and stores the same bytes again), or, under 4 bytes, the
// bytes at offsets clamped to rem - 1; never a byte outside [0, rem).
// (Round 5 copied dword by dword and byte by byte, each store before the next
// load: up to 6 dependent round trips per partial chunk.)
__device__ __forceinline__ void copy_tail(uint8_t* d, const uint8_t* s, uint32_t rem) {
	if (rem >= 4) {
		uint32_t w[4], o[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			o[k] = umin32(4 * k, rem - 4);
			w[k] = *reinterpret_cast<const u32_u*>(s + o[k]);
		}
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k)
			if (4 * k < rem) *reinterpret_cast<u32_u*>(d + o[k]) = w[k];
	} else {
		uint8_t b[3];
#pragma unroll
		for (uint32_t k = 0; k < 3; ++k) b[k] = s[umin32(k, rem - 1)];
#pragma unroll
		for (uint32_t k = 0; k < 3; ++k)
			if (k < rem) d[k] = b[k];
	}
}

// Per-wave LDS scratch of the flat copy.
struct DecScratch {
	uint32_t* cum;        // [64] chunk prefix per non-empty command
	uint32_t* row;        // [128] row start masks (lo dwords, then hi dwords)
	const uint8_t** sp;   // [64]
	uint8_t** dp;         // [64]
	uint32_t* len;        // [64] bytes per non-empty command
};

// Copy an independent batch (no command overlaps another one's writes, or
// in-place, reads) in 16-byte chunks: chunk j of the batch's concatenation
// (every command cut into 16-byte chunks, its last one partial) goes to lane
// j % 64 in row j / 64; the owning command comes from per-row start masks
// (owner = starts before the row + popcount(mask bits <= lane) - 1).  Full
// chunks are one unaligned 16-byte load and store; a command's partial last
// chunk is copied by dwords and bytes, never touching the next command's
// bytes.  In-place COPYs whose source and destination overlap are memmoved
// after.
__device__ void dec_flat_batch(const DecCmd& c, bool inplace, uint8_t* O, const uint8_t* R, const uint8_t* D,
                               const DecScratch& x) {
	const uint32_t lane = lane_id();
	const uint8_t* sp = c.kind == 1 ? (inplace ? O + c.src : R + c.src) : D + c.src;
	const bool selfov = c.mine && c.kind == 1 && inplace && c.src != c.dst && overlap(c.src, c.len, c.dst, c.len);
	const bool noop = c.mine && c.kind == 1 && inplace && c.src == c.dst;
	const uint32_t flen = (c.mine && !selfov && !noop) ? (uint32_t)c.len : 0u;
	const uint32_t fch = (flen + 15u) >> 4;
	const uint32_t incl = wave_incl_scan(fch);
	const uint32_t cum = incl - fch;
	const uint32_t total = rdlane(incl, 63);   // chunks
	const bool nz = fch != 0;
	const uint32_t ord = wave_incl_scan(nz ? 1u : 0u) - 1u;
	if (nz) {
		x.cum[ord] = cum;
		x.sp[ord] = sp;
		x.dp[ord] = O + c.dst;
		x.len[ord] = flen;
	}
	for (uint32_t r0 = 0; 64 * r0 < total; r0 += 64) {   // 64 rows of 64 chunks = 64 KiB per round
		x.row[lane] = 0;
		x.row[64 + lane] = 0;
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		if (nz && cum >= 64 * r0 && cum < 64 * (r0 + 64)) {
			const uint32_t row = cum / 64 - r0, bit = cum % 64;
			atomicOr(&x.row[(bit >> 5) * 64 + row], 1u << (bit & 31));
		}
		const uint32_t carry = (uint32_t)__builtin_popcountll(__ballot(nz && cum < 64 * r0));
		__builtin_amdgcn_s_waitcnt(0xc07f);
		__builtin_amdgcn_wave_barrier();
		const uint64_t mrow = ((uint64_t)x.row[64 + lane] << 32) | x.row[lane];   // row r0 + lane
		const uint32_t pc = (uint32_t)__builtin_popcountll(mrow);
		const uint32_t rbase = carry + wave_incl_scan(pc) - pc;   // starts before row r0 + lane
		const uint32_t nrows = min(64u, (total + 63) / 64 - r0);
		constexpr int kQ = 4;   // rows per pass (VGPR budget: 4 waves per SIMD)
		for (uint32_t q0 = 0; q0 < nrows; q0 += kQ) {
			uint8_t* da[kQ];
			const uint8_t* sa[kQ];
			u32x4_u v[kQ];
			uint32_t rem[kQ];
#pragma unroll
			for (int uu = 0; uu < kQ; ++uu) {
				const uint32_t u = q0 + uu;
				const uint32_t j = 64 * (r0 + u) + lane;
				const bool ok = u < nrows && j < total;
				const uint64_t m = ((uint64_t)rdlane((uint32_t)(mrow >> 32), u) << 32) | rdlane((uint32_t)mrow, u);
				const uint32_t oo = rdlane(rbase, u) + (uint32_t)__builtin_popcountll(m & mask_le(lane));
				const uint32_t o = ok && oo ? oo - 1u : 0u;
				const uint32_t boff = 16u * (j - x.cum[o]);
				rem[uu] = ok ? x.len[o] - boff : 0u;   // >= 1 for a valid chunk
				sa[uu] = x.sp[o] + boff;
				da[uu] = x.dp[o] + boff;
				v[uu] = rem[uu] >= 16 ? *reinterpret_cast<const u32x4_u*>(sa[uu]) : u32x4_u{0, 0, 0, 0};
			}
#pragma unroll
			for (int uu = 0; uu < kQ; ++uu) {
				if (rem[uu] >= 16) {
					*reinterpret_cast<u32x4_u*>(da[uu]) = v[uu];
				} else if (rem[uu]) {   // the command's last, partial chunk
					copy_tail(da[uu], sa[uu], rem[uu]);
				}
			}
		}
	}
	for (uint64_t m = __ballot(selfov); m; m &= m - 1) {
		const uint32_t kk = ffs64(m);
		const uint64_t ks = ((uint64_t)rdlane((uint32_t)(c.src >> 32), kk) << 32) | rdlane((uint32_t)c.src, kk);
		const uint64_t kd = ((uint64_t)rdlane((uint32_t)(c.dst >> 32), kk) << 32) | rdlane((uint32_t)c.dst, kk);
		const uint64_t kl = ((uint64_t)rdlane((uint32_t)(c.len >> 32), kk) << 32) | rdlane((uint32_t)c.len, kk);
		wave_memmove(O + kd, O + ks, kl);
	}
}

// ── windows that are not order-free (in-place deltas whose COPYs move):
// conflict-free groups, applied by the whole block ──
//
// The reference replays such a stream strictly in order, one memmove per
// command (apply.c:253-267).  Two commands commute unless one writes bytes
// the other reads or writes, so the window is cut into groups: a group is
// the longest run of consecutive commands none of which conflicts with an
// earlier command of the run.  A group's bytes are independent and are
// copied by all four waves at once in 16-byte chunks; a COPY whose own source
// and destination overlap (a real memmove) is a group of its own, moved by
// the block in 4 KiB passes in the direction that never reads a byte it has
// already written.  Block barriers that order global memory separate groups.
struct DecGroupLds {
	uint32_t* src;    // [kDecMaxCmds] COPY source (O or R offset); ADD: payload offset in the window
	uint32_t* dst;    // [kDecMaxCmds]
	uint32_t* len;    // [kDecMaxCmds]
	uint32_t* pre;    // [kDecMaxCmds + 1] exclusive prefix of the 16-byte chunks each command copies
	int16_t* last;    // [kDecMaxCmds] latest earlier command it conflicts with, -1: none
	uint8_t* flag;    // [kDecMaxCmds] kGf* bits
	uint16_t* gs;     // [kDecMaxCmds + 1] group starts, then cnt
	uint32_t* red;    // [8] block scratch
};
constexpr uint8_t kGfCopy = 1, kGfReadsOut = 2, kGfWrites = 4, kGfSelf = 8;

__device__ __forceinline__ bool ov32(uint32_t a, uint32_t al, uint32_t b, uint32_t bl) {
	return al && bl && a < b + bl && b < a + al;
}

template <typename WP>
__device__ void dec_grouped_window(WP w, const uint16_t* cmds, uint32_t cnt, uint64_t pos, bool inplace, uint8_t* O,
                                   const uint8_t* R, const uint8_t* D, const DecGroupLds& g) {
	const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
	static_assert(kDecMaxCmds == 2 * kDecBlock, "two commands per thread in the prefix");
	// 1. headers -> LDS, flags, chunk counts (two consecutive commands per thread)
	uint32_t f2[2];
#pragma unroll
	for (int u = 0; u < 2; ++u) {
		const uint32_t c = 2 * tid + u;
		f2[u] = 0;
		if (c < cnt) {
			const uint32_t cx = cmds[c];
			uint32_t h[4];
			win16(w + cx, h);
			const bool copy = (h[0] & 0xFFu) == 1u;
			const uint32_t src = copy ? hdr_be32(h, 0) : cx + 9u;
			const uint32_t dst = copy ? hdr_be32(h, 1) : hdr_be32(h, 0);
			const uint32_t len = copy ? hdr_be32(h, 2) : hdr_be32(h, 1);
			const bool noop = inplace && copy && src == dst;   // memmove onto itself
			const bool writes = len != 0 && !noop;
			const bool reads_out = inplace && copy && writes;
			const bool self = reads_out && ov32(src, len, dst, len);
			g.src[c] = src;
			g.dst[c] = dst;
			g.len[c] = len;
			g.flag[c] = (copy ? kGfCopy : 0) | (reads_out ? kGfReadsOut : 0) | (writes ? kGfWrites : 0) |
			            (self ? kGfSelf : 0);
			f2[u] = writes && !self ? (len + 15u) >> 4 : 0u;
		}
	}
	{
		const uint32_t v = f2[0] + f2[1];
		const uint32_t incl = wave_incl_scan(v);
		if (lane == 63) g.red[wave] = incl;
		__syncthreads();
		uint32_t off = 0;
		for (uint32_t k = 0; k < wave; ++k) off += g.red[k];
		g.pre[2 * tid] = off + incl - v;
		g.pre[2 * tid + 1] = off + incl - v + f2[0];
		if (tid == kDecBlock - 1) g.pre[kDecMaxCmds] = off + incl;
	}
	__syncthreads();
	// 2. the latest earlier command each one conflicts with (write/write,
	//    write/read, read/write; only in-place COPYs read the output)
	for (uint32_t c = tid; c < cnt; c += kDecBlock) {
		const uint8_t fc = g.flag[c];
		int32_t L = -1;
		if (fc & kGfWrites) {
			const uint32_t sc = g.src[c], dc = g.dst[c], lc = g.len[c];
			const bool rc = fc & kGfReadsOut;
			for (int32_t e = (int32_t)c - 1; e >= 0; --e) {
				const uint8_t fe = g.flag[e];
				if (!(fe & kGfWrites)) continue;
				const uint32_t se = g.src[e], de = g.dst[e], le = g.len[e];
				if (ov32(de, le, dc, lc) || (rc && ov32(de, le, sc, lc)) || ((fe & kGfReadsOut) && ov32(se, le, dc, lc))) {
					L = e;
					break;
				}
			}
		}
		g.last[c] = (int16_t)L;
	}
	__syncthreads();
	// 3. group starts (wave 0): a group ends before the first command that
	//    conflicts with one of the group's, and around every self-overlapping move
	if (wave == 0) {
		uint32_t s = 0, ng = 1;
		if (lane == 0) g.gs[0] = 0;
		for (uint32_t c0 = 1; c0 < cnt; c0 += 64) {
			const uint32_t c = c0 + lane;
			const bool live = c < cnt;
			const int32_t lc = live ? (int32_t)g.last[c] : -1;
			const bool sf = live && ((g.flag[c] & kGfSelf) || (g.flag[c - 1] & kGfSelf));
			for (;;) {
				const uint64_t m = __ballot(live && c > s && (lc >= (int32_t)s || sf));
				if (!m) break;
				const uint32_t b = c0 + ffs64(m);
				if (lane == 0) g.gs[ng] = (uint16_t)b;
				++ng;
				s = b;
			}
		}
		if (lane == 0) {
			g.gs[ng] = (uint16_t)cnt;
			g.red[4] = ng;
		}
	}
	__syncthreads();
	const uint32_t ng = g.red[4];
	// 4. the groups, in stream order
	for (uint32_t k = 0; k < ng; ++k) {
		const uint32_t s = g.gs[k], e = g.gs[k + 1];
		if (e == s + 1 && (g.flag[s] & kGfSelf)) {
			// one in-place COPY onto an overlapping range: memmove by the block
			const uint32_t len = g.len[s];
			const uint8_t* sp = O + g.src[s];
			uint8_t* dp = O + g.dst[s];
			const bool backward = dp > sp;
			const uint32_t npass = (len + 16u * kDecBlock - 1) / (16u * kDecBlock);
			for (uint32_t q = 0; q < npass; ++q) {
				const uint32_t pass = backward ? npass - 1 - q : q;
				const uint32_t b = pass * 16u * kDecBlock + 16u * tid;
				const uint32_t n = b < len ? umin32(len - b, 16u) : 0u;
				u32x4_u v{0, 0, 0, 0};
				uint8_t t[16];
				if (n == 16) {
					v = *reinterpret_cast<const u32x4_u*>(sp + b);
				} else {
					for (uint32_t i = 0; i < n; ++i) t[i] = sp[b + i];
				}
				// every thread's loads of this pass land before any store of
				// it; later passes read only bytes no earlier pass wrote
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__syncthreads();
				if (n == 16) {
					*reinterpret_cast<u32x4_u*>(dp + b) = v;
				} else {
					for (uint32_t i = 0; i < n; ++i) dp[b + i] = t[i];
				}
			}
		} else {
			// independent commands: chunk j of the group -> thread j % 256
			const uint32_t j0 = g.pre[s], j1 = g.pre[e];
			constexpr int kQ = 4;   // chunks in flight per thread
			for (uint32_t jb = j0; jb < j1; jb += kQ * kDecBlock) {
				uint8_t* da[kQ];
				const uint8_t* sa[kQ];
				u32x4_u v[kQ];
				uint32_t rem[kQ];
#pragma unroll
				for (int u = 0; u < kQ; ++u) {
					const uint32_t j = jb + u * kDecBlock + tid;
					rem[u] = 0;
					da[u] = O;
					sa[u] = O;
					if (j < j1) {
						uint32_t lo = s, hi = e;   // the command holding chunk j: pre[lo] <= j < pre[lo + 1]
						while (hi - lo > 1) {
							const uint32_t mid = (lo + hi) >> 1;
							if (g.pre[mid] <= j) lo = mid;
							else hi = mid;
						}
						const uint32_t boff = 16u * (j - g.pre[lo]);
						rem[u] = g.len[lo] - boff;
						const uint8_t fl = g.flag[lo];
						sa[u] = ((fl & kGfCopy) ? ((fl & kGfReadsOut) ? O : R) + g.src[lo] : D + pos + g.src[lo]) + boff;
						da[u] = O + g.dst[lo] + boff;
					}
					v[u] = rem[u] >= 16 ? *reinterpret_cast<const u32x4_u*>(sa[u]) : u32x4_u{0, 0, 0, 0};
				}
#pragma unroll
				for (int u = 0; u < kQ; ++u) {
					if (rem[u] >= 16) {
						*reinterpret_cast<u32x4_u*>(da[u]) = v[u];
					} else if (rem[u]) {   // the command's last, partial chunk
						copy_tail(da[u], sa[u], rem[u]);
					}
				}
			}
		}
		block_sync_global();   // the group's stores land before the next group reads or writes
	}
}

// ── the block's LDS and the window step ──
//
// A kernel declares one `__shared__ DecLdsMem M;` and dec_lds carves it.  NX
// holds N2, N4, N8 during the parse; afterwards the waves' flat-copy scratch,
// then the grouped apply's arrays (or, outside the window loop, the CRC
// tables: dec_crc_tables).
struct DecLdsMem {
	alignas(16) uint8_t win[kDecWin + 32];
	alignas(16) uint16_t N1[kDecWin];
	alignas(16) uint16_t NX[3 * kDecWin];
	uint16_t cmds[kDecMaxCmds];
	uint16_t jumps[kDecMaxCmds / 16 + 2];    // 16-command jumps, then the one 8-command jump
	uint32_t sh[8];                          // walk results and window flags
	uint32_t bsum[2 * (kDecMaxCmds / 64 + 1)];
};
struct DecLds {
	ChainLds ch;       // win, N1, N2..N8 (NX), cmds, jumps, sh ([0..3], [6]: the walk's result)
	uint16_t* NX;
	uint32_t* sh;      // [4]: a batch out of bounds, [5]: the window is not order-free
	uint32_t* bsum;    // per batch of 64 commands: first written dst, max end
	DecScratch xs;     // this wave's
	DecGroupLds grp;
};
__device__ __forceinline__ DecLds dec_lds(DecLdsMem& M) {
	uint16_t* const NX = M.NX;
	constexpr uint32_t kScratch = 64 * 4 + 128 * 4 + 64 * 8 + 64 * 8 + 64 * 4;
	static_assert(kDecWaves * kScratch <= 3 * kDecWin * 2, "scratch fits NX");
	static_assert(kDecWaves * kScratch + 4 * (4 * kDecMaxCmds + 4 + 8) + 2 * (2 * kDecMaxCmds + 2) + kDecMaxCmds <=
	                  3 * kDecWin * 2,
	              "grouped-apply arrays fit NX");
	DecLds L;
	L.ch = ChainLds{M.N1, NX, NX + kDecWin, NX + 2 * kDecWin, M.win, M.cmds, M.jumps, M.sh};
	L.NX = NX;
	L.sh = M.sh;
	L.bsum = M.bsum;
	uint8_t* base = reinterpret_cast<uint8_t*>(NX) + (threadIdx.x >> 6) * kScratch;
	L.xs.sp = reinterpret_cast<const uint8_t**>(base);
	L.xs.dp = reinterpret_cast<uint8_t**>(base + 64 * 8);
	L.xs.cum = reinterpret_cast<uint32_t*>(base + 128 * 8);
	L.xs.row = reinterpret_cast<uint32_t*>(base + 128 * 8 + 64 * 4);
	L.xs.len = reinterpret_cast<uint32_t*>(base + 128 * 8 + 64 * 4 + 128 * 4);
	DecGroupLds& g = L.grp;   // after the four waves' flat-copy scratch
	g.src = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(NX) + kDecWaves * kScratch);
	g.dst = g.src + kDecMaxCmds;
	g.len = g.dst + kDecMaxCmds;
	g.pre = g.len + kDecMaxCmds;                                  // kDecMaxCmds + 1 (+3 pad)
	g.red = g.pre + kDecMaxCmds + 4;                              // 8
	g.last = reinterpret_cast<int16_t*>(g.red + 8);               // kDecMaxCmds
	g.gs = reinterpret_cast<uint16_t*>(g.last + kDecMaxCmds);     // kDecMaxCmds + 1 (+1 pad)
	g.flag = reinterpret_cast<uint8_t*>(g.gs + kDecMaxCmds + 2);
	return L;
}

// The window at pos to LDS: the aligned 16-byte blocks that hold stream bytes
// (a block never crosses a page); returns shf, win[shf + x] = D[pos + x].
// The caller puts a barrier after it (chain_window begins with one).
__device__ __forceinline__ uint32_t dec_load_window(uint8_t* win, const uint8_t* D, uint64_t dl, uint64_t pos) {
	const uintptr_t wa = (uintptr_t)(D + pos) & ~(uintptr_t)15;
	const uintptr_t dend = (uintptr_t)(D + dl);
	for (uint32_t q = threadIdx.x; q < (kDecWin + 32) / 16; q += kDecBlock) {
		const uintptr_t ad = wa + 16 * q;
		uint4 x = make_uint4(0, 0, 0, 0);
		if (ad < dend) x = *reinterpret_cast<const uint4*>(ad);
		reinterpret_cast<uint4*>(win)[q] = x;
	}
	return (uint32_t)((uintptr_t)(D + pos) - wa);
}

struct DecWin {
	uint32_t cnt;        // commands of the window, their offsets in cmds
	uint32_t shf;        // win + shf is the window's first stream byte
	uint64_t next_pos;   // where the next window starts
	bool done;           // END seen
	bool bad;            // malformed, or a command out of bounds
	bool free_win;       // order-free: applied flat
};

// One window of the stream at pos < dl (a command boundary): the window to
// LDS, its command chain, and the bounds (dst + len <= lim_dst, a COPY's
// src + len <= lim_src) and order checks of every batch of 64 commands.
// Every thread returns the same values.  The caller puts a block barrier
// between two calls.
template <class Prof = ChainNoProf>
__device__ __forceinline__ DecWin dec_window(const DecLds& L, const uint8_t* D, uint64_t dl, uint64_t pos, bool inplace,
                                             uint64_t lim_dst, uint64_t lim_src, Prof&& pf = Prof()) {
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	DecWin r{};
	pf.count(DP_WINDOWS);
	pf.start();
	if (tid == 0) L.sh[4] = L.sh[5] = 0;
	r.shf = dec_load_window(L.ch.win, D, dl, pos);
	const uint8_t* w = L.ch.win + r.shf;
	const auto cw = chain_window<kDecBlock>(L.ch, w, (uint32_t)min((uint64_t)kDecWin, dl - pos), pos, dl, pf);
	r.cnt = cw.cnt;
	r.next_pos = cw.next_pos;
	r.done = cw.term == kChEnd;
	r.bad = cw.term == kChBad;
	// bounds and order checks of every batch (waves in parallel)
	const uint32_t nb = (r.cnt + 63) / 64;
	for (uint32_t b = wave; b < nb; b += kDecWaves) {
		const DecCmd c = dec_cmd(w, L.ch.cmds, 64 * b, r.cnt, pos);
		bool bad = false;
		if (c.mine) {
			if (c.dst + c.len > lim_dst) bad = true;
			if (c.kind == 1 && c.src + c.len > lim_src) bad = true;
		}
		// order-free: the commands that write (an in-place COPY with src ==
		// dst writes nothing: apply.c:257-266 memmoves a range onto itself,
		// and the in-place format puts the ADDs after the COPYs,
		// inplace.c:711-725) have increasing, disjoint destinations (< 2^32:
		// lim_dst checked), and no in-place COPY moves.  Within the batch by a
		// prefix max of the write ends; across batches by the summaries.
		const bool writes = c.mine && c.len != 0 && !(inplace && c.kind == 1 && c.src == c.dst);
		const uint32_t end32 = writes ? (uint32_t)(c.dst + c.len) : 0u, dst32 = (uint32_t)c.dst;
		const uint32_t incl_end = wave_incl_max(end32);
		const bool unordered = writes && dst32 < wave_shr1z(incl_end);
		const bool moves = c.mine && inplace && c.kind == 1 && c.src != c.dst;
		const uint64_t wm = __ballot(writes);
		const uint32_t first_dst = wm ? rdlane(dst32, ffs64(wm)) : ~0u;
		if (lane == 0) {
			L.bsum[2 * b] = first_dst;
			L.bsum[2 * b + 1] = rdlane(incl_end, 63);
		}
		if (__ballot(bad) && lane == 0) atomicOr(&L.sh[4], 1u);
		if (__ballot(unordered || moves) && lane == 0) atomicOr(&L.sh[5], 1u);
	}
	__syncthreads();
	if (L.sh[4]) r.bad = true;
	bool cross = false;   // a batch writes below the end of an earlier batch's writes
	for (uint32_t b = 0, run = 0; b < nb; ++b) {
		const uint32_t f = L.bsum[2 * b], e = L.bsum[2 * b + 1];
		if (f != ~0u) {
			cross = cross || f < run;
			run = umax32(run, e);
		}
	}
	r.free_win = !L.sh[5] && !cross;
	if (!r.free_win) pf.count(DP_ORDERED);
	pf.lap(DP_HDR);
	return r;
}

// The decode kernel's CRC segments: 16 KiB segments as rows of 64 x 8 bytes
// (dg_crc.h).  The byte tables go to LDS at tb (256-byte aligned, inside the
// dead doubling arrays), then the nibble table of x^(8 * 64 KiB) (the Horner
// step of a wave's segments) at TK.
constexpr int kDecTab = kCrcByte;
constexpr uint32_t kDecTabWords = 8 * 256;
struct DecCrc {
	uint32_t tb;
	const uint64_t* TK;
	uint64_t klane;
};
__device__ __forceinline__ DecCrc dec_crc_tables(uint16_t* NX, const DecodeArgs& a) {
	const uint32_t tid = threadIdx.x;
	const uint32_t base = lds_addr(NX), tb = (base + 255u) & ~255u;
	uint64_t* T = reinterpret_cast<uint64_t*>(NX) + (tb - base) / 8;
	const uint64_t* src = a.tables + kCrcRows8;
	for (uint32_t k = tid; k < kDecTabWords; k += kDecBlock) T[k] = src[k];
	uint64_t* TK = T + kDecTabWords;
	const uint64_t* KF = a.tables + 8 * 256 + kCrcLevels * kCrcNibTabWords;
	for (uint32_t k = tid; k < kCrcNibTabWords; k += kDecBlock) TK[k] = KF[k];   // x^(8 * 64 KiB)
	static_assert(8 * (8 * 256 + kCrcNibTabWords) + 256 <= 3 * kDecWin * 2, "CRC tables fit NX");
	return DecCrc{tb, TK, a.tables[kCrcRowK8 + lane_id()]};
}
template <bool kCopy = false>
__device__ __forceinline__ uint64_t dec_seg_crc(const DecCrc& t, uintptr_t start, uint64_t len, uint32_t nseg,
                                                uint32_t j, intptr_t copy_delta = 0, uintptr_t copy_hi = 0) {
	return crc_seg_rows<8, 1, 8, kDecCrcSeg, kCopy, kDecTab>(start, len, nseg, j, t.tb, t.tb, t.klane, copy_delta, copy_hi);
}

}  // namespace dg
