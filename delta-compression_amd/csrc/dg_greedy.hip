// dg_greedy.hip — the greedy encoder (src/c/greedy.c:88-267) for gfx950.
//
// Greedy takes, at every position v_c of V, the longest match among all
// offsets a of R whose p-byte seed equals V[v_c .. v_c + p); its output does
// not depend on the reference's hash table: the candidates are exactly the
// equal seeds, the winner is the longest, and among the longest the largest
// offset (hash table: head-inserted chains, strict >) or, with --splay, the
// smallest.  So the index here is whatever suits the GPU:
//
//   index   per pair a CSR bucket index over every seed of R: nb buckets (a
//           power of two >= the seed count), heads[nb + 1] and one (offset,
//           tag) entry per seed, grouped by bucket.  The hash covers the
//           seed's first min(p, 16) bytes; its high half is the tag, by which
//           a candidate is rejected without touching R.  Built on the run
//           stream in three steps (count with atomics, per-pair exclusive
//           scan, scatter) after heads is zeroed, so every word a walk reads
//           is rewritten by every run.  The order of a bucket's entries
//           depends on the atomics' arrival order; the scan's result does not
//           (below).  A walk is bounded by [heads[b], heads[b + 1]), clamped
//           to the pair's entries, and every offset is checked against
//           |R| - p before R is read.
//   scan    one wave per pair.  Miss run: lane l looks position v_c + l up
//           (a miss does not depend on the encoder's state), the lowest lane
//           with a verified candidate is where greedy stops.  Match: the
//           position's bucket, 64 candidates at a time; each lane extends its
//           own candidate in 8-byte words, a candidate whose cap min(|R| - a,
//           |V| - v_c) cannot beat the best so far under (length, offset) is
//           skipped, one longer than kLaneExt is extended by the whole wave
//           (64 x 16 bytes a step); the winner is the maximum of (length,
//           offset or ~offset), which no visiting order changes.
//
// Records are the onepass layout (v, r, len, head: kRecWordsOnepass), sizes
// and status as the other scans write them, so scan_sizes_kernel, the
// serialiser and the CRC passes run unchanged.
//
// Reads never pass R + |R| or V + |V|: every multi-byte load is an unaligned
// load that ends inside the buffer, tails are read bytewise.
#include <hip/hip_runtime.h>

#include "dg_device.h"
#include "dg_devutil.h"

namespace dg {

namespace {

constexpr uint32_t kGreedyBlock = 256;            // build kernels
constexpr uint32_t kGreedySeedsPerThread = 16;
constexpr uint32_t kGreedySeedsPerBlock = kGreedyBlock * kGreedySeedsPerThread;
constexpr uint32_t kGreedyScanBlock = 1024;       // the heads scan: 4 buckets per thread per step
constexpr uint32_t kLaneExt = 256;                // a lane's own extension; longer candidates go to the wave

// the bytes [off, off + 4) of B below `end`, zero above it
__device__ __forceinline__ uint32_t ld4_below(const uint8_t* B, uint32_t off, uint32_t end) {
	uint32_t w = 0;
	if (off + 4u <= end) {
		__builtin_memcpy(&w, B + off, 4);
	} else {
		for (uint32_t b = 0; b < 4u && off + b < end; ++b) w |= (uint32_t)B[off + b] << (8u * b);
	}
	return w;
}

// hash of the k <= 16 bytes B[off .. off + k): low bits = bucket, high half = tag
__device__ __forceinline__ uint64_t seed_hash(const uint8_t* B, uint32_t off, uint32_t k) {
	uint32_t w[4];
	if (k == 16u) {
		__builtin_memcpy(w, B + off, 16);
	} else {
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) w[j] = ld4_below(B, off + 4u * j, off + k);
	}
	uint64_t h = (((uint64_t)w[1] << 32) | w[0]) * 0x9E3779B97F4A7C15ull;
	h ^= h >> 29;
	h += ((uint64_t)w[3] << 32) | w[2];
	h *= 0xBF58476D1CE4E5B9ull;
	h ^= h >> 32;
	h *= 0x94D049BB133111EBull;
	h ^= h >> 29;
	return h;
}

// equal leading bytes of A[] and B[], at most `limit` (one lane's own loop)
__device__ __forceinline__ uint32_t lane_prefix(const uint8_t* A, const uint8_t* B, uint32_t limit) {
	uint32_t n = 0;
	while (n + 8u <= limit) {
		uint64_t x, y;
		__builtin_memcpy(&x, A + n, 8);
		__builtin_memcpy(&y, B + n, 8);
		const uint64_t d = x ^ y;
		if (d) return n + ((uint32_t)__builtin_ctzll(d) >> 3);
		n += 8u;
	}
	while (n < limit && A[n] == B[n]) ++n;
	return n;
}

// the same by the whole wave from `from` on (equal up to there): 16 bytes per
// lane per step.  Uniform call, uniform result.
__device__ __forceinline__ uint32_t wave_prefix(const uint8_t* A, const uint8_t* B, uint32_t from, uint32_t limit) {
	const uint32_t lane = lane_id();
	for (uint32_t n = from; n < limit; n += 1024u) {
		const uint32_t o = n + 16u * lane;
		const uint32_t len = o < limit ? umin32(16u, limit - o) : 0u;
		uint32_t m = 0;   // equal leading bytes of this lane's piece
		if (len == 16u) {
			uint64_t x[2], y[2];
			__builtin_memcpy(x, A + o, 16);
			__builtin_memcpy(y, B + o, 16);
			const uint64_t d0 = x[0] ^ y[0], d1 = x[1] ^ y[1];
			m = d0 ? (uint32_t)__builtin_ctzll(d0) >> 3 : (d1 ? 8u + ((uint32_t)__builtin_ctzll(d1) >> 3) : 16u);
		} else {
			while (m < len && A[o + m] == B[o + m]) ++m;
		}
		// the first lane whose piece is not 16 equal bytes: a mismatch, or the limit
		const uint64_t stop = __ballot(m < 16u);
		if (stop) {
			const uint32_t f = ffs64(stop);
			return umin32(limit, n + 16u * f + rdlane(m, f));
		}
	}
	return limit;
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t x) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64);
		const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64);
		const uint64_t y = ((uint64_t)hi << 32) | lo;
		x = y > x ? y : x;
	}
	return x;
}

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

struct GreedyPair {
	const uint8_t* R;
	const uint8_t* V;
	uint32_t rl, vl, seeds, mask;
	uint32_t* G;      // heads: G[0] = 0, bucket b = entries [G[b], G[b + 1])
	uint2* E;         // (offset, tag) per seed, grouped by bucket
};

__device__ __forceinline__ GreedyPair greedy_pair(const GreedyArgs& g, uint32_t pair) {
	const PairDev pd = g.pairs[pair];
	const PairPlanDev pp = g.pplan[pair];
	GreedyPair x;
	x.R = g.ref + pd.r_off;
	x.V = g.ver + pd.v_off;
	x.rl = (uint32_t)pd.r_len;
	x.vl = (uint32_t)pd.v_len;
	x.seeds = x.rl >= g.p ? x.rl - g.p + 1u : 0u;
	x.mask = (uint32_t)(pp.f_size - 1u);   // f_size: the bucket count (a power of two)
	x.G = g.heads + pp.tab_base;
	x.E = g.ent + pp.m;
	return x;
}

// count (kScatter = false: heads[b + 1] += 1 per seed of bucket b) and scatter
// (after the scan made heads[b + 1] the bucket's start: each seed takes the
// next slot, which leaves heads[b + 1] at the bucket's end).  Block = pair x
// chunk of kGreedySeedsPerBlock seeds, a pair's chunks in consecutive blocks.
// (The correcting build's XCD-aware grid, block b taking pairs == b (mod 8),
// measured slower here: C2's build 30.1 -> 35.5 ms, profiles/greedy_rate.json
// holds the faster one.)
template <bool kScatter>
__global__ __launch_bounds__(kGreedyBlock) void greedy_build_kernel(GreedyArgs g, uint32_t nchunk) {
	const uint32_t pair = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
	const GreedyPair x = greedy_pair(g, pair);
	const uint64_t a0 = (uint64_t)chunk * kGreedySeedsPerBlock;
	if (a0 >= x.seeds) return;
	const uint32_t k = umin32(g.p, 16u);
	for (uint32_t i = 0; i < kGreedySeedsPerThread; ++i) {
		const uint64_t a = a0 + (uint64_t)i * kGreedyBlock + threadIdx.x;
		if (a >= x.seeds) break;
		const uint64_t h = seed_hash(x.R, (uint32_t)a, k);   // a + k <= a + p <= |R|
		uint32_t* head = x.G + ((uint64_t)((uint32_t)h & x.mask) + 1u);
		const uint32_t slot = atomicAdd(head, 1u);
		if (kScatter && slot < x.seeds) x.E[slot] = make_uint2((uint32_t)a, (uint32_t)(h >> 32));
	}
}

// per-pair exclusive scan of the bucket counts, in place: one block per pair
__global__ __launch_bounds__(kGreedyScanBlock) void greedy_heads_kernel(GreedyArgs g) {
	__shared__ uint32_t wsum[kGreedyScanBlock / 64];
	const PairPlanDev pp = g.pplan[blockIdx.x];
	const uint64_t nb = pp.f_size;
	uint32_t* C = g.heads + pp.tab_base + 1;   // C[b]: count in, start out
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t carry = 0;
	for (uint64_t base = 0; base < nb; base += 4ull * kGreedyScanBlock) {
		const uint64_t i = base + 4ull * tid;
		uint32_t c[4];
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) c[j] = i + j < nb ? C[i + j] : 0u;
		const uint32_t s = c[0] + c[1] + c[2] + c[3];
		const uint32_t incl = wave_incl_scan(s);
		if (lane == 63u) wsum[wave] = incl;
		__syncthreads();
		uint32_t before = 0, total = 0;
#pragma unroll
		for (uint32_t w = 0; w < kGreedyScanBlock / 64; ++w) {
			const uint32_t t = wsum[w];
			before += w < wave ? t : 0u;
			total += t;
		}
		uint32_t run = carry + before + incl - s;
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			if (i + j < nb) C[i + j] = run;
			run += c[j];
		}
		carry += total;
		__syncthreads();
	}
}

// the scan over V: one wave per pair
__global__ __launch_bounds__(64) void greedy_match_kernel(GreedyArgs g) {
	const uint32_t pair = blockIdx.x;
	const uint32_t lane = lane_id();
	const GreedyPair x = greedy_pair(g, pair);
	const PairPlanDev pp = g.pplan[pair];
	const uint32_t p = g.p, k = umin32(p, 16u);
	const uint32_t vl = uni(x.vl), rl = uni(x.rl), seeds = uni(x.seeds);
	const uint8_t* R = x.R;
	const uint8_t* V = x.V;
	const bool splay = g.splay != 0u;
	const uint32_t rec_cap = uni(pp.rec_cap);
	uint32_t* __restrict__ rec = g.rec + (uint64_t)kRecWordsOnepass * pp.rec_base;

	uint32_t nrec = 0, vc = 0, vs = 0;
	uint64_t dsz = 26;   // header + END
	int32_t st = 0;
	// candidate (length, offset) as one ordered key; offset descending with --splay
	auto key_of = [&](uint32_t ml, uint32_t a) { return ((uint64_t)ml << 32) | (splay ? ~a : a); };
	// can a candidate at `a` whose match is at most `cap` long still win?
	auto may_beat = [&](uint32_t cap, uint32_t a, uint64_t best) { return key_of(cap, a) > best; };

	while (seeds && st == 0 && vc + p <= vl) {
		// ── miss run: positions vc .. vc + 63, each lane its own bucket ──
		const uint32_t pos = vc + lane;
		bool hit = false;
		uint32_t b0 = 0, b1 = 0, tag = 0;
		if (pos + p <= vl) {
			const uint64_t h = seed_hash(V, pos, k);
			const uint64_t b = (uint32_t)h & x.mask;
			tag = (uint32_t)(h >> 32);
			b1 = umin32(x.G[b + 1], seeds);
			b0 = umin32(x.G[b], b1);
			for (uint32_t e = b0; e < b1 && !hit; ++e) {
				const uint2 en = x.E[e];
				if (en.y == tag && en.x <= rl - p) hit = lane_prefix(R + en.x, V + pos, p) == p;
			}
		}
		const uint64_t M = __ballot(hit);
		if (!M) { vc += 64u; continue; }
		const uint32_t jf = ffs64(M);
		vc = uni(vc + jf);
		const uint32_t B0 = rdlane(b0, jf), B1 = rdlane(b1, jf), T = rdlane(tag, jf);

		// ── match: the longest over the bucket's equal seeds, 64 at a time ──
		uint64_t best = 0;
		const uint32_t vrem = vl - vc;
		for (uint32_t base = B0; base < B1; base += 64u) {
			const uint32_t e = base + lane;
			uint32_t a = 0, cap = 0, ml = 0;
			bool live = false;
			if (e < B1) {
				const uint2 en = x.E[e];
				if (en.y == T && en.x <= rl - p) {
					a = en.x;
					cap = umin32(rl - a, vrem);
					live = may_beat(cap, a, best);
				}
			}
			if (live) ml = lane_prefix(R + a, V + vc, umin32(cap, kLaneExt));
			const bool longer = live && ml == kLaneExt && cap > kLaneExt;
			best = uni64(wave_max64(umax64(best, live && !longer && ml >= p ? key_of(ml, a) : 0ull)));
			for (uint64_t L = __ballot(longer); L; L &= L - 1) {
				const uint32_t l = ffs64(L);
				const uint32_t A = rdlane(a, l), C = rdlane(cap, l);
				if (!may_beat(C, A, best)) continue;
				const uint32_t full = uni(wave_prefix(R + A, V + vc, kLaneExt, C));
				if (full >= p) best = umax64(best, key_of(full, A));
			}
		}
		const uint32_t bl = (uint32_t)(best >> 32);
		if (bl < p) { vc += 1u; continue; }   // (not reached: the verified candidate is in the bucket)
		const uint32_t br = splay ? ~(uint32_t)best : (uint32_t)best;

		// ── ADD (the gap, implicit) + COPY (greedy.c:223-242) ──
		if (nrec >= rec_cap) { st = 7; break; }
		const uint32_t head = ld4_below(V, vs, vl);
		if (lane < 4u) rec[kRecWordsOnepass * nrec + lane] = lane == 0 ? vc : (lane == 1 ? br : (lane == 2 ? bl : head));
		++nrec;
		dsz += 13u + (vc > vs ? 9ull + (vc - vs) : 0ull);
		vs = vc = vc + bl;
	}
	if (vs < vl) dsz += 9ull + (vl - vs);   // trailing ADD (greedy.c:245-253)
	if (lane == 0) {
		g.n_rec[pair] = nrec;
		g.dsize[pair] = dsz;
		g.status[pair] = st;
	}
}

}  // namespace

hipError_t launch_greedy(const GreedyArgs& g, uint64_t head_words, hipStream_t st, hipEvent_t ev_built) {
	if (g.n_pairs == 0) return hipSuccess;
	// fresh bucket counts; the scatter rewrites every entry
	hipError_t e = hipMemsetAsync(g.heads, 0, 4ull * head_words, st);
	if (e != hipSuccess) return e;
	if (g.max_seeds) {
		const uint32_t nchunk = (uint32_t)((g.max_seeds + kGreedySeedsPerBlock - 1) / kGreedySeedsPerBlock);
		const uint64_t blocks = (uint64_t)g.n_pairs * nchunk;
		if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
		hipLaunchKernelGGL(greedy_build_kernel<false>, dim3((uint32_t)blocks), dim3(kGreedyBlock), 0, st, g, nchunk);
		hipLaunchKernelGGL(greedy_heads_kernel, dim3(g.n_pairs), dim3(kGreedyScanBlock), 0, st, g);
		hipLaunchKernelGGL(greedy_build_kernel<true>, dim3((uint32_t)blocks), dim3(kGreedyBlock), 0, st, g, nchunk);
	}
	if (ev_built) {
		e = hipEventRecord(ev_built, st);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(greedy_match_kernel, dim3(g.n_pairs), dim3(64), 0, st, g);
	return hipGetLastError();
}

}  // namespace dg
