// dg_sketch_dev.hip — resemblance sketches of a batch of spans, and base
// matching over sketch arrays, on the device: word for word what dg_sketch and
// dg_sketch_match (dg_sketch.cpp) produce; the definitions are in
// include/delta_gpu.h.
//
// Built on its own as lib/dg_sketch.hsaco and loaded by dg_sketch_host.cpp.
//
//   dg_sketch_kernel   one 256-thread block per (span, chunk) of the plan's
//     work list (dg_plan.cpp).  Phases:
//       1. the K bins in LDS are set empty; thread x computes entry x of the
//          roll table (-x 263^p mod M);
//       2. the chunk's bytes and the p - 1 after them are staged in LDS in
//          16-byte pieces: a piece wholly inside the bytes the chunk may read
//          is one aligned 16-byte load, the piece in front and the piece
//          behind are assembled from guarded byte loads, so nothing outside
//          the span is read;
//       3. every lane takes `per` consecutive windows (a multiple of four,
//          the chunk's windows spread over the block): the first window's
//          fingerprint by fp16_dot (p = 16) or by the dot product with the
//          plan's constants, every next one by a rolling step; the leaving
//          and the entering bytes come from LDS a dword per four windows.
//          h = mix(fp) goes to its bin by an LDS 64-bit minimum, issued only
//          when a plain read of the bin shows that h would lower it: after
//          the first few hundred windows almost none does;
//       4. the block folds its non-empty bins into the span's K output words
//          with 64-bit unsigned-minimum atomics.  The host set the output to
//          DG_SKETCH_EMPTY on the stream before the launch.
//     A minimum is order-independent, so the words do not depend on the
//     schedule.
//
//   dg_sketch_match_kernel   one wave per kMatchTargets targets (one from 512
//     bins up: match_targets_per_wave), whose sketches
//     stay in registers (K / 64 words per lane each).  The wave streams the
//     candidate sketches (coalesced: lane l reads word 64 w + l, the next
//     candidate's words are requested before this one's are counted), counts
//     `equal` and `used` by compare -> ballot -> population count, and keeps
//     the running best by the integer rule; all of that is wave-uniform.
//     O(n_t n_c K).
//
// LDS of a sketch block (sketch_lds_bytes): K x 8 bytes of bins, 2 KiB of roll
// table, then the image: dword d at word d + d / 16, which puts lanes whose
// windows start 64 bytes apart on different banks.
#include <hip/hip_runtime.h>

#include "dg_devutil.h"
#include "dg_sketch_dev.h"

using namespace dg;
using namespace dgsk;

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // the splitmix64 finaliser
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}

// the staged image: dword d (clamped to the last staged one: a lane's last
// group of four may look one dword past the bytes its windows need)
struct Image {
	const uint32_t* w;
	uint32_t last;
	__device__ __forceinline__ uint32_t dword(uint32_t d) const {
		d = umin32(d, last);
		return w[d + (d >> 4)];
	}
	__device__ __forceinline__ uint32_t byte(uint32_t x) const { return (dword(x >> 2) >> (8u * (x & 3u))) & 0xFFu; }
};

}  // namespace

extern "C" __global__ __launch_bounds__(256) void dg_sketch_kernel(SkArgs a) {
	extern __shared__ uint64_t lds[];
	uint64_t* bins = lds;             // K
	uint64_t* nb = lds + a.K;         // 256: the roll table
	uint32_t* img = reinterpret_cast<uint32_t*>(nb + 256);
	const uint32_t tid = threadIdx.x;
	const uint32_t p = a.p, K = a.K;
	const SkItem it = a.items[blockIdx.x];
	const SkSpan sp = a.spans[it.span];

	// the chunk: windows [w0, w0 + nwin) of the span; bytes [lo, hi) of the arena
	const uint64_t windows = sp.len - p + 1;   // the work list has only spans of p bytes or more
	const uint64_t w0 = (uint64_t)it.chunk * a.chunk_bytes;
	const uint32_t nwin = (uint32_t)min((uint64_t)a.chunk_bytes, windows - w0);
	const uint64_t lo = sp.off + w0;
	const uint64_t hi = lo + nwin + p - 1;     // <= sp.off + sp.len
	const uint64_t base = lo & ~15ull;
	const uint32_t pieces = (uint32_t)((hi - base + 15) >> 4);

	for (uint32_t b = tid; b < K; b += kSkBlock) bins[b] = kEmpty;
	nb[tid] = roll_table(tid, a.top);
	for (uint32_t q = tid; q < pieces; q += kSkBlock) {
		const uint64_t at = base + 16ull * q;
		uint32_t w[4];
		if (at >= lo && at + 16 <= hi) {
			const uint4 v = *reinterpret_cast<const uint4*>(a.arena + at);   // the arena is 16-byte aligned
			w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
		} else {
#pragma unroll
			for (uint32_t k = 0; k < 4; ++k) {
				w[k] = 0;
#pragma unroll
				for (uint32_t j = 0; j < 4; ++j) {
					const uint64_t x = at + 4 * k + j;
					if (x >= lo && x < hi) w[k] |= (uint32_t)a.arena[x] << (8 * j);
				}
			}
		}
		uint32_t* dst = img + 4 * q + (q >> 2);   // dwords 4q .. 4q + 3 share one pad group
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) dst[k] = w[k];
	}
	__syncthreads();

	const Image I{img, 4 * pieces - 1};
	const uint32_t per = umax32(4u, ((nwin + kSkBlock - 1) / kSkBlock + 3u) & ~3u);
	const uint32_t j0 = tid * per;
	if (j0 < nwin) {
		const uint32_t cnt = umin32(per, nwin - j0);
		const uint32_t x = (uint32_t)(lo - base) + j0;   // the lane's first window in the image
		uint64_t fp;
		if (p == 16) {
			const uint32_t d = x >> 2, s = x & 3u;
			const uint32_t d0 = I.dword(d), d1 = I.dword(d + 1), d2 = I.dword(d + 2), d3 = I.dword(d + 3), d4 = I.dword(d + 4);
			fp = fp16_dot(__builtin_amdgcn_alignbyte(d1, d0, s), __builtin_amdgcn_alignbyte(d2, d1, s),
			              __builtin_amdgcn_alignbyte(d3, d2, s), __builtin_amdgcn_alignbyte(d4, d3, s));
		} else {   // window_fp's sums (dg_devutil.h) over bytes from LDS
			uint64_t l = 0, h = 0;
			for (uint32_t k = 0; k < p; ++k) {
				const uint64_t c = a.powc[k];
				const uint64_t b = I.byte(x + k);
				l += b * (uint32_t)c;
				h += b * (uint32_t)(c >> 32);
			}
			fp = fold61c(l, h);
		}
		// the byte leaving window j is x + j, the byte entering is x + j + p
		const uint32_t od = x >> 2, so = x & 3u, id = (x + p) >> 2, si = (x + p) & 3u;
		uint32_t o0 = I.dword(od), i0 = I.dword(id);
		for (uint32_t g = 0; g < cnt; g += 4) {
			const uint32_t o1 = I.dword(od + 1 + (g >> 2)), i1 = I.dword(id + 1 + (g >> 2));
			const uint32_t ow = __builtin_amdgcn_alignbyte(o1, o0, so), iw = __builtin_amdgcn_alignbyte(i1, i0, si);
			o0 = o1, i0 = i1;
#pragma unroll
			for (uint32_t k = 0; k < 4; ++k) {
				if (g + k < cnt) {
					const uint64_t h = mix64(fp);
					uint64_t* bin = bins + (h >> a.shift);
					if (h < *bin) atomicMin(reinterpret_cast<unsigned long long*>(bin), (unsigned long long)h);
					fp = roll61(fp, nb[(ow >> (8 * k)) & 0xFFu], (iw >> (8 * k)) & 0xFFu);
				}
			}
		}
	}
	__syncthreads();

	uint64_t* out = a.out + (uint64_t)it.span * K;
	for (uint32_t b = tid; b < K; b += kSkBlock) {
		const uint64_t v = bins[b];
		if (v != kEmpty) atomicMin(reinterpret_cast<unsigned long long*>(out + b), (unsigned long long)v);
	}
}

namespace {

// W = words per lane per sketch: K / 64, and 1 for K < 64 (lanes K and up hold
// empty bins, which count neither as equal nor as used); T = targets per wave
template <uint32_t W, uint32_t T>
__device__ __forceinline__ void match_targets(const MatchArgs& a, uint32_t t0) {
	const uint32_t lane = lane_id(), K = a.K;
	uint64_t tw[T][W];
#pragma unroll
	for (uint32_t i = 0; i < T; ++i)
#pragma unroll
		for (uint32_t w = 0; w < W; ++w) {
			const uint32_t b = 64 * w + lane;
			tw[i][w] = t0 + i < a.n_t && b < K ? a.targets[(uint64_t)(t0 + i) * K + b] : kEmpty;
		}
	uint32_t best[T], beq[T], bus[T];
#pragma unroll
	for (uint32_t i = 0; i < T; ++i) best[i] = kNone, beq[i] = 0, bus[i] = 0;

	// DG_MATCH_EARLIER: no candidate at or past the group's last target is admissible
	uint64_t end = a.n_c;
	if (a.mode == DG_MATCH_EARLIER) end = min(end, (uint64_t)a.target_base + t0 + T - 1);
	const uint32_t n_c = (uint32_t)end;

	// candidate c's words; up to four words per lane the next candidate's are
	// requested before this one's are counted
	constexpr bool kAhead = W <= 4;
	auto load = [&](uint32_t c, uint64_t (&v)[W]) {
#pragma unroll
		for (uint32_t w = 0; w < W; ++w) {
			const uint32_t b = 64 * w + lane;
			v[w] = c < n_c && b < K ? a.cands[(uint64_t)c * K + b] : kEmpty;
		}
	};
	uint64_t cw[W], nx[kAhead ? W : 1];
	if constexpr (kAhead) load(0, nx);
	for (uint32_t c = 0; c < n_c; ++c) {
		if constexpr (kAhead) {
#pragma unroll
			for (uint32_t w = 0; w < W; ++w) cw[w] = nx[w];
			load(c + 1, nx);
		} else {
			load(c, cw);
		}
#pragma unroll
		for (uint32_t i = 0; i < T; ++i) {
			uint32_t eq = 0, us = 0;
#pragma unroll
			for (uint32_t w = 0; w < W; ++w) {
				eq += (uint32_t)__popcll(__ballot(cw[w] == tw[i][w] && cw[w] != kEmpty));
				us += (uint32_t)__popcll(__ballot(cw[w] != kEmpty || tw[i][w] != kEmpty));
			}
			const uint64_t self = (uint64_t)a.target_base + t0 + i;
			const bool admissible = a.mode == DG_MATCH_ALL || (a.mode == DG_MATCH_NOT_SELF ? c != self : c < self);
			// strictly higher only: of equal scores the smallest index stays
			if (admissible && eq >= a.min_equal && (best[i] == kNone || eq * bus[i] > beq[i] * us))
				best[i] = c, beq[i] = eq, bus[i] = us;
		}
	}
	if (lane < 4) {   // a dg_match_t is four words with no alignment beyond theirs
#pragma unroll
		for (uint32_t i = 0; i < T; ++i)
			if (t0 + i < a.n_t) a.out[4ull * (t0 + i) + lane] = lane == 0 ? best[i] : lane == 1 ? beq[i] : lane == 2 ? bus[i] : 0u;
	}
}

template <uint32_t W>
__device__ __forceinline__ void match_waves(const MatchArgs& a) {
	constexpr uint32_t T = match_targets_per_wave(64 * W);
	const uint32_t groups = (a.n_t + T - 1) / T;
	const uint32_t waves = gridDim.x * (kMatchBlock / 64);
	for (uint32_t g = uni(blockIdx.x * (kMatchBlock / 64) + threadIdx.x / 64); g < groups; g += waves)
		match_targets<W, T>(a, g * T);
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void dg_sketch_match_kernel(MatchArgs a) {
	switch (a.K >> 6) {
	case 0:
	case 1: match_waves<1>(a); break;
	case 2: match_waves<2>(a); break;
	case 4: match_waves<4>(a); break;
	case 8: match_waves<8>(a); break;
	default: match_waves<16>(a); break;
	}
}
