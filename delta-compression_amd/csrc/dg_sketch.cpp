// dg_sketch.cpp — resemblance sketches and base selection on the host
// (dg_sketch, dg_sketch_match; the definitions are in include/delta_gpu.h).
//
// Pure host code with no HIP dependency, like dg_invert.cpp: it is also
// compiled alone under AddressSanitizer/UBSan with tests/sanitize/
// sketch_check.cpp.  The device path (dg_sketch_dev.hip) and the tests' Python
// model (tests/sketch_cases.py) produce the same words.
#include <cstring>

#include "../../include/delta_gpu.h"
#include "dg_layout.h"
#include "dg_sketch_dev.h"

using namespace dg;
using namespace dgsk;

namespace {

typedef unsigned __int128 u128;

uint64_t mod61(u128 x) {   // x < 2^122
	uint64_t r = (uint64_t)(x & kMersenne) + (uint64_t)(x >> 61);   // < 2^62
	r = (r & kMersenne) + (r >> 61);
	return r >= kMersenne ? r - kMersenne : r;
}

uint64_t mix(uint64_t z) {   // the splitmix64 finaliser
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

bool bins_ok(uint32_t K) { return K >= kMinBins && K <= kMaxBins && (K & (K - 1)) == 0; }

}  // namespace

extern "C" {

int dg_sketch(const uint8_t* data, size_t len, uint32_t p, uint32_t K, uint64_t* out) {
	if (!out || (len && !data) || p < 1 || p > kMaxSeed || !bins_ok(K)) return DG_ERR_INVALID_ARG;
	if ((uint64_t)len >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	for (uint32_t b = 0; b < K; ++b) out[b] = kEmpty;
	if (len < p) return DG_OK;
	const uint32_t shift = 64 - (uint32_t)__builtin_ctz(K);
	uint64_t top = 1, fp = 0;   // 263^(p-1); the fingerprint of the first window, by Horner
	for (uint32_t k = 0; k < p; ++k) {
		if (k) top = mod61((u128)top * kBase);
		fp = mod61((u128)fp * kBase + data[k]);
	}
	for (size_t a = 0;; ++a) {
		const uint64_t h = mix(fp);
		uint64_t& bin = out[h >> shift];
		if (h < bin) bin = h;
		if (a + p >= len) break;
		// drop data[a], take data[a + p]
		const uint64_t gone = mod61((u128)top * data[a]);
		fp = mod61((u128)(fp + kMersenne - gone) * kBase + data[a + p]);
	}
	return DG_OK;
}

int dg_sketch_match(const uint64_t* targets, uint32_t n_t, const uint64_t* cands, uint32_t n_c, uint32_t K, int mode,
                    uint32_t target_base, uint32_t min_equal, dg_match_t* out) {
	if ((n_t && (!targets || !out)) || (n_c && !cands) || !bins_ok(K) || min_equal == 0 ||
	    (mode != DG_MATCH_ALL && mode != DG_MATCH_NOT_SELF && mode != DG_MATCH_EARLIER))
		return DG_ERR_INVALID_ARG;
	for (uint32_t t = 0; t < n_t; ++t) {
		const uint64_t* T = targets + (size_t)t * K;
		const uint64_t self = (uint64_t)target_base + t;
		dg_match_t best = {DG_MATCH_NONE, 0, 0, 0};
		const uint64_t end = mode == DG_MATCH_EARLIER && self < n_c ? self : n_c;
		for (uint32_t c = 0; c < end; ++c) {
			if (mode == DG_MATCH_NOT_SELF && c == self) continue;
			const uint64_t* Cd = cands + (size_t)c * K;
			uint32_t equal = 0, used = 0;
			for (uint32_t b = 0; b < K; ++b) {
				equal += T[b] == Cd[b] && T[b] != kEmpty;
				used += T[b] != kEmpty || Cd[b] != kEmpty;
			}
			// c beats the best so far iff its score is strictly higher: of equal scores the smallest index stays
			if (equal >= min_equal && (best.best == DG_MATCH_NONE || equal * best.used > best.equal * used))
				best = dg_match_t{c, equal, used, 0};
		}
		out[t] = best;
	}
	return DG_OK;
}

}  // extern "C"
