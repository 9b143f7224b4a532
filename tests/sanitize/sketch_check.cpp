// sketch_check.cpp — dg_sketch and dg_sketch_match (csrc/dg_sketch.cpp) under
// ASan + UBSan, as its own program (tests/test_sketch_sanitize_cpu.py compiles
// it with dg_sketch.cpp).
//
// argv[1] is a corpus file: per buffer u32 len and the bytes (little endian),
// written by the test from tests/sketch_cases.py.  Every buffer is sketched at
// every (p, K) of the sweep, whole and cut short at a few lengths; every input
// and output is an exact-size heap block, so a read or a write past a buffer's
// end is an ASan report.  A sketch must keep every word in its own bin.  Then
// the sketches of each (p, K) are matched against each other in every mode.
// Prints one line of counts and the XOR of the whole buffers' sketch words,
// which the test compares with the model's; exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

const uint32_t kSeeds[] = {1, 4, 16, 17, 64};
const uint32_t kBins[] = {16, 64, 256, 1024};
uint64_t n_sketches = 0, n_matches = 0, digest = 0;

void fail(const char* what) {
	fprintf(stderr, "%s\n", what);
	exit(2);
}

// the sketch of exactly len bytes, in an exact-size block
std::vector<uint64_t> sketch_of(const uint8_t* d, size_t len, uint32_t p, uint32_t K) {
	uint8_t* h = (uint8_t*)malloc(len ? len : 1);
	if (len) memcpy(h, d, len);
	uint64_t* out = (uint64_t*)malloc(8ull * K);
	if (dg_sketch(len ? h : nullptr, len, p, K, out) != DG_OK) fail("dg_sketch failed");
	uint32_t shift = 64;
	for (uint32_t k = K; k > 1; k >>= 1) --shift;
	for (uint32_t b = 0; b < K; ++b)
		if (out[b] != DG_SKETCH_EMPTY && (out[b] >> shift) != b) fail("a word outside its bin");
	if (len < p)
		for (uint32_t b = 0; b < K; ++b)
			if (out[b] != DG_SKETCH_EMPTY) fail("a buffer shorter than the seed has a feature");
	std::vector<uint64_t> v(out, out + K);
	free(out);
	free(h);
	++n_sketches;
	return v;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<std::vector<uint8_t>> bufs;
	for (;;) {
		uint32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::vector<uint8_t> b(n);
		if (n && fread(b.data(), 1, n, f) != n) return 2;
		bufs.push_back(b);
	}
	fclose(f);
	for (uint32_t p : kSeeds)
		for (uint32_t K : kBins) {
			std::vector<uint64_t> all;   // the whole buffers' sketches, in corpus order
			for (const auto& b : bufs) {
				const std::vector<uint64_t> s = sketch_of(b.data(), b.size(), p, K);
				for (uint64_t w : s) digest ^= w;
				all.insert(all.end(), s.begin(), s.end());
				// cut short: the last window must end with the buffer
				for (size_t cut : {(size_t)1, (size_t)p - 1, (size_t)p, (size_t)p + 1, b.size() / 2})
					if (cut && cut < b.size()) sketch_of(b.data(), b.size() - cut, p, K);
			}
			const uint32_t n = (uint32_t)bufs.size();
			for (int mode : {DG_MATCH_ALL, DG_MATCH_NOT_SELF, DG_MATCH_EARLIER})
				for (uint32_t min_equal : {1u, 5u}) {
					// exact-size blocks again; a window of the targets at a base
					const uint32_t base = n / 3, n_t = n - base;
					uint64_t* c = (uint64_t*)malloc(8ull * n * K);
					memcpy(c, all.data(), 8ull * n * K);
					dg_match_t* out = (dg_match_t*)malloc(sizeof(dg_match_t) * (n_t ? n_t : 1));
					if (dg_sketch_match(c + (size_t)base * K, n_t, c, n, K, mode, base, min_equal, out) != DG_OK)
						fail("dg_sketch_match failed");
					for (uint32_t t = 0; t < n_t; ++t) {
						const dg_match_t& m = out[t];
						if (m.reserved) fail("reserved is not 0");
						if (m.best == DG_MATCH_NONE ? (m.equal || m.used) : (m.best >= n || m.equal < min_equal || m.equal > m.used || m.used > K))
							fail("an impossible match");
						if (m.best != DG_MATCH_NONE && ((mode == DG_MATCH_NOT_SELF && m.best == base + t) || (mode == DG_MATCH_EARLIER && m.best >= base + t)))
							fail("an inadmissible match");
						++n_matches;
					}
					free(out);
					free(c);
				}
		}
	// the argument errors touch nothing
	uint64_t w = 7;
	dg_match_t m = {1, 2, 3, 4};
	if (dg_sketch(nullptr, 0, 0, 256, &w) != DG_ERR_INVALID_ARG || dg_sketch(nullptr, 0, 16, 48, &w) != DG_ERR_INVALID_ARG ||
	    dg_sketch_match(&w, 1, &w, 1, 16, 3, 0, 1, &m) != DG_ERR_INVALID_ARG ||
	    dg_sketch_match(&w, 1, &w, 1, 16, 0, 0, 0, &m) != DG_ERR_INVALID_ARG || w != 7 || m.best != 1 || m.reserved != 4)
		fail("an argument error wrote something");
	printf("buffers %zu sketches %llu matches %llu digest %llu\n", bufs.size(), (unsigned long long)n_sketches,
	       (unsigned long long)n_matches, (unsigned long long)digest);
	return 0;
}
