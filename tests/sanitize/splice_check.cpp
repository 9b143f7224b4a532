// splice_check.cpp — dg_splice and dg_segment_pairs (csrc/dg_splice.cpp) under
// ASan + UBSan, as its own program (tests/test_splice_sanitize_cpu.py compiles
// it with dg_splice.cpp, dg_plan.cpp and dg_format.cpp).
//
// argv[1] is a corpus file: per case four u64 of the whole pair, u32 n_seg,
// then per segment four u64, i32 status, u32 length and the stream (little
// endian), written by the test from tests/splice_cases.py.  Every case is
// spliced; then every segment stream of the case is cut at every length up to
// kCut bytes in turn.  Every input is an exact-size heap block, so a read past
// a buffer's end is an ASan report.  An OK result must be a standard delta
// whose lengths sum to the whole's v_len.  Prints counts and an FNV-1a digest
// of (status, result) over the uncut cases; exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr size_t kCut = 64;
uint64_t n_ok = 0, n_fail = 0;
const uint8_t kCrc[8] = {1, 2, 3, 4, 5, 6, 7, 8};

struct Case {
	dg_pair_t whole;
	std::vector<dg_pair_t> segs;
	std::vector<int32_t> st;
	std::vector<std::vector<uint8_t>> d;
};

uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) {
	for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
	return h;
}

// cut: segment `which` is given only its first `cut` bytes
int run(const Case& c, size_t which, size_t cut, uint64_t* digest) {
	const size_t n = c.segs.size();
	std::vector<uint8_t*> ptr(n);
	std::vector<size_t> len(n);
	for (size_t j = 0; j < n; ++j) {
		len[j] = j == which ? cut : c.d[j].size();
		// exact-size copies: the redzone starts at the buffer's end
		ptr[j] = (uint8_t*)malloc(len[j] ? len[j] : 1);
		if (len[j]) memcpy(ptr[j], c.d[j].data(), len[j]);
	}
	dg_buffer_t out = {nullptr, 0};
	const int rc = dg_splice(&c.whole, c.segs.data(), (uint32_t)n, ptr.data(), len.data(), c.st.data(), kCrc, &out);
	if (rc == DG_OK) {
		dg_delta_info_t inf;
		if (dg_delta_info(out.data, out.len, &inf) != DG_OK || inf.inplace || inf.version_size != c.whole.v_len ||
		    inf.copy_bytes + inf.add_bytes != inf.version_size || out.data[out.len - 1] != 0 || memcmp(inf.src_crc, kCrc, 8) != 0) {
			fprintf(stderr, "an OK result is not a well-formed delta of the whole pair\n");
			exit(2);
		}
		++n_ok;
	} else {
		if (out.data || out.len) {
			fprintf(stderr, "a failed splice left an output\n");
			exit(2);
		}
		++n_fail;
	}
	if (digest) {
		const uint8_t s = (uint8_t)rc;
		*digest = fnv(*digest, &s, 1);
		if (rc == DG_OK) *digest = fnv(*digest, out.data, out.len);
	}
	dg_buffer_free(&out);
	for (uint8_t* p : ptr) free(p);
	return rc;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<Case> cases;
	for (;;) {
		Case c;
		uint64_t w[4];
		if (fread(w, 8, 4, f) != 4) break;
		c.whole = dg_pair_t{w[0], w[1], w[2], w[3]};
		uint32_t n;
		if (fread(&n, 4, 1, f) != 1) return 2;
		for (uint32_t j = 0; j < n; ++j) {
			int32_t st;
			uint32_t len;
			if (fread(w, 8, 4, f) != 4 || fread(&st, 4, 1, f) != 1 || fread(&len, 4, 1, f) != 1) return 2;
			std::vector<uint8_t> d(len);
			if (len && fread(d.data(), 1, len, f) != len) return 2;
			c.segs.push_back(dg_pair_t{w[0], w[1], w[2], w[3]});
			c.st.push_back(st);
			c.d.push_back(d);
		}
		cases.push_back(c);
	}
	fclose(f);
	uint64_t digest = 0xcbf29ce484222325ull;
	for (const Case& c : cases) {
		run(c, c.segs.size(), 0, &digest);
		for (size_t j = 0; j < c.segs.size(); ++j)
			for (size_t k = 0; k < kCut && k < c.d[j].size(); ++k) run(c, j, k, nullptr);
	}
	// the segmentation rule at its edges: counted first, then filled into an exact-size block
	uint64_t segs_made = 0;
	static const uint64_t kLens[] = {0, 1, 15, 16, 17, 255, 256, 257, 4096, 100000};
	for (uint64_t rl : kLens)
		for (uint64_t vl : kLens)
			for (uint64_t S : {16ull, 256ull, 4096ull})
				for (uint64_t W : {0ull, 16ull, 8192ull}) {
					const dg_pair_t w{32, rl, 64, vl};
					uint32_t first[2];
					if (dg_segment_pairs(&w, 1, S, W, nullptr, 0, first) != DG_OK) return 2;
					dg_pair_t* s = (dg_pair_t*)malloc(sizeof(dg_pair_t) * first[1]);
					if (dg_segment_pairs(&w, 1, S, W, s, first[1], first) != DG_OK) return 2;
					if (first[1] > 1 && dg_segment_pairs(&w, 1, S, W, s, first[1] - 1, first) != DG_ERR_CAPACITY) return 2;
					segs_made += first[1];
					free(s);
				}
	printf("cases %zu ok %llu failed %llu segments %llu digest %llu\n", cases.size(), (unsigned long long)n_ok,
	       (unsigned long long)n_fail, (unsigned long long)segs_made, (unsigned long long)digest);
	return 0;
}
