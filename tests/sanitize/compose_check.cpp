// compose_check.cpp — dg_compose (csrc/dg_compose.cpp) under ASan + UBSan, as
// its own program (tests/test_compose_sanitize_cpu.py compiles it with
// dg_compose.cpp and dg_format.cpp).
//
// argv[1] is a corpus file: per pair u32 a_len, A, u32 b_len, B (little
// endian), written by the test from tests/compose_cases.py.  Every pair is
// composed; pairs of streams up to kSweep bytes are also composed with either
// stream cut at every length and with every byte of either stream damaged.
// Every input is an exact-size heap block, so a read past a stream's end is an
// ASan report.  An OK result must be a delta whose lengths sum to its header's
// version size.  Prints one line of counts; exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr size_t kSweep = 1500;
uint64_t n_ok = 0, n_fail = 0;

int run(const uint8_t* a, size_t al, const uint8_t* b, size_t bl, int ignore_hash) {
	// exact-size copies: the redzone starts at the stream's end
	uint8_t* ha = (uint8_t*)malloc(al ? al : 1);
	uint8_t* hb = (uint8_t*)malloc(bl ? bl : 1);
	if (al) memcpy(ha, a, al);
	if (bl) memcpy(hb, b, bl);
	dg_buffer_t out = {nullptr, 0};
	const int rc = dg_compose(al ? ha : nullptr, al, bl ? hb : nullptr, bl, ignore_hash, &out);
	if (rc == DG_OK) {
		dg_delta_info_t inf;
		if (dg_delta_info(out.data, out.len, &inf) != DG_OK || inf.inplace ||
		    inf.copy_bytes + inf.add_bytes != inf.version_size || out.data[out.len - 1] != 0) {
			fprintf(stderr, "an OK result is not a well-formed standard delta\n");
			exit(2);
		}
		++n_ok;
	} else {
		if (out.data || out.len) {
			fprintf(stderr, "a failed compose left an output\n");
			exit(2);
		}
		++n_fail;
	}
	dg_buffer_free(&out);
	free(ha);
	free(hb);
	return rc;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<std::vector<uint8_t>> as, bs;
	for (;;) {
		uint32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::vector<uint8_t> a(n);
		if (n && fread(a.data(), 1, n, f) != n) return 2;
		if (fread(&n, 4, 1, f) != 1) return 2;
		std::vector<uint8_t> b(n);
		if (n && fread(b.data(), 1, n, f) != n) return 2;
		as.push_back(a);
		bs.push_back(b);
	}
	fclose(f);
	uint64_t pairs_bad = 0;
	for (size_t i = 0; i < as.size(); ++i) {
		std::vector<uint8_t>&a = as[i], &b = bs[i];
		if (run(a.data(), a.size(), b.data(), b.size(), 0) != DG_OK) ++pairs_bad;
		if (a.size() > kSweep || b.size() > kSweep) continue;
		for (size_t k = 0; k < a.size(); ++k) run(a.data(), k, b.data(), b.size(), 0);
		for (size_t k = 0; k < b.size(); ++k) run(a.data(), a.size(), b.data(), k, 0);
		static const uint8_t kDamage[] = {0x00, 0x01, 0x02, 0x80, 0xFF};
		for (int which = 0; which < 2; ++which) {
			std::vector<uint8_t>& s = which ? b : a;
			for (size_t k = 0; k < s.size(); ++k) {
				const uint8_t keep = s[k];
				for (uint8_t d : kDamage) {
					if (d == keep) continue;
					s[k] = d;
					run(a.data(), a.size(), b.data(), b.size(), (int)(k & 1));
				}
				s[k] = (uint8_t)(keep ^ 0x40);
				run(a.data(), a.size(), b.data(), b.size(), 1);
				s[k] = keep;
			}
		}
	}
	printf("pairs %zu corpus_failures %llu ok %llu failed %llu\n", as.size(), (unsigned long long)pairs_bad,
	       (unsigned long long)n_ok, (unsigned long long)n_fail);
	return 0;
}
