// invert_check.cpp — dg_invert (csrc/dg_invert.cpp) under ASan + UBSan, as its
// own program (tests/test_invert_sanitize_cpu.py compiles it with dg_invert.cpp
// and dg_format.cpp).
//
// argv[1] is a corpus file: per case u32 r_len, R, u32 a_len, A (little
// endian), written by the test from tests/invert_cases.py.  Every case is
// inverted; cases with a stream up to kSweep bytes are also inverted with the
// stream cut at every length, with R cut short, and with every byte of the
// stream damaged.  Every input is an exact-size heap block, so a read past a
// buffer's end is an ASan report.  An OK result must be a standard delta whose
// lengths sum to |R|, with the stream's CRCs swapped.  Prints one line of
// counts; exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr size_t kSweep = 1500;
uint64_t n_ok = 0, n_fail = 0;

int run(const uint8_t* r, size_t rl, const uint8_t* a, size_t al) {
	// exact-size copies: the redzone starts at the buffer's end
	uint8_t* hr = (uint8_t*)malloc(rl ? rl : 1);
	uint8_t* ha = (uint8_t*)malloc(al ? al : 1);
	if (rl) memcpy(hr, r, rl);
	if (al) memcpy(ha, a, al);
	dg_buffer_t out = {nullptr, 0};
	const int rc = dg_invert(rl ? hr : nullptr, rl, al ? ha : nullptr, al, &out);
	if (rc == DG_OK) {
		dg_delta_info_t inf;
		if (dg_delta_info(out.data, out.len, &inf) != DG_OK || inf.inplace || inf.version_size != rl ||
		    inf.copy_bytes + inf.add_bytes != inf.version_size || out.data[out.len - 1] != 0 ||
		    memcmp(inf.src_crc, ha + 17, 8) != 0 || memcmp(inf.dst_crc, ha + 9, 8) != 0) {
			fprintf(stderr, "an OK result is not a well-formed inverse\n");
			exit(2);
		}
		++n_ok;
	} else {
		if (out.data || out.len) {
			fprintf(stderr, "a failed invert left an output\n");
			exit(2);
		}
		++n_fail;
	}
	dg_buffer_free(&out);
	free(hr);
	free(ha);
	return rc;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<std::vector<uint8_t>> rs, as;
	for (;;) {
		uint32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::vector<uint8_t> r(n);
		if (n && fread(r.data(), 1, n, f) != n) return 2;
		if (fread(&n, 4, 1, f) != 1) return 2;
		std::vector<uint8_t> a(n);
		if (n && fread(a.data(), 1, n, f) != n) return 2;
		rs.push_back(r);
		as.push_back(a);
	}
	fclose(f);
	uint64_t cases_bad = 0;
	for (size_t i = 0; i < rs.size(); ++i) {
		std::vector<uint8_t>&r = rs[i], &a = as[i];
		if (run(r.data(), r.size(), a.data(), a.size()) != DG_OK) ++cases_bad;
		if (a.size() > kSweep) continue;
		for (size_t k = 0; k < a.size(); ++k) run(r.data(), r.size(), a.data(), k);
		// R cut short: a COPY past its end must be refused, never read
		const size_t rcut = r.size() < kSweep ? r.size() : kSweep;
		for (size_t k = 0; k < rcut; ++k) run(r.data(), r.size() - 1 - k, a.data(), a.size());
		static const uint8_t kDamage[] = {0x00, 0x01, 0x02, 0x80, 0xFF};
		for (size_t k = 0; k < a.size(); ++k) {
			const uint8_t keep = a[k];
			for (uint8_t d : kDamage) {
				if (d == keep) continue;
				a[k] = d;
				run(r.data(), r.size(), a.data(), a.size());
			}
			a[k] = (uint8_t)(keep ^ 0x40);
			run(r.data(), r.size(), a.data(), a.size());
			a[k] = keep;
		}
	}
	printf("cases %zu corpus_failures %llu ok %llu failed %llu\n", rs.size(), (unsigned long long)cases_bad,
	       (unsigned long long)n_ok, (unsigned long long)n_fail);
	return 0;
}
