// read_check.cpp — dg_read (csrc/dg_read.cpp) under ASan + UBSan, as its own
// program (tests/test_read_sanitize_cpu.py compiles it with dg_read.cpp and
// dg_format.cpp).
//
// argv[1] is a corpus file, little endian: per case u32 r_len, R, u32 d_len,
// the delta, u32 n, then n ranges (u64 off, u64 len), written by the test from
// tests/read_cases.py.  Every range of every case is read; every stream is
// also read whole when cut at every length up to kCut bytes, and, for short
// streams, with R cut short.  Every input is an exact-size heap block, so a
// read past a buffer's end is an ASan report.  An OK result holds at most
// `len` bytes; a failed one leaves no output.  Prints one line: counts, and an
// FNV-1a digest of the corpus reads' statuses and bytes in order, which the
// test compares with the model's.  Exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr size_t kCut = 64, kSweep = 1500;
uint64_t n_ok = 0, n_fail = 0, digest = 0xcbf29ce484222325ull;

void mix(const uint8_t* p, size_t n) {
	for (size_t k = 0; k < n; ++k) digest = (digest ^ p[k]) * 0x100000001b3ull;
}

int run(const uint8_t* r, size_t rl, const uint8_t* d, size_t dl, uint64_t off, uint64_t len, bool count) {
	// exact-size copies: the redzone starts at the buffer's end
	uint8_t* hr = (uint8_t*)malloc(rl ? rl : 1);
	uint8_t* hd = (uint8_t*)malloc(dl ? dl : 1);
	if (rl) memcpy(hr, r, rl);
	if (dl) memcpy(hd, d, dl);
	dg_buffer_t out = {nullptr, 0};
	const int rc = dg_read(rl ? hr : nullptr, rl, dl ? hd : nullptr, dl, off, len, &out);
	if (rc == DG_OK) {
		if (!out.data || out.len > len) {
			fprintf(stderr, "an OK read returned more than it was asked for, or nothing\n");
			exit(2);
		}
		++n_ok;
	} else {
		if (out.data || out.len) {
			fprintf(stderr, "a failed read left an output\n");
			exit(2);
		}
		++n_fail;
	}
	if (count) {
		const uint8_t s = (uint8_t)rc;
		mix(&s, 1);
		if (rc == DG_OK) mix(out.data, out.len);
	}
	dg_buffer_free(&out);
	free(hr);
	free(hd);
	return rc;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint64_t cases = 0, reads = 0;
	for (;;) {
		uint32_t n;
		if (fread(&n, 4, 1, f) != 1) break;
		std::vector<uint8_t> r(n);
		if (n && fread(r.data(), 1, n, f) != n) return 2;
		if (fread(&n, 4, 1, f) != 1) return 2;
		std::vector<uint8_t> d(n);
		if (n && fread(d.data(), 1, n, f) != n) return 2;
		if (fread(&n, 4, 1, f) != 1) return 2;
		std::vector<uint64_t> rg(2 * (size_t)n);
		if (n && fread(rg.data(), 16, n, f) != n) return 2;
		++cases;
		for (uint32_t k = 0; k < n; ++k, ++reads) run(r.data(), r.size(), d.data(), d.size(), rg[2 * k], rg[2 * k + 1], true);
		for (size_t k = 0; k <= kCut && k < d.size(); ++k) {
			run(r.data(), r.size(), d.data(), k, 0, ~0ull, false);
			run(r.data(), r.size(), d.data(), k, 7, 9, false);
		}
		if (d.size() > kSweep) continue;
		for (size_t k = 0; k < d.size(); ++k) run(r.data(), r.size(), d.data(), k, 0, ~0ull, false);
		// R cut short: a COPY past its end must be refused, never read
		const size_t rcut = r.size() < kSweep ? r.size() : kSweep;
		for (size_t k = 0; k < rcut; ++k) run(r.data(), r.size() - 1 - k, d.data(), d.size(), 0, ~0ull, false);
	}
	fclose(f);
	printf("cases %llu reads %llu ok %llu failed %llu digest %llu\n", (unsigned long long)cases, (unsigned long long)reads,
	       (unsigned long long)n_ok, (unsigned long long)n_fail, (unsigned long long)digest);
	return 0;
}
