// lineage_check.cpp — dg_read_lineage (csrc/dg_lineage.cpp) under ASan + UBSan,
// as its own program (tests/test_lineage_sanitize_cpu.py compiles it with
// dg_lineage.cpp and dg_format.cpp).
//
// argv[1] is a corpus file, little endian: per lineage u32 r_len, R, u32 k,
// then k times (u32 d_len, the delta), the one on R first, then u32 n and n
// ranges (u64 off, u64 len), written by the test from tests/lineage_cases.py.
// Every range of every lineage is read; every lineage is also read whole with
// its last and with its first delta cut at every length up to kCut bytes.
// Every input is an exact-size heap block, so a read past a buffer's end is an
// ASan report.  An OK result holds at most `len` bytes; a failed one leaves no
// output.  Prints one line: counts, and an FNV-1a digest of the corpus reads'
// statuses and bytes in order, which the test compares with the model's.
// Exit status 0 unless a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr size_t kCut = 64;
uint64_t n_ok = 0, n_fail = 0, digest = 0xcbf29ce484222325ull;

void mix(const uint8_t* p, size_t n) {
	for (size_t k = 0; k < n; ++k) digest = (digest ^ p[k]) * 0x100000001b3ull;
}

uint8_t* exact(const uint8_t* p, size_t n) {
	// exact-size copies: the redzone starts at the buffer's end
	uint8_t* h = (uint8_t*)malloc(n ? n : 1);
	if (n) memcpy(h, p, n);
	return h;
}

// the lineage with delta `cut_at` (or none: -1) cut to cut_len bytes
int run(const std::vector<uint8_t>& r, const std::vector<std::vector<uint8_t>>& ds, int cut_at, size_t cut_len, uint64_t off,
        uint64_t len, bool count) {
	uint8_t* hr = exact(r.data(), r.size());
	std::vector<uint8_t*> hd(ds.size());
	std::vector<const uint8_t*> dp(ds.size());
	std::vector<size_t> dl(ds.size());
	for (size_t j = 0; j < ds.size(); ++j) {
		dl[j] = (int)j == cut_at ? cut_len : ds[j].size();
		hd[j] = exact(ds[j].data(), dl[j]);
		dp[j] = dl[j] ? hd[j] : nullptr;
	}
	dg_buffer_t out = {nullptr, 0};
	const int rc = dg_read_lineage(r.size() ? hr : nullptr, r.size(), dp.data(), dl.data(), (uint32_t)ds.size(), off, len, &out);
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
	for (uint8_t* p : hd) free(p);
	return rc;
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint64_t cases = 0, reads = 0;
	for (;;) {
		uint32_t n, k;
		if (fread(&n, 4, 1, f) != 1) break;
		std::vector<uint8_t> r(n);
		if (n && fread(r.data(), 1, n, f) != n) return 2;
		if (fread(&k, 4, 1, f) != 1) return 2;
		std::vector<std::vector<uint8_t>> ds(k);
		for (auto& d : ds) {
			if (fread(&n, 4, 1, f) != 1) return 2;
			d.resize(n);
			if (n && fread(d.data(), 1, n, f) != n) return 2;
		}
		if (fread(&n, 4, 1, f) != 1) return 2;
		std::vector<uint64_t> rg(2 * (size_t)n);
		if (n && fread(rg.data(), 16, n, f) != n) return 2;
		++cases;
		for (uint32_t q = 0; q < n; ++q, ++reads) run(r, ds, -1, 0, rg[2 * q], rg[2 * q + 1], true);
		if (k == 0) continue;
		for (int at : {(int)k - 1, 0})
			for (size_t c = 0; c <= kCut && c < ds[at].size(); ++c) {
				run(r, ds, at, c, 0, ~0ull, false);
				run(r, ds, at, c, 7, 9, false);
			}
	}
	fclose(f);
	printf("cases %llu reads %llu ok %llu failed %llu digest %llu\n", (unsigned long long)cases, (unsigned long long)reads,
	       (unsigned long long)n_ok, (unsigned long long)n_fail, (unsigned long long)digest);
	return 0;
}
