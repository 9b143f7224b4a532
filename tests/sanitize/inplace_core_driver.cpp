// inplace_core_driver.cpp — dg_inplace_core.h on the CPU, under the sanitizers.
//
// The device converter (dg_inplace_dev.hip) shares its serial parts with this
// program: the neighbour ranges, Tarjan, the resumable cycle search and the
// stall policy of dg_inplace_core.h.  Here they run with lane width 1
// (dgip::order_serial) over caller-supplied work arrays sized exactly, so an
// index past any array is an AddressSanitizer report, and the bytes assembled
// from the resulting order must equal dg_make_inplace's (dg_inplace.cpp, which
// keeps explicit adjacency lists: an independent implementation).
//
// Input: a corpus file of records, little endian: the reference, either dense
// (u32 0, u32 |R|, R) or sparse (u32 1, u64 |R|, u32 windows, then per window
// u64 offset, u32 bytes, the bytes: zero everywhere else, held in an anonymous
// mapping whose untouched pages cost nothing, so an R of 4 GiB is cheap); then
// u32 |delta|, delta, and u32 policies (bit p: converted under policy p).  Then
// `random` more seeded random command lists are built here, converted under both
// policies.  Prints "checked N failures F".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include <sys/mman.h>

#include "../../delta-compression_amd/csrc/dg_inplace_core.h"
#include "../../include/delta_gpu.h"

namespace {

void put_be32(std::vector<uint8_t>& o, uint64_t x) {
	for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(x >> s));
}

// The conversion through the shared core; false: the delta is not one the
// device converts (commands not placed sequentially), nothing to compare.
bool convert_core(const uint8_t* R, size_t r_len, const std::vector<uint8_t>& delta, int policy,
                  std::vector<uint8_t>& out) {
	dg_commands_t cl{};
	if (dg_delta_decode(delta.data(), delta.size(), &cl, nullptr) != DG_OK) return false;
	std::vector<uint32_t> src, dst, len;
	std::vector<size_t> adds;
	uint64_t wpos = 0;
	bool ok = !(delta[4] & 1);
	for (size_t k = 0; ok && k < cl.len; ++k) {
		const dg_placed_command_t& c = cl.data[k];
		if (c.dst != wpos) ok = false;
		if (c.tag == DG_CMD_COPY) {
			if (c.src + c.length > r_len) ok = false;
			src.push_back((uint32_t)c.src);
			dst.push_back((uint32_t)c.dst);
			len.push_back((uint32_t)c.length);
		} else {
			adds.push_back(k);
		}
		wpos += c.length;
	}
	if (!ok) {
		dg_commands_free(&cl);
		return false;
	}
	const uint32_t n = (uint32_t)src.size();
	// exact sizes: the sanitizer sees any index past n
	std::vector<uint32_t> a(n), b(n), indeg(n), rank_of(n), by_rank(n), order(n);
	std::vector<uint32_t> idx(n), low(n), tstk(n), callv(n), calln(n), scc(n), cverts(n), cstart(n), active(n);
	std::vector<uint8_t> flag(n), ready(n);
	std::iota(by_rank.begin(), by_rank.end(), 0u);
	std::stable_sort(by_rank.begin(), by_rank.end(), [&](uint32_t x, uint32_t y) { return len[x] < len[y]; });
	for (uint32_t r = 0; r < n; ++r) rank_of[by_rank[r]] = r;
	const dgip::Work w{flag.data(), idx.data(), low.data(), tstk.data(), callv.data(), calln.data(),
	                   scc.data(), cverts.data(), cstart.data(), active.data()};
	uint32_t kept = 0, victims = 0;
	dgip::order_serial(n, src.data(), dst.data(), len.data(), policy, a.data(), b.data(), indeg.data(), rank_of.data(),
	                   by_rank.data(), ready.data(), w, order.data(), &kept, &victims);
	out.assign(delta.begin(), delta.begin() + DG_HEADER_SIZE);
	out[4] = 1;
	for (uint32_t k = 0; k < kept; ++k) {
		const uint32_t v = order[k];
		out.push_back(1);
		put_be32(out, src[v]);
		put_be32(out, dst[v]);
		put_be32(out, len[v]);
	}
	for (size_t k : adds) {
		const dg_placed_command_t& c = cl.data[k];
		out.push_back(2);
		put_be32(out, c.dst);
		put_be32(out, c.length);
		out.insert(out.end(), c.data, c.data + c.length);
	}
	for (uint32_t k = 0; k < victims; ++k) {
		const uint32_t v = order[n - 1 - k];
		out.push_back(2);
		put_be32(out, dst[v]);
		put_be32(out, len[v]);
		out.insert(out.end(), R + src[v], R + src[v] + len[v]);
	}
	out.push_back(0);
	dg_commands_free(&cl);
	return true;
}

uint64_t g_state = 0x243F6A8885A308D3ull;
uint32_t rnd(uint32_t m) {   // splitmix64
	uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return (uint32_t)((z ^ (z >> 31)) % m);
}

// a random sequential delta over a random R: COPYs of random (src, len 0..200),
// with many reads landing in the written range, and short ADDs
void random_case(std::vector<uint8_t>& R, std::vector<uint8_t>& delta) {
	R.resize(256 + rnd(4096));
	for (auto& x : R) x = (uint8_t)rnd(256);
	const uint32_t ncmd = 1 + rnd(120);
	std::vector<dg_placed_command_t> cmds;
	std::vector<std::vector<uint8_t>> lit;
	lit.reserve(ncmd);
	uint64_t wpos = 0;
	for (uint32_t k = 0; k < ncmd; ++k) {
		dg_placed_command_t c{};
		if (rnd(5) == 0) {
			lit.emplace_back(1 + rnd(16));
			for (auto& x : lit.back()) x = (uint8_t)rnd(256);
			c.tag = DG_CMD_ADD;
			c.length = lit.back().size();
			c.data = lit.back().data();
		} else {
			c.tag = DG_CMD_COPY;
			c.length = rnd(8) == 0 ? rnd(3) : 1 + rnd(200);
			if (c.length > R.size()) c.length = R.size();
			c.src = rnd((uint32_t)(R.size() - c.length + 1));
		}
		c.dst = wpos;
		wpos += c.length;
		cmds.push_back(c);
	}
	const uint8_t crc[8] = {0};
	dg_buffer_t b{nullptr, 0};
	if (dg_encode_commands(cmds.data(), cmds.size(), 0, wpos, crc, crc, &b) != DG_OK) abort();
	delta.assign(b.data, b.data + b.len);
	dg_buffer_free(&b);
}

struct Case {
	std::vector<uint8_t> dense;   // R, or
	struct Window {
		uint64_t off;
		std::vector<uint8_t> bytes;
	};
	std::vector<Window> windows;  // what of a sparse R is not zero
	uint64_t r_len = 0;
	bool sparse = false;
	std::vector<uint8_t> delta;
	uint32_t policies = 3;
};

}  // namespace

int main(int argc, char** argv) {
	if (argc < 3) {
		fprintf(stderr, "usage: %s corpus.bin n_random\n", argv[0]);
		return 2;
	}
	std::vector<Case> cases;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	for (;;) {
		uint32_t tag, dl;
		if (fread(&tag, 4, 1, f) != 1) break;
		Case c;
		if (tag == 0) {
			uint32_t rl;
			if (fread(&rl, 4, 1, f) != 1) return 2;
			c.dense.resize(rl);
			if (rl && fread(c.dense.data(), 1, rl, f) != rl) return 2;
			c.r_len = rl;
		} else if (tag == 1) {
			uint32_t nw;
			c.sparse = true;
			if (fread(&c.r_len, 8, 1, f) != 1 || fread(&nw, 4, 1, f) != 1) return 2;
			for (uint32_t k = 0; k < nw; ++k) {
				Case::Window w;
				uint32_t nb;
				if (fread(&w.off, 8, 1, f) != 1 || fread(&nb, 4, 1, f) != 1) return 2;
				w.bytes.resize(nb);
				if (nb && fread(w.bytes.data(), 1, nb, f) != nb) return 2;
				if (w.off + nb > c.r_len) return 2;
				c.windows.push_back(std::move(w));
			}
		} else {
			return 2;
		}
		if (fread(&dl, 4, 1, f) != 1) return 2;
		c.delta.resize(dl);
		if (dl && fread(c.delta.data(), 1, dl, f) != dl) return 2;
		if (fread(&c.policies, 4, 1, f) != 1) return 2;
		cases.push_back(std::move(c));
	}
	fclose(f);
	const int n_random = atoi(argv[2]);
	for (int k = 0; k < n_random; ++k) {
		cases.emplace_back();
		random_case(cases.back().dense, cases.back().delta);
		cases.back().r_len = cases.back().dense.size();
	}
	size_t checked = 0, failures = 0, victims_seen = 0;
	for (size_t i = 0; i < cases.size(); ++i) {
		const Case& c = cases[i];
		const uint8_t* R = c.dense.data();
		void* map = nullptr;
		if (c.sparse && c.r_len) {
			map = mmap(nullptr, c.r_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
			if (map == MAP_FAILED) return 2;
			for (const auto& w : c.windows) memcpy((uint8_t*)map + w.off, w.bytes.data(), w.bytes.size());
			R = (const uint8_t*)map;
		}
		const size_t r_len = c.r_len;
		const auto& d = c.delta;
		for (int policy = 0; policy < 2; ++policy) {
			if (!(c.policies >> policy & 1)) continue;
			std::vector<uint8_t> got;
			if (!convert_core(R, r_len, d, policy, got)) {
				fprintf(stderr, "case %zu: not a sequential standard delta\n", i);
				++failures;
				continue;
			}
			dg_buffer_t exp{nullptr, 0};
			dg_inplace_stats_t st{};
			const int rc = dg_make_inplace(R, r_len, d.data(), d.size(), policy, &exp, &st);
			if (rc != DG_OK || exp.len != got.size() || memcmp(exp.data, got.data(), got.size()) != 0) {
				fprintf(stderr, "case %zu policy %d: core differs from dg_make_inplace (rc %d, %zu vs %zu bytes)\n", i,
				        policy, rc, exp.len, got.size());
				++failures;
			}
			victims_seen += st.num_adds;
			dg_buffer_free(&exp);
			++checked;
		}
		if (map) munmap(map, c.r_len);
	}
	printf("checked %zu failures %zu adds %zu\n", checked, failures, victims_seen);
	return failures ? 1 : 0;
}
