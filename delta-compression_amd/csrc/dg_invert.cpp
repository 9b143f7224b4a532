// dg_invert.cpp — inversion of a standard delta on the host: R and
// A = delta(R -> V) give delta(V -> R), without V (dg_invert;
// include/delta_gpu.h states the contract and the normal form).
//
// Pure host code with no HIP dependency and no context: the comparator of the
// device path (dg_invert_dev.hip) and the engine of `delta invert`.  It is also
// compiled alone under AddressSanitizer/UBSan with dg_format.cpp by
// tests/test_invert_sanitize_cpu.py.
//
// Every byte of R that a COPY of A reads is in V at a known offset; every other
// byte of R is a literal.  The COPYs are sorted by (src ascending, len
// descending, stream order) and swept with the running maximum of their ends:
// a COPY owns what it reads beyond that maximum, and what lies between the
// maximum and a later COPY's src is literal.  The pieces go through one run
// builder that merges neighbouring COPY pieces.  Cost: linear in input plus
// output apart from the sort.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

void put32(uint8_t* p, uint64_t x) {
	p[0] = (uint8_t)(x >> 24);
	p[1] = (uint8_t)(x >> 16);
	p[2] = (uint8_t)(x >> 8);
	p[3] = (uint8_t)x;
}

struct Copy {
	uint64_t src, len, dst;
	size_t index;
};

// The output under construction: the COPY that is still open merges with the
// next piece when that piece continues it in V.
struct Builder {
	std::vector<uint8_t> out;
	uint64_t at = 0;          // bytes of R placed so far
	bool open = false;
	uint64_t src = 0, len = 0;

	void close() {
		if (!open) return;
		uint8_t h[13] = {1};
		put32(h + 1, src);
		put32(h + 5, at - len);
		put32(h + 9, len);
		out.insert(out.end(), h, h + 13);
		open = false;
	}
	void copy(uint64_t s, uint64_t l) {
		if (open && src + len == s) {
			len += l;
		} else {
			close();
			open = true;
			src = s;
			len = l;
		}
		at += l;
	}
	void add(const uint8_t* p, uint64_t l) {
		close();
		uint8_t h[9] = {2};
		put32(h + 1, at);
		put32(h + 5, l);
		out.insert(out.end(), h, h + 9);
		out.insert(out.end(), p, p + l);
		at += l;
	}
};

int invert(const uint8_t* r, size_t r_len, const uint8_t* a, size_t a_len, dg_buffer_t* out) {
	dg_commands_t cl;
	dg_delta_info_t info;
	int rc = dg_delta_decode(a, a_len, &cl, &info);
	if (rc) return rc;   // magic, framing, an unknown command, a payload past the end
	bool past = false, placed = true;
	uint64_t at = 0;
	std::vector<Copy> cs;
	try {
		for (size_t k = 0; k < cl.len; ++k) {
			const dg_placed_command_t& c = cl.data[k];
			if (c.tag == DG_CMD_COPY) {
				if (c.src + c.length > r_len) past = true;
				if (c.length) cs.push_back(Copy{c.src, c.length, c.dst, k});
			}
			if (c.dst != at) placed = false;
			at += c.length;
		}
	} catch (...) {
		dg_commands_free(&cl);
		throw;
	}
	dg_commands_free(&cl);
	if (past) return DG_ERR_MALFORMED;
	if (info.inplace || !placed || at != info.version_size) return DG_ERR_UNSUPPORTED;

	std::sort(cs.begin(), cs.end(), [](const Copy& x, const Copy& y) {
		if (x.src != y.src) return x.src < y.src;
		if (x.len != y.len) return x.len > y.len;
		return x.index < y.index;
	});
	Builder w;
	w.out.resize(DG_HEADER_SIZE);
	memcpy(&w.out[0], "DLT\x03", 4);
	w.out[4] = 0;
	put32(&w.out[5], r_len);
	memcpy(&w.out[9], a + 17, DG_CRC_SIZE);
	memcpy(&w.out[17], a + 9, DG_CRC_SIZE);
	uint64_t reach = 0;   // the bytes of R accounted for so far end here
	for (const Copy& c : cs) {
		if (c.src > reach) w.add(r + reach, c.src - reach);
		const uint64_t s = std::max(c.src, reach), e = c.src + c.len;
		if (s < e) {
			w.copy(c.dst + (s - c.src), e - s);
			reach = e;
		}
	}
	if (reach < r_len) w.add(r + reach, r_len - reach);
	w.close();
	w.out.push_back(0);
	if (w.out.size() >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	uint8_t* buf = (uint8_t*)malloc(w.out.size());
	if (!buf) return DG_ERR_NOMEM;
	memcpy(buf, w.out.data(), w.out.size());
	out->data = buf;
	out->len = w.out.size();
	return DG_OK;
}

}  // namespace

extern "C" int dg_invert(const uint8_t* r, size_t r_len, const uint8_t* a, size_t a_len, dg_buffer_t* out) {
	if (!out || (r_len && !r) || (a_len && !a)) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	if (r_len >= (1ull << 32) || a_len >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	try {
		return invert(r, r_len, a, a_len, out);
	} catch (const std::bad_alloc&) {
		return DG_ERR_NOMEM;
	}
}
