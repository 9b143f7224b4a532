// dg_read.cpp — a byte range of the version a standard delta makes of R, on
// the host (dg_read; include/delta_gpu.h states the contract).
//
// Pure host code with no HIP dependency and no context: the comparator of the
// device path (dg_read_dev.hip) and the engine of `delta read`.  It is also
// compiled alone under AddressSanitizer/UBSan with dg_format.cpp by
// tests/test_read_sanitize_cpu.py.
//
// The result is the reference's replay (src/c/apply.c:229-249), sliced: a
// zeroed buffer, then every command's intersection with the range in stream
// order, later writes over earlier ones.  One walk over the stream, which is
// validated whole: linear in the stream plus the range.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/delta_gpu.h"

namespace {

uint64_t get32(const uint8_t* p) {
	return ((uint64_t)p[0] << 24) | ((uint64_t)p[1] << 16) | ((uint64_t)p[2] << 8) | p[3];
}

}  // namespace

extern "C" int dg_read(const uint8_t* r, size_t r_len, const uint8_t* delta, size_t delta_len, uint64_t off, uint64_t len,
                       dg_buffer_t* out) {
	if (!out || (r_len && !r) || (delta_len && !delta)) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	if (r_len >= (1ull << 32) || delta_len >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	if (delta_len < DG_HEADER_SIZE || memcmp(delta, "DLT\x03", 4) != 0) return DG_ERR_MALFORMED;
	if (delta[4] & 1) return DG_ERR_UNSUPPORTED;   // in-place: a slice of its replay needs the whole replay
	const uint64_t vsize = get32(delta + 5);
	const uint64_t n = off >= vsize ? 0 : std::min(len, vsize - off);   // pread
	const uint64_t hi = off + n;
	uint8_t* buf = (uint8_t*)calloc(n ? n : 1, 1);
	if (!buf) return DG_ERR_NOMEM;
	size_t pos = DG_HEADER_SIZE;
	bool bad = false;
	while (pos < delta_len) {   // a missing END is the end of input (encoding.c:111-178)
		const uint8_t t = delta[pos];
		if (t == 0) break;
		uint64_t src = 0, dst, l;
		const uint8_t* from;
		if (t == 1) {
			if (delta_len - pos < 13) { bad = true; break; }
			src = get32(delta + pos + 1);
			dst = get32(delta + pos + 5);
			l = get32(delta + pos + 9);
			pos += 13;
			if (src + l > r_len) { bad = true; break; }
			from = r + src;
		} else if (t == 2) {
			if (delta_len - pos < 9) { bad = true; break; }
			dst = get32(delta + pos + 1);
			l = get32(delta + pos + 5);
			pos += 9;
			if (l > delta_len - pos) { bad = true; break; }
			from = delta + pos;
			pos += l;
		} else {
			bad = true;
			break;
		}
		if (dst + l > vsize) { bad = true; break; }
		const uint64_t s = std::max(dst, off), e = std::min(dst + l, hi);
		if (e > s) memcpy(buf + (s - off), from + (s - dst), e - s);
	}
	if (bad) {
		free(buf);
		return DG_ERR_MALFORMED;
	}
	out->data = buf;
	out->len = n;
	return DG_OK;
}
