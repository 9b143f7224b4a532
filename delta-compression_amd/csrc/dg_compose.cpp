// dg_compose.cpp — composition of two standard deltas on the host:
// A = delta(R -> V1) and B = delta(V1 -> V2) give C = delta(R -> V2), without
// R, V1 or V2 (dg_compose; include/delta_gpu.h states the contract and the
// normal form).
//
// Pure host code with no HIP dependency and no context: the comparator of the
// device path (dg_compose_dev.hip) and the engine of `delta compose`.  It is
// also compiled alone under AddressSanitizer/UBSan with dg_format.cpp by
// tests/test_compose_sanitize_cpu.py.
//
// Every byte of V2 is a literal of B, a literal of A, or a byte of R.  A's
// non-empty commands tile V1, so a COPY(s, l) of B is the slice [s, s + l) of
// that tiling: one binary search finds its first command of A, a walk yields
// the pieces.  Pieces go through one run builder that merges neighbours
// maximally, wherever they came from.  Cost: linear in input plus output, one
// binary search per COPY of B.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

uint32_t be32(const uint8_t* p) {
	return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
void put32(uint8_t* p, uint64_t x) {
	p[0] = (uint8_t)(x >> 24);
	p[1] = (uint8_t)(x >> 16);
	p[2] = (uint8_t)(x >> 8);
	p[3] = (uint8_t)x;
}

struct Cmd {
	uint32_t kind;   // 1 COPY, 2 ADD
	uint32_t v;      // where it starts in the stream's version
	uint32_t len;
	uint64_t ref;    // COPY: the source offset; ADD: the payload's offset in the stream
};

struct Parsed {
	bool malformed = false;   // magic, framing, an unknown command, a payload past the end
	bool inplace = false;
	bool placed = true;       // every dst = the sum of the earlier lengths, and they sum to version_size
	bool wide = false;        // a COPY with src + len > 2^32
	uint32_t version_size = 0;
	std::vector<Cmd> cmds;    // the non-empty commands, in stream order
};

// One walk of the stream (the framing of dg_format.cpp's walk: a stream
// without the END byte ends at the buffer's end; bytes after END are ignored).
void parse(const uint8_t* d, size_t len, Parsed& p) {
	if (len < DG_HEADER_SIZE || memcmp(d, "DLT\x03", 4) != 0) {
		p.malformed = true;
		return;
	}
	p.inplace = d[4] & 1;
	p.version_size = be32(d + 5);
	uint64_t at = 0;
	size_t pos = DG_HEADER_SIZE;
	while (pos < len) {
		const uint8_t t = d[pos++];
		if (t == 0) break;
		uint64_t src = 0, dst, l, ref;
		if (t == 1) {
			if (len - pos < 12) { p.malformed = true; return; }
			src = be32(d + pos);
			dst = be32(d + pos + 4);
			l = be32(d + pos + 8);
			pos += 12;
			ref = src;
			if (src + l > (1ull << 32)) p.wide = true;
		} else if (t == 2) {
			if (len - pos < 8) { p.malformed = true; return; }
			dst = be32(d + pos);
			l = be32(d + pos + 4);
			pos += 8;
			if (len - pos < l) { p.malformed = true; return; }
			ref = pos;
			pos += l;
		} else {
			p.malformed = true;
			return;
		}
		if (dst != at) p.placed = false;
		if (l && p.placed) p.cmds.push_back(Cmd{t, (uint32_t)dst, (uint32_t)l, ref});
		at += l;
	}
	if (at != p.version_size) p.placed = false;
}

// The output under construction: the run that is still open merges with the
// next piece when that piece continues it.
struct Builder {
	std::vector<uint8_t> out;
	uint64_t at = 0;          // bytes of V2 placed so far
	uint32_t kind = 0;        // the open run's: 0 none, 1 COPY, 2 ADD
	uint64_t src = 0, len = 0;
	size_t hdr = 0;           // the open ADD's header in out

	void close() {
		if (kind == 1) {
			uint8_t h[13] = {1};
			put32(h + 1, src);
			put32(h + 5, at - len);
			put32(h + 9, len);
			out.insert(out.end(), h, h + 13);
		} else if (kind == 2) {
			put32(&out[hdr + 5], len);
		}
		kind = 0;
	}
	void copy(uint64_t s, uint64_t l) {
		if (kind == 1 && src + len == s) {
			len += l;
		} else {
			close();
			kind = 1;
			src = s;
			len = l;
		}
		at += l;
	}
	void add(const uint8_t* p, uint64_t l) {
		if (kind != 2) {
			close();
			kind = 2;
			len = 0;
			hdr = out.size();
			uint8_t h[9] = {2};
			put32(h + 1, at);
			out.insert(out.end(), h, h + 9);
		}
		out.insert(out.end(), p, p + l);
		len += l;
		at += l;
	}
};

int compose(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int ignore_hash, dg_buffer_t* out) {
	Parsed A, B;
	parse(a, a_len, A);
	parse(b, b_len, B);
	if (A.malformed || B.malformed || A.wide) return DG_ERR_MALFORMED;
	// a COPY of B reads V1: past A's version size it reads nothing
	{
		size_t pos = DG_HEADER_SIZE;
		while (pos < b_len && b[pos] != 0) {
			if (b[pos] == 1) {
				if ((uint64_t)be32(b + pos + 1) + be32(b + pos + 9) > A.version_size) return DG_ERR_MALFORMED;
				pos += 13;
			} else {
				pos += 9 + (size_t)be32(b + pos + 5);
			}
		}
	}
	if (A.inplace || B.inplace || !A.placed || !B.placed) return DG_ERR_UNSUPPORTED;
	if (!ignore_hash && memcmp(a + 17, b + 9, DG_CRC_SIZE) != 0) return DG_ERR_SRC_CRC;

	Builder w;
	w.out.resize(DG_HEADER_SIZE);
	memcpy(&w.out[0], "DLT\x03", 4);
	w.out[4] = 0;
	put32(&w.out[5], B.version_size);
	memcpy(&w.out[9], a + 9, DG_CRC_SIZE);
	memcpy(&w.out[17], b + 17, DG_CRC_SIZE);
	const std::vector<Cmd>& ac = A.cmds;
	for (const Cmd& c : B.cmds) {
		if (c.kind == 2) {
			w.add(b + c.ref, c.len);
			continue;
		}
		const uint64_t s = c.ref, e = s + c.len;
		// the last command of A that starts at or before s
		size_t j = (size_t)(std::upper_bound(ac.begin(), ac.end(), s, [](uint64_t x, const Cmd& k) { return x < k.v; }) -
		                    ac.begin()) - 1;
		for (uint64_t x = s; x < e; ++j) {
			const Cmd& k = ac[j];
			const uint64_t y = std::min<uint64_t>(e, (uint64_t)k.v + k.len);
			if (k.kind == 1) w.copy(k.ref + (x - k.v), y - x);
			else w.add(a + k.ref + (x - k.v), y - x);
			x = y;
		}
	}
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

extern "C" int dg_compose(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, int ignore_hash,
                          dg_buffer_t* out) {
	if (!out || (a_len && !a) || (b_len && !b)) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	if (a_len >= (1ull << 32) || b_len >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	try {
		return compose(a, a_len, b, b_len, ignore_hash, out);
	} catch (const std::bad_alloc&) {
		return DG_ERR_NOMEM;
	}
}
