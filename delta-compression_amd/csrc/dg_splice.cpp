// dg_splice.cpp — the segmentation rule of a large pair and the splice of its
// segments' deltas on the host: the k deltas of k consecutive segments of V,
// each against a window of R, give one standard delta R -> V (dg_segment_pairs,
// dg_splice; include/delta_gpu.h states the rule, the contract and the normal
// form).
//
// Pure host code with no HIP dependency and no context: the comparator of the
// device path (dg_splice_dev.hip).  It is also compiled alone under
// AddressSanitizer/UBSan with dg_plan.cpp and dg_format.cpp by
// tests/test_splice_sanitize_cpu.py.
//
// Every byte of V is a literal of one segment's delta or a byte of that
// segment's window, which is a byte of R at the window's offset.  The
// segments' non-empty commands, sources rebased, go in order through the run
// builder that composition uses: neighbours merge maximally, inside a stream
// and across the seams alike.  Linear in the input.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/delta_gpu.h"
#include "dg_plan.h"

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
uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

struct Cmd {
	uint32_t kind;   // 1 COPY, 2 ADD
	uint32_t len;
	uint64_t ref;    // COPY: the source offset in the window; ADD: the payload's offset in the stream
};

struct Parsed {
	bool malformed = false;   // magic, framing, an unknown command, a payload past the end, a COPY past the window
	bool inplace = false;
	bool placed = true;       // every dst = the sum of the earlier lengths, and they sum to version_size
	uint32_t version_size = 0;
	std::vector<Cmd> cmds;    // the non-empty commands, in stream order
};

// One walk of the stream (the framing of dg_format.cpp's walk: a stream
// without the END byte ends at the buffer's end; bytes after END are ignored).
void parse(const uint8_t* d, size_t len, uint64_t window, Parsed& p) {
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
		uint64_t dst, l, ref;
		if (t == 1) {
			if (len - pos < 12) { p.malformed = true; return; }
			ref = be32(d + pos);
			dst = be32(d + pos + 4);
			l = be32(d + pos + 8);
			pos += 12;
			// the splicer knows the window: rebased, such a COPY would read valid but wrong bytes of R
			if (ref + l > window) p.malformed = true;
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
		if (l && p.placed && !p.malformed) p.cmds.push_back(Cmd{t, (uint32_t)l, ref});
		at += l;
	}
	if (at != p.version_size) p.placed = false;
}

// The output under construction: the run that is still open merges with the
// next piece when that piece continues it.
struct Builder {
	std::vector<uint8_t> out;
	uint64_t at = 0;          // bytes of V placed so far
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

int splice(const dg_pair_t& whole, const dg::SpliceGeometry& g, uint32_t n_seg, const uint8_t* const* deltas,
           const size_t* delta_len, const int32_t* seg_status, const uint8_t* src_crc, dg_buffer_t* out) {
	if (seg_status)
		for (uint32_t j = 0; j < n_seg; ++j)
			if (seg_status[j] != 0) return seg_status[j];
	std::vector<Parsed> P(n_seg);
	bool bad = false, unsup = false;
	for (uint32_t j = 0; j < n_seg; ++j) {
		if (delta_len[j] >= (1ull << 32)) return DG_ERR_TOO_LARGE;
		parse(deltas[j], delta_len[j], g.descs[j].r_len, P[j]);
		if (P[j].malformed) bad = true;
		else if (P[j].inplace || !P[j].placed || P[j].version_size != g.descs[j].v_len) unsup = true;
	}
	if (bad) return DG_ERR_MALFORMED;
	if (unsup) return DG_ERR_UNSUPPORTED;

	Builder w;
	w.out.resize(DG_HEADER_SIZE);
	memcpy(&w.out[0], "DLT\x03", 4);
	w.out[4] = 0;
	put32(&w.out[5], whole.v_len);
	memcpy(&w.out[9], src_crc, DG_CRC_SIZE);
	// crc(X || Y) = crc(X) x^(8 |Y|) + crc(Y): every segment's dst_crc weighted by the bytes after it
	uint64_t crc = 0;
	for (uint32_t j = 0; j < n_seg; ++j) {
		crc ^= dg::gf2_mul(be64(deltas[j] + 17), g.descs[j].shift);
		for (const Cmd& c : P[j].cmds) {
			if (c.kind == 1) w.copy(c.ref + g.descs[j].rebase, c.len);
			else w.add(deltas[j] + c.ref, c.len);
		}
	}
	put32(&w.out[17], crc >> 32);
	put32(&w.out[21], crc);
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

extern "C" int dg_segment_pairs(const dg_pair_t* wholes, uint32_t n_groups, uint64_t seg_bytes, uint64_t window_bytes,
                                dg_pair_t* segs, uint64_t segs_cap, uint32_t* seg_first) {
	if ((n_groups && !wholes) || !seg_first || seg_bytes == 0 || (seg_bytes & 15) || (window_bytes & 15)) return DG_ERR_INVALID_ARG;
	const uint64_t S = seg_bytes, W = window_bytes;
	uint64_t n = 0;
	seg_first[0] = 0;
	for (uint32_t g = 0; g < n_groups; ++g) {
		const dg_pair_t& w = wholes[g];
		if (w.r_len >= (1ull << 32) - (1ull << 20) || w.v_len >= (1ull << 32) - (1ull << 20)) return DG_ERR_TOO_LARGE;
		const uint64_t k = std::max<uint64_t>(1, (w.v_len + S - 1) / S);
		if (n + k > 0xFFFFFFFFull) return DG_ERR_TOO_LARGE;
		if (segs) {
			if (n + k > segs_cap) return DG_ERR_CAPACITY;
			for (uint64_t j = 0; j < k; ++j) {
				const uint64_t v0 = std::min(j * S, w.v_len), v1 = std::min((j + 1) * S, w.v_len);
				const uint64_t lo = std::min(j * S, w.r_len);
				const uint64_t a = lo - std::min(lo, W);
				const uint64_t b = std::min(w.r_len, j * S + S + W);
				segs[n + j] = dg_pair_t{w.r_off + a, std::max(a, b) - a, w.v_off + v0, v1 - v0};
			}
		}
		n += k;
		seg_first[g + 1] = (uint32_t)n;
	}
	return DG_OK;
}

extern "C" int dg_splice(const dg_pair_t* whole, const dg_pair_t* segs, uint32_t n_seg, const uint8_t* const* deltas,
                         const size_t* delta_len, const int32_t* seg_status, const uint8_t src_crc[DG_CRC_SIZE],
                         dg_buffer_t* out) {
	if (!out) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	if (!whole || !segs || !deltas || !delta_len || !src_crc || n_seg == 0) return DG_ERR_INVALID_ARG;
	for (uint32_t j = 0; j < n_seg; ++j)
		if (delta_len[j] && !deltas[j]) return DG_ERR_INVALID_ARG;
	try {
		dg::SpliceGeometry g;
		std::string err;
		const uint32_t first[2] = {0, n_seg};
		const int rc = dg::splice_plan_geometry(segs, n_seg, whole, first, 1, nullptr, g, err);
		if (rc) return rc;
		return splice(*whole, g, n_seg, deltas, delta_len, seg_status, src_crc, out);
	} catch (const std::bad_alloc&) {
		return DG_ERR_NOMEM;
	}
}
