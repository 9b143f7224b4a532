// dg_lineage.cpp — a byte range of a version that is k standard deltas away
// from a whole buffer, on the host (dg_read_lineage; include/delta_gpu.h states
// the contract).
//
// Pure host code with no HIP dependency and no context: the comparator of the
// device path (dg_lineage_dev.hip) and the engine of `delta lineage`.  It is
// also compiled alone under AddressSanitizer/UBSan by
// tests/test_lineage_sanitize_cpu.py.
//
// V_j = apply(V_{j-1}, d_j), V_0 = R.  No V_j is built.  Every level is
// validated whole, from the requested one towards R, exactly as the index
// pass of the read plan validates a stream (dg_read_dev.hip), which also
// leaves a sparse index of it: per kStride bytes of stream the first command
// at or after that offset and its dst.  The range is then resolved by
// recursion: the commands of d_k that meet [off, off + n) are found through
// the index; an ADD's bytes are copied out, a COPY becomes the range
// [src, src + len) of V_{k-1}, resolved the same way one level down, and at
// level 1 copied from R.  Every level is sequential (its commands tile its
// version in stream order), so every output byte is written exactly once.
// Work memory: the n output bytes, one frame per level, and 16 bytes per
// kStride bytes of the deltas.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/delta_gpu.h"

namespace {

constexpr uint64_t kStride = 1024;            // stream bytes per index entry
constexpr uint64_t kNoLimit = 0xFFFFFFFFull;  // ref_len of a level whose parent has no readable header

uint64_t get32(const uint8_t* p) {
	return ((uint64_t)p[0] << 24) | ((uint64_t)p[1] << 16) | ((uint64_t)p[2] << 8) | p[3];
}

bool has_header(const uint8_t* d, size_t dl) { return dl >= DG_HEADER_SIZE && memcmp(d, "DLT\x03", 4) == 0; }

struct Ent {
	uint64_t spos, dst;
};

struct Level {
	const uint8_t* d = nullptr;
	size_t dl = 0;
	uint64_t vsize = 0;
	std::vector<Ent> ix;   // entry k: the first command at or after stream offset kStride * k
};

// one command at pos of a validated stream; false at END or the end of input
struct Cmd {
	bool copy;
	uint64_t src, dst, len;   // src: of the level below, or the payload's stream offset
	size_t next;
};
bool cmd_at(const Level& L, size_t pos, Cmd* c) {
	if (pos >= L.dl || L.d[pos] == 0) return false;
	const uint8_t* p = L.d + pos;
	if (p[0] == 1) {
		*c = Cmd{true, get32(p + 1), get32(p + 5), get32(p + 9), pos + 13};
	} else {
		const uint64_t l = get32(p + 5);
		*c = Cmd{false, pos + 9, get32(p + 1), l, pos + 9 + (size_t)l};
	}
	return true;
}

// the index pass's verdict on one level (status a, then b) and its index
int validate(Level& L, uint64_t ref_len) {
	const uint8_t* d = L.d;
	const size_t dl = L.dl;
	if (!has_header(d, dl)) return DG_ERR_MALFORMED;
	if (d[4] & 1) return DG_ERR_UNSUPPORTED;   // in-place
	L.vsize = get32(d + 5);
	bool seq = true;
	uint64_t run_end = 0;
	size_t pos = DG_HEADER_SIZE, next_ent = 0;
	try {
		L.ix.reserve(dl / kStride + 1);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	while (pos < dl) {   // a missing END is the end of input (encoding.c:111-178)
		const uint8_t t = d[pos];
		if (t == 0) break;
		uint64_t dst, l;
		size_t next;
		if (t == 1) {
			if (dl - pos < 13) return DG_ERR_MALFORMED;
			const uint64_t src = get32(d + pos + 1);
			dst = get32(d + pos + 5);
			l = get32(d + pos + 9);
			next = pos + 13;
			if (src + l > ref_len) return DG_ERR_MALFORMED;
		} else if (t == 2) {
			if (dl - pos < 9) return DG_ERR_MALFORMED;
			dst = get32(d + pos + 1);
			l = get32(d + pos + 5);
			if (l > dl - pos - 9) return DG_ERR_MALFORMED;
			next = pos + 9 + (size_t)l;
		} else {
			return DG_ERR_MALFORMED;
		}
		if (dst + l > L.vsize) return DG_ERR_MALFORMED;
		if (dst != run_end) seq = false;
		run_end = dst + l;
		for (; next_ent * kStride <= pos; ++next_ent) L.ix.push_back(Ent{pos, dst});
		pos = next;
	}
	if (run_end != L.vsize) seq = false;
	return seq ? DG_OK : DG_ERR_UNSUPPORTED;
}

struct Walk {
	const uint8_t* r;
	std::vector<Level> lv;   // lv[j - 1]: d_j
};

// bytes [lo, hi) of V_j to out; lo < hi <= |V_j|
void resolve(const Walk& w, uint32_t j, uint64_t lo, uint64_t hi, uint8_t* out) {
	if (j == 0) {
		memcpy(out, w.r + lo, hi - lo);
		return;
	}
	const Level& L = w.lv[j - 1];
	// the last entry whose dst is <= lo: the commands before its command end at or before its dst
	size_t x = 0, y = L.ix.size();
	while (x < y) {
		const size_t mid = (x + y) / 2;
		if (L.ix[mid].dst <= lo) x = mid + 1;
		else y = mid;
	}
	size_t pos = x ? (size_t)L.ix[x - 1].spos : DG_HEADER_SIZE;
	Cmd c;
	while (cmd_at(L, pos, &c) && c.dst < hi) {
		const uint64_t s = std::max(c.dst, lo), e = std::min(c.dst + c.len, hi);
		if (e > s) {
			if (c.copy) resolve(w, j - 1, c.src + (s - c.dst), c.src + (e - c.dst), out + (s - lo));
			else memcpy(out + (s - lo), L.d + c.src + (s - c.dst), e - s);
		}
		pos = c.next;
	}
}

}  // namespace

extern "C" int dg_read_lineage(const uint8_t* r, size_t r_len, const uint8_t* const* deltas, const size_t* delta_len,
                               uint32_t k, uint64_t off, uint64_t len, dg_buffer_t* out) {
	if (!out || (r_len && !r) || (k && (!deltas || !delta_len)) || k > DG_LINEAGE_MAX_DEPTH) return DG_ERR_INVALID_ARG;
	out->data = nullptr;
	out->len = 0;
	for (uint32_t j = 0; j < k; ++j)
		if (delta_len[j] && !deltas[j]) return DG_ERR_INVALID_ARG;
	if (r_len >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	for (uint32_t j = 0; j < k; ++j)
		if (delta_len[j] >= (1ull << 32)) return DG_ERR_TOO_LARGE;
	Walk w;
	w.r = r;
	try {
		w.lv.resize(k);
	} catch (...) {
		return DG_ERR_NOMEM;
	}
	// from the requested level towards R: the first failing level's status
	for (uint32_t j = k; j >= 1; --j) {
		Level& L = w.lv[j - 1];
		L.d = deltas[j - 1];
		L.dl = delta_len[j - 1];
		uint64_t ref_len = r_len;
		if (j > 1) ref_len = has_header(deltas[j - 2], delta_len[j - 2]) ? get32(deltas[j - 2] + 5) : kNoLimit;
		const int st = validate(L, ref_len);
		if (st) return st;
	}
	const uint64_t vsize = k ? w.lv[k - 1].vsize : r_len;
	const uint64_t n = off >= vsize ? 0 : std::min(len, vsize - off);   // pread
	uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
	if (!buf) return DG_ERR_NOMEM;
	if (n) resolve(w, k, off, off + n, buf);
	out->data = buf;
	out->len = n;
	return DG_OK;
}
