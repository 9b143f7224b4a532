// dg_splice_dev.hip — the splice of segment deltas on the device: the deltas of
// the consecutive segments of a large V, each against a window of R, become one
// standard delta R -> V per group, byte for byte what dg_splice (dg_splice.cpp)
// produces: the normal form of include/delta_gpu.h.
//
// Built on its own as lib/dg_splice.hsaco and loaded by dg_splice_host.cpp.
// Three kernels, with the library's size scan before the last:
//
//   dg_splice_map_kernel      one wave per segment.  Parses the stream through
//     a 1 KiB LDS window (dg_parse_chain.h), checks every field, and reduces
//     the segment to a fixed-size summary: its status, the bytes of its own
//     normal form, kind / start in R / length of its first run, kind / end in
//     R / length of its last run, whether it is one run, and its dst_crc
//     weighted by the bytes of V that follow it.
//   dg_splice_resolve_kernel  one wave per group walks the summaries 64 at a
//     time with wave scans and a carry: decides every seam (a run may cross
//     any number of segments), gives each segment its place in the group's
//     output, says whether its first run continues its predecessor's (no
//     header then) and gives the run that begins as a segment's last run its
//     whole length; reduces status, size and dst_crc.
//   dg_splice_emit_kernel     one wave per segment parses the stream again and
//     writes the rebased commands and the payloads.  A run's length field is
//     written by the command that begins the next run of the segment, and the
//     last run's from the resolve stage's record.  The first segment's block
//     writes the header, the last one the END byte.
//
// No byte outside [0, len) of a stream is read.  Every store of the emit stage
// is checked against the segment's own resolved range (a miss is
// DG_ERR_INTERNAL, never a stray byte), so a wrong summary cannot write
// outside the group's slot.
#include <hip/hip_runtime.h>

#include "dg_devutil.h"
#include "dg_parse_chain.h"
#include "dg_splice_dev.h"
#include "dg_stream_dev.h"

using namespace dg;
using namespace dgsp;

namespace {

__device__ __forceinline__ uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

__device__ __forceinline__ uint64_t wave_xor64(uint64_t x, uint32_t lane) {
	for (uint32_t o = 32; o; o >>= 1) x ^= shfl64(x, lane ^ o);
	return x;
}

// What the walk of a segment's stream finds.
struct Walk {
	bool bad = false, unsup = false;
	uint32_t heads = 0;                     // runs that begin in the segment
	uint32_t first_kind = 0, first_src = 0;
	uint32_t second_v = 0, last_head_v = 0; // where the second and the last run begin in the segment's version
	uint32_t last_kind = 0, last_end = 0;   // the last non-empty command
	uint64_t body = 0;
	bool o_has = false;                     // emit: the run open at the end, its length field
	uint32_t o_lf = 0;
};

// One wave walks stream S of dl bytes (a DLT\x03 magic was seen).  With kEmit
// the runs' bytes go to O[0 .. limit): cont says that the first non-empty
// command continues a run of an earlier segment.
template <bool kEmit>
__device__ __forceinline__ Walk seg_walk(const ChainLds& cl, const uint8_t* S, uint32_t dl, const SpDesc& dd, bool cont,
                                         uint8_t* O, uint32_t limit, bool* stray) {
	const uint32_t lane = lane_id();
	const uint8_t* win = cl.win;
	const uint16_t* cmds = cl.cmds;
	Walk w;
	auto fits = [&](const uint8_t* p, uint32_t n) {
		const uint64_t at = (uint64_t)(p - O);
		const bool ok = at + n <= limit;
		if (!ok) *stray = true;
		return ok;
	};
	uint32_t pos = 25;
	uint64_t wpos = 0;
	bool c_has = false, ended = false;   // the last non-empty command so far: its kind and where its COPY ends in R
	uint32_t c_kind = 0, c_end = 0;
	uint32_t o_v = 0;                    // emit: where the open run begins in the segment's version
	while (!ended && !w.bad) {
		if (pos >= dl) break;   // the stream ends without an END byte
		const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, S, dl, pos), pos, dl);
		for (uint32_t b0 = 0; b0 < cw.cnt; b0 += 64) {
			const bool mine = b0 + lane < cw.cnt;
			const Hdr h = decode_hdr(win, cmds, b0 + lane, mine);
			const bool is_copy = mine && h.kind == 1;
			uint64_t tot_len, tot_bytes;
			const uint64_t pre_len = wave_excl_scan64(h.len, &tot_len);
			// commands placed sequentially: dst = the sum of the earlier lengths
			if (__ballot(mine && (uint64_t)h.dst != wpos + pre_len)) w.unsup = true;
			// a COPY reads the segment's window
			if (__ballot(is_copy && (uint64_t)h.src + h.len > dd.r_len)) w.bad = true;
			const bool ne = mine && h.len > 0;
			const uint32_t gsrc = h.src + dd.rebase;
			const uint32_t my_end = gsrc + h.len;
			const uint32_t pl = prev_set(ne, lane);
			// (every lane takes part in a shuffle: select afterwards)
			const uint32_t sh_kind = shfl32(h.kind, pl - 1);
			const uint32_t sh_end = shfl32(my_end, pl - 1);
			const bool p_has = pl || c_has;
			const uint32_t p_kind = pl ? sh_kind : c_kind;
			const uint32_t p_end = pl ? sh_end : c_end;
			const bool merge = ne && (p_has ? p_kind == h.kind && (h.kind == 2 || p_end == gsrc) : cont);
			const bool head = ne && !merge;
			const uint32_t bytes = ne ? (head ? (h.kind == 1 ? 13u : 9u) : 0u) + (h.kind == 2 ? h.len : 0u) : 0u;
			const uint64_t out_rel = w.body + wave_excl_scan64(bytes, &tot_bytes);
			const uint64_t nm = __ballot(ne), hm = __ballot(head);
			if (nm && !c_has) {
				const uint32_t f = ffs64(nm);
				w.first_kind = shfl32(h.kind, f);
				w.first_src = shfl32(gsrc, f);
			}
			if (hm) {
				const uint64_t m2 = w.heads == 0 ? (hm & (hm - 1)) : hm;
				const uint32_t k2 = shfl32(h.dst, m2 ? ffs64(m2) : 0u);
				if (w.heads < 2 && m2) w.second_v = k2;
				w.last_head_v = shfl32(h.dst, 63u - (uint32_t)__builtin_clzll(hm));
			}
			if constexpr (kEmit) {
				const uint32_t orel = (uint32_t)out_rel;
				uint8_t* dp = O + orel;
				if (head) {
					if (h.kind == 1) {
						if (fits(dp, 9)) {
							dp[0] = 1;
							put_be32(dp + 1, gsrc);
							put_be32(dp + 5, dd.v_rel + h.dst);
						}
					} else if (fits(dp, 5)) {
						dp[0] = 2;
						put_be32(dp + 1, dd.v_rel + h.dst);
					}
				}
				// a run's length: written by the command that begins the next run
				const uint32_t my_lf = orel + (h.kind == 1 ? 9u : 5u);
				const uint32_t ps = prev_set(head, lane);
				const uint32_t sh_lf = shfl32(my_lf, ps - 1);
				const uint32_t sh_v = shfl32(h.dst, ps - 1);
				const uint32_t p_lf = ps ? sh_lf : w.o_lf;
				const uint32_t p_v = ps ? sh_v : o_v;
				if (head && (ps || w.o_has) && fits(O + p_lf, 4)) put_be32(O + p_lf, h.dst - p_v);
				const uint32_t lo = last_set(head);
				if (lo) {
					w.o_has = true;
					w.o_lf = shfl32(my_lf, lo - 1);
					o_v = shfl32(h.dst, lo - 1);
				}
				// payloads: small spans by their lane, long ones by the whole wave in ballot order
				uint32_t nb = ne && h.kind == 2 ? h.len : 0u;
				const uint8_t* sp = S + pos + h.cx + 9;
				uint8_t* cp = dp + (head ? 9u : 0u);
				if (nb && !fits(cp, nb)) nb = 0;
				if (nb <= kSmallCopy)
					for (uint32_t k = 0; k < nb; ++k) cp[k] = sp[k];
				for (uint64_t mk = __ballot(nb > kSmallCopy); mk; mk &= mk - 1) {
					const uint32_t f = ffs64(mk);
					const uint8_t* s2 = reinterpret_cast<const uint8_t*>(uni64((uint64_t)(uintptr_t)__shfl((unsigned long long)(uintptr_t)sp, (int)f, 64)));
					uint8_t* d2 = reinterpret_cast<uint8_t*>(uni64((uint64_t)(uintptr_t)__shfl((unsigned long long)(uintptr_t)cp, (int)f, 64)));
					wave_copy(d2, s2, rdlane(nb, f), lane);
				}
			}
			const uint32_t ls = last_set(ne);
			if (ls) {
				c_has = true;
				c_kind = shfl32(h.kind, ls - 1);
				c_end = shfl32(my_end, ls - 1);
			}
			w.heads += (uint32_t)__builtin_popcountll(hm);
			w.body += tot_bytes;
			wpos += tot_len;
		}
		if (cw.term == kChBad) w.bad = true;
		if (cw.term == kChEnd) ended = true;
		pos = cw.next_pos;
		wave_sync();   // the window is rewritten next
	}
	if (wpos != dd.v_len) w.unsup = true;
	w.last_kind = c_kind;
	w.last_end = c_end;
	return w;
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void dg_splice_map_kernel(SpArgs a) {
	__shared__ __attribute__((aligned(16))) uint32_t lds[(kChainLdsBytes + 3) / 4];
	const uint32_t j = blockIdx.x;
	if (j >= a.n_seg) return;
	const uint32_t lane = lane_id();
	const SpDesc dd = a.descs[j];
	SpSum s{};
	auto finish = [&](int32_t own) {
		s.own = own;
		if (lane == 0) a.sums[j] = s;
	};
	if (a.seg_status && a.seg_status[j] != 0) {
		s.incoming = a.seg_status[j];
		return finish(0);
	}
	const uint64_t off = a.offsets[j];
	const uint64_t len = a.offsets[j + 1] - off;
	// (a stream of 4 GiB or more cannot be parsed with 32-bit offsets; its
	// capacity is below that, so it is longer than its capacity)
	if (len >= (1ull << 32)) return finish(7);
	const uint8_t* S = a.deltas + off;
	const uint32_t dl = (uint32_t)len;
	if (bad_magic(S, dl)) return finish(8);
	bool stray = false;
	const Walk w = seg_walk<false>(chain_lds(lds), S, dl, dd, false, nullptr, 0, &stray);
	if (w.bad) return finish(8);
	if (len > dd.cap) return finish(7);
	if (w.unsup || (S[4] & 1) || be32(S + 5) != dd.v_len) return finish(2);
	s.runs = w.heads;
	s.flags = w.heads == 1 ? kSingle : 0u;
	s.first_kind = w.first_kind;
	s.first_src = w.first_src;
	s.first_len = w.heads >= 2 ? w.second_v : dd.v_len;
	s.last_kind = w.last_kind;
	s.last_end = w.last_end;
	s.last_len = dd.v_len - w.last_head_v;
	s.body = w.body;
	s.crc_term = gf2_mulmod(be64(S + 17), dd.shift);
	finish(0);
}

extern "C" __global__ __launch_bounds__(64) void dg_splice_resolve_kernel(SpArgs a) {
	const uint32_t g = blockIdx.x;
	if (g >= a.n_groups) return;
	const uint32_t lane = lane_id();
	const SpGroup G = a.groups[g];
	int32_t incoming = 0;
	bool any8 = false, any7 = false, any2 = false;
	bool c_has = false, o_has = false;   // the last contributing segment's last run; the run that is open
	uint32_t c_kind = 0, c_end = 0, o_idx = 0, o_v = 0;
	uint64_t osize = 0, crc = 0;
	for (uint32_t b0 = 0; b0 < G.count; b0 += 64) {
		const bool mine = b0 + lane < G.count;
		const uint32_t j = G.first + b0 + (mine ? lane : 0u);
		SpSum s{};
		uint32_t v_rel = 0, v_len = 0;
		if (mine) {
			s = a.sums[j];
			v_rel = a.descs[j].v_rel;
			v_len = a.descs[j].v_len;
		}
		const uint64_t im = __ballot(mine && s.incoming != 0);
		const int32_t sh_in = (int32_t)shfl32((uint32_t)s.incoming, im ? ffs64(im) : 0u);
		if (!incoming && im) incoming = sh_in;
		if (__ballot(mine && s.own == 8)) any8 = true;
		if (__ballot(mine && s.own == 7)) any7 = true;
		if (__ballot(mine && s.own == 2)) any2 = true;
		const bool ok = mine && s.incoming == 0 && s.own == 0;
		crc ^= wave_xor64(ok ? s.crc_term : 0ull, lane);
		const bool ne = ok && s.runs > 0;
		const uint32_t pl = prev_set(ne, lane);
		const uint32_t sh_kind = shfl32(s.last_kind, pl - 1);
		const uint32_t sh_end = shfl32(s.last_end, pl - 1);
		const bool p_has = pl || c_has;
		const uint32_t p_kind = pl ? sh_kind : c_kind;
		const uint32_t p_end = pl ? sh_end : c_end;
		const bool merge = ne && p_has && p_kind == s.first_kind && (s.first_kind == 2 || p_end == s.first_src);
		const uint32_t bytes = ne ? (uint32_t)s.body - (merge ? (s.first_kind == 1 ? 13u : 9u) : 0u) : 0u;
		uint64_t tot_bytes;
		const uint64_t out_rel = osize + wave_excl_scan64(bytes, &tot_bytes);
		// the segment's last run begins a run of the output unless the segment is one run that continues another
		const bool setter = ne && (!merge || !(s.flags & kSingle));
		const uint32_t start_v = v_rel + v_len - s.last_len;
		const uint32_t close_v = merge ? v_rel + s.first_len : v_rel;   // where the run open before it ends
		const uint32_t ps = prev_set(setter, lane);
		const uint32_t sh_v = shfl32(start_v, ps - 1);
		const uint32_t p_idx = ps ? G.first + b0 + ps - 1 : o_idx;
		const uint32_t p_v = ps ? sh_v : o_v;
		if (setter && (ps || o_has)) a.recs[p_idx].last_len = close_v - p_v;
		if (mine) {
			// (field by field: last_len belongs to whoever closes the run)
			a.recs[j].out = (uint32_t)out_rel;
			a.recs[j].out_end = (uint32_t)out_rel + bytes;
			a.recs[j].flags = (merge ? kContinues : 0u) | (setter ? kOwnsRun : 0u);
		}
		const uint32_t ls = last_set(ne);
		if (ls) {
			c_has = true;
			c_kind = shfl32(s.last_kind, ls - 1);
			c_end = shfl32(s.last_end, ls - 1);
		}
		const uint32_t lo = last_set(setter);
		if (lo) {
			o_has = true;
			o_idx = G.first + b0 + lo - 1;
			o_v = shfl32(start_v, lo - 1);
		}
		osize += tot_bytes;
	}
	const uint64_t size = 25 + osize + 1;
	const int32_t st = incoming ? incoming : any8 ? 8 : any7 ? 7 : any2 ? 2 : size >= (1ull << 32) ? 3 : 0;
	if (lane == 0) {
		if (o_has) a.recs[o_idx].last_len = G.v_len - o_v;
		a.status[g] = st;
		a.sizes[g] = st ? 0 : size;
		a.res[g].dst_crc = crc;
	}
}

extern "C" __global__ __launch_bounds__(64) void dg_splice_emit_kernel(SpArgs a) {
	__shared__ __attribute__((aligned(16))) uint32_t lds[(kChainLdsBytes + 3) / 4];
	const uint32_t j = blockIdx.x;
	if (j >= a.n_seg) return;
	const uint32_t lane = lane_id();
	const SpDesc dd = a.descs[j];
	const uint32_t g = dd.group;
	if (a.status[g] != 0) return;
	const SpGroup G = a.groups[g];
	const uint64_t base = a.out_offsets[g], end = a.out_offsets[g + 1];
	if (end > a.out_cap) {
		if (j == G.first && lane == 0) a.status[g] = 7;
		return;
	}
	if (end - base < 26) return;   // (never: a group that is DG_OK has its header and END byte)
	const uint32_t body = (uint32_t)(end - base) - 26;   // the command bytes
	uint8_t* B = a.out + base + 25;
	if (j == G.first && lane < 25) {
		const uint64_t sc = a.src_crc[g], dc = a.res[g].dst_crc;
		uint8_t x;
		if (lane < 4) x = lane == 0 ? 'D' : lane == 1 ? 'L' : lane == 2 ? 'T' : 3;
		else if (lane == 4) x = 0;
		else if (lane < 9) x = (uint8_t)(G.v_len >> (8 * (8 - lane)));
		else if (lane < 17) x = (uint8_t)(sc >> (8 * (16 - lane)));
		else x = (uint8_t)(dc >> (8 * (24 - lane)));
		B[(int)lane - 25] = x;
	}
	if (j == G.first + G.count - 1 && lane == 0) B[body] = 0;
	const SpRec r = a.recs[j];
	// the segment's own range, inside the group's command bytes
	if (r.out_end <= r.out || r.out_end > body) {
		if (r.out_end > body && lane == 0) a.status[g] = 12;
		return;
	}
	const uint64_t off = a.offsets[j];
	const uint32_t dl = (uint32_t)(a.offsets[j + 1] - off);
	const uint8_t* S = a.deltas + off;
	uint8_t* O = B + r.out;
	const uint32_t limit = r.out_end - r.out;
	bool stray = false;
	const Walk w = seg_walk<true>(chain_lds(lds), S, dl, dd, (r.flags & kContinues) != 0, O, limit, &stray);
	if (lane == 0 && w.o_has && (r.flags & kOwnsRun)) {
		if ((uint64_t)w.o_lf + 4 <= limit) put_be32(O + w.o_lf, r.last_len);
		else stray = true;
	}
	if (stray || w.body != limit) a.status[g] = 12;
}
