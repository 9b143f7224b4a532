// dg_invert_dev.hip — inversion of a batch of deltas on the device:
// R_i and A_i = delta(R -> V) give delta(V -> R), byte for byte what dg_invert
// (dg_invert.cpp) produces: the normal form of include/delta_gpu.h.
//
// Built on its own as lib/dg_invert.hsaco and loaded by dg_invert_host.cpp.
// Two kernels, with the library's size scan between them:
//
//   dg_invert_map_kernel    one wave per delta.  Parses the stream through a
//     1 KiB LDS window (dg_parse_chain.h; all lanes decode the headers), checks
//     every field and writes one record per non-empty COPY.  The records are
//     wanted in key order (src ascending, len descending, stream order): one
//     ballot per tile finds out whether the stream already has them so (every
//     encoder whose matches move forward in both buffers), else the wave sorts
//     them: a stable least-significant-digit radix sort over (src, ~len), 8-bit
//     digits, a 256-bin histogram in LDS, ranks inside a tile from ballots over
//     the digit's bits, ping-pong between two record buffers; a pass whose
//     digit is the same in every record is skipped.  The sweep then runs over
//     tiles of 64 records: the exclusive prefix max of the COPYs' ends (carried
//     across tiles) is where the bytes of R accounted for so far end, so each
//     lane has the literals before its COPY and the interval its COPY owns.
//     Whether that interval continues the COPY open before it, and which COPY
//     of the output a record closes, are "nearest earlier lane" lookups.
//     Writes one emit record per COPY, one for the literals at R's end, and the
//     delta's size.
//   dg_invert_emit_kernel   one 256-thread block per delta writes the header,
//     the ADDs with their payload from R, the COPY headers and the END byte.
//     A COPY's length field is written by the record that begins the next run.
//
// No byte outside [0, len) of the stream or [0, ref_len) of R is read and none
// outside the delta's output range is written: every multi-byte load is issued
// only where it fits, and every store is checked against the delta's end (a
// miss is DG_ERR_INTERNAL, never a stray byte).
#include <hip/hip_runtime.h>

#include "dg_devutil.h"
#include "dg_invert_dev.h"
#include "dg_parse_chain.h"
#include "dg_stream_dev.h"

using namespace dg;
using namespace dgiv;

namespace {

struct Work {
	IvRec* rec[2];    // C each
	IvEmit* emit;     // C + 1
};
__device__ __forceinline__ Work work_of(uint8_t* base, uint32_t C) {
	Work w;
	w.rec[0] = reinterpret_cast<IvRec*>(base);
	w.rec[1] = w.rec[0] + C;
	w.emit = reinterpret_cast<IvEmit*>(w.rec[1] + C);
	return w;
}

// digit `pass` of the key (src, ~len), least significant first
__device__ __forceinline__ uint32_t digit_of(const IvRec& r, uint32_t pass) {
	const uint32_t w = pass < 4 ? ~r.len : r.src;
	return (w >> (8u * (pass & 3u))) & 0xFFu;
}

// n records of from[] into key order, stably, by one wave; hist: 256 LDS words.
// Returns the buffer that holds them.
__device__ __forceinline__ IvRec* wave_sort(IvRec* from, IvRec* to, uint32_t n, uint32_t* hist, uint32_t lane) {
	for (uint32_t pass = 0; pass < 8; ++pass) {
		for (uint32_t k = lane; k < 256; k += 64) hist[k] = 0;
		wave_sync();
		for (uint32_t k = lane; k < n; k += 64) atomicAdd(&hist[digit_of(from[k], pass)], 1u);
		wave_sync();
		uint32_t h[4];
		bool one = false;
		for (uint32_t t = 0; t < 4; ++t) {
			h[t] = hist[4 * lane + t];
			one |= h[t] == n;
		}
		const bool skip = __ballot(one) != 0;   // every record has this digit: the pass changes nothing
		wave_sync();
		if (skip) continue;
		const uint32_t sum = h[0] + h[1] + h[2] + h[3];
		uint32_t at = wave_incl_scan(sum) - sum;
		for (uint32_t t = 0; t < 4; ++t) {
			hist[4 * lane + t] = at;   // the bin's next slot
			at += h[t];
		}
		wave_sync();
		for (uint32_t k0 = 0; k0 < n; k0 += 64) {
			const bool mine = k0 + lane < n;
			IvRec r{0, 0, 0, 0};
			if (mine) r = from[k0 + lane];
			const uint32_t d = digit_of(r, pass);
			uint64_t same = __ballot(mine);   // the tile's lanes with my digit
			for (uint32_t b = 0; b < 8; ++b) {
				const uint64_t bb = __ballot(mine && ((d >> b) & 1u));
				same &= ((d >> b) & 1u) ? bb : ~bb;
			}
			const uint32_t rank = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
			const uint32_t base = mine ? hist[d] : 0u;
			wave_sync();   // every lane has read its bin
			if (mine) {
				to[base + rank] = r;
				if ((same >> lane) == 1ull) hist[d] = base + rank + 1;   // the group's last lane
			}
			wave_sync();
		}
		IvRec* t = from;
		from = to;
		to = t;
	}
	return from;
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void dg_invert_map_kernel(IvArgs a) {
	__shared__ __attribute__((aligned(16))) uint32_t lds[(kChainLdsBytes + 3) / 4];
	static_assert(kChainLdsBytes >= 1024, "the sort's histogram takes the parser's LDS");
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t lane = lane_id();
	const IvDesc dd = a.descs[i];
	IvRes res{};
	auto finish = [&](int32_t st, uint64_t size) {
		if (lane == 0) {
			a.status[i] = st;
			a.sizes[i] = st ? 0 : size;
			a.res[i] = res;
		}
	};
	if (a.delta_status && a.delta_status[i] != 0) return finish(a.delta_status[i], 0);
	const uint64_t d_off = a.delta_offsets ? a.delta_offsets[i] : dd.delta_off;
	const uint64_t d_len = a.delta_offsets ? a.delta_offsets[i + 1] - d_off : dd.delta_cap;
	// (a stream of 4 GiB or more cannot be parsed with 32-bit offsets; its
	// capacity is below that, so it is longer than its capacity)
	if (d_len >= (1ull << 32)) return finish(7, 0);
	const bool over_cap = d_len > dd.delta_cap;
	const uint8_t* S = a.delta + d_off;
	const uint32_t dl = (uint32_t)d_len;
	const uint32_t ref_len = (uint32_t)dd.ref_len;   // below 4 GiB: the plan's geometry
	res.delta_off = d_off;
	const uint32_t C = dd.max_copies;
	const Work w = work_of(a.work + dd.work_off, C);

	const ChainLds cl = chain_lds(lds);
	const uint8_t* win = cl.win;
	const uint16_t* cmds = cl.cmds;
	bool bad = false, unsup = false, full = false, sorted = true;

	// ── the stream: validate, one record per non-empty COPY ──
	uint32_t nC = 0;
	if (bad_magic(S, dl)) {
		bad = true;
	} else {
		if (S[4] & 1) unsup = true;
		const uint32_t vs = be32(S + 5);
		uint32_t pos = 25;
		uint64_t wpos = 0;
		bool c_has = false, ended = false;   // the last record so far: its key
		uint64_t c_key = 0;
		while (!ended && !bad) {
			if (pos >= dl) break;   // the stream ends without an END byte
			const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, S, dl, pos), pos, dl);
			for (uint32_t b0 = 0; b0 < cw.cnt; b0 += 64) {
				const bool mine = b0 + lane < cw.cnt;
				const Hdr h = decode_hdr(win, cmds, b0 + lane, mine);
				const bool is_copy = mine && h.kind == 1;
				uint64_t tot_len;
				const uint64_t pre_len = wave_excl_scan64(h.len, &tot_len);
				// commands placed sequentially: dst = the sum of the earlier lengths
				if (__ballot(mine && (uint64_t)h.dst != wpos + pre_len)) unsup = true;
				// a COPY reads R
				if (__ballot(is_copy && (uint64_t)h.src + h.len > ref_len)) bad = true;
				const bool isrec = is_copy && h.len > 0;
				const uint32_t inc = wave_incl_scan(isrec ? 1u : 0u);
				const uint32_t cnt = rdlane(inc, 63);
				if (nC + cnt > C || nC + cnt < nC) full = true;
				// already in key order?  (stream order breaks ties, so equal keys are in order)
				const uint64_t key = ((uint64_t)h.src << 32) | (uint32_t)~h.len;
				const uint32_t pl = prev_set(isrec, lane);
				const uint64_t sh_key = shfl64(key, pl - 1);
				const uint64_t p_key = pl ? sh_key : c_key;
				if (__ballot(isrec && (pl || c_has) && key < p_key)) sorted = false;
				if (!bad && !full && isrec) {
					const uint32_t k = nC + inc - 1;
					w.rec[0][k] = IvRec{h.src, h.len, h.dst, k};
				}
				const uint32_t ls = last_set(isrec);
				if (ls) {
					c_has = true;
					c_key = shfl64(key, ls - 1);
				}
				if (!full) nC += cnt;
				wpos += tot_len;
			}
			if (cw.term == kChBad) bad = true;
			if (cw.term == kChEnd) ended = true;
			pos = cw.next_pos;
			wave_sync();   // the window is rewritten next
		}
		if (wpos != vs) unsup = true;
	}
	// ── the status, by kind of defect ──
	if (bad) return finish(8, 0);
	if (over_cap || full) return finish(7, 0);
	if (unsup) return finish(2, 0);
	wave_sync();

	// ── key order ──
	const IvRec* recs = w.rec[0];
	if (!sorted && nC > 1) recs = wave_sort(w.rec[0], w.rec[1], nC, lds, lane);

	// ── the sweep: literals before each COPY, the interval it owns, runs of the output ──
	uint32_t reach = 0;       // the bytes of R accounted for so far end here
	uint64_t osize = 0;       // command bytes of the output so far
	bool huge = false;
	bool c_has = false;       // the last non-empty owned interval so far: where it ends in V
	uint32_t c_vend = 0;
	bool o_has = false;       // the COPY of the output open so far: its length field and where it starts in R
	uint32_t o_lf = 0, o_x = 0;
	for (uint32_t k0 = 0; k0 < nC; k0 += 64) {
		const bool mine = k0 + lane < nC;
		IvRec r{0, 0, 0, 0};
		if (mine) r = recs[k0 + lane];
		const uint32_t end = r.src + r.len;   // <= ref_len
		const uint32_t incl = wave_incl_max(end);
		const uint32_t before = umax32(reach, wave_shr1z(incl));   // the exclusive prefix max
		const uint32_t gap = mine && r.src > before ? r.src - before : 0u;
		const uint32_t s = umax32(r.src, before);
		const bool owned = mine && s < end;   // (a gap implies it)
		const uint32_t vsrc = r.dst + (s - r.src);
		const uint32_t vend = owned ? vsrc + (end - s) : 0u;
		// does the interval continue the COPY piece before it?
		const uint32_t pl = prev_set(owned, lane);
		const uint32_t sh_vend = shfl32(vend, pl - 1);
		const uint32_t p_vend = pl ? sh_vend : c_vend;
		const bool merge = owned && gap == 0 && (pl || c_has) && p_vend == vsrc;
		const bool head = owned && !merge;
		const uint64_t bytes = (gap ? 9ull + gap : 0ull) + (head ? 13ull : 0ull);
		if (__ballot(bytes >= (1ull << 32))) huge = true;
		uint64_t tot_bytes;
		const uint32_t out_rel = (uint32_t)(osize + wave_excl_scan64((uint32_t)bytes, &tot_bytes));
		// a record that begins a run (its ADD, or its COPY when there are no
		// literals) closes the COPY open before it; both begin at `before`
		const uint32_t my_lf = out_rel + (gap ? 9u + gap : 0u) + 9u;
		const uint32_t ps = prev_set(head, lane);
		const uint32_t sh_lf = shfl32(my_lf, ps - 1);
		const uint32_t sh_x = shfl32(s, ps - 1);
		const uint32_t p_lf = ps ? sh_lf : o_lf;
		const uint32_t p_x = ps ? sh_x : o_x;
		const bool closes = head && (ps || o_has);
		if (mine) {
			IvEmit e;
			e.gap_x = before;
			e.gap_len = gap;
			e.out = out_rel;
			e.vsrc = vsrc;
			e.close_off = closes ? p_lf : kNoClose;
			e.close_len = before - p_x;
			e.head = head ? 1u : 0u;
			e.pad = 0;
			w.emit[k0 + lane] = e;
		}
		const uint32_t ls = last_set(owned);
		if (ls) {
			c_has = true;
			c_vend = shfl32(vend, ls - 1);
		}
		const uint32_t lh = last_set(head);
		if (lh) {
			o_has = true;
			o_lf = shfl32(my_lf, lh - 1);
			o_x = shfl32(s, lh - 1);
		}
		reach = umax32(reach, rdlane(incl, 63));
		osize += tot_bytes;
	}
	// the literals after the last COPY; this record closes the last COPY of the output
	const uint32_t tail = ref_len - reach;
	const uint64_t size = 25 + osize + (tail ? 9ull + tail : 0ull) + 1;
	if (huge || size >= (1ull << 32)) return finish(3, 0);
	if (lane == 0) {
		IvEmit e;
		e.gap_x = reach;
		e.gap_len = tail;
		e.out = (uint32_t)osize;
		e.vsrc = 0;
		e.close_off = o_has ? o_lf : kNoClose;
		e.close_len = reach - o_x;
		e.head = 0;
		e.pad = 0;
		w.emit[nC] = e;
	}
	res.n_emit = nC + 1;
	finish(0, size);
}

extern "C" __global__ __launch_bounds__(256) void dg_invert_emit_kernel(IvArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	if (a.status[i] != 0) return;
	const uint64_t base = a.out_offsets[i], end = a.out_offsets[i + 1];
	if (end > a.out_cap) {
		if (tid == 0) a.status[i] = 7;
		return;
	}
	const IvRes res = a.res[i];
	const IvDesc dd = a.descs[i];
	const uint8_t* S = a.delta + res.delta_off;
	const uint8_t* R = a.ref + dd.ref_off;
	const uint32_t ref_len = (uint32_t)dd.ref_len;
	const uint32_t body = (uint32_t)(end - base) - 26;   // the command bytes
	uint8_t* O = a.out + base + 25;
	const IvEmit* recs = work_of(a.work + dd.work_off, dd.max_copies).emit;
	const uint32_t n = res.n_emit;
	bool stray = false;   // a store that would leave the delta's range, or a load that would leave R: a bug, never issued
	auto fits = [&](const uint8_t* p, uint32_t nb) {
		const uint64_t at = (uint64_t)(p - O);
		const bool ok = at + nb <= body;
		if (!ok) stray = true;
		return ok;
	};
	// header: flag byte 0, R's length, the stream's destination CRC as source CRC and the other way round
	if (tid < 25) {
		uint8_t v;
		if (tid < 4) v = S[tid];
		else if (tid == 4) v = 0;
		else if (tid < 9) v = (uint8_t)(ref_len >> (8u * (8u - tid)));
		else if (tid < 17) v = S[tid + 8];
		else v = S[tid - 8];
		O[(int)tid - 25] = v;
	}
	if (tid == 0) O[body] = 0;
	for (uint32_t c0 = 64 * wave; c0 < n; c0 += 256) {
		const uint32_t m = c0 + lane;
		uint32_t nb = 0;
		const uint8_t* sp = R;
		uint8_t* cp = O;
		if (m < n) {
			const IvEmit r = recs[m];
			uint8_t* dp = O + r.out;
			if (r.close_off != kNoClose && fits(O + r.close_off, 4)) put_be32(O + r.close_off, r.close_len);
			if (r.gap_len) {
				if (fits(dp, 9)) {
					dp[0] = 2;
					put_be32(dp + 1, r.gap_x);
					put_be32(dp + 5, r.gap_len);
				}
				sp = R + r.gap_x;
				cp = dp + 9;
				nb = r.gap_len;
				if ((uint64_t)r.gap_x + r.gap_len > ref_len) {
					stray = true;
					nb = 0;
				}
				dp += 9 + r.gap_len;
			}
			// (the length field is the closing record's)
			if (r.head && fits(dp, 13)) {
				dp[0] = 1;
				put_be32(dp + 1, r.vsrc);
				put_be32(dp + 5, r.gap_x + r.gap_len);
			}
		}
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
	if (stray) a.status[i] = 12;
}
