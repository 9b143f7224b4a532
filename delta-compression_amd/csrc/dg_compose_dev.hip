// dg_compose_dev.hip — composition of a batch of delta pairs on the device:
// A_i = delta(R -> V1) and B_i = delta(V1 -> V2) give C_i = delta(R -> V2),
// byte for byte what dg_compose (dg_compose.cpp) produces: the normal form of
// include/delta_gpu.h.
//
// Built on its own as lib/dg_compose.hsaco and loaded by dg_compose_host.cpp.
// Two kernels, with the library's size scan between them:
//
//   dg_compose_map_kernel    one wave per pair.  Parses stream A through a
//     1 KiB LDS window (dg_parse_chain.h; all lanes decode the headers),
//     checks every field and fills the tables over A's non-empty commands: V1
//     start, R source or payload offset, prefix counts of run heads and of ADD
//     run heads, prefix of ADD bytes.  A run head is a command that does not
//     merge with its predecessor.  Then parses B, one lane per command: a COPY
//     finds its range of A with two binary searches, and the prefix tables
//     give its run count, its bytes and the kind and ends of its first and
//     last run without a walk.  Whether a command's first run continues the
//     run open before it, and which run a command closes, are "nearest earlier
//     lane" lookups (a prefix max over lane numbers), carried across the
//     64-command tiles.  Writes one emit record per command of B and the
//     pair's size.
//   dg_compose_emit_kernel   one 256-thread block per pair writes the header,
//     the runs and the END byte: one lane per command of B walks its pieces.
//     A run's length field is written by whoever closes the run: the same lane
//     for a run that ends inside its command, else the record of the command
//     that begins the next run, else the pair's last close.
//
// No byte outside [0, len) of either stream is read and none outside the
// pair's output range is written: every multi-byte load is issued only where
// it fits, the rest byte by byte, and every store is checked against the
// pair's end (a miss is DG_ERR_INTERNAL, never a stray byte).
#include <hip/hip_runtime.h>

#include "dg_compose_dev.h"
#include "dg_devutil.h"
#include "dg_parse_chain.h"
#include "dg_stream_dev.h"

using namespace dg;
using namespace dgcp;

namespace {

struct ATab {
	uint32_t *v, *ref, *H, *HA, *AP;
};
__device__ __forceinline__ ATab a_tab(uint8_t* base, uint32_t CA) {
	ATab t;
	uint32_t* w = reinterpret_cast<uint32_t*>(base);
	t.v = w; w += CA + 1;
	t.ref = w; w += CA + 1;
	t.H = w; w += CA + 1;
	t.HA = w; w += CA + 1;
	t.AP = w;
	return t;
}
__device__ __forceinline__ CpRec* b_recs(uint8_t* base, uint32_t CA) {
	return reinterpret_cast<CpRec*>(base + 4ull * kAWords * ((uint64_t)CA + 1));
}

// first index in [lo, hi) with t[index] > x (upper) or >= x (lower); hi when none
__device__ __forceinline__ uint32_t upper(const uint32_t* t, uint32_t lo, uint32_t hi, uint32_t x) {
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (t[mid] <= x) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}
__device__ __forceinline__ uint32_t lower(const uint32_t* t, uint32_t lo, uint32_t hi, uint32_t x) {
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (t[mid] < x) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void dg_compose_map_kernel(CpArgs a) {
	__shared__ __attribute__((aligned(16))) uint32_t lds[(kChainLdsBytes + 3) / 4];
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t lane = lane_id();
	const CpDesc dd = a.descs[i];
	CpRes res{};
	res.close_off = kNoClose;
	auto finish = [&](int32_t st, uint64_t size) {
		if (lane == 0) {
			a.status[i] = st;
			a.sizes[i] = st ? 0 : size;
			a.res[i] = res;
		}
	};
	if (a.a_status && a.a_status[i] != 0) return finish(a.a_status[i], 0);
	if (a.b_status && a.b_status[i] != 0) return finish(a.b_status[i], 0);
	const uint64_t a_off = a.a_offsets ? a.a_offsets[i] : dd.a_off;
	const uint64_t a_len = a.a_offsets ? a.a_offsets[i + 1] - a_off : dd.a_cap;
	const uint64_t b_off = a.b_offsets ? a.b_offsets[i] : dd.b_off;
	const uint64_t b_len = a.b_offsets ? a.b_offsets[i + 1] - b_off : dd.b_cap;
	// (a stream of 4 GiB or more cannot be parsed with 32-bit offsets; its
	// capacity is below that, so it is longer than its capacity)
	if (a_len >= (1ull << 32) || b_len >= (1ull << 32)) return finish(7, 0);
	const bool over_cap = a_len > dd.a_cap || b_len > dd.b_cap;
	const uint8_t* SA = a.a + a_off;
	const uint8_t* SB = a.b + b_off;
	const uint32_t al = (uint32_t)a_len, bl = (uint32_t)b_len;
	res.a_off = a_off;
	res.b_off = b_off;
	const uint32_t CA = dd.max_a, CB = dd.max_b;
	const ATab t = a_tab(a.work + dd.work_off, CA);
	CpRec* recs = b_recs(a.work + dd.work_off, CA);

	const ChainLds cl = chain_lds(lds);
	const uint8_t* win = cl.win;
	const uint16_t* cmds = cl.cmds;
	bool bad = false, unsup = false, full = false;

	// ── stream A: validate, fill the tables ──
	uint32_t vsA = 0, nA = 0;
	if (bad_magic(SA, al)) {
		bad = true;
	} else {
		if (SA[4] & 1) unsup = true;
		vsA = be32(SA + 5);
		uint32_t pos = 25, heads = 0, aheads = 0;
		uint64_t wpos = 0, addb = 0;
		bool c_has = false, ended = false;   // the last non-empty command so far: its kind and where its COPY ends in R
		uint32_t c_kind = 0;
		uint64_t c_end = 0;
		while (!ended && !bad) {
			if (pos >= al) break;   // the stream ends without an END byte
			const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, SA, al, pos), pos, al);
			for (uint32_t b0 = 0; b0 < cw.cnt; b0 += 64) {
				const bool mine = b0 + lane < cw.cnt;
				const Hdr h = decode_hdr(win, cmds, b0 + lane, mine);
				const bool is_copy = mine && h.kind == 1;
				uint64_t tot_len, tot_add;
				const uint64_t pre_len = wave_excl_scan64(h.len, &tot_len);
				// commands placed sequentially: dst = the sum of the earlier lengths
				if (__ballot(mine && (uint64_t)h.dst != wpos + pre_len)) unsup = true;
				// no reference of this format holds such a COPY
				const uint64_t my_end = (uint64_t)h.src + h.len;
				if (__ballot(is_copy && my_end > (1ull << 32))) bad = true;
				const bool ne = mine && h.len > 0;
				const bool ne_add = ne && h.kind == 2;
				const uint32_t pl = prev_set(ne, lane);
				// (every lane takes part in a shuffle: select afterwards)
				const uint32_t sh_kind = shfl32(h.kind, pl - 1);
				const uint64_t sh_end = shfl64(my_end, pl - 1);
				const uint32_t p_kind = pl ? sh_kind : c_kind;
				const uint64_t p_end = pl ? sh_end : c_end;
				const bool p_has = pl || c_has;
				const bool merge = ne && p_has && p_kind == h.kind && (h.kind == 2 || p_end == h.src);
				const bool head = ne && !merge;
				const uint32_t inc_ne = wave_incl_scan(ne ? 1u : 0u);
				const uint32_t inc_h = wave_incl_scan(head ? 1u : 0u);
				const uint32_t inc_ha = wave_incl_scan(head && h.kind == 2 ? 1u : 0u);
				const uint64_t pre_add = wave_excl_scan64(ne_add ? h.len : 0u, &tot_add);
				const uint32_t cnt_ne = rdlane(inc_ne, 63);
				if (nA + cnt_ne > CA) full = true;
				if (!bad && !unsup && !full && ne) {
					const uint32_t k = nA + inc_ne - 1;
					t.v[k] = h.dst;
					t.ref[k] = h.kind == 1 ? h.src : pos + h.cx + 9;
					t.H[k] = heads + inc_h;
					t.HA[k] = aheads + inc_ha;
					t.AP[k] = (uint32_t)(addb + pre_add);
				}
				const uint32_t ls = last_set(ne);
				if (ls) {
					c_has = true;
					c_kind = shfl32(h.kind, ls - 1);
					c_end = shfl64(my_end, ls - 1);
				}
				if (!full) nA += cnt_ne;
				heads += rdlane(inc_h, 63);
				aheads += rdlane(inc_ha, 63);
				wpos += tot_len;
				addb += tot_add;
			}
			if (cw.term == kChBad) bad = true;
			if (cw.term == kChEnd) ended = true;
			pos = cw.next_pos;
			wave_sync();   // the window is rewritten next
		}
		if (wpos != vsA) unsup = true;
		if (!bad && !unsup && !full && lane == 0) {   // the entry that closes the tiling
			t.v[nA] = vsA;
			t.AP[nA] = (uint32_t)addb;
		}
	}
	const bool tables = !bad && !unsup && !full;
	wave_sync();

	// ── stream B: validate, one emit record per non-empty command ──
	uint32_t vsB = 0, nB = 0;
	uint64_t osize = 0;   // command bytes of the output so far
	bool huge = false;
	bool o_has = false;   // the run open after the commands so far: its length field and where it starts in V2
	uint32_t o_lf = 0, o_v = 0;
	if (bad_magic(SB, bl)) {
		bad = true;
	} else {
		if (SB[4] & 1) unsup = true;
		vsB = be32(SB + 5);
		uint32_t pos = 25;
		uint64_t wpos = 0;
		bool c_has = false, ended = false;   // the last non-empty command so far: its last run's kind and end in R
		uint32_t c_lk = 0;
		uint64_t c_rend = 0;
		while (!ended && !bad) {
			if (pos >= bl) break;
			const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, SB, bl, pos), pos, bl);
			for (uint32_t b0 = 0; b0 < cw.cnt; b0 += 64) {
				const bool mine = b0 + lane < cw.cnt;
				const Hdr h = decode_hdr(win, cmds, b0 + lane, mine);
				const bool is_copy = mine && h.kind == 1;
				uint64_t tot_len, tot_bytes;
				const uint64_t pre_len = wave_excl_scan64(h.len, &tot_len);
				if (__ballot(mine && (uint64_t)h.dst != wpos + pre_len)) unsup = true;
				// a COPY of B reads V1
				if (__ballot(is_copy && (uint64_t)h.src + h.len > vsA)) bad = true;
				const bool ne = mine && h.len > 0;
				const uint32_t inc_ne = wave_incl_scan(ne ? 1u : 0u);
				const uint32_t cnt_ne = rdlane(inc_ne, 63);
				if (nB + cnt_ne > CB) full = true;
				wpos += tot_len;
				if (!tables || bad || unsup || full) continue;   // validation goes on; the status is decided

				// this command alone: kinds and ends of its first and last run, runs, bytes
				uint32_t fk = 2, lk = 2, runs = 1, j0 = 0, last_size = 0, last_v2 = 0, second_v2 = 0;
				uint64_t iso = 9ull + h.len, rstart = 0, rend = 0;
				if (ne && h.kind == 1) {
					const uint32_t s = h.src, e = h.src + h.len;
					j0 = upper(t.v, 0, nA, s) - 1;
					const uint32_t j1 = lower(t.v, 0, nA, e) - 1;
					const uint32_t v0 = t.v[j0], v1 = t.v[j1];
					const uint32_t ap0 = t.AP[j0], ap1 = t.AP[j1];
					fk = t.AP[j0 + 1] != ap0 ? 2u : 1u;
					lk = t.AP[j1 + 1] != ap1 ? 2u : 1u;
					const uint32_t h0 = t.H[j0], h1 = t.H[j1];
					runs = 1 + h1 - h0;
					const uint32_t aruns = (fk == 2 ? 1u : 0u) + t.HA[j1] - t.HA[j0];
					const uint32_t ap_s = ap0 + (fk == 2 ? s - v0 : 0u), ap_e = ap1 + (lk == 2 ? e - v1 : 0u);
					iso = 13ull * (runs - aruns) + 9ull * aruns + (ap_e - ap_s);
					rstart = (uint64_t)t.ref[j0] + (s - v0);
					rend = (uint64_t)t.ref[j1] + (e - v1);
					if (runs >= 2) {
						const uint32_t kl = lower(t.H, j0 + 1, j1 + 1, h1);   // the head of the last run
						last_v2 = h.dst + (t.v[kl] - s);
						last_size = lk == 1 ? 13u : 9u + (ap_e - t.AP[kl]);
						const uint32_t k2 = upper(t.H, j0 + 1, j1 + 1, h0);   // the head of the second run
						second_v2 = h.dst + (t.v[k2] - s);
					}
				}
				if (__ballot(ne && iso >= (1ull << 32))) huge = true;
				// does the first run continue the last run of the command before?
				const uint32_t pl = prev_set(ne, lane);
				const uint32_t sh_lk = shfl32(lk, pl - 1);
				const uint64_t sh_rend = shfl64(rend, pl - 1);
				const uint32_t p_lk = pl ? sh_lk : c_lk;
				const uint64_t p_rend = pl ? sh_rend : c_rend;
				const bool merge = ne && (pl || c_has) && p_lk == fk && (fk == 2 || p_rend == rstart);
				const uint32_t bytes = ne ? (uint32_t)iso - (merge ? (fk == 1 ? 13u : 9u) : 0u) : 0u;
				const uint32_t out_rel = (uint32_t)(osize + wave_excl_scan64(bytes, &tot_bytes));
				// the run this command leaves open, and the one it closes
				const bool setter = ne && (!merge || runs >= 2);
				const uint32_t my_lf = runs >= 2 ? out_rel + bytes - last_size + (lk == 1 ? 9u : 5u) : out_rel + (fk == 1 ? 9u : 5u);
				const uint32_t my_v = runs >= 2 ? last_v2 : h.dst;
				const uint32_t ps = prev_set(setter, lane);
				const uint32_t sh_lf = shfl32(my_lf, ps - 1);
				const uint32_t sh_v = shfl32(my_v, ps - 1);
				const uint32_t p_lf = ps ? sh_lf : o_lf;
				const uint32_t p_v = ps ? sh_v : o_v;
				const bool closes = setter && (ps || o_has);
				if (ne) {
					CpRec r;
					r.pos = pos + h.cx;
					r.out = out_rel;
					r.j0 = j0 | (merge ? 0u : kHeadBit);
					r.close_off = closes ? p_lf : kNoClose;
					r.close_len = (merge ? second_v2 : h.dst) - p_v;
					recs[nB + inc_ne - 1] = r;
				}
				const uint32_t ls = last_set(ne);
				if (ls) {
					c_has = true;
					c_lk = shfl32(lk, ls - 1);
					c_rend = shfl64(rend, ls - 1);
				}
				const uint32_t lo = last_set(setter);
				if (lo) {
					o_has = true;
					o_lf = shfl32(my_lf, lo - 1);
					o_v = shfl32(my_v, lo - 1);
				}
				nB += cnt_ne;
				osize += tot_bytes;
			}
			if (cw.term == kChBad) bad = true;
			if (cw.term == kChEnd) ended = true;
			pos = cw.next_pos;
			wave_sync();
		}
		if (wpos != vsB) unsup = true;
	}
	// ── the status, by kind of defect ──
	if (bad) return finish(8, 0);
	if (over_cap || full) return finish(7, 0);
	if (unsup) return finish(2, 0);
	if (!a.ignore_hash) {   // B must be a delta against A's output
		if (__ballot(lane < 8 && SA[17 + (lane & 7u)] != SB[9 + (lane & 7u)])) return finish(9, 0);
	}
	const uint64_t size = 25 + osize + 1;
	if (huge || size >= (1ull << 32)) return finish(3, 0);
	res.n_a = nA;
	res.n_b = nB;
	if (o_has) {
		res.close_off = o_lf;
		res.close_len = vsB - o_v;
	}
	finish(0, size);
}

extern "C" __global__ __launch_bounds__(256) void dg_compose_emit_kernel(CpArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	if (a.status[i] != 0) return;
	const uint64_t base = a.out_offsets[i], end = a.out_offsets[i + 1];
	if (end > a.out_cap) {
		if (tid == 0) a.status[i] = 7;
		return;
	}
	const CpRes res = a.res[i];
	const CpDesc dd = a.descs[i];
	const uint8_t* SA = a.a + res.a_off;
	const uint8_t* SB = a.b + res.b_off;
	const uint32_t body = (uint32_t)(end - base) - 26;   // the command bytes
	uint8_t* O = a.out + base + 25;
	const ATab t = a_tab(a.work + dd.work_off, dd.max_a);
	const CpRec* recs = b_recs(a.work + dd.work_off, dd.max_a);
	const uint32_t nA = res.n_a, nB = res.n_b;
	bool stray = false;   // a store that would leave the pair's range: a bug, never issued
	auto fits = [&](const uint8_t* p, uint32_t n) {
		const uint64_t at = (uint64_t)(p - O);
		const bool ok = at + n <= body;
		if (!ok) stray = true;
		return ok;
	};
	// header: flag byte 0, B's version size, A's source CRC, B's destination CRC
	if (tid < 25) O[(int)tid - 25] = tid < 4 ? SA[tid] : (tid == 4 ? (uint8_t)0 : (tid < 9 ? SB[tid] : (tid < 17 ? SA[tid] : SB[tid])));
	if (tid == 0) {
		O[body] = 0;
		if (res.close_off != kNoClose && fits(O + res.close_off, 4)) put_be32(O + res.close_off, res.close_len);
	}
	for (uint32_t c0 = 64 * wave; c0 < nB; c0 += 256) {
		const uint32_t m = c0 + lane;
		bool more = m < nB;
		uint32_t kind = 0, s = 0, x = 0, e = 0, j = 0, vcur = 0, len = 0, run_v = 0;
		bool head = false;
		uint8_t* dp = O;
		uint8_t* lenptr = nullptr;
		const uint8_t* cmd = SB;
		if (more) {
			const CpRec r = recs[m];
			cmd = SB + r.pos;
			kind = cmd[0];
			if (kind == 1) {
				s = be32(cmd + 1);
				vcur = be32(cmd + 5);
				len = be32(cmd + 9);
			} else {
				vcur = be32(cmd + 1);
				len = be32(cmd + 5);
			}
			x = s;
			e = s + len;
			head = (r.j0 & kHeadBit) != 0;
			j = r.j0 & ~kHeadBit;
			dp = O + r.out;
			if (r.close_off != kNoClose && fits(O + r.close_off, 4)) put_be32(O + r.close_off, r.close_len);
		}
		while (__ballot(more)) {
			// one piece per lane and step: its header if it begins a run, its payload span
			uint32_t nb = 0;
			const uint8_t* sp = SB;
			uint8_t* cp = O;
			if (more && kind == 2) {
				if (head && fits(dp, 9)) {
					dp[0] = 2;
					put_be32(dp + 1, vcur);
				}
				if (head) dp += 9;
				sp = cmd + 9;
				cp = dp;
				nb = len;
				more = false;
			} else if (more) {
				const uint32_t vj = t.v[j], vn = t.v[j + 1];
				const bool jadd = t.AP[j + 1] != t.AP[j];
				const uint32_t y = umin32(e, vn);
				const bool h = x == s ? head : t.H[j] != t.H[j - 1];
				if (h) {
					if (lenptr && fits(lenptr, 4)) put_be32(lenptr, vcur - run_v);
					run_v = vcur;
					if (jadd) {
						if (fits(dp, 9)) {
							dp[0] = 2;
							put_be32(dp + 1, vcur);
						}
						lenptr = dp + 5;
						dp += 9;
					} else {
						if (fits(dp, 13)) {
							dp[0] = 1;
							put_be32(dp + 1, t.ref[j] + (x - vj));
							put_be32(dp + 5, vcur);
						}
						lenptr = dp + 9;
						dp += 13;
					}
				}
				if (jadd) {
					sp = SA + t.ref[j] + (x - vj);
					cp = dp;
					nb = y - x;
					dp += nb;
				}
				vcur += y - x;
				x = y;
				++j;
				more = x < e && j < nA && y > vj;
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
	}
	if (stray) a.status[i] = 12;
}
