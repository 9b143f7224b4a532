// dg_update_dev.hip — the in-place update kernel (dg_update_plan_run), built
// as the stand-alone gfx950 code object lib/dg_update.hsaco.
//
// One 256-thread block per stream turns the stream's buffer, which holds R,
// into V by replaying an in-place delta in it (src/c/apply.c:253-284).  The
// buffer is the only copy of R, so nothing is stored before the whole stream
// has been validated (the reference parses the whole stream, encoding.c:
// 111-178, and checks the source CRC, main.c:341-356, before it applies):
//
//   A  read only: header, capacity, every window of the command chain parsed
//      and every command's bounds checked (dec_window, dg_decode_dev.h, which
//      decode_kernel calls too), then R's CRC-64/XZ over the buffer.  One block-
//      uniform status; nonzero ends the block with the buffer untouched.
//   B  [ref_len, bsz) zeroed (apply.c:276-278), then the stream is applied
//      window by window as decode_kernel applies an in-place stream: order-
//      free windows flat over the four waves (a COPY with src == dst neither
//      reads nor writes), the others in conflict-free groups.  Phase A leaves
//      every window's command offsets in the plan's memory (2 bytes per
//      command), so phase B loads a window and its list instead of parsing
//      again; a stream whose lists do not fit is parsed again.
//   C  the CRC-64/XZ of [0, version_size) against the header.
//
// The phases are separated by block barriers that order global memory
// (block_sync_global).  Stores are byte-exact: none falls outside
// [buf, buf + bsz).  Loads of the delta window and of the CRC rows are whole
// aligned 16-byte (8-byte) words that hold at least one byte of the stream's
// own region, as in decode_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_decode_dev.h"
#include "dg_update_dev.h"

using namespace dg;
using namespace dgup;

namespace {

static_assert(kUpBlock == kDecBlock, "the window step is written for decode's block");

// CRC-64/XZ of [s0, s0 + len) by the whole block, the value as the header
// stores it (big-endian u64 of the finalised register), on every thread.
// 16 KiB segments, segment j on wave j % 4 folding Horner-wise, wave 0
// combining (decode_kernel's step 7 for one span).  ct: tables in LDS.
__device__ uint64_t up_span_crc(const DecCrc& ct, const uint64_t* tables, uintptr_t s0, uint64_t len, uint64_t* cpart,
                                uint32_t* clast, uint64_t* res) {
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	const uint64_t* Lv = tables + 8 * 256;
	const uint64_t* KF = Lv + kCrcLevels * kCrcNibTabWords;
	// crc_seg_rows inverts the span's first 8 bytes (init = ~0) inside segment 0
	// only.  The segments are tiled back from the span's aligned-up end, so a
	// span that starts at an unaligned address and whose padded length is 16
	// bytes more than whole segments has fewer than 16 of its bytes in segment
	// 0, and of its first 8 some may lie in segment 1 (buffers at any buf_off
	// reach this; a 64 KiB buffer at offset 11 does).  Such a span is folded
	// without its last 16 bytes, which moves the tiling to the span's aligned
	// start, and lane 0 steps the register over those 16 bytes.
	const uint64_t full = len;
	if (len >= 8) {
		const uintptr_t a0 = s0 & ~(uintptr_t)15, a1 = (s0 + len + 15) & ~(uintptr_t)15;
		if (s0 != a0 && a1 - a0 > kDecCrcSeg && (a1 - a0) % kDecCrcSeg == 16) len -= 16;
	}
	const uint32_t nseg = len >= 8 ? crc_nseg(s0, len, kDecCrcSeg) : 0u;
	uint64_t acc = 0;
	uint32_t last = ~0u;
	for (uint32_t j = wave; j < nseg; j += kDecWaves) {
		const uint64_t c = dec_seg_crc(ct, s0, len, nseg, j);
		acc = (last != ~0u ? mul_nib(acc, ct.TK) : 0ull) ^ c;   // TK: x^(8 * 64 KiB) = 4 segments
		last = j;
	}
	if (lane == 0) {
		cpart[wave] = acc;
		clast[wave] = last;
	}
	__syncthreads();
	if (wave == 0) {
		uint64_t v = 0;
		if (lane < kDecWaves && clast[lane] != ~0u) {
			const uint32_t k = nseg - 1 - clast[lane];   // 0..3 segments after its last
			v = cpart[lane];
			if (k)
				v = mul_nib(v, k == 1 ? Lv + 4 * kCrcNibTabWords      // x^(8 * 16 KiB)
				               : k == 2 ? Lv + 5 * kCrcNibTabWords    // x^(8 * 32 KiB)
				                        : KF + kCrcFinX48K * kCrcNibTabWords);
		}
		const uint64_t raw = wave_xor64(v);
		if (lane == 0) {
			uint64_t c;
			if (len < 8) {
				const uint8_t* d = reinterpret_cast<const uint8_t*>(s0);
				c = ~0ULL;
				for (uint64_t k = 0; k < len; ++k) c = tables[(uint8_t)(c ^ d[k])] ^ (c >> 8);
			} else {
				c = raw;
				const uintptr_t end = s0 + len;
				const uint32_t t = (uint32_t)(((end + 15) & ~(uintptr_t)15) - end);
				if (t) c = mul_nib(c, KF + (1 + t) * kCrcNibTabWords);   // undo the trailing pad
				const uint8_t* d = reinterpret_cast<const uint8_t*>(s0);
				for (uint64_t k = len; k < full; ++k) c = tables[(uint8_t)(c ^ d[k])] ^ (c >> 8);
			}
			*res = ~c;
		}
	}
	__syncthreads();
	return *res;
}

// a window's record in the plan's memory: 16 bytes (next_pos, cnt, flags), then cnt u16 offsets, padded to 16
__device__ __forceinline__ uint64_t up_rec_bytes(uint32_t cnt) { return 16 + ((2ull * cnt + 15) & ~15ull); }
constexpr uint32_t kUpRecDone = 1, kUpRecFree = 2;

__device__ __forceinline__ uint64_t be64(const uint8_t* p) {
	uint64_t h = 0;
	for (int k = 0; k < 8; ++k) h = (h << 8) | p[k];
	return h;
}

}  // namespace

// profiling build only (make update_prof): per-phase cycles of every block,
// summed into UpArgs::prof
#ifdef DG_UPDATE_PROF
#define UPROF_T(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define UPROF_ADD(i, t0) (uprof[(i)] += __builtin_amdgcn_s_memtime() - (t0))
#else
#define UPROF_T(v) ((void)0)
#define UPROF_ADD(i, t0) ((void)0)
#endif

extern "C" __global__ __launch_bounds__(kUpBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void dg_update_kernel(
    UpArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x, wave = tid >> 6;
	__shared__ DecLdsMem M;
	__shared__ uint64_t cpart[kDecWaves];
	__shared__ uint32_t clast[kDecWaves];
	__shared__ uint64_t cres;
	const DecLds L = dec_lds(M);

#ifdef DG_UPDATE_PROF
	uint64_t uprof[kUpProfN] = {};
	const uint64_t t_start = __builtin_amdgcn_s_memtime();
	auto prof_flush = [&]() {
		uprof[UP_TOTAL] = __builtin_amdgcn_s_memtime() - t_start;
		uprof[UP_BLOCKS] = 1;
		if (tid == 0 && a.prof)
			for (int k = 0; k < kUpProfN; ++k) atomicAdd(&a.prof[k], (unsigned long long)uprof[k]);
	};
#endif
	const UpDesc dd = a.descs[i];
	uint8_t* O = a.buf + dd.buf_off;
	const uint64_t rl = dd.ref_len;
	uint64_t doff = dd.delta_off, dl = dd.delta_len;
	int32_t st = a.delta_status ? a.delta_status[i] : 0;   // an earlier stage's failure is passed on
	if (!st && a.delta_offsets) {
		doff = a.delta_offsets[i];
		dl = a.delta_offsets[i + 1] - doff;
		if (dl > dd.delta_len) st = 7;   // longer than the plan allowed for
	}
	const uint8_t* D = a.delta + doff;
	// phase A's command lists for phase B (nullptr or too small: phase B parses again)
	uint8_t* SC = a.scratch ? a.scratch + a.scratch_off[i] : nullptr;
	const uint64_t sc_cap = a.scratch ? a.scratch_off[i + 1] - a.scratch_off[i] : 0;
	uint64_t sc_used = 0;
	uint32_t sc_wins = 0;
	bool cached = SC != nullptr;

	// ── A. validate: nothing is stored before the status is known ──
	uint64_t vsize = 0;
	bool inplace = false;
	if (!st && bad_magic(D, dl)) st = 8;
	if (!st) {
		inplace = D[4] & 1;
		vsize = be32(D + 5);
	}
	const uint64_t bsz = max(rl, vsize);
	if (!st && bsz > dd.buf_cap) st = 7;
	UPROF_T(ta0);
	if (!st) {
		// a standard delta is checked as decode checks it: it is malformed or
		// unsupported, never applied
		const uint64_t lim_dst = inplace ? bsz : vsize, lim_src = inplace ? bsz : rl;
		uint64_t pos = 25;
		bool done = false;
		while (!done && !st) {
			if (pos >= dl) break;   // missing END: end of input (as the reference's loop)
			const DecWin w = dec_window(L, D, dl, pos, inplace, lim_dst, lim_src);
			if (w.bad) st = 8;
			if (!st && inplace && cached) {
				const uint64_t rec = up_rec_bytes(w.cnt);
				if (sc_used + rec <= sc_cap) {
					if (tid == 0)
						*reinterpret_cast<uint4*>(SC + sc_used) =
						    make_uint4((uint32_t)w.next_pos, (uint32_t)(w.next_pos >> 32), w.cnt,
						               (w.done ? kUpRecDone : 0u) | (w.free_win ? kUpRecFree : 0u));
					uint16_t* q = reinterpret_cast<uint16_t*>(SC + sc_used + 16);
					for (uint32_t k = tid; k < w.cnt; k += kUpBlock) q[k] = M.cmds[k];
					sc_used += rec;
					++sc_wins;
				} else {
					cached = false;
				}
			}
			done = w.done;
			pos = w.next_pos;
			__syncthreads();   // the window's LDS is the next window's
		}
	}
	UPROF_ADD(UP_A_PARSE, ta0);
	if (!st && !inplace) st = 2;
	UPROF_T(ta1);
	if (!st && a.crc_check) {
		DecodeArgs da{};
		da.tables = a.tables;
		const DecCrc ct = dec_crc_tables(M.NX, da);
		__syncthreads();
		if (up_span_crc(ct, a.tables, (uintptr_t)O, rl, cpart, clast, &cres) != be64(D + 9)) st = 9;
		__syncthreads();   // the tables' LDS is the parse's next
	}
	UPROF_ADD(UP_A_CRC, ta1);
	if (st) {
		if (tid == 0) {
			a.status[i] = st;
			a.out_len[i] = 0;
		}
#ifdef DG_UPDATE_PROF
		prof_flush();
#endif
		return;
	}

	// ── B. apply ──
	UPROF_T(tb0);
	if (bsz > rl) {   // zeros up to bsz (apply.c:276-278): byte edges, whole 16-byte words between
		uint8_t* z = O + rl;
		const uint64_t zn = bsz - rl;
		const uint64_t head = min(zn, (uint64_t)((16u - (uint32_t)((uintptr_t)z & 15u)) & 15u));
		const uint64_t nw = (zn - head) / 16;
		for (uint64_t k = tid; k < head; k += kUpBlock) z[k] = 0;
		for (uint64_t q = tid; q < nw; q += kUpBlock) reinterpret_cast<uint4*>(z + head)[q] = make_uint4(0, 0, 0, 0);
		for (uint64_t k = head + 16 * nw + tid; k < zn; k += kUpBlock) z[k] = 0;
	}
	block_sync_global();   // the zeros (and phase A's lists) land before any command reads or writes them
	UPROF_ADD(UP_B_ZERO, tb0);
	{
		uint64_t pos = 25, used = 0;
		uint32_t r = 0;
		bool done = false;
		while (true) {
			UPROF_T(tb1);
			uint32_t cnt, shf;
			uint64_t next_pos;
			bool free_win;
			if (cached) {   // the window and the list phase A left for it
				if (r == sc_wins) break;
				const uint4 h = *reinterpret_cast<const uint4*>(SC + used);
				cnt = umin32(uni(h.z), kDecMaxCmds);
				free_win = uni(h.w) & kUpRecFree;
				next_pos = ((uint64_t)uni(h.y) << 32) | uni(h.x);
				shf = dec_load_window(M.win, D, dl, pos);
				const uint16_t* q = reinterpret_cast<const uint16_t*>(SC + used + 16);
				for (uint32_t k = tid; k < cnt; k += kUpBlock) M.cmds[k] = q[k];
				__syncthreads();
				used += up_rec_bytes(cnt);
				++r;
			} else {
				if (done || pos >= dl) break;
				const DecWin w = dec_window(L, D, dl, pos, true, bsz, bsz);
				if (w.bad) break;   // (phase A accepted these bytes: not reached)
				cnt = w.cnt;
				shf = w.shf;
				next_pos = w.next_pos;
				free_win = w.free_win;
				done = w.done;
			}
			UPROF_ADD(UP_B_PARSE, tb1);
			UPROF_T(tb2);
			const uint8_t* wp = M.win + shf;
			if (free_win) {
				const uint32_t nb = (cnt + 63) / 64;
				for (uint32_t b = wave; b < nb; b += kDecWaves) {
					const DecCmd c = dec_cmd(wp, M.cmds, 64 * b, cnt, pos);
					dec_flat_batch(c, true, O, O, D, L.xs);
				}
			} else {
				dec_grouped_window(wp, M.cmds, cnt, pos, true, O, O, D, L.grp);
			}
			block_sync_global();   // the window's stores complete before the next window
			UPROF_ADD(UP_B_APPLY, tb2);
			pos = next_pos;
		}
	}

	// ── C. the result's CRC against the header (main.c:376-385) ──
	int32_t cst = 0;
	UPROF_T(tc0);
	if (a.crc_check) {
		block_sync_global();   // every wave's stores before any CRC read
		DecodeArgs da{};
		da.tables = a.tables;
		const DecCrc ct = dec_crc_tables(M.NX, da);
		__syncthreads();
		if (up_span_crc(ct, a.tables, (uintptr_t)O, vsize, cpart, clast, &cres) != be64(D + 17)) cst = 10;
	}
	UPROF_ADD(UP_C_CRC, tc0);
	if (tid == 0) {
		a.status[i] = cst;
		a.out_len[i] = vsize;
	}
#ifdef DG_UPDATE_PROF
	prof_flush();
#endif
}
