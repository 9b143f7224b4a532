// dg_read_walk_dev.h — the device functions the read kernels
// (dg_read_dev.hip), the chunked index pass (dg_index_dev.hip) and the lineage
// walk (dg_lineage_dev.hip) share: the clip of a command to a range, the entry
// lookup in a stream's index, the tiling summary of a window's commands, and
// the index walk both index passes run.  Device only; the layouts are
// dg_read_dev.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_decode_dev.h"
#include "dg_read_dev.h"

namespace dgrd {

using namespace dg;

static_assert(kRdBlock == kDecBlock, "the window step is written for decode's block");
static_assert(sizeof(RdHead) == 32 && sizeof(RdEnt) == 8, "index layout");
constexpr uint32_t kRdBatches = kDecMaxCmds / 64;

// the command's intersection with V[lo, hi), its destination relative to lo
__device__ __forceinline__ void rd_clip(DecCmd& c, uint64_t lo, uint64_t hi) {
	if (!c.mine) return;
	const uint64_t s = max(c.dst, lo), e = min(c.dst + c.len, hi);
	if (e > s) {
		c.src += s - c.dst;
		c.len = e - s;
		c.dst = s - lo;
	} else {
		c.len = 0;
		c.dst = 0;
	}
}

// dst of the command at window offset cx
template <typename WP>
__device__ __forceinline__ uint32_t rd_dst_at(WP w, uint32_t cx) {
	uint32_t h[4];
	win16(w + cx, h);
	return (h[0] & 0xFFu) == 1u ? hdr_be32(h, 1) : hdr_be32(h, 0);
}

// Where a sequential stream of dl bytes is entered for V[lo, ...): the command
// of the last of the n_ent entries whose dst is <= lo (the commands before it
// end at or before its dst), else the stream's first command.  What a stale
// index holds is not trusted: an offset outside [25, dl) is the first command's.
__device__ __forceinline__ uint32_t rd_entry_pos(const RdEnt* E, uint32_t n_ent, uint64_t lo, uint32_t dl) {
	uint32_t x = 0, y = n_ent;
	while (x < y) {
		const uint32_t mid = (x + y) >> 1;
		if (E[mid].dst <= lo) x = mid + 1;
		else y = mid;
	}
	if (x > 0) {
		const uint32_t p = E[x - 1].spos;
		if (p >= 25 && p < dl) return p;
	}
	return 25;
}

// ── the tiling summary ──
//
// Do a window's commands tile a piece of V, each starting where the one before
// it ends?  Per batch of 64 commands a wave leaves, of the batch's own
// commands (a prefix of the batch: the caller's predicate), the first dst, the
// last end, and their count with whether one of them breaks the run; after a
// block barrier every thread folds the batches in order into an RdTiling.
struct RdTileLds {
	uint32_t first[kRdBatches], end[kRdBatches];
	uint32_t own[kRdBatches];   // 2 * the count + (a break inside)
};
struct RdTiling {   // of the own commands folded so far
	bool any = false, brk = false;   // there is one; one does not start where the one before it ends
	uint32_t first = 0, end = 0;     // dst of the first, dst + len of the last
};

// batch b of the window, by one wave (every lane takes part); own: a prefix of the batch's commands
__device__ __forceinline__ void rd_tile_batch(RdTileLds& T, uint32_t b, const DecCmd& c, bool own) {
	const uint32_t lane = lane_id();
	const uint32_t dst32 = (uint32_t)c.dst, end32 = (uint32_t)(c.dst + c.len);   // <= version_size: checked
	const uint32_t prev_end = wave_shr1z(end32);
	const uint64_t bm = __ballot(own && lane > 0 && dst32 != prev_end);
	const uint32_t no = uni((uint32_t)__builtin_popcountll(__ballot(own)));
	const uint32_t f = rdlane(dst32, 0), e = rdlane(end32, no ? no - 1 : 0);
	if (lane == 0) {
		T.first[b] = f;
		T.end[b] = e;
		T.own[b] = 2 * no + (bm ? 1u : 0u);
	}
}

// the window's nb batches after those t holds (the own commands are a prefix of the window's)
__device__ __forceinline__ void rd_tile_fold(const RdTileLds& T, uint32_t nb, RdTiling& t) {
	// (selects, no exit at the first batch without own commands: the LDS loads do not wait for one another)
	for (uint32_t b = 0; b < nb; ++b) {
		const uint32_t o = T.own[b], f = T.first[b], e = T.end[b];
		const bool has = o >= 2;
		t.brk |= has & (((o & 1) != 0) | (t.any & (f != t.end)));
		t.first = (has & !t.any) ? f : t.first;
		t.any |= has;
		t.end = has ? e : t.end;
	}
}

// ── the index walk ──
//
// Both index passes: from the command at pos, the real window step
// (dec_window, bounds checks included) until END, the stream's end or a
// command at or after cend has been seen.  The block writes exactly the index
// entries [klo, khi], and returns the tiling of the commands that start before
// cend.  The one-block pass is the walk of one chunk that spans the stream:
// pos 25, cend kRdNoEnd, entries [0, n_ent - 1].
constexpr uint64_t kRdNoEnd = ~0ull;
struct RdWalk {
	RdTiling t;
	bool failed = false;   // a command on the chain is malformed or out of bounds (nothing after it is written)
};
__device__ __forceinline__ RdWalk rd_index_walk(const DecLds& L, RdTileLds& T, const uint8_t* D, uint64_t dl, uint32_t vsize,
                                                uint64_t ref_len, RdEnt* E, uint64_t pos, uint64_t cend, uint32_t klo,
                                                uint32_t khi) {
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	const uint16_t* cmds = L.ch.cmds;
	RdWalk r;
	bool any = false;       // a command has been seen
	uint32_t prev_s = 0;    // the stream offset of the last one
	bool done = false, past = false;
	while (!done && !past && pos < dl) {   // (a missing END: end of input, as the reference's loop)
		const DecWin w = dec_window(L, D, dl, pos, false, vsize, ref_len);
		if (w.bad) {
			r.failed = true;
			return r;
		}
		const uint8_t* wp = L.ch.win + w.shf;
		const uint32_t nb = (w.cnt + 63) / 64;
		for (uint32_t b = wave; b < nb; b += kDecWaves) {
			const DecCmd c = dec_cmd(wp, cmds, 64 * b, w.cnt, pos);
			const uint32_t j = 64 * b + lane;
			const uint32_t sp = c.mine ? (uint32_t)pos + cmds[j] : 0u;
			rd_tile_batch(T, b, c, c.mine && sp < cend);   // it starts before cend (the window may run past it)
			// the entries this command is the first at or after: [k0, k1], the
			// strides after the previous command's up to its own.  Up to four
			// by its lane; more (after a long ADD payload) by the whole wave.
			const uint32_t dst32 = (uint32_t)c.dst;
			uint32_t k0 = 1, k1 = 0;
			if (c.mine) {
				k0 = j > 0 ? ((uint32_t)pos + cmds[j - 1]) / kRdStride + 1u : (any ? prev_s / kRdStride + 1u : klo);
				k1 = umin32(sp / kRdStride, khi);
			}
			const bool wide = c.mine && k1 >= k0 && k1 - k0 >= 4;
			if (c.mine && !wide)
				for (uint32_t q = k0; q <= k1; ++q) E[q] = RdEnt{sp, dst32};
			for (uint64_t m = __ballot(wide); m; m &= m - 1) {
				const uint32_t kk = ffs64(m);
				const RdEnt ent{rdlane(sp, kk), rdlane(dst32, kk)};
				const uint32_t e1 = rdlane(k1, kk);
				for (uint32_t q = rdlane(k0, kk) + lane; q <= e1; q += 64) E[q] = ent;
			}
		}
		__syncthreads();
		rd_tile_fold(T, nb, r.t);
		if (w.cnt) {
			prev_s = (uint32_t)pos + cmds[w.cnt - 1];
			any = true;
			past = prev_s >= cend;
		}
		done = w.done;
		pos = w.next_pos;
		__syncthreads();   // the window's LDS is the next window's
	}
	// the strides after the last command: nothing follows (END, the stream's end, or a chunk past them)
	const uint32_t q0 = any ? prev_s / kRdStride + 1u : klo;
	for (uint32_t q = q0 + tid; q <= khi; q += kRdBlock) E[q] = RdEnt{(uint32_t)dl, ~0u};
	return r;
}

}  // namespace dgrd
