// dg_lineage_dev.hip — the lineage-read kernel (dg_lineage_plan_run), built as
// the stand-alone gfx950 code object lib/dg_lineage.hsaco.
//
// A lineage read serves bytes [off, off + n) of a version that is k standard
// deltas away from bytes of the reference arena: stream -> parent[stream] ->
// ... -> a stream whose parent is the base.  Every stream is one of a read
// plan's, indexed by dg_read_index_kernel or the chunked pass (dg_read_dev.h).
//
//   dg_lineage_read_kernel  one 256-thread block per request.
//      1. The path: from the requested stream to its base, every stream's
//         head (status, the sequential flag, version_size) is read in the
//         order the contract gives, and what a walk needs of each level is
//         kept in LDS.  The first failure is the request's status.
//      2. The walk: a LIFO stack of work items (level, lo, hi, out_base, pos)
//         in LDS: bytes [lo, hi) of that level's version go to slot offset
//         out_base.  One step enters the top item's stream at pos, or through
//         the index at lo (the last entry whose dst is <= lo), and parses ONE
//         window (dec_window, dg_decode_dev.h).  The window then serves a run:
//         the items on top of the stack that are of the same level and start
//         inside the bytes the window's commands tile (children of one window
//         are neighbours one level down, so a run is usually all of them).
//         Per item every command is clipped to [lo, hi).  ADDs, and COPYs of a
//         level whose parent is the base, are pieces copied as they are: they
//         are staged in LDS and copied after the run, 64 per wave at a time
//         (dec_flat_batch, as the read kernel's).  COPYs of any other level
//         become child items one level down.  If the window ends before hi, a
//         continuation of the item is staged.  After the run its items leave
//         the stack, the continuations go where they were and the children on
//         top, the first in stream order uppermost.
//      Every stream on the path is sequential, so every output byte is written
//      exactly once by exactly one item: no zero fill, no ordering of stores.
//
// The stack never overflows and always makes progress: an item d deltas above
// the base can be finished with d - 1 free slots, so a step stages only as
// many children as leave d - 2 slots free above them, lets the continuation
// restart at the first command it did not push, and leaves the rest of the run
// on the stack ("Lineage reads on the device").
//
// Under a stale index the walk re-checks what it relies on: every command of
// a window starts where the one before it ends, an item starts inside the
// bytes its window tiles (or where a window of zero-length commands stands), a
// window moves the item forward in the version or in the stream, and
// dec_window re-checks every dst + len <= version_size and every COPY's
// src + len <= ref_len.  Any violation ends the request with DG_ERR_MALFORMED.  Stores go
// to [out_off, out_off + n) only: an item's range is clipped from its
// parent's, and its out_base moves with it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_decode_dev.h"
#include "dg_lineage_dev.h"
#include "dg_read_walk_dev.h"

using namespace dg;
using namespace dgrd;
using namespace dgln;

namespace {

static_assert(kLnBlock == kDecBlock, "the window step is written for decode's block");
static_assert(kLnItems >= kLnMaxDepth + 2, "the stack's progress argument");

// one stream of the request's path (level 0: the requested one)
struct LnLevel {
	uint64_t doff;      // where the stream was when it was indexed
	uint64_t ent_off;   // its index entries in the plan's index memory
	uint64_t ref_off;   // (the base's level only)
	uint32_t dl, vsize, ref_len, n_ent;
};

}  // namespace

extern "C" __global__ __launch_bounds__(kLnBlock) void dg_lineage_read_kernel(LnArgs a) {
	const uint32_t jq = blockIdx.x;
	if (jq >= a.n_req) return;
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	__shared__ DecLdsMem M;
	__shared__ RdTileLds T;   // per batch: where it starts and ends in V, whether its commands follow one another
	__shared__ uint32_t qkids[kRdBatches], qdir[kRdBatches];   // and an item's child COPYs and pieces in it
	__shared__ LnLevel path[kLnMaxDepth];
	__shared__ __attribute__((aligned(16))) uint4 stk[kLnItems];   // lo, hi, out_base, pos (0: enter through the index)
	__shared__ uint8_t stk_lv[kLnItems];
	__shared__ __attribute__((aligned(16))) uint4 stg[kLnItems];   // a run's children, in stream order
	__shared__ __attribute__((aligned(16))) uint4 cst[kLnRun];     // and its continuations
	const DecLds L = dec_lds(M);
	// the pieces a run copies as they are: (src, slot offset, len, kind), in NX behind the waves' flat-copy
	// scratch (the grouped apply's arrays, which this kernel never uses); dead while a window is parsed
	static_assert(kDecWaves * 2048 + 16 * kLnDirect <= 3 * kDecWin * 2, "the piece list fits NX");
	uint4* dls = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(M.NX) + kDecWaves * 2048);

	// ── 1. the path and the status (every thread, uniform; thread 0 keeps the levels) ──
	const RdReq rq = a.reqs[jq];
	int32_t st = 0;
	uint32_t depth = 0;    // deltas from the requested stream down to its base
	uint32_t vsize0 = 0;   // the requested version's size
	if (rq.stream >= a.n_streams || rq.reserved) st = 1;
	{
		uint32_t s = rq.stream;
		RdHead h{};
		if (!st) h = *reinterpret_cast<const RdHead*>(a.index + a.index_off[s]);
		while (!st) {
			if (depth >= kLnMaxDepth) st = 8;              // (create refuses such a forest)
			else if (h.status) st = h.status;              // a. the stream's index status
			else if (!(h.flags & kRdSeq)) st = 2;          // b. not sequential
			if (st) break;
			const RdStream sd = a.streams[s];
			const uint64_t ix0 = a.index_off[s], ix1 = a.index_off[s + 1];
			if (tid == 0) {
				LnLevel pl;
				pl.doff = h.doff;
				pl.ent_off = ix0 + sizeof(RdHead);
				pl.ref_off = sd.ref_off;
				pl.dl = h.dl;
				pl.vsize = h.vsize;
				pl.ref_len = (uint32_t)sd.ref_len;
				pl.n_ent = (uint32_t)min((uint64_t)h.n_ent, (ix1 - ix0 - sizeof(RdHead)) / sizeof(RdEnt));
				path[depth] = pl;
			}
			if (depth == 0) vsize0 = h.vsize;
			++depth;
			const uint32_t p = a.parent[s];
			if (p == kLnBase) break;
			if (p >= a.n_streams) {
				st = 8;   // (create refuses it)
				break;
			}
			const RdHead hp = *reinterpret_cast<const RdHead*>(a.index + a.index_off[p]);
			// c. the stated size of the parent's version (a parent that failed has none: its status is next)
			if (!hp.status && sd.ref_len != hp.vsize) st = 1;
			s = p;
			h = hp;
		}
	}
	// pread: what of [off, off + len) lies inside V
	const uint32_t n = st || rq.off >= vsize0 ? 0u : umin32(rq.len, vsize0 - rq.off);
	if (st || n == 0) {
		if (tid == 0) {
			a.status[jq] = st;
			a.out_len[jq] = 0;
		}
		return;
	}

	// ── 2. the walk ──
	uint8_t* O = a.out + rq.out_off;
	if (tid == 0) {
		stk[0] = make_uint4(rq.off, rq.off + n, 0u, 0u);
		stk_lv[0] = 0;
	}
	uint32_t sp = 1;
	bool bad = false;
	__syncthreads();
	while (sp && !bad) {
		// the top item's window
		const uint4 top = stk[sp - 1];
		const uint32_t lv = uni(stk_lv[sp - 1]);
		const uint32_t d = depth - lv;   // deltas from this level down to the base
		const bool on_base = d == 1;
		const LnLevel* pl = &path[lv];
		const uint32_t dl = uni(pl->dl), vs = uni(pl->vsize), rl = uni(pl->ref_len);
		const uint8_t* D = a.delta + uni64(pl->doff);
		const uint8_t* R = a.ref + (on_base ? uni64(pl->ref_off) : 0ull);
		uint32_t pos = uni(top.w);
		if (pos == 0) {
			const RdEnt* E = reinterpret_cast<const RdEnt*>(a.index + uni64(pl->ent_off));
			pos = rd_entry_pos(E, uni(pl->n_ent), uni(top.x), dl);
		}
		if (pos >= dl) {
			bad = true;   // the index accepted this stream and lo < hi <= its version_size: reached only with a stale index
			break;
		}
		const DecWin w = dec_window(L, D, dl, pos, false, vs, rl);
		if (w.bad || !w.free_win || w.cnt == 0) {
			bad = true;   // (stale index)
			break;
		}
		const uint8_t* wp = M.win + w.shf;
		const uint32_t nb = (w.cnt + 63) / 64;
		for (uint32_t b = wave; b < nb; b += kDecWaves) {
			const DecCmd c = dec_cmd(wp, M.cmds, 64 * b, w.cnt, (uint64_t)pos);
			rd_tile_batch(T, b, c, c.mine);
		}
		__syncthreads();
		RdTiling wt;
		rd_tile_fold(T, nb, wt);
		const uint32_t wfirst = wt.first, wend = wt.end;   // the window's commands tile [wfirst, wend)
		if (wt.brk) {
			bad = true;   // (stale index)
			break;
		}
		// the run: the items on top of the stack, of this level, that start inside the window
		const uint32_t sp0 = sp;
		uint32_t g = 0, nk = 0, nc = 0, nd = 0;   // items served; children, continuations and pieces staged
		// the staged pieces, 64 per wave at a time (after a block barrier: the list is complete)
		auto flush = [&](uint32_t cnt) {
			for (uint32_t b0 = 64 * wave; b0 < cnt; b0 += 64 * kDecWaves) {
				DecCmd c{false, 0, 0, 0, 0};
				c.mine = b0 + lane < cnt;
				if (c.mine) {
					const uint4 e = dls[b0 + lane];
					c.src = e.x;
					c.dst = e.y;
					c.len = e.z;
					c.kind = e.w;
				}
				dec_flat_batch(c, false, O, R, D, L.xs);
			}
			__syncthreads();   // the list is free again
		};
		while (g < kLnRun && g < sp0) {
			const uint32_t at = sp0 - 1 - g;
			const uint4 it = stk[at];
			const uint32_t lo = uni(it.x), hi = uni(it.y), ob = uni(it.z);
			const bool inside = lo >= wfirst && lo < wend;
			// a window of zero-length commands only, where the item starts, holds no byte of V: the top item
			// moves on in the stream (its continuation: the same range at the next window)
			const bool hollow = wfirst == wend && lo == wend;
			if (g == 0 && !inside && !hollow) {
				bad = true;   // the walk covers [lo, ...: (stale index)
				break;
			}
			if (g > 0 && (uni(stk_lv[at]) != lv || !inside)) break;
			// room for its continuation and children: d - 2 slots stay free above the children
			const uint32_t below = sp0 - (g + 1) + nc + nk;
			if (g > 0 && !on_base && below + (d - 2) + 2 > kLnItems) break;
			const bool complete = wend >= hi;
			if (!complete && (w.done || w.next_pos >= dl || w.next_pos <= pos)) {
				bad = true;   // (stale index)
				break;
			}
			// its child COPYs and the pieces copied as they are (ADDs; COPYs from R), per batch
			for (uint32_t b = wave; b < nb; b += kDecWaves) {
				uint64_t km = 0, dm = 0;
				if (T.end[b] > lo && T.first[b] < hi) {
					DecCmd c = dec_cmd(wp, M.cmds, 64 * b, w.cnt, (uint64_t)pos);
					rd_clip(c, lo, hi);
					const bool kid = c.mine && !on_base && c.kind == 1 && c.len != 0;
					km = __ballot(kid);
					dm = __ballot(c.mine && c.len != 0 && !kid);
				}
				if (lane == 0) {
					qkids[b] = (uint32_t)__builtin_popcountll(km);
					qdir[b] = (uint32_t)__builtin_popcountll(dm);
				}
			}
			__syncthreads();
			uint32_t kids = 0, ndir = 0;
			for (uint32_t b = 0; b < nb; ++b) {
				kids += qkids[b];
				ndir += qdir[b];
			}
			if (nd + ndir > kLnDirect) {   // (ndir <= kDecMaxCmds <= kLnDirect)
				flush(nd);
				nd = 0;
			}
			uint32_t cont = complete ? 0u : 1u, push = kids;
			if (kids && below + (d - 2) + cont + kids > kLnItems) {
				cont = 1;
				if (below + (d - 2) + 2 > kLnItems) {
					bad = true;   // (never: the top item sat on the stack with d - 1 slots free)
					break;
				}
				push = kLnItems - below - (d - 2) - 1;
			}
			const bool cut = push < kids;
			// the clipped commands: pieces and child COPYs staged
			for (uint32_t b = wave; b < nb; b += kDecWaves) {
				if (!(T.end[b] > lo && T.first[b] < hi)) continue;
				uint32_t kb = 0, db = 0;
				for (uint32_t q = 0; q < b; ++q) {
					kb += qkids[q];
					db += qdir[q];
				}
				DecCmd c = dec_cmd(wp, M.cmds, 64 * b, w.cnt, (uint64_t)pos);
				rd_clip(c, lo, hi);
				const bool kid = c.mine && !on_base && c.kind == 1 && c.len != 0;
				const bool direct = c.mine && c.len != 0 && !kid;
				const uint64_t km = __ballot(kid), dm = __ballot(direct);
				const uint64_t lt = mask_le(lane) >> 1;
				const uint32_t before = kb + (uint32_t)__builtin_popcountll(km & lt);   // children before this command
				// (a piece at or after the first command that was not pushed is the continuation's: length 0 here)
				if (direct)
					dls[nd + db + (uint32_t)__builtin_popcountll(dm & lt)] =
					    make_uint4((uint32_t)c.src, ob + (uint32_t)c.dst, before > push ? 0u : (uint32_t)c.len, c.kind);
				if (kid && before < push) stg[nk + before] = make_uint4((uint32_t)c.src, (uint32_t)(c.src + c.len), ob + (uint32_t)c.dst, 0u);
				if (kid && cut && before == push)
					// the continuation restarts at this command: its dst is lo + c.dst (children before it: dst > lo)
					cst[nc] = make_uint4(lo + (uint32_t)c.dst, hi, ob + (uint32_t)c.dst, pos + M.cmds[64 * b + lane]);
			}
			if (!cut && cont && tid == 0) cst[nc] = make_uint4(wend, hi, ob + (wend - lo), (uint32_t)w.next_pos);
			nk += push;
			nc += cont;
			nd += ndir;
			++g;
			__syncthreads();   // qkids is the next item's; the staged items
			if (cut) break;
		}
		if (bad) break;
		if (nd) flush(nd);
		// the served items leave the stack; their continuations go beneath their children, the first of each on top
		const uint32_t base = sp0 - g;
		for (uint32_t t = tid; t < nc + nk; t += kLnBlock) {
			stk[base + t] = t < nc ? cst[nc - 1 - t] : stg[nk - 1 - (t - nc)];
			stk_lv[base + t] = (uint8_t)(t < nc ? lv : lv + 1);
		}
		sp = base + nc + nk;
		__syncthreads();   // the pushes; the window's LDS is the next window's
	}
	if (tid == 0) {
		a.status[jq] = bad ? 8 : 0;
		a.out_len[jq] = bad ? 0u : n;
	}
}
