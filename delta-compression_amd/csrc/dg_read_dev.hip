// dg_read_dev.hip — the range-read kernels (dg_read_plan_index,
// dg_read_plan_run), built as the stand-alone gfx950 code object
// lib/dg_read.hsaco.
//
// A read serves bytes [off, off + n) of the version a standard delta makes of
// R: the reference's replay (src/c/apply.c:229-249: zeros, then the commands
// in stream order, later writes over earlier ones), sliced.
//
//   dg_read_index_kernel  one 256-thread block per stream, once per batch of
//      deltas: the whole stream is parsed and bounds-checked window by window
//      (dec_window, dg_decode_dev.h, as decode and update do), and the block
//      leaves in the plan's memory the stream's status, version_size, whether
//      the stream is sequential (every command starts where the one before it
//      ends and the last ends at version_size: what every encoder, compose and
//      invert emit) and, per kRdStride bytes of the stream, the first command
//      at or after that offset with its dst (dg_read_dev.h).  The loop is
//      rd_index_walk (dg_read_walk_dev.h), which the chunked pass's fill
//      kernel runs per chunk: here one chunk spans the stream.
//   dg_read_kernel  one block per request: 256 threads and decode's 4 KiB
//      window step, or (DG_READ_BLOCK=64, lib/dg_read_alt.hsaco, measurements
//      only) one wave and 1 KiB windows.  A sequential stream is
//      entered at the last index entry whose dst is <= off and left at the
//      first window whose last command starts at or after off + n: its
//      commands tile V, so no zero fill and no ordering are needed.  Any other
//      valid stream is zero-filled and replayed whole, window by window.
//      Every command is clipped to the range on its lane before it is applied,
//      and destinations become slot-relative: no store falls outside
//      [out_off, out_off + n) whatever the index and the stream hold, and the
//      window step re-checks every COPY's src + len <= ref_len.
//
// Loads of the delta window are whole aligned 16-byte words that hold at least
// one byte of the stream, as in decode_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dg_decode_dev.h"
#include "dg_read_dev.h"
#include "dg_read_walk_dev.h"

using namespace dg;
using namespace dgrd;

extern "C" __global__ __launch_bounds__(kRdBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void dg_read_index_kernel(
    RdIndexArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x;
	__shared__ DecLdsMem M;
	__shared__ RdTileLds T;
	const DecLds L = dec_lds(M);

	const RdStream sd = a.streams[i];
	uint64_t doff = sd.delta_off, dl = sd.delta_len;
	int32_t st = a.delta_status ? a.delta_status[i] : 0;   // an earlier stage's failure is passed on
	if (!st && a.delta_offsets) {
		doff = a.delta_offsets[i];
		dl = a.delta_offsets[i + 1] - doff;
		if (dl > sd.delta_len) st = 7;   // longer than the plan allowed for
	}
	const uint8_t* D = a.delta + doff;
	uint8_t* IX = a.index + a.index_off[i];
	RdEnt* E = reinterpret_cast<RdEnt*>(IX + sizeof(RdHead));
	uint32_t vsize = 0;
	if (!st && bad_magic(D, dl)) st = 8;
	if (!st && (D[4] & 1)) st = 2;   // in-place: a slice of its replay needs the whole replay
	if (!st) vsize = be32(D + 5);
	const uint32_t n_ent = st ? 0u : (uint32_t)(dl / kRdStride) + 1u;

	// the walk of one chunk that spans the stream (dg_read_walk_dev.h).  Sequential: its
	// commands start at 0, each where the one before it ends, and the last ends at version_size
	bool seq = false;
	if (!st) {
		const RdWalk r = rd_index_walk(L, T, D, dl, vsize, sd.ref_len, E, 25, kRdNoEnd, 0, n_ent - 1u);
		if (r.failed) st = 8;
		seq = !r.t.brk && r.t.first == 0 && r.t.end == vsize;
	}
	if (tid == 0) {
		RdHead h;
		h.doff = doff;
		h.dl = st ? 0u : (uint32_t)dl;
		h.vsize = vsize;
		h.status = st;
		h.flags = (!st && seq) ? kRdSeq : 0u;
		h.n_ent = n_ent;
		h.pad = 0;
		*reinterpret_cast<RdHead*>(IX) = h;
		if (a.stream_status) a.stream_status[i] = st;
	}
}

// One request by a block of T threads: T = 256 parses 4 KiB windows with
// decode's window step, T = 64 (one wave) 1 KiB windows with the one-wave
// kernels' loader.  The build's DG_READ_BLOCK chooses (dg_read_dev.h).
template <uint32_t T>
__device__ __forceinline__ void rd_request(const RdArgs& a) {
	static_assert(T == 64 || T == 256, "one wave or four");
	const uint32_t jq = blockIdx.x;
	if (jq >= a.n_req) return;
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();

	const RdReq rq = a.reqs[jq];
	int32_t st = 0;
	if (rq.stream >= a.n_streams || rq.reserved) st = 1;
	RdHead h{};
	uint64_t ix0 = 0, ix1 = 0;
	if (!st) {
		ix0 = a.index_off[rq.stream];
		ix1 = a.index_off[rq.stream + 1];
		h = *reinterpret_cast<const RdHead*>(a.index + ix0);
		st = h.status;
	}
	// pread: what of [off, off + len) lies inside V
	const uint32_t n = st || rq.off >= h.vsize ? 0u : umin32(rq.len, h.vsize - rq.off);
	if (tid == 0) {
		a.status[jq] = st;
		a.out_len[jq] = n;
	}
	if (st || n == 0) return;

	const RdStream sd = a.streams[rq.stream];
	const uint8_t* R = a.ref + sd.ref_off;
	const uint64_t rl = sd.ref_len;
	const uint8_t* D = a.delta + h.doff;
	const uint32_t dl = h.dl;
	uint8_t* O = a.out + rq.out_off;
	const uint64_t lo = rq.off, hi = lo + n;
	const bool seq = h.flags & kRdSeq;

	uint32_t pos = 25;
	if (seq) {
		const RdEnt* E = reinterpret_cast<const RdEnt*>(a.index + ix0 + sizeof(RdHead));
		const uint64_t cap = (ix1 - ix0 - sizeof(RdHead)) / sizeof(RdEnt);
		pos = rd_entry_pos(E, (uint32_t)min((uint64_t)h.n_ent, cap), lo, dl);
	} else {
		// zeros where no command writes (apply.c:233): byte edges, whole 16-byte words between
		const uint32_t head = umin32(n, (16u - (uint32_t)((uintptr_t)O & 15u)) & 15u);
		const uint32_t nw = (n - head) / 16;
		for (uint32_t k = tid; k < head; k += T) O[k] = 0;
		for (uint32_t q = tid; q < nw; q += T) reinterpret_cast<uint4*>(O + head)[q] = make_uint4(0, 0, 0, 0);
		for (uint32_t k = head + 16 * nw + tid; k < n; k += T) O[k] = 0;
		block_sync_global();   // the zeros land before any command's bytes
	}

	// the clipped commands of a batch one by one in stream order (uniform call by one wave)
	auto in_order = [&](const DecCmd& c) {
		for (uint64_t m = __ballot(c.mine && c.len != 0); m; m &= m - 1) {
			const uint32_t kk = ffs64(m);
			const uint64_t ks = ((uint64_t)rdlane((uint32_t)(c.src >> 32), kk) << 32) | rdlane((uint32_t)c.src, kk);
			const uint32_t kd = rdlane((uint32_t)c.dst, kk), kl = rdlane((uint32_t)c.len, kk);
			const uint32_t kind = rdlane(c.kind, kk);
			wave_copy(O + kd, (kind == 1 ? R : D) + ks, kl, lane);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // its stores before the next command's
		}
	};

	bool done = false;
	if constexpr (T == 256) {
		__shared__ DecLdsMem M;
		const DecLds L = dec_lds(M);
		while (!done) {
			if (pos >= dl) break;
			const DecWin w = dec_window(L, D, dl, pos, false, h.vsize, rl);
			if (w.bad) break;   // (the index accepted these bytes: reached only with a stale index)
			const uint8_t* wp = M.win + w.shf;
			const uint32_t nb = (w.cnt + 63) / 64;
			// a sequential stream has nothing for the range after a command that starts at or after its end
			if (seq && w.cnt && rd_dst_at(wp, M.cmds[w.cnt - 1]) >= hi) done = true;
			if (w.free_win) {
				for (uint32_t b = wave; b < nb; b += kDecWaves) {
					DecCmd c = dec_cmd(wp, M.cmds, 64 * b, w.cnt, pos);
					rd_clip(c, lo, hi);
					dec_flat_batch(c, false, O, R, D, L.xs);
				}
			} else if (wave == 0) {
				// writes that overlap or go backwards: the clipped commands one by one in stream order
				for (uint32_t b = 0; b < nb; ++b) {
					DecCmd c = dec_cmd(wp, M.cmds, 64 * b, w.cnt, pos);
					rd_clip(c, lo, hi);
					in_order(c);
				}
			}
			done = done || w.done;
			pos = (uint32_t)w.next_pos;
			if (seq) __syncthreads();   // the window's LDS is the next window's
			else block_sync_global();   // and a later window's stores go over this one's
		}
	} else {
		__shared__ __attribute__((aligned(16))) uint8_t lds[kChainLdsBytes];
		__shared__ __attribute__((aligned(16))) uint8_t xlds[64 * 8 + 64 * 8 + 64 * 4 + 128 * 4 + 64 * 4];
		const ChainLds cl = chain_lds(lds);
		DecScratch xs;
		xs.sp = reinterpret_cast<const uint8_t**>(xlds);
		xs.dp = reinterpret_cast<uint8_t**>(xlds + 64 * 8);
		xs.cum = reinterpret_cast<uint32_t*>(xlds + 128 * 8);
		xs.row = reinterpret_cast<uint32_t*>(xlds + 128 * 8 + 64 * 4);
		xs.len = reinterpret_cast<uint32_t*>(xlds + 128 * 8 + 64 * 4 + 128 * 4);
		while (!done) {
			if (pos >= dl) break;
			const auto cw = chain_window<64>(cl, cl.win, chain_load_wave(cl.win, D, dl, pos), pos, dl);
			if (seq && cw.cnt && rd_dst_at(cl.win, cl.cmds[cw.cnt - 1]) >= hi) done = true;
			bool bad = false;
			for (uint32_t b0 = 0; b0 < cw.cnt && !bad; b0 += 64) {
				DecCmd c = dec_cmd(cl.win, cl.cmds, b0, cw.cnt, (uint64_t)pos);
				// the bounds, and whether the batch's writes are increasing and disjoint (dec_window's rule)
				const bool out = c.mine && (c.dst + c.len > h.vsize || (c.kind == 1 && c.src + c.len > rl));
				if (__ballot(out)) {
					bad = true;   // (the index accepted these bytes: reached only with a stale index)
					break;
				}
				const bool writes = c.mine && c.len != 0;
				const uint32_t end32 = writes ? (uint32_t)(c.dst + c.len) : 0u;
				const uint32_t before = wave_shr1z(wave_incl_max(end32));
				const bool unordered = writes && (uint32_t)c.dst < before;
				const bool flat = __ballot(unordered) == 0;
				rd_clip(c, lo, hi);
				if (flat) dec_flat_batch(c, false, O, R, D, xs);
				else in_order(c);
				// a later batch's stores go over this one's (a sequential stream's never meet)
				if (!seq) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			}
			if (bad || cw.term == kChBad) break;
			if (cw.term == kChEnd) done = true;
			pos = cw.next_pos;
			wave_sync();   // the window is rewritten next
		}
	}
}

#ifndef DG_READ_BLOCK
#define DG_READ_BLOCK kRdReadBlock
#endif

extern "C" __global__ __launch_bounds__(DG_READ_BLOCK) void dg_read_kernel(RdArgs a) { rd_request<DG_READ_BLOCK>(a); }
