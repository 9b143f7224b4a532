// dg_inplace_core.h — the serial heart of in-place conversion, shared by the
// device kernel (dg_inplace_dev.hip, run by one lane of the delta's wave) and
// by CPU code (tests/sanitize/inplace_core_driver.cpp).  No HIP and no
// allocation: every array is supplied by the caller.
//
// The CRWI digraph of a delta whose commands are placed sequentially is held
// in interval-range form.  Copy i writes [dst_i, dst_i + len_i) and the dst
// column is non-decreasing, so the copies whose writes intersect copy i's read
// interval [src_i, src_i + len_i) are a contiguous index range [a_i, b_i); the
// neighbours of i, in the order the reference lists them (inplace.c:387-445),
// are a_i, a_i + 1, ..., b_i - 1 without i itself.  No edge list exists.
//
// What is here reproduces dg_inplace.cpp (and through it inplace.c) exactly:
//   ranges()      the two binary searches per copy;
//   tarjan()      iterative Tarjan over vertices 0..n-1, neighbours in range
//                 order; non-trivial components are numbered in completion
//                 order (sinks first), their vertices in stack-pop order;
//   find_cycle()  the resumable DFS inside one component: black vertices
//                 persist, the grey path is whitened when a cycle is returned;
//   next_victim() the stall policy: the lowest-index pending copy (constant)
//                 or the smallest (length, index) on the first cycle of the
//                 first component, sources first, that still has one
//                 (localmin), with the safety fallback;
//   order_serial()the whole conversion order with lane width 1 (the device
//                 kernel runs the data-parallel parts wave-wide instead).
//
// Work memory, u32 words per copy: idx, low, tstk, callv, calln, scc, cverts,
// cstart, active (9 words) and one flag byte.  Tarjan runs lazily, at the
// first stall; find_cycle's path and cursor reuse idx and low afterwards.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DGIP_HD __host__ __device__ inline
#else
#define DGIP_HD inline
#endif

namespace dgip {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint8_t kDone = 1, kGrey = 2, kBlack = 4, kOnStack = 8;
constexpr int kPolicyLocalmin = 0, kPolicyConstant = 1;
constexpr uint32_t kCoreWords = 9;   // u32 work words per copy (plus one flag byte)

struct Graph {
	uint32_t n;
	const uint32_t* len;
	const uint32_t* a;   // neighbours of v: a[v] .. b[v] - 1, without v
	const uint32_t* b;
};

struct Work {        // n entries each (cstart: n + 1 are never needed, comps <= n / 2)
	uint8_t* flag;   // kDone | colour | kOnStack
	uint32_t* idx;   // Tarjan index; afterwards find_cycle's path
	uint32_t* low;   // Tarjan lowlink; afterwards find_cycle's next-neighbour cursor
	uint32_t* tstk;  // Tarjan's vertex stack
	uint32_t* callv; // Tarjan's call stack: vertex
	uint32_t* calln; //                      next neighbour
	uint32_t* scc;   // component of v (kNone: trivial)
	uint32_t* cverts;   // vertices of the non-trivial components, component by component
	uint32_t* cstart;   // component c = cverts[cstart[c] .. cstart[c + 1])
	uint32_t* active;   // pending vertices of component c
};

struct Stall {
	int policy = kPolicyLocalmin;
	bool have_scc = false;
	uint32_t n_comp = 0;
	uint32_t visited = 0;     // components passed (the reference's scc_ptr)
	uint32_t scan = 0;        // resume position inside the current component
	uint32_t low_ptr = 0;     // every copy below it is done
};

// first k in [lo, hi) with col[k] >= x (col non-decreasing)
DGIP_HD uint32_t lower_bound_u32(const uint32_t* col, uint32_t lo, uint32_t hi, uint64_t x) {
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if ((uint64_t)col[mid] < x) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the neighbour range of copy i (dg_inplace.cpp step 3)
DGIP_HD void range_of(uint32_t i, uint32_t n, uint32_t src, uint32_t len, const uint32_t* dst_col,
                      const uint32_t* len_col, uint32_t* a, uint32_t* b) {
	const uint64_t lo_v = src, hi_v = (uint64_t)src + len;
	const uint32_t lo = lower_bound_u32(dst_col, 0, n, lo_v);
	const uint32_t hi = lower_bound_u32(dst_col, lo, n, hi_v);
	uint32_t first = lo;
	if (lo > 0) {
		const uint32_t j = lo - 1;
		if (j != i && (uint64_t)dst_col[j] + len_col[j] > lo_v) first = j;
	}
	*a = first;
	*b = hi;
}

DGIP_HD void tarjan(const Graph& g, const Work& w, uint32_t* n_comp) {
	const uint32_t n = g.n;
	for (uint32_t v = 0; v < n; ++v) {
		w.idx[v] = kNone;
		w.scc[v] = kNone;
		w.flag[v] &= (uint8_t)~kOnStack;
	}
	uint32_t counter = 0, sp = 0, cp = 0, nc = 0, nv = 0;
	w.cstart[0] = 0;
	for (uint32_t s = 0; s < n; ++s) {
		if (w.idx[s] != kNone) continue;
		w.idx[s] = w.low[s] = counter++;
		w.flag[s] |= kOnStack;
		w.tstk[sp++] = s;
		w.callv[cp] = s;
		w.calln[cp++] = g.a[s];
		while (cp) {
			const uint32_t v = w.callv[cp - 1];
			uint32_t x = w.calln[cp - 1];
			if (x == v) ++x;
			if (x < g.b[v]) {
				w.calln[cp - 1] = x + 1;
				if (w.idx[x] == kNone) {
					w.idx[x] = w.low[x] = counter++;
					w.flag[x] |= kOnStack;
					w.tstk[sp++] = x;
					w.callv[cp] = x;
					w.calln[cp++] = g.a[x];
				} else if ((w.flag[x] & kOnStack) && w.idx[x] < w.low[v]) {
					w.low[v] = w.idx[x];
				}
				continue;
			}
			--cp;
			if (cp) {
				const uint32_t parent = w.callv[cp - 1];
				if (w.low[v] < w.low[parent]) w.low[parent] = w.low[v];
			}
			if (w.low[v] == w.idx[v]) {
				if (w.tstk[sp - 1] == v) {   // trivial component
					--sp;
					w.flag[v] &= (uint8_t)~kOnStack;
				} else {
					uint32_t x2, pend = 0;
					do {
						x2 = w.tstk[--sp];
						w.flag[x2] &= (uint8_t)~kOnStack;
						w.scc[x2] = nc;
						w.cverts[nv++] = x2;
						if (!(w.flag[x2] & kDone)) ++pend;
					} while (x2 != v);
					w.active[nc] = pend;
					w.cstart[++nc] = nv;
				}
			}
		}
	}
	*n_comp = nc;
}

// First cycle among the pending vertices of component c, searching from its
// vertex *scan onwards; returns the smallest (length, index) vertex on it, or
// kNone.  path = w.idx, cursor = w.low (Tarjan is over).
DGIP_HD uint32_t find_cycle(const Graph& g, const Work& w, uint32_t c, uint32_t* scan) {
	uint32_t* path = w.idx;
	uint32_t* next = w.low;
	const uint32_t v0 = w.cstart[c], nverts = w.cstart[c + 1] - v0;
	for (uint32_t at = *scan; at < nverts; ++at) {
		const uint32_t start = w.cverts[v0 + at];
		if (w.flag[start] & (kDone | kGrey | kBlack)) continue;
		uint32_t d = 0;
		w.flag[start] |= kGrey;
		path[d] = start;
		next[d++] = g.a[start];
		while (d) {
			const uint32_t v = path[d - 1];
			uint32_t x = next[d - 1];
			bool pushed = false;
			for (; x < g.b[v]; ++x) {
				if (x == v || w.scc[x] != c) continue;
				const uint8_t f = w.flag[x];
				if (f & kDone) continue;
				if (f & kGrey) {   // back edge: the cycle is path[pos .. d)
					uint32_t pos = 0;
					while (path[pos] != x) ++pos;
					uint32_t best = path[pos];
					for (uint32_t k = pos; k < d; ++k) {
						const uint32_t u = path[k];
						if (g.len[u] < g.len[best] || (g.len[u] == g.len[best] && u < best)) best = u;
					}
					for (uint32_t k = 0; k < d; ++k) w.flag[path[k]] &= (uint8_t)~kGrey;
					*scan = at;
					return best;
				}
				if (!(f & kBlack)) {
					next[d - 1] = x + 1;
					w.flag[x] |= kGrey;
					path[d] = x;
					next[d++] = g.a[x];
					pushed = true;
					break;
				}
			}
			if (!pushed) {
				--d;
				w.flag[v] = (uint8_t)((w.flag[v] & ~kGrey) | kBlack);
			}
		}
	}
	*scan = nverts;
	return kNone;
}

// The victim of a stall (dg_inplace.cpp:281-309).  Some copy is pending.
DGIP_HD uint32_t next_victim(const Graph& g, const Work& w, Stall& s) {
	if (s.policy != kPolicyConstant) {
		if (!s.have_scc) {
			tarjan(g, w, &s.n_comp);
			s.have_scc = true;
			s.visited = 0;
			s.scan = 0;
		}
		for (;;) {
			// sources first: the reference visits its components in reverse
			// completion order
			while (s.visited < s.n_comp && w.active[s.n_comp - 1 - s.visited] == 0) {
				++s.visited;
				s.scan = 0;
			}
			if (s.visited >= s.n_comp) break;   // safety fallback (inplace.c:634-640)
			const uint32_t v = find_cycle(g, w, s.n_comp - 1 - s.visited, &s.scan);
			if (v != kNone) return v;
			++s.visited;
			s.scan = 0;
		}
	}
	while (s.low_ptr < g.n && (w.flag[s.low_ptr] & kDone)) ++s.low_ptr;
	return s.low_ptr;
}

// bookkeeping of a retired vertex the stall code depends on
DGIP_HD void mark_done(const Work& w, const Stall& s, uint32_t v) {
	w.flag[v] |= kDone;
	if (s.have_scc && w.scc[v] != kNone) w.active[w.scc[v]]--;
}

// The conversion order with lane width 1: order[0 .. *kept) are the copies
// that stay, in Kahn order; order[n - 1], order[n - 2], ... the *victims, in
// conversion order.  rank_of / by_rank order the copies by (length, index);
// indeg and ready (one byte per rank) are scratch.  a and b are written here.
DGIP_HD void order_serial(uint32_t n, const uint32_t* src, const uint32_t* dst, const uint32_t* len, int policy,
                          uint32_t* a, uint32_t* b, uint32_t* indeg, const uint32_t* rank_of,
                          const uint32_t* by_rank, uint8_t* ready, const Work& w, uint32_t* order,
                          uint32_t* kept, uint32_t* victims) {
	for (uint32_t i = 0; i < n; ++i) {
		range_of(i, n, src[i], len[i], dst, len, &a[i], &b[i]);
		indeg[i] = 0;
		w.flag[i] = 0;
		ready[i] = 0;
	}
	// in-degrees by a difference array over [a_i, b_i), minus the self hit
	for (uint32_t i = 0; i < n; ++i) {
		if (a[i] >= b[i]) continue;
		indeg[a[i]] += 1;
		if (b[i] < n) indeg[b[i]] -= 1;
	}
	uint32_t run = 0;
	for (uint32_t i = 0; i < n; ++i) {
		run += indeg[i];
		indeg[i] = run - ((a[i] <= i && i < b[i]) ? 1u : 0u);
		if (indeg[i] == 0) ready[rank_of[i]] = 1;
	}
	const Graph g{n, len, a, b};
	Stall s;
	s.policy = policy;
	uint32_t nk = 0, nv = 0, first = 0;
	while (nk + nv < n) {
		while (first < n && !ready[first]) ++first;
		uint32_t v;
		if (first < n) {
			ready[first] = 0;
			v = by_rank[first];
			order[nk++] = v;
		} else {
			v = next_victim(g, w, s);
			order[n - 1 - nv++] = v;
		}
		mark_done(w, s, v);
		for (uint32_t x = a[v]; x < b[v]; ++x) {
			if (x == v || (w.flag[x] & kDone)) continue;
			if (--indeg[x] == 0) {
				ready[rank_of[x]] = 1;
				if (rank_of[x] < first) first = rank_of[x];
			}
		}
	}
	*kept = nk;
	*victims = nv;
}

}  // namespace dgip
