// dg_plan.cpp — the host arithmetic of dg_plan.h.
//
// Pure host code with no HIP dependency, like dg_format.cpp: it is also
// compiled alone under AddressSanitizer/UBSan with tests/sanitize/
// plan_check.cpp, and tests/test_plan_cpu.py compares what it computes with
// the oracle.  It reads no environment variable (PlanEnv carries the A/B
// switches dg_host.cpp read).
#include "dg_plan.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace dg {

// ───────────────────────────── small host math ────────────────────────────

namespace {

typedef unsigned __int128 u128;

uint64_t mulmod64(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)a * b % m); }

uint64_t powmod64(uint64_t b, uint64_t e, uint64_t m) {
	uint64_t r = 1 % m;
	b %= m;
	for (; e; e >>= 1) {
		if (e & 1) r = mulmod64(r, b, m);
		b = mulmod64(b, b, m);
	}
	return r;
}

int fail(std::string& err, int code, const char* fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	err = buf;
	return code;
}

}  // namespace

// Deterministic Miller-Rabin; the first 12 prime bases decide every n < 2^64.
// (The reference uses 100 time-seeded random bases, src/c/hash.c:163-178.)
bool is_prime_u64(uint64_t n) {
	static const uint64_t B[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
	if (n < 2) return false;
	for (uint64_t b : B) {
		if (n == b) return true;
		if (n % b == 0) return false;
	}
	uint64_t d = n - 1;
	int s = 0;
	while (!(d & 1)) { d >>= 1; ++s; }
	for (uint64_t b : B) {
		uint64_t x = powmod64(b, d, n);
		if (x == 1 || x == n - 1) continue;
		bool composite = true;
		for (int i = 1; i < s && composite; ++i) {
			x = mulmod64(x, x, n);
			if (x == n - 1) composite = false;
		}
		if (composite) return false;
	}
	return true;
}

// src/c/hash.c:180-190
uint64_t next_prime(uint64_t n) {
	if (n <= 2) return 2;
	uint64_t c = (n % 2 == 0) ? n + 1 : n;
	while (!is_prime_u64(c)) c += 2;
	return c;
}

// ── GF(2)[x] mod P, reflected representation (bit 63 = x^0) ──
uint64_t gf2_mul(uint64_t a, uint64_t b) {
	uint64_t p = 0;
	for (int i = 0; i < 64; ++i) {
		if ((a >> (63 - i)) & 1) p ^= b;
		b = (b & 1) ? (b >> 1) ^ kCrcPoly : (b >> 1);
	}
	return p;
}

uint64_t gf2_pow(uint64_t base, uint64_t e) {   // base^e mod P
	uint64_t r = 1ULL << 63;
	for (; e; e >>= 1) {
		if (e & 1) r = gf2_mul(r, base);
		base = gf2_mul(base, base);
	}
	return r;
}

uint64_t gf2_xpow(uint64_t n) { return gf2_pow(1ULL << 62, n); }   // x^n mod P

uint64_t gf2_div_x(uint64_t z) {   // z * x^-1 mod P
	const uint64_t l = z >> 63;   // bit 63 of z*... equals the lsb shifted out
	return ((z ^ (l ? kCrcPoly : 0)) << 1) | l;
}

// ───────────────────────────── CRC tables ─────────────────────────────────

// CRC tables: slicing-by-8 and nibble tables of the combine constants
// + the finaliser's constants: x^(8 kCrcSegBytes) and the 16 pad inverses
void crc_tables_build(CrcTables& t) {
	std::vector<uint64_t>& tab = t.tab;
	uint64_t* xinv = t.xinv;
	tab.assign(kCrcTabWords, 0);
	for (int i = 0; i < 256; ++i) {
		uint64_t c = (uint64_t)i;
		for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
		tab[i] = c;
	}
	for (int k = 1; k < 8; ++k)
		for (int i = 0; i < 256; ++i) {
			const uint64_t prev = tab[(k - 1) * 256 + i];
			tab[k * 256 + i] = (prev >> 8) ^ tab[prev & 0xff];
		}
	for (int lv = 0; lv < kCrcLevels; ++lv) {
		const uint64_t K = gf2_xpow(8ull * 1024 << lv);
		for (int j = 0; j < 16; ++j)
			for (int nb = 0; nb < 16; ++nb)
				tab[8 * 256 + lv * kCrcNibTabWords + 16 * j + nb] = gf2_mul(K, (uint64_t)nb << (4 * j));
	}
	xinv[0] = 1ULL << 63;
	for (int i = 1; i < 16; ++i) {
		uint64_t z = xinv[i - 1];
		for (int b = 0; b < 8; ++b) z = gf2_div_x(z);
		xinv[i] = z;
	}
	t.kseg = gf2_xpow(8ull * kCrcSegBytes);
	for (int c = 0; c < kCrcFinTabs; ++c) {   // nibble tables: kseg, xinv[0..15], kseg^2..4, x^(8*256|512|48Ki)
		const uint64_t K = c == 0 ? t.kseg
		                 : c <= 16 ? xinv[c - 1]
		                 : c <= 19 ? gf2_xpow(8ull * kCrcSegBytes * (uint64_t)(c - 15))
		                 : c == kCrcFinX256 ? gf2_xpow(8ull * 256)
		                 : c == kCrcFinX512 ? gf2_xpow(8ull * 512) : gf2_xpow(8ull * 48 * 1024);
		for (int j = 0; j < 16; ++j)
			for (int nb = 0; nb < 16; ++nb)
				tab[8 * 256 + (kCrcLevels + c) * kCrcNibTabWords + 16 * j + nb] = gf2_mul(K, (uint64_t)nb << (4 * j));
	}
	{
		// row-interleaved segment tables: byte j of a PB-byte piece followed by
		// the 64 PB - PB bytes of the other lanes' pieces of its row
		std::vector<uint64_t> adv(256);
		for (int i = 0; i < 256; ++i) adv[i] = tab[i];   // T advanced by 0 bytes
		for (int n = 1; n <= 1023; ++n) {
			for (int i = 0; i < 256; ++i) adv[i] = (adv[i] >> 8) ^ tab[adv[i] & 0xff];
			if (n >= 1008)   // n = 1023 - j
				for (int i = 0; i < 256; ++i) tab[kCrcRows16 + (1023 - n) * 256 + i] = adv[i];
			if (n >= 504 && n <= 511)   // n = 511 - j
				for (int i = 0; i < 256; ++i) tab[kCrcRows8 + (511 - n) * 256 + i] = adv[i];
		}
		uint64_t z = 1ULL << 63;   // x^0
		for (int l = 0; l < 64; ++l) {   // x^(-8*16*l), x^(-8*8*l)
			tab[kCrcRowK16 + l] = z;
			for (int b = 0; b < 128; ++b) z = gf2_div_x(z);
		}
		z = 1ULL << 63;
		for (int l = 0; l < 64; ++l) {
			tab[kCrcRowK8 + l] = z;
			for (int b = 0; b < 64; ++b) z = gf2_div_x(z);
		}
		// five-bit row tables: the images Z^n(2^i) of the 64 register bits
		// (Z = one zero byte through the register), combined per 5-bit field
		auto five = [&](uint32_t base, int n) {
			uint64_t col[64];
			for (int i = 0; i < 64; ++i) {
				uint64_t x = 1ULL << i;
				for (int k = 0; k < n; ++k) x = (x >> 8) ^ tab[x & 0xff];
				col[i] = x;
			}
			for (int k = 0; k < 13; ++k)
				for (int v = 0; v < 32; ++v) {
					uint64_t r = 0;
					for (int b = 0; b < 5; ++b)
						if (((v >> b) & 1) && 5 * k + b < 64) r ^= col[5 * k + b];
					tab[base + 32 * k + v] = r;
				}
		};
		five(kCrc5R8, 512);
		five(kCrc5R16, 1024);
		five(kCrc5R16 + 32 * 13, 1016);
	}
	const uint64_t step = gf2_xpow(8ull * 32);
	t.k32[0] = 1ULL << 63;
	for (int i = 1; i < 1024; ++i) t.k32[i] = gf2_mul(t.k32[i - 1], step);
}

// ───────────────────────────── CRC planning ───────────────────────────────

void plan_crc_spans(const std::vector<dg_span_t>& spans, const std::vector<uint32_t>& which,
                    std::vector<CrcSpanDev>& sd, std::vector<CrcSegDev>& seg,
                    const std::vector<uint32_t>* outs) {
	sd.resize(spans.size());
	seg.clear();
	for (size_t i = 0; i < spans.size(); ++i) {
		CrcSpanDev& s = sd[i];
		s.off = spans[i].off;
		s.len = spans[i].len;
		s.seg_base = (uint32_t)seg.size();
		s.nseg = 0;
		s.which = which[i];
		s.out = outs ? (*outs)[i] : (uint32_t)i;
		if (s.len >= 8) {
			const uint64_t a0 = s.off & ~15ull, a1 = (s.off + s.len + 15) & ~15ull;
			s.nseg = (uint32_t)((a1 - a0 + kCrcSegBytes - 1) / kCrcSegBytes);
			for (uint32_t j = 0; j < s.nseg; ++j) seg.push_back(CrcSegDev{(uint32_t)i, j});
		}
	}
}

// ───────────────────────────── encode geometry ────────────────────────────

namespace {

bool is_one(const char* v) { return v && v[0] == '1'; }

// member mode wanted for this batch (automatic choice by mean pair size:
// measured C3 (256 KiB pairs) +56 %, C2 (64 KiB pairs) -22 %,
// profiles/r02_experiments.md); the context's mode and the A/B switches
// DG_NO_MEMBERS / DG_MEMBERS override it
bool members_wanted(const PlanEnv& env, const dg_pair_t* pairs, uint32_t n) {
	uint64_t vsum = 0;
	for (uint32_t i = 0; i < n; ++i) vsum += pairs[i].v_len;
	bool want = n && vsum / n >= (128u << 10);
	if (env.onepass_members == 1) want = true;
	if (env.onepass_members == 2) want = false;
	if (is_one(env.no_members)) want = false;
	if (is_one(env.members)) want = true;
	return want;
}

}  // namespace

// onepass: every COPY covers >= p bytes, so
//   delta <= 35 + |V| + (|V|/p) * max(0, 22 - p);
// correcting: a tail-corrected COPY may be shorter than p, but there
// are at most |V|/p + 1 of them, each with at most one ADD header
// (greedy: as onepass)
uint64_t pair_out_bound(dg_algorithm_t algo, uint64_t p, uint64_t v_len) {
	if (algo != DG_ALGO_CORRECTING) return 35 + v_len + (v_len / p) * (p < 22 ? 22 - p : 0);
	return 57 + v_len + 22 * (v_len / p);
}

int encode_geometry(dg_algorithm_t algo, const dg_diff_options_t& o, const dg_pair_t* pairs, uint32_t n,
                    const PlanEnv& env, EncodeGeometry& g, std::string& err) {
	if (algo != DG_ALGO_GREEDY && algo != DG_ALGO_ONEPASS && algo != DG_ALGO_CORRECTING)
		return fail(err, DG_ERR_INVALID_ARG, "unknown algorithm %d", (int)algo);
	// greedy: --splay only picks the smallest offset among the longest matches
	// (greedy.c:174-195); for the other two it changes which seeds are kept
	if (((o.flags >> DG_OPT_SPLAY) & 1) && algo != DG_ALGO_GREEDY)
		return fail(err, DG_ERR_UNSUPPORTED, "--splay is not supported (hash-table path only)");
	if ((o.flags >> DG_OPT_INPLACE) & 1)
		return fail(err, DG_ERR_UNSUPPORTED,
		            "in-place conversion is a host step: encode standard deltas, then dg_make_inplace");
	if (o.p == 0) return fail(err, DG_ERR_INVALID_ARG, "--seed-len must be >= 1");
	if (o.p > 65536) return fail(err, DG_ERR_INVALID_ARG, "--seed-len above 65536 is not supported");
	if (algo == DG_ALGO_CORRECTING && o.buf_cap > 4095)
		return fail(err, DG_ERR_UNSUPPORTED, "--buffer-size above 4095 is not supported (LDS lookback ring)");
	if (n > 0 && !pairs) return DG_ERR_INVALID_ARG;

	g = EncodeGeometry();
	g.pp.resize(n);
	std::map<uint64_t, uint64_t> qcache;
	uint64_t rec = 0, bound = 0, ctab = 0, gents = 0;
	const uint64_t p = o.p;
	for (uint32_t i = 0; i < n; ++i) {
		const dg_pair_t& d = pairs[i];
		// the format's u32 fields cap every buffer below 4 GiB (encoding.c:63,72-78);
		// the kernels keep 32-bit cursors with 1 MiB of headroom
		if (d.r_len >= (1ull << 32) - (1ull << 20) || d.v_len >= (1ull << 32) - (1ull << 20))
			return fail(err, DG_ERR_TOO_LARGE, "pair %u: buffers of 4 GiB or more do not fit the u32 format", i);
		if ((d.r_off | d.v_off) & 15) g.aligned16 = false;
		PairPlanDev& x = g.pp[i];
		memset(&x, 0, sizeof x);
		const uint64_t seeds = d.r_len >= p ? d.r_len - p + 1 : 0;
		if (algo == DG_ALGO_ONEPASS) {
			const uint64_t want = std::max<uint64_t>(o.q, seeds / p);   // onepass.c:61-62
			auto it = qcache.find(want);
			x.q = it != qcache.end() ? it->second : (qcache[want] = next_prime(want));
		} else if (algo == DG_ALGO_GREEDY) {
			// the seed index (dg_greedy.hip): a power-of-two bucket count >= the
			// seed count, heads[buckets + 1] and one entry per seed;
			// --table-size and --max-table do not apply (q stays 0)
			uint64_t nb = 1;
			while (nb < seeds) nb <<= 1;
			x.f_size = nb;
			x.tab_base = ctab;
			x.m = gents;
			ctab += nb + 1;
			gents += seeds;
			g.max_seeds = std::max<uint64_t>(g.max_seeds, seeds);
		} else {
			// correcting.c:116-129
			const uint64_t mt = o.max_table > 0 ? o.max_table : DG_MAX_TABLE_SIZE;
			uint64_t raw = seeds > 0 ? std::max<uint64_t>(o.q, 2 * seeds / p) : o.q;
			raw = std::min<uint64_t>(raw, mt);
			auto it = qcache.find(raw);
			x.q = it != qcache.end() ? it->second : (qcache[raw] = next_prime(raw));
			x.f_size = seeds > 0 ? next_prime(2 * seeds) : 1;
			x.m = x.f_size <= x.q ? 1 : (x.f_size + x.q - 1) / x.q;
			x.f_magic = UINT64_MAX / x.f_size;
			x.m_magic = UINT64_MAX / x.m;
			x.tab_base = ctab;
			ctab += x.q;
			g.max_seeds = std::max<uint64_t>(g.max_seeds, seeds);
		}
		if (x.q >= 0xFFFFFFFFull)
			return fail(err, DG_ERR_TOO_LARGE, "table size %llu too large", (unsigned long long)x.q);
		x.q_magic = x.q ? UINT64_MAX / x.q : 0;
		x.rec_base = rec;
		x.rec_cap = (uint32_t)(d.v_len / p + 1);
		rec += x.rec_cap;
		bound += pair_out_bound(algo, p, d.v_len);
		g.qmax = std::max<uint64_t>(g.qmax, x.q);
		g.qmin = std::min<uint64_t>(g.qmin, x.q);
		g.v_total += d.v_len;
	}
	g.out_bound = bound;
	g.total_rec = rec;
	g.ctab_entries = ctab;
	if (algo == DG_ALGO_GREEDY) {
		g.greedy_heads = ctab;
		g.greedy_entries = gents;
		if (ctab * 4 + gents * 8 > (64ull << 30))
			return fail(err, DG_ERR_NOMEM, "greedy seed indexes need %llu GiB (limit 64)",
			            (unsigned long long)((ctab * 4 + gents * 8) >> 30));
	} else if (ctab * 4 > (64ull << 30)) {
		return fail(err, DG_ERR_NOMEM, "correcting R indexes need %llu GiB (limit 64)",
		            (unsigned long long)(ctab >> 28));
	}

	// constants 263^(p-1-k) mod (2^61-1)
	g.powc.resize(p);
	{
		uint64_t c = 1;
		for (uint64_t k = 0; k < p; ++k) {
			g.powc[p - 1 - k] = c;
			c = (uint64_t)((u128)c * kBase % kMersenne);
		}
	}
	{
		// Correcting plans compute the CRCs in one of two ways:
		//   fused   where some R index fits LDS: the LDS build computes R's CRC
		//           from the bytes it holds and V's runs beside the V scan (C4:
		//           2.77 ms per step);
		//   beside  otherwise, the onepass arrangement: both CRCs on the side
		//           stream beside the build.
		// One block's LDS less the 2 KiB roll table, the fused R CRC's tables
		// (10 KiB) and reduction words, and some slack
		const int fixed = 2048 + 10240 + 128 + 256;
		const char* cb = env.corr_build;
		if (algo == DG_ALGO_CORRECTING && !(cb && strcmp(cb, "global") == 0) && env.lds_bytes > fixed + 4096)
			g.corr_lds_cap = (uint32_t)((env.lds_bytes - fixed) / 4);
		// fused: only R indexes built in LDS compute R's CRC; the others' R
		// CRCs run in V's pass
		g.crc_fused = g.corr_lds_cap && g.qmin <= g.corr_lds_cap;
	}
	if (g.crc_fused) {   // x^(-8 pad) of each R's zero padding to a multiple of 32 KiB
		const uint64_t xm8 = gf2_pow(gf2_div_x(1ULL << 63), 8);
		std::map<uint64_t, uint64_t> cache;
		for (uint32_t i = 0; i < n; ++i) {
			const uint64_t pad = (32768 - pairs[i].r_len % 32768) % 32768;
			auto it = cache.find(pad);
			if (it == cache.end()) it = cache.emplace(pad, gf2_pow(xm8, pad)).first;
			g.pp[i].crc_unpad = it->second;
		}
	}
	if (algo == DG_ALGO_CORRECTING)
		for (uint32_t i = 0; i < n; ++i)
			if (g.pp[i].q > g.corr_lds_cap) g.gpairs.push_back(i);
	// CRC spans: 2 per pair (R then V; V only when the build computes R's);
	// arena offsets are rebased at run time
	{
		std::vector<dg_span_t> spans;
		std::vector<uint32_t> which, outs;
		for (uint32_t i = 0; i < n; ++i) {
			if (!g.crc_fused || g.pp[i].q > g.corr_lds_cap) {
				spans.push_back(dg_span_t{pairs[i].r_off, pairs[i].r_len});
				which.push_back(0);
				outs.push_back(2 * i);
			}
			spans.push_back(dg_span_t{pairs[i].v_off, pairs[i].v_len});
			which.push_back(1);
			outs.push_back(2 * i + 1);
		}
		plan_crc_spans(spans, which, g.spans, g.segs, &outs);
	}

	// table-tier pool: 2 x qmax u64 per table.  Automatic size: one table per
	// resident onepass wave (CUs x 4 SIMDs x 5 waves) where that fits in
	// 4 GiB, at least 1 GiB; never more tables than pairs.
	const uint64_t per = g.table_bytes = 16ull * std::max<uint64_t>(g.qmax, 1);
	uint64_t pool = env.table_pool_bytes;
	if (pool == 0) {
		const uint64_t resident = 20ull * env.n_cu;
		pool = std::max<uint64_t>(1ull << 30, std::min<uint64_t>(resident * per, 4ull << 30));
	}
	g.n_tables = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint32_t>(n, 1), pool / per));
	// the device partitions the pool by XCD (8 per GPU): a multiple of 8
	// tables, at least 8 where the pool holds them
	if (pool / per >= 8) g.n_tables = std::max<uint32_t>(8, g.n_tables & ~7u);

	// the LDS-window chain: p = 16 onepass over 16-byte aligned pairs, i.e.
	// the batched hot configuration
	const bool window = algo == DG_ALGO_ONEPASS && o.p == 16 && g.aligned16 && env.onepass16;
	// DG_FUSED=1: onepass16 serialises in-kernel behind a decoupled look-back.
	// Off by default: the look-back couples every wave to the slowest pair
	// before it, which cost 20-25% at C2/C3 on MI355X (profiles/r01_ab_fused_vs_unfused.txt).
	g.fused = window && is_one(env.fused);
	// member mode: DG_NO_MEMBERS=1 (A/B builds) runs the plain chain
	// automatic choice by mean pair size for now: measured
	// (profiles/r02_experiments.md) C3 (256 KiB pairs) +56 %, C2 (64 KiB
	// pairs, where the plain chain's latency-bound waves overlap the CRC)
	// -22 %
	g.members = window && !g.fused && members_wanted(env, pairs, n);
	// automatic mode: a pair averaging fewer than 2 verified members per
	// 2 KiB chunk runs the plain chain (C3: ~39; shift and transposition
	// pairs, whose matches leave diagonal 0: ~0); forced member mode
	// keeps every pair on the member chain
	g.route_min = env.onepass_members == 0 ? (env.route_min ? (uint32_t)strtoul(env.route_min, nullptr, 0) : 2u) : 0u;
	if (g.members) {
		// chunks of kMemChunk positions covering [0, min(|R|, |V|)]; member
		// slots per chunk; the (pair, chunk) table the member kernel's waves index
		for (uint32_t i = 0; i < n; ++i) {
			const uint64_t E = std::min<uint64_t>(pairs[i].r_len, pairs[i].v_len);
			const uint32_t nch = (uint32_t)(E / kMemChunk + 1);
			g.pp[i].mem_base = g.mem_slots;
			g.pp[i].chunk_base = g.n_chunks;
			g.pp[i].n_chunks = nch;
			for (uint32_t c = 0; c < nch; ++c) {
				g.jobs.push_back(i);
				g.jobs.push_back(c);
			}
			g.mem_slots += (uint64_t)nch * kMemChunkSlots;
			g.n_chunks += nch;
		}
	}
	return DG_OK;
}

// ── --verbose: the reference's diagnostics from device counters and the delta ──

namespace {
// delta_print_command_stats (correcting.c:523-576)
void print_command_stats(const dg_commands_t& cmds) {
	uint64_t tc = 0, ta = 0, nc = 0, na = 0;
	std::vector<uint64_t> lens;
	for (size_t i = 0; i < cmds.len; ++i) {
		const dg_placed_command_t& c = cmds.data[i];
		if (c.tag == DG_CMD_COPY) { tc += c.length; ++nc; lens.push_back(c.length); }
		else { ta += c.length; ++na; }
	}
	const uint64_t tot = tc + ta;
	fprintf(stderr,
	        "  result: %llu copies (%llu bytes), %llu adds (%llu bytes)\n"
	        "  result: copy coverage %.1f%%, output %llu bytes\n",
	        (unsigned long long)nc, (unsigned long long)tc, (unsigned long long)na, (unsigned long long)ta,
	        tot > 0 ? (double)tc / tot * 100.0 : 0.0, (unsigned long long)tot);
	if (!lens.empty()) {
		std::sort(lens.begin(), lens.end());
		fprintf(stderr, "  copies: %llu regions, min=%llu max=%llu mean=%.1f median=%llu bytes\n",
		        (unsigned long long)lens.size(), (unsigned long long)lens.front(), (unsigned long long)lens.back(),
		        (double)tc / lens.size(), (unsigned long long)lens[lens.size() / 2]);
	}
}

// the delta's commands in stream order (none when it does not parse)
struct Commands : dg_commands_t {
	Commands(const uint8_t* delta, size_t len) {
		if (dg_delta_decode(delta, len, this, nullptr) != DG_OK) data = nullptr, this->len = 0, storage = nullptr;
	}
	~Commands() { dg_commands_free(this); }
	Commands(const Commands&) = delete;
	Commands& operator=(const Commands&) = delete;
};
}  // namespace

void print_verbose(dg_algorithm_t algo, const dg_diff_options_t& o, const dg_pair_t& d, const PairPlanDev& x,
                   const uint64_t* st, const uint8_t* delta, size_t delta_len) {
	const uint64_t p = o.p;
	if (d.v_len == 0) return;   // the reference returns before printing (onepass.c:58, correcting.c:112)
	const Commands cmds(delta, delta_len);
	if (algo == DG_ALGO_ONEPASS) {
		// onepass.c:64-69 and :277-285.  positions: every epoch's steps up to
		// its match (t + 1, t = max(v_m - v0, r_m - r0)) plus the final
		// epoch's steps while either stream has a window; lookups: one per
		// match (a probe counts only on a full-fingerprint hit, onepass.c:169-
		// 219, and fingerprints of distinct 16-byte windows coincide with
		// probability ~2^-61)
		fprintf(stderr, "onepass: %s, q=%llu, |R|=%llu, |V|=%llu, seed_len=%llu\n", "hash table",
		        (unsigned long long)x.q, (unsigned long long)d.r_len, (unsigned long long)d.v_len,
		        (unsigned long long)p);
		uint64_t pos = 0, matches = 0, v0 = 0, r0 = 0;
		for (size_t i = 0; i < cmds.len; ++i) {
			const dg_placed_command_t& c = cmds.data[i];
			if (c.tag != DG_CMD_COPY) continue;
			pos += std::max(c.dst - v0, c.src - r0) + 1;
			++matches;
			v0 = c.dst + c.length;
			r0 = c.src + c.length;
		}
		const uint64_t nv = d.v_len + 1 >= v0 + p ? d.v_len + 1 - p - v0 : 0;
		const uint64_t nr = d.r_len + 1 >= r0 + p ? d.r_len + 1 - p - r0 : 0;
		pos += std::max(nv, nr);
		fprintf(stderr,
		        "  scan: %llu positions, %llu lookups, %llu matches (flushes)\n"
		        "  scan: hit rate %.1f%% (of lookups)\n",
		        (unsigned long long)pos, (unsigned long long)matches, (unsigned long long)matches,
		        matches > 0 ? 100.0 : 0.0);
		print_command_stats(cmds);
		return;
	}
	if (algo == DG_ALGO_GREEDY) {   // greedy.c:146-150, 255-257
		fprintf(stderr, "greedy: %s, |R|=%llu, |V|=%llu, seed_len=%llu\n",
		        ((o.flags >> DG_OPT_SPLAY) & 1) ? "splay tree" : "hash table", (unsigned long long)d.r_len,
		        (unsigned long long)d.v_len, (unsigned long long)p);
		print_command_stats(cmds);
		return;
	}
	// correcting.c:137-152, 200-214, 470-485
	const uint64_t seeds = d.r_len >= p ? d.r_len - p + 1 : 0;
	const uint64_t cap = x.q, m = x.m, k = st ? st[6] : 0;
	const uint64_t expected = m > 0 ? seeds / m : 0;
	fprintf(stderr,
	        "correcting: %s, |C|=%llu |F|=%llu m=%llu k=%llu\n"
	        "  checkpoint gap=%llu bytes, expected fill ~%llu (~%llu%% table occupancy)\n"
	        "  table memory ~%llu MB\n",
	        "hash table", (unsigned long long)cap, (unsigned long long)x.f_size, (unsigned long long)m,
	        (unsigned long long)k, (unsigned long long)m, (unsigned long long)expected,
	        (unsigned long long)(cap > 0 ? expected * 100 / cap : 0), (unsigned long long)(cap * 24 / 1048576));
	const uint64_t passed = st ? st[0] : 0, stored = st ? st[1] : 0, in_cap = st ? st[7] : 0;
	fprintf(stderr,
	        "  build: %llu seeds, %llu passed checkpoint (%.2f%%), %llu stored, %llu collisions\n"
	        "  build: table occupancy %llu/%llu (%.1f%%)\n",
	        (unsigned long long)seeds, (unsigned long long)passed, seeds > 0 ? (double)passed / seeds * 100.0 : 0.0,
	        (unsigned long long)stored, (unsigned long long)(in_cap - stored), (unsigned long long)stored,
	        (unsigned long long)cap, cap > 0 ? (double)stored / cap * 100.0 : 0.0);
	const uint64_t vseeds = d.v_len >= p ? d.v_len - p + 1 : 0;
	const uint64_t ck = st ? st[2] : 0, fpm = st ? st[3] : 0, bm = st ? st[4] : 0, mt = st ? st[5] : 0;
	fprintf(stderr,
	        "  scan: %llu V positions, %llu checkpoints (%.3f%%), %llu matches\n"
	        "  scan: hit rate %.1f%% (of checkpoints), fp collisions %llu, byte mismatches %llu\n",
	        (unsigned long long)vseeds, (unsigned long long)ck, vseeds > 0 ? (double)ck / vseeds * 100.0 : 0.0,
	        (unsigned long long)mt, ck > 0 ? (double)mt / ck * 100.0 : 0.0, (unsigned long long)fpm,
	        (unsigned long long)bm);
	print_command_stats(cmds);
}

// ── in-place, compose and invert plans: descriptors, work memory, bounds ──

namespace {

// descs with max_copies and max_adds filled; extra[i]: the version bytes
// delta i's COPYs can turn into ADD payload
int inplace_finish(const std::vector<uint64_t>& extra, InplaceGeometry& g, std::string& err) {
	g.work = g.bound = 0;
	for (size_t i = 0; i < g.descs.size(); ++i) {
		dgip::IpDesc& d = g.descs[i];
		if (d.ref_len >= (1ull << 32) || d.delta_cap >= (1ull << 32))
			return fail(err, DG_ERR_TOO_LARGE, "in-place plan: a stream of 4 GiB or more does not fit the u32 format");
		d.work_off = g.work;
		g.work += dgip::work_bytes(d.max_copies, d.max_adds);
		g.bound += d.delta_cap + extra[i];
	}
	return DG_OK;
}

// descs with a_cap, b_cap, max_a and max_b filled
int compose_finish(ComposeGeometry& g, std::string& err) {
	g.work = 0;
	for (dgcp::CpDesc& d : g.descs) {
		if (d.a_cap >= (1ull << 32) || d.b_cap >= (1ull << 32))
			return fail(err, DG_ERR_TOO_LARGE, "compose plan: a stream of 4 GiB or more does not fit the u32 format");
		d.work_off = g.work;
		g.work += dgcp::work_bytes(d.max_a, d.max_b);
	}
	return DG_OK;
}

// pair i's worst-case delta size and command count in an encode plan
void compose_enc_pair(const EncodePlanView& e, uint32_t i, uint64_t* cap, uint32_t* cmds) {
	*cap = pair_out_bound(e.algo, e.p, e.pairs[i].v_len);
	// the encoders alternate COPY and ADD: at most one ADD before each COPY and one at the end
	*cmds = (uint32_t)std::min<uint64_t>(2ull * e.pp[i].rec_cap + 1, compose_max_cmds(*cap));
}

// descs with ref_len, delta_cap and max_copies filled
int invert_finish(InvertGeometry& g, std::string& err) {
	g.work = g.bound = 0;
	for (dgiv::IvDesc& d : g.descs) {
		if (d.ref_len >= (1ull << 32) || d.delta_cap >= (1ull << 32))
			return fail(err, DG_ERR_TOO_LARGE, "invert plan: a stream or reference of 4 GiB or more does not fit the u32 format");
		d.work_off = g.work;
		g.work += dgiv::work_bytes(d.max_copies);
		g.bound += dgiv::out_bound(d.max_copies, d.ref_len);
	}
	return DG_OK;
}

}  // namespace

int inplace_plan_geometry(const dg_inplace_desc_t* descs, uint32_t n, InplaceGeometry& g, std::string& err) {
	g.descs.resize(n);
	std::vector<uint64_t> extra(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t cap = descs[i].delta_cap;
		// 25 header bytes, then 13 per COPY and at least 9 per ADD
		// (the END byte may be missing: encoding.c:111-178 stops at the stream's end too)
		const uint64_t body = cap > 25 ? cap - 25 : 0;
		g.descs[i] = dgip::IpDesc{descs[i].ref_off, descs[i].ref_len, descs[i].delta_off, cap, 0,
		                          (uint32_t)std::min<uint64_t>(body / 13, 0xFFFFFFFFull),
		                          (uint32_t)std::min<uint64_t>(body / 9, 0xFFFFFFFFull)};
		extra[i] = std::min<uint64_t>((body / 13) * descs[i].ref_len, 1ull << 32);
	}
	return inplace_finish(extra, g, err);
}

int inplace_plan_geometry_for(const EncodePlanView& e, uint32_t n, InplaceGeometry& g, std::string& err) {
	g.descs.resize(n);
	std::vector<uint64_t> extra(n);
	for (uint32_t i = 0; i < n; ++i) {
		// the encoders alternate COPY and ADD: at most one ADD before each COPY and one at the end
		g.descs[i] = dgip::IpDesc{e.pairs[i].r_off, e.pairs[i].r_len, 0, pair_out_bound(e.algo, e.p, e.pairs[i].v_len), 0,
		                          e.pp[i].rec_cap, e.pp[i].rec_cap + 1};
		extra[i] = e.pairs[i].v_len;
	}
	return inplace_finish(extra, g, err);
}

uint32_t compose_max_cmds(uint64_t cap) { return (uint32_t)std::min<uint64_t>(cap > 25 ? (cap - 25) / 9 : 0, 0xFFFFFFFEull); }

int compose_plan_geometry(const dg_compose_desc_t* descs, uint32_t n, ComposeGeometry& g, std::string& err) {
	g.descs.resize(n);
	for (uint32_t i = 0; i < n; ++i)
		g.descs[i] = dgcp::CpDesc{descs[i].a_off, descs[i].a_cap, descs[i].b_off, descs[i].b_cap, 0,
		                          compose_max_cmds(descs[i].a_cap), compose_max_cmds(descs[i].b_cap)};
	return compose_finish(g, err);
}

int compose_plan_geometry_for(const EncodePlanView& a, const EncodePlanView& b, uint32_t n, ComposeGeometry& g,
                              std::string& err) {
	g.descs.resize(n);
	for (uint32_t i = 0; i < n; ++i) {
		g.descs[i] = dgcp::CpDesc{};
		compose_enc_pair(a, i, &g.descs[i].a_cap, &g.descs[i].max_a);
		compose_enc_pair(b, i, &g.descs[i].b_cap, &g.descs[i].max_b);
	}
	return compose_finish(g, err);
}

// 25 header bytes, 13 per COPY and the END byte
uint32_t invert_max_copies(uint64_t cap) { return (uint32_t)std::min<uint64_t>(cap > 26 ? (cap - 26) / 13 : 0, 0xFFFFFFFEull); }

int invert_plan_geometry(const dg_invert_desc_t* descs, uint32_t n, InvertGeometry& g, std::string& err) {
	g.descs.resize(n);
	for (uint32_t i = 0; i < n; ++i)
		g.descs[i] = dgiv::IvDesc{descs[i].ref_off, descs[i].ref_len, descs[i].delta_off, descs[i].delta_cap, 0,
		                          invert_max_copies(descs[i].delta_cap), 0};
	return invert_finish(g, err);
}

int invert_plan_geometry_for(const EncodePlanView& e, uint32_t n, InvertGeometry& g, std::string& err) {
	g.descs.resize(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t cap = pair_out_bound(e.algo, e.p, e.pairs[i].v_len);
		g.descs[i] = dgiv::IvDesc{e.pairs[i].r_off, e.pairs[i].r_len, 0, cap, 0,
		                          std::min<uint32_t>(e.pp[i].rec_cap, invert_max_copies(cap)), 0};
	}
	return invert_finish(g, err);
}

// ── splice plan: groups, segments, CRC weights ──

int splice_plan_geometry(const dg_pair_t* segs, uint32_t n_seg, const dg_pair_t* wholes, const uint32_t* seg_first,
                         uint32_t n_groups, const uint64_t* caps, SpliceGeometry& g, std::string& err) {
	g.descs.assign(n_seg, dgsp::SpDesc{});
	g.groups.assign(n_groups, dgsp::SpGroup{});
	g.bound = 0;
	if (seg_first[0] != 0 || seg_first[n_groups] != n_seg)
		return fail(err, DG_ERR_INVALID_ARG, "splice plan: seg_first does not run from 0 to the segment count");
	constexpr uint64_t kLimit = (1ull << 32) - (1ull << 20);
	for (uint32_t k = 0; k < n_groups; ++k) {
		const dg_pair_t& w = wholes[k];
		const uint32_t first = seg_first[k], end = seg_first[k + 1];
		if (end <= first || end > n_seg) return fail(err, DG_ERR_INVALID_ARG, "splice plan: group %u has no segment", k);
		if (w.r_len >= kLimit || w.v_len >= kLimit)
			return fail(err, DG_ERR_TOO_LARGE, "splice plan: group %u: buffers of 4 GiB or more do not fit the u32 format", k);
		g.groups[k] = dgsp::SpGroup{first, end - first, (uint32_t)w.v_len, 0};
		uint64_t at = w.v_off;
		for (uint32_t j = first; j < end; ++j) {
			const dg_pair_t& s = segs[j];
			if (s.v_off != at || s.v_len > w.v_off + w.v_len - at)
				return fail(err, DG_ERR_INVALID_ARG, "splice plan: segment %u does not continue the tiling of its group's V", j);
			at += s.v_len;
			if (s.r_off < w.r_off || s.r_off - w.r_off > w.r_len || s.r_len > w.r_len - (s.r_off - w.r_off))
				return fail(err, DG_ERR_INVALID_ARG, "splice plan: segment %u: its window is not inside its group's R", j);
			const uint64_t cap = caps ? caps[j] : (1ull << 32) - 1;
			if (cap >= (1ull << 32))
				return fail(err, DG_ERR_TOO_LARGE, "splice plan: a stream of 4 GiB or more does not fit the u32 format");
			dgsp::SpDesc& d = g.descs[j];
			d.cap = cap;
			d.rebase = (uint32_t)(s.r_off - w.r_off);
			d.r_len = (uint32_t)s.r_len;
			d.v_rel = (uint32_t)(s.v_off - w.v_off);
			d.v_len = (uint32_t)s.v_len;
			d.group = k;
			if (caps) g.bound += cap;
		}
		if (at != w.v_off + w.v_len)
			return fail(err, DG_ERR_INVALID_ARG, "splice plan: group %u: the segments do not cover its V", k);
		// x^(8 * suffix), from the last segment back: one power per segment
		uint64_t shift = 1ULL << 63;
		for (uint32_t j = end; j-- > first;) {
			g.descs[j].shift = shift;
			if (segs[j].v_len) shift = gf2_mul(shift, gf2_xpow(8 * segs[j].v_len));
		}
		if (caps) g.bound += 1;
	}
	return DG_OK;
}

// ── sketch plan: the (span, chunk) work list ──

int sketch_plan_geometry(const dg_span_t* spans, uint32_t n, uint32_t p, uint32_t K, uint32_t chunk_bytes,
                         SketchGeometry& g, std::string& err) {
	using namespace dgsk;
	if (p < 1 || p > kMaxSeed) return fail(err, DG_ERR_INVALID_ARG, "sketch plan: seed length %u is not in 1..%u", p, kMaxSeed);
	if (K < kMinBins || K > kMaxBins || (K & (K - 1)))
		return fail(err, DG_ERR_INVALID_ARG, "sketch plan: %u bins is not a power of two in %u..%u", K, kMinBins, kMaxBins);
	if (!chunk_bytes) chunk_bytes = kChunkBytes;
	if (chunk_bytes % (4 * kSkBlock) || chunk_bytes > 16384)
		return fail(err, DG_ERR_INVALID_ARG, "sketch plan: a chunk of %u bytes is not a multiple of %u up to 16384", chunk_bytes,
		            4 * kSkBlock);
	g.chunk_bytes = chunk_bytes;
	g.shift = 64 - (uint32_t)__builtin_ctz(K);
	g.powc.resize(p);
	uint64_t c = 1;
	for (uint32_t k = 0; k < p; ++k) {
		g.powc[p - 1 - k] = c;
		c = (uint64_t)((u128)c * kBase % kMersenne);
	}
	g.items.clear();
	for (uint32_t i = 0; i < n; ++i) {
		if (spans[i].len >= (1ull << 32))
			return fail(err, DG_ERR_TOO_LARGE, "sketch plan: span %u: 4 GiB or more", i);
		if (spans[i].off + spans[i].len < spans[i].off)
			return fail(err, DG_ERR_INVALID_ARG, "sketch plan: span %u wraps the address space", i);
		if (spans[i].len < p) continue;
		const uint64_t windows = spans[i].len - p + 1;
		const uint64_t chunks = (windows + chunk_bytes - 1) / chunk_bytes;
		if (g.items.size() + chunks > 0x7FFFFFFFull)
			return fail(err, DG_ERR_TOO_LARGE, "sketch plan: more than 2^31 - 1 chunks");
		for (uint32_t k = 0; k < chunks; ++k) g.items.push_back(SkItem{i, k});
	}
	return DG_OK;
}

// ── update plan: descriptor checks ──

int update_check_descs(const dg_update_desc_t* descs, uint32_t n, std::string& err) {
	char msg[160];
	std::vector<std::pair<uint64_t, uint64_t>> iv;   // the non-empty buffer regions
	iv.reserve(n);
	for (uint32_t i = 0; i < n; ++i) {
		const dg_update_desc_t& d = descs[i];
		if (d.buf_cap >= (1ull << 32) || d.ref_len >= (1ull << 32) || d.delta_len >= (1ull << 32)) {
			snprintf(msg, sizeof msg, "update plan: stream %u: a buffer or a length of 4 GiB or more does not fit the u32 format", i);
			err = msg;
			return DG_ERR_TOO_LARGE;
		}
		if (d.buf_off + d.buf_cap < d.buf_off || d.delta_off + d.delta_len < d.delta_off) {
			snprintf(msg, sizeof msg, "update plan: stream %u: a region wraps the address space", i);
			err = msg;
			return DG_ERR_INVALID_ARG;
		}
		if (d.buf_cap) iv.push_back({d.buf_off, d.buf_off + d.buf_cap});
	}
	std::sort(iv.begin(), iv.end());
	for (size_t k = 1; k < iv.size(); ++k)
		if (iv[k].first < iv[k - 1].second) {
			snprintf(msg, sizeof msg, "update plan: the buffer regions at %llu and %llu overlap",
			         (unsigned long long)iv[k - 1].first, (unsigned long long)iv[k].first);
			err = msg;
			return DG_ERR_INVALID_ARG;
		}
	return DG_OK;
}

}  // namespace dg
