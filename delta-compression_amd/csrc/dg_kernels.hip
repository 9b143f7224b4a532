// dg_kernels.hip — CDNA4 (gfx950) kernels of the delta codec.
//
//   crc_rows_kernel / crc_rows_wide_kernel / crc_finalize_kernel  CRC-64/XZ
//       of every R and V (segment folds in dg_crc.h)
//       (src/c/delta.h:294-322; main.c:259-260)
//   onepass_kernel   one wave64 per pair, onepass differencing
//       (src/c/onepass.c:32-297) in its epoch form
//   scan_sizes_kernel  exclusive scan of per-pair delta sizes
//   serialize_wave_kernel   placement + DLT\x03 serialisation
//       (src/c/apply.c:136-164, src/c/encoding.c:39-90)
//   synth_*            synthetic batch generators (bench/test inputs)
//
// Written for wave64 / gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dg_device.h"
#include "dg_devutil.h"
#include "dg_crc.h"
#include "dg_serialize_wave.h"

namespace dg {

// ───────────────────────────── scan of sizes ──────────────────────────────

// One block: each thread sums a contiguous run of ceil(n / 1024) sizes, the
// block scans the 1024 run sums (wave shuffles + 16 wave totals in LDS), and
// each thread writes its run's exclusive offsets.  One barrier pair.
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t x) {
	const uint32_t lane = lane_id();
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64);
		const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
		if (lane >= (uint32_t)d) x += ((uint64_t)hi << 32) | lo;
	}
	return x;
}

__global__ __launch_bounds__(1024) void scan_sizes_kernel(const uint64_t* __restrict__ sz,
                                                          uint64_t* __restrict__ off, uint32_t n,
                                                          uint32_t* route_cnt, uint32_t* route_fb) {
	__shared__ uint64_t wsum[16];
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	if (route_cnt && tid == 0) {
		// member plans: the pairs the run routed to the plain chain, for the
		// host's next run (dg_host.cpp, chain_join); zeroed for that run
		__hip_atomic_store(route_fb, *route_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		*route_cnt = 0u;
	}
	const uint32_t per = (n + 1023) / 1024;
	const uint32_t b = tid * per, e = min(b + per, n);
	uint64_t s = 0;
	for (uint32_t k = b; k < e; ++k) s += sz[k];
	const uint64_t incl = wave_incl_scan64(s);
	if (lane == 63) wsum[wave] = incl;
	__syncthreads();
	if (wave == 0) {
		const uint64_t w = lane < 16 ? wsum[lane] : 0;
		const uint64_t wi = wave_incl_scan64(w);
		if (lane < 16) wsum[lane] = wi - w;   // exclusive wave offsets
	}
	__syncthreads();
	uint64_t run = wsum[wave] + incl - s;
	for (uint32_t k = b; k < e; ++k) {
		off[k] = run;
		run += sz[k];
	}
	if (tid == 1023) off[n] = wsum[15] + incl;   // the grand total (thread 1023 holds the last run)
}

// ───────────────────────────── CRC-64/XZ ──────────────────────────────────
//
// Tables (built on the host, uploaded once per context; dg_device.h):
//   slice[8][256]    slicing-by-8 tables of the reflected polynomial
//   lvl[6][256]      nibble tables of "multiply by x^(8*1024*2^l) mod P"
//   the row tables and per-lane constants of dg_crc.h
// The raw CRC (init 0, no xorout) is linear, leading zero bytes are no-ops
// and init = ~0 equals XOR-ing 0xFF into the first 8 data bytes, so each
// segment is hashed from a zero register over a zero-front-padded span and
// the segments are combined as c_left * x^(8*len_right) ^ c_right.

// ── row-interleaved segments (dg_crc.h) ──

// Wide: 16-byte pieces (8 of the 16 lookups per piece do not wait for the
// register), the 16 tables in 32 KiB, one 1024-thread block per CU: for a CRC
// pass that has the GPU to itself.  (Four bank-spread table copies, 128 KiB,
// measured slower: 4.8 vs 5.1 TB/s alone, profiles/r05_crc_lab_product.txt.)
constexpr uint32_t kCrcWideBlock = 1024;
template <uint32_t kBlock = kCrcWideBlock>
__global__ __launch_bounds__(kBlock) void crc_rows_wide_kernel(CrcArgs a) {
	__shared__ __attribute__((aligned(256))) uint64_t TW[16 * 256];
	for (uint32_t i = threadIdx.x; i < 16 * 256; i += kBlock) TW[i] = a.tables[kCrcRows16 + i];
	__syncthreads();
	const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
	const uint32_t tb = lds_addr(TW), tbh = tb + 8u * 2048u;
	const uint64_t kl = a.tables[kCrcRowK16 + lane];
	constexpr uint32_t kWaves = kBlock / 64;
	for (uint32_t seg = uni(blockIdx.x * kWaves + wave); seg < a.n_segs; seg += gridDim.x * kWaves) {
		const CrcSegDev sd = a.segs[seg];
		const CrcSpanDev sp = a.spans[sd.span];
		const uint64_t c = crc_seg_rows<16, 1, 4>((uintptr_t)(a.arena[sp.which] + sp.off), sp.len, sp.nseg, sd.j, tb,
		                                          tbh, kl);
		if (lane == 0) a.seg_crc[seg] = c;
	}
}

// Beside another kernel: 8-byte pieces, one table copy (byte tables: 16 KiB;
// five-bit tables: 3.25 KiB), DG_CRC_PF (byte tables) / DG_CRC_PF5 (five-bit)
// pieces per lane per batch (two batches in flight), at most 72 VGPRs (a
// register budget for 7 blocks per CU).  Four pieces per batch: byte tables
// (58 VGPRs) C2 1762 -> 1801-1819 GiB/s beside the onepass kernel; five-bit
// tables (67 VGPRs; at a 64-VGPR budget they spilled) c6 1340 -> 1358
// (profiles/r06_experiments.md).
#ifndef DG_CRC_PF
#define DG_CRC_PF 4
#endif
#ifndef DG_CRC_PF5
#define DG_CRC_PF5 4
#endif
#ifndef DG_CRC_PRIO   // A/B: issue priority of the rows pass beside another kernel (0..3)
#define DG_CRC_PRIO 0
#endif
#ifndef DG_CRC_MINBLOCKS   // blocks per CU the register budget is sized for (7: 72 VGPRs, 8: 64)
#define DG_CRC_MINBLOCKS 7
#endif
template <int TAB>
__global__ __launch_bounds__(256, DG_CRC_MINBLOCKS) void crc_rows_kernel(CrcArgs a) {
	if constexpr (DG_CRC_PRIO > 0) __builtin_amdgcn_s_setprio(DG_CRC_PRIO);
	constexpr uint32_t nt = TAB == kCrcByte ? 8 * 256 : 32 * kCrc5Tabs8;
	__shared__ __attribute__((aligned(256))) uint64_t T8[nt];
	for (uint32_t i = threadIdx.x; i < nt; i += 256) T8[i] = a.tables[(TAB == kCrcByte ? kCrcRows8 : kCrc5R8) + i];
	__syncthreads();
	const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
	const uint32_t tb = lds_addr(T8);
	const uint64_t kl = a.tables[kCrcRowK8 + lane];
	bool raised = false;
	for (uint32_t seg = uni(blockIdx.x * kCrcWavesPerBlock + wave); seg < a.n_segs;
	     seg += gridDim.x * kCrcWavesPerBlock) {
		if (a.prio_flag && !raised) {
			// member plans: once the member kernel is done, the rows pass
			// outranks the chains beside it (the routed plain chain's waves
			// otherwise leave it the last issue slots)
			if (uni(__hip_atomic_load(a.prio_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
				__builtin_amdgcn_s_setprio(1);
				raised = true;
			}
		}
		const CrcSegDev sd = a.segs[seg];
		const CrcSpanDev sp = a.spans[sd.span];
		const uint64_t c = crc_seg_rows<8, 1, TAB == kCrcByte ? DG_CRC_PF : DG_CRC_PF5, kCrcSegBytes, false, TAB>(
		    (uintptr_t)(a.arena[sp.which] + sp.off), sp.len, sp.nseg, sd.j, tb, tb, kl);
		if (lane == 0) a.seg_crc[seg] = c;
	}
}

__global__ __launch_bounds__(64) void crc_finalize_kernel(CrcArgs a) {
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i >= a.n_spans) return;
	const CrcSpanDev sp = a.spans[i];
	uint64_t crc;
	if (sp.len < 8) {
		const uint8_t* d = a.arena[sp.which] + sp.off;
		uint64_t c = ~0ULL;
		for (uint64_t k = 0; k < sp.len; ++k) c = a.tables[(uint8_t)(c ^ d[k])] ^ (c >> 8);
		crc = ~c;
	} else {
		// constant multiplications by nibble tables (16 cached loads instead
		// of a 64-step bit-serial product), skipped where they are trivial
		const uint64_t* KS = a.tables + 8 * 256 + kCrcLevels * kCrcNibTabWords;   // x^(8 kCrcSegBytes)
		uint64_t acc = 0;
		for (uint32_t j = 0; j < sp.nseg; ++j)
			acc = (j ? mul_nib(acc, KS) : 0ull) ^ a.seg_crc[sp.seg_base + j];
		const uintptr_t end = (uintptr_t)(a.arena[sp.which] + sp.off) + sp.len;
		const uint32_t t = (uint32_t)(((end + 15) & ~(uintptr_t)15) - end);
		if (t) acc = mul_nib(acc, KS + (1 + t) * kCrcNibTabWords);   // undo the trailing pad bytes (x^-8t)
		crc = ~acc;
	}
	a.out[sp.out] = crc;
}

// ───────────────────────────── synthetic inputs ───────────────────────────

__device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t k) {
	uint64_t z = seed + k * 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}

// R_i = splitmix64 bytes (seed_base + i); V_i = R_i (edits applied after)
__global__ __launch_bounds__(256) void synth_random_kernel(uint8_t* ref, uint8_t* ver,
                                                           uint64_t pair_len, uint64_t seed_base,
                                                           uint64_t words_total) {
	const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (w >= words_total) return;
	const uint64_t words_per_pair = (pair_len + 7) / 8;
	const uint64_t pair = w / words_per_pair, k = w % words_per_pair;
	const uint64_t val = splitmix_at(seed_base + pair, k + 1);
	const uint64_t off = pair * pair_len + 8 * k;
	if (8 * k + 8 <= pair_len) {
		uint8_t* r = ref + off;
		uint8_t* v = ver + off;
		for (int b = 0; b < 8; ++b) { r[b] = (uint8_t)(val >> (8 * b)); v[b] = (uint8_t)(val >> (8 * b)); }
	} else {
		for (uint64_t b = 0; 8 * k + b < pair_len; ++b) {
			ref[off + b] = (uint8_t)(val >> (8 * b));
			ver[off + b] = (uint8_t)(val >> (8 * b));
		}
	}
}

__global__ __launch_bounds__(64) void synth_edits_kernel(uint8_t* ver, uint32_t n_pairs,
                                                         uint64_t pair_len, uint64_t seed_base,
                                                         uint64_t n_edits) {
	const uint32_t pair = blockIdx.x * 64 + threadIdx.x;
	if (pair >= n_pairs || pair_len == 0) return;
	const uint64_t s = (seed_base + pair) ^ 0xD1B54A32D192ED03ULL;
	uint8_t* v = ver + (uint64_t)pair * pair_len;
	for (uint64_t e = 0; e < n_edits; ++e) {
		const uint64_t pos = splitmix_at(s, 2 * e + 1) % pair_len;
		v[pos] = (uint8_t)splitmix_at(s, 2 * e + 2);
	}
}

// Transposition pairs (tests/gen_transpositions.py recipe, planned on the
// host): R bytes are the splitmix64 stream of the pair's seed; V is R's
// blocks in permuted order, one copy command per block.
__global__ __launch_bounds__(256) void synth_stream_kernel(uint8_t* ref, const SynthSpan* spans,
                                                           uint32_t n) {
	const uint32_t i = blockIdx.y;
	if (i >= n) return;
	const SynthSpan sp = spans[i];
	const uint64_t words = (sp.len + 7) / 8;
	for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < words; k += (uint64_t)gridDim.x * 256) {
		const uint64_t val = splitmix_at(sp.seed, k + 1);
		uint8_t* r = ref + sp.off + 8 * k;
		for (uint64_t b = 0; b < 8 && 8 * k + b < sp.len; ++b) r[b] = (uint8_t)(val >> (8 * b));
	}
}

__global__ __launch_bounds__(256) void synth_copy_kernel(uint8_t* ver, const uint8_t* ref,
                                                         const SynthCopy* cmds, uint32_t n) {
	const SynthCopy c = cmds[blockIdx.x];
	for (uint64_t b = threadIdx.x; b < c.len; b += 256) ver[c.dst + b] = ref[c.src + b];
}

// Shift pairs (oracle/delta_oracle.c or_synth_shift): V = R with one edit per
// stratum of R — a substitution, or an insertion / deletion of 1..8 bytes.
// One block per pair; thread t takes a contiguous range of strata, the
// block's exclusive scan of their length changes places them in V.
struct ShiftEdit {
	uint64_t pos, k, bytes;
	uint32_t kind;   // 0 substitution, 1 insertion, 2 deletion
};
__device__ __forceinline__ ShiftEdit shift_edit(uint64_t s, uint64_t e, uint64_t a, uint64_t b, uint32_t pct) {
	const uint64_t h1 = splitmix_at(s, 3 * e + 1), h2 = splitmix_at(s, 3 * e + 2), h3 = splitmix_at(s, 3 * e + 3);
	ShiftEdit x;
	x.pos = a + h1 % (b - a);
	const uint64_t u = h2 % 100;
	x.k = 1 + (h2 >> 32) % 8;
	x.bytes = h3;
	x.kind = 2 * u < pct ? 1u : (u < pct ? 2u : 0u);
	if (x.kind == 2 && x.k > b - x.pos) x.k = b - x.pos;
	return x;
}
__global__ __launch_bounds__(256) void synth_shift_kernel(uint8_t* ver, const uint8_t* ref, const SynthSpan* spans,
                                                          const uint64_t* v_off, uint32_t n_pairs, uint64_t n_edits,
                                                          uint32_t pct) {
	__shared__ int64_t part[256];
	const uint32_t i = blockIdx.x, tid = threadIdx.x;
	if (i >= n_pairs) return;
	const SynthSpan sp = spans[i];
	const uint64_t len = sp.len;
	const uint8_t* R = ref + sp.off;
	uint8_t* V = ver + v_off[i];
	const uint64_t n = n_edits < len ? n_edits : len;
	if (n == 0) {
		for (uint64_t b = tid; b < len; b += 256) V[b] = R[b];
		return;
	}
	const uint64_t s = sp.seed ^ 0x2545F4914F6CDD1DULL, S = len / n;
	const uint64_t e0 = n * tid / 256, e1 = n * (tid + 1) / 256;
	auto bounds = [&](uint64_t e, uint64_t& a, uint64_t& b) {
		a = e * S;
		b = e + 1 == n ? len : (e + 1) * S;
	};
	int64_t d = 0;
	for (uint64_t e = e0; e < e1; ++e) {
		uint64_t a, b;
		bounds(e, a, b);
		const ShiftEdit x = shift_edit(s, e, a, b, pct);
		d += x.kind == 1 ? (int64_t)x.k : (x.kind == 2 ? -(int64_t)x.k : 0);
	}
	part[tid] = d;
	__syncthreads();
	int64_t before = 0;
	for (uint32_t t = 0; t < tid; ++t) before += part[t];
	uint64_t o = (uint64_t)((int64_t)(e0 * S) + before);
	for (uint64_t e = e0; e < e1; ++e) {
		uint64_t a, b;
		bounds(e, a, b);
		const ShiftEdit x = shift_edit(s, e, a, b, pct);
		for (uint64_t p = a; p < x.pos; ++p) V[o++] = R[p];
		if (x.kind == 1) {
			for (uint64_t j = 0; j < x.k; ++j) V[o++] = (uint8_t)(x.bytes >> (8 * j));
			for (uint64_t p = x.pos; p < b; ++p) V[o++] = R[p];
		} else if (x.kind == 2) {
			for (uint64_t p = x.pos + x.k; p < b; ++p) V[o++] = R[p];
		} else {
			V[o++] = (uint8_t)x.bytes;
			for (uint64_t p = x.pos + 1; p < b; ++p) V[o++] = R[p];
		}
	}
}

}  // namespace dg

// ───────────────────────────── launchers (C++ linkage, internal) ──────────

namespace dg {

hipError_t launch_synth_shift(uint8_t* ref, uint8_t* ver, const SynthSpan* spans, const uint64_t* v_off,
                              uint32_t n, uint64_t n_edits, uint32_t pct, hipStream_t st) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(synth_stream_kernel, dim3(64, n), dim3(256), 0, st, ref, spans, n);
	hipLaunchKernelGGL(synth_shift_kernel, dim3(n), dim3(256), 0, st, ver, ref, spans, v_off, n, n_edits, pct);
	return hipGetLastError();
}

hipError_t launch_synth_transpose(uint8_t* ref, uint8_t* ver, const SynthSpan* spans, uint32_t n_spans,
                                  const SynthCopy* cmds, uint32_t n_cmds, hipStream_t st) {
	if (n_spans) hipLaunchKernelGGL(synth_stream_kernel, dim3(64, n_spans), dim3(256), 0, st, ref, spans, n_spans);
	if (n_cmds) hipLaunchKernelGGL(synth_copy_kernel, dim3(n_cmds), dim3(256), 0, st, ver, ref, cmds, n_cmds);
	return hipGetLastError();
}

// One wave per pair (dg_serialize_wave.h): DPP scans instead of block
// barriers, 64 commands per tile staged in a 4 KiB LDS slice, so 32 pairs
// per CU are in flight and their record / payload loads overlap.  The CRC
// stream has joined before it, so it writes the header CRC bytes itself.
// (one record per lane per tile: 4 measured slower, C2 +18 %, C3 3.6x)
constexpr uint32_t kSerWaveStage = 4096;
constexpr uint32_t kSerWaveLds = kSerWaveStage + 32;

__global__ __launch_bounds__(64) void serialize_wave_kernel(SerArgs s) {
	__shared__ __attribute__((aligned(16))) uint8_t stage[kSerWaveLds];
	const uint32_t pair = blockIdx.x;
	const uint64_t base = s.offsets[pair];
	const uint64_t end = s.offsets[pair + 1];
	if (end > s.out_cap) {
		if (lane_id() == 0) s.status[pair] = 7;
		return;
	}
	if (s.status[pair] != 0) return;
	const PairDev pd = s.pairs[pair];
	const PairPlanDev pp = s.pplan[pair];
	const int32_t st = serialize_wave<kSerWaveStage>(s.out + base, end - base, s.ver + pd.v_off, (uint32_t)pd.v_len,
	                                                 s.rec + (uint64_t)s.rec_words * pp.rec_base, s.rec_words,
	                                                 s.n_rec[pair], (sw_lds8*)stage);
	if (st != 0 && lane_id() == 0) s.status[pair] = st;
	if (st == 0) {   // header bytes 9..24: CRC of R, CRC of V, big-endian (encoding.c:52-54)
		const uint32_t lane = lane_id();
		if (lane < 16) {
			const uint64_t c = s.crc[2ull * pair + (lane >> 3)];
			s.out[base + 9 + lane] = (uint8_t)(c >> (56 - 8 * (lane & 7)));
		}
	}
}

// header bytes 9..24 (src/dst CRC, big-endian, encoding.c:52-54) of deltas
// serialised before their CRCs were known (member plans)
__global__ __launch_bounds__(256) void crc_patch_kernel(uint8_t* out, const uint64_t* offsets,
                                                        const uint64_t* crc, const int32_t* status,
                                                        uint32_t n) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || status[i] != 0) return;
	uint8_t* h = out + offsets[i];
	const uint64_t cs = crc[2ull * i], cd = crc[2ull * i + 1];
	for (int k = 0; k < 8; ++k) {
		h[9 + k] = (uint8_t)(cs >> (56 - 8 * k));
		h[17 + k] = (uint8_t)(cd >> (56 - 8 * k));
	}
}

hipError_t launch_crc_patch(uint8_t* out, const uint64_t* offsets, const uint64_t* crc,
                            const int32_t* status, uint32_t n, hipStream_t st) {
	if (n) hipLaunchKernelGGL(crc_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out, offsets, crc, status, n);
	return hipGetLastError();
}

hipError_t launch_scan(const uint64_t* sz, uint64_t* off, uint32_t n, hipStream_t st, uint32_t* route_cnt,
                       uint32_t* route_fb) {
	hipLaunchKernelGGL(scan_sizes_kernel, dim3(1), dim3(1024), 0, st, sz, off, n, route_cnt, route_fb);
	return hipGetLastError();
}

hipError_t launch_serialize_wave(const SerArgs& s, hipStream_t st) {
	if (s.n_pairs == 0) return hipSuccess;
	hipLaunchKernelGGL(serialize_wave_kernel, dim3(s.n_pairs), dim3(64), 0, st, s);
	return hipGetLastError();
}

// overlap_cap: grid cap when the CRC runs beside another kernel (0 = none).
// A grid-stride CRC of 2 blocks per CU leaves the co-running kernel its
// issue slots instead of queueing 32 CRC waves per CU behind it (C2: step
// 0.400 -> 0.372 ms).  DG_CRC_BLOCKS overrides (A/B builds only).
hipError_t launch_crc_wide(const CrcArgs& a, uint32_t n_cu, hipStream_t st) {
	if (a.n_segs) {
		const uint32_t blocks = std::min<uint32_t>(n_cu, (a.n_segs + 15) / 16);
		hipLaunchKernelGGL(crc_rows_wide_kernel<kCrcWideBlock>, dim3(blocks), dim3(kCrcWideBlock), 0, st, a);
	}
	if (a.n_spans)
		hipLaunchKernelGGL(crc_finalize_kernel, dim3((a.n_spans + 63) / 64), dim3(64), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_crc_finalize(const CrcArgs& a, hipStream_t st) {
	if (a.n_spans) hipLaunchKernelGGL(crc_finalize_kernel, dim3((a.n_spans + 63) / 64), dim3(64), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_crc(const CrcArgs& a, hipStream_t st, uint32_t overlap_cap, int pass, bool finalize) {
	if (a.n_segs) {
		uint32_t blocks = (a.n_segs + kCrcWavesPerBlock - 1) / kCrcWavesPerBlock;
		static const uint32_t env_cap = [] {
			const char* e = ab_env("DG_CRC_BLOCKS");
			return e ? (uint32_t)strtoul(e, nullptr, 0) : 0u;
		}();
		const uint32_t cap = env_cap ? env_cap : overlap_cap;
		if (cap && blocks > cap) blocks = cap;
		if (pass == kCrcPassRows5)
			hipLaunchKernelGGL(crc_rows_kernel<kCrcFive>, dim3(blocks), dim3(64 * kCrcWavesPerBlock), 0, st, a);
		else
			hipLaunchKernelGGL(crc_rows_kernel<kCrcByte>, dim3(blocks), dim3(64 * kCrcWavesPerBlock), 0, st, a);
	}
	if (finalize) return launch_crc_finalize(a, st);
	return hipGetLastError();
}

hipError_t launch_synth(uint8_t* ref, uint8_t* ver, uint32_t n_pairs, uint64_t pair_len,
                        uint64_t seed_base, uint64_t n_edits, hipStream_t st) {
	const uint64_t words = (uint64_t)n_pairs * ((pair_len + 7) / 8);
	if (words)
		hipLaunchKernelGGL(synth_random_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st,
		                   ref, ver, pair_len, seed_base, words);
	if (n_edits && n_pairs)
		hipLaunchKernelGGL(synth_edits_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, ver,
		                   n_pairs, pair_len, seed_base, n_edits);
	return hipGetLastError();
}

}  // namespace dg

// ───────────────────────────── decode + apply ─────────────────────────────
//
// One wave per delta stream (src/c/encoding.c:111-178 parse,
// src/c/apply.c:229-284 apply).  Lane 0 parses command headers out of an LDS
// window of the stream; commands are applied in batches of up to 64, one per
// lane, when no command of the batch touches bytes another one (earlier in
// stream order) reads or writes; otherwise the batch is replayed strictly in
// order with a wave-wide memmove per command.  Either way the result equals
// the reference's sequential memcpy/memmove replay.  All offsets are bounds
// checked (the reference does not check, apply.c:236-243).
// The parser's and the apply's device functions are in dg_decode_dev.h.

#include "dg_decode_dev.h"

namespace dg {

__global__ __launch_bounds__(kDecBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void decode_kernel(DecodeArgs a) {
	const uint32_t i = blockIdx.x;
	if (i >= a.n) return;
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
	__shared__ DecLdsMem M;
	__shared__ uint64_t cpart[2][kDecWaves];   // crc_check: per span, each wave's Horner partial
	__shared__ uint32_t clast[2][kDecWaves];   // and its last segment
	const DecLds L = dec_lds(M);

#ifdef DG_ONEPASS_PROF
	uint64_t dprof[kDecProfN] = {};
	const uint64_t t_start = __builtin_amdgcn_s_memtime();
#endif
	const dg_decode_desc_dev dd = a.descs[i];
	const uint8_t* D = a.delta + dd.delta_off;
	const uint64_t dl = dd.delta_len;
	const uint8_t* R = a.ref + dd.ref_off;
	const uint64_t rl = dd.ref_len;
	uint8_t* O = a.out + dd.out_off;

	int32_t st = 0;
	uint64_t vsize = 0;
	if (bad_magic(D, dl)) st = 8;
	bool inplace = false;
	if (!st) {
		inplace = D[4] & 1;
		vsize = be32(D + 5);
	}
	const uint64_t bsz = inplace ? max(rl, vsize) : vsize;
	if (!st && bsz > dd.out_cap) st = 7;
	if (st) {
		if (tid == 0) {
			a.status[i] = st;
			a.out_len[i] = 0;
			}
		return;
	}
	// initial image: R then zeros (in-place, apply.c:276-278) or zeros (apply.c:233)
	const uint64_t init = inplace ? (rl < bsz ? rl : bsz) : 0;
	// R's CRC-64/XZ from the loads that make the in-place image (R is read
	// once): 16 KiB segments as rows of 64 x 8 bytes, segment j on wave j % 4,
	// each wave folding its segments Horner-wise; the image's whole 16-byte
	// words are stored from the same pieces
	const bool aligned_or = (((uintptr_t)O | (uintptr_t)R) & 15) == 0;
	const bool rcrc_early = a.crc_check && aligned_or && rl >= 8;
	uint64_t racc = 0;
	uint32_t rlast = ~0u;
	DPROF_T(tf0);
	if (rcrc_early) {
		const DecCrc ct = dec_crc_tables(M.NX, a);
		__syncthreads();
		const uint32_t nseg = crc_nseg((uintptr_t)R, rl, kDecCrcSeg);
		const uintptr_t copy_hi = (uintptr_t)R + init / 16 * 16;
		for (uint32_t j = wave; j < nseg; j += kDecWaves) {
			const uint64_t c = dec_seg_crc<true>(ct, (uintptr_t)R, rl, nseg, j, (intptr_t)O - (intptr_t)R, copy_hi);
			racc = (rlast != ~0u ? mul_nib(racc, ct.TK) : 0ull) ^ c;
			rlast = j;
		}
		__syncthreads();   // the tables' LDS is the parse's next
	}
	{
		uint64_t k0 = 0;
		if (aligned_or) {   // 16 B per thread, 4 in flight
			const uint64_t n16 = init / 16;
			const uint64_t ncopy = rcrc_early ? 0 : n16;   // (else made with R's CRC above)
			for (uint64_t b = 0; b < ncopy; b += 4 * kDecBlock) {
				typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
				u32x4 x[4];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const uint64_t q = b + kDecBlock * u + tid;
					x[u] = q < n16 ? reinterpret_cast<const u32x4*>(R)[q] : u32x4{0, 0, 0, 0};
				}
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const uint64_t q = b + kDecBlock * u + tid;
					if (q < n16) reinterpret_cast<u32x4*>(O)[q] = x[u];
				}
			}
			const uint64_t z0 = (init + 15) / 16, z1 = bsz / 16;   // whole zero words [z0, z1)
			for (uint64_t q = z0 + tid; q < z1; q += kDecBlock) reinterpret_cast<uint4*>(O)[q] = make_uint4(0, 0, 0, 0);
			for (uint64_t k = n16 * 16 + tid; k < z0 * 16 && k < bsz; k += kDecBlock) O[k] = k < init ? R[k] : 0;
			k0 = (z1 > z0 ? z1 : z0) * 16;
		}
		for (uint64_t k = k0 + tid; k < bsz; k += kDecBlock) O[k] = k < init ? R[k] : 0;
	}
	block_sync_global();   // every wave's image stores complete before any command load or store
	DPROF_ADD(DP_FILL, tf0);

	uint64_t pos = 25;   // stream offset of the current window: a command boundary
	bool done = false;
	while (!done && !st) {
		if (pos >= dl) break;   // missing END: end of input (as the reference's loop)
		// ── 1-5. the window: load, command chain, bounds and order checks ──
		const DecWin W = dec_window(L, D, dl, pos, inplace, bsz, inplace ? bsz : rl, DPROF_HOOK);
		const uint8_t* w = M.win + W.shf;
		const uint32_t cnt = W.cnt, nb = (cnt + 63) / 64;
		done = W.done;
		if (W.bad) st = 8;
		DPROF_T(tc0);
		// ── 6. apply ──
		if (!st) {
			if (W.free_win) {
				for (uint32_t b = wave; b < nb; b += kDecWaves) {
					DPROF_INC(DP_BATCHES);
					DPROF_T(tq0);
					const DecCmd c = dec_cmd(w, M.cmds, 64 * b, cnt, pos);
#ifdef DG_ONEPASS_PROF
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
					DPROF_ADD(DP_C_CMD, tq0);
					DPROF_T(tq1);
					dec_flat_batch(c, inplace, O, R, D, L.xs);
					DPROF_ADD(DP_C_FLAT, tq1);
				}
			} else {
				dec_grouped_window(w, M.cmds, cnt, pos, inplace, O, R, D, L.grp);
			}
		}
		DPROF_T(tq2);
		block_sync_global();   // the window's stores complete before the next window
		DPROF_ADD(DP_C_BAR, tq2);
		DPROF_ADD(DP_COPY, tc0);
		pos = W.next_pos;
	}
	// ── 7. CRC-64/XZ of R and of the output, checked against the header
	//    (main.c:341-356 before the apply, :376-385 after; a source mismatch
	//    takes precedence, the output is then unspecified).  Segments of
	//    16 KiB (256-byte lanes: a quarter of the encode CRC's serial chain
	//    per lane, every wave busy on a 64 KiB stream); segment j of a span
	//    goes to wave j % 4, which folds its segments Horner-wise by
	//    x^(8 * 64 KiB); thread 0 shifts the partials into place. ──
	int32_t cst = 0;
	if (a.crc_check && !st) {
		DPROF_T(tk0);
		block_sync_global();   // every wave's output stores before any CRC read
		DPROF_ADD(DP_CRC_SYNC, tk0);
		DPROF_T(tk1);
		const uint64_t* Lv = a.tables + 8 * 256;
		const uint64_t* KF = Lv + kCrcLevels * kCrcNibTabWords;   // x^(8 seg), x^(-8t), x^(8 seg k) k = 2..4
		// LDS (the dead doubling arrays): the row tables and x^(8 * 64 KiB);
		// 16 KiB segments read as rows of 64 x 8 bytes (coalesced)
		const DecCrc ct = dec_crc_tables(M.NX, a);
		const uint64_t* TK = ct.TK;
		__syncthreads();
		const uintptr_t sa[2] = {(uintptr_t)R, (uintptr_t)O};
		const uint64_t sl[2] = {rl, vsize};
#pragma unroll
		for (int sp = 0; sp < 2; ++sp) {
			uint64_t acc = 0;
			uint32_t last = ~0u;
			if (sp == 0 && rcrc_early) {   // R's, from the fill
				acc = racc;
				last = rlast;
			} else if (sl[sp] >= 8) {
				const uint32_t nseg = crc_nseg(sa[sp], sl[sp], kDecCrcSeg);
				for (uint32_t j = wave; j < nseg; j += kDecWaves) {
					const uint64_t c = dec_seg_crc(ct, sa[sp], sl[sp], nseg, j);
					acc = (last != ~0u ? mul_nib(acc, TK) : 0ull) ^ c;   // TK: x^(8 * 64 KiB) = 4 segments
					last = j;
				}
			}
			if (lane == 0) {
				cpart[sp][wave] = acc;
				clast[sp][wave] = last;
			}
		}
		__syncthreads();
		DPROF_ADD(DP_CRC_SEG, tk1);
		DPROF_T(tk2);
		// Wave 0 combines, one lane per (span, wave) partial: the shifts
		// x^(8 * 16 KiB * k) run side by side (one gather round, not eight in
		// a row on thread 0), then the two spans' pad fixes side by side.
		if (wave == 0) {
			const uint32_t sp = lane / kDecWaves, w2 = lane % kDecWaves;
			uint64_t v = 0;
			if (lane < 2 * kDecWaves && sl[sp] >= 8 && clast[sp][w2] != ~0u) {
				const uint32_t k = crc_nseg(sa[sp], sl[sp], kDecCrcSeg) - 1 - clast[sp][w2];   // 0..3 segments after its last
				v = cpart[sp][w2];
				if (k)
					v = mul_nib(v, k == 1 ? Lv + 4 * kCrcNibTabWords      // x^(8 * 16 KiB)
					               : k == 2 ? Lv + 5 * kCrcNibTabWords    // x^(8 * 32 KiB)
					                        : KF + kCrcFinX48K * kCrcNibTabWords);
			}
			const uint64_t raw0 = wave_xor64(lane < kDecWaves ? v : 0ull);
			const uint64_t raw1 = wave_xor64(lane >= kDecWaves && lane < 2 * kDecWaves ? v : 0ull);
			bool bad = false;
			if (lane < 2) {   // lane s: span s (0 = R, 1 = output)
				const uintptr_t s0 = lane ? sa[1] : sa[0];
				const uint64_t len = lane ? sl[1] : sl[0];
				uint64_t c;
				if (len < 8) {
					const uint8_t* d = reinterpret_cast<const uint8_t*>(s0);
					c = ~0ULL;
					for (uint64_t k = 0; k < len; ++k) c = a.tables[(uint8_t)(c ^ d[k])] ^ (c >> 8);
				} else {
					c = lane ? raw1 : raw0;
					const uintptr_t end = s0 + len;
					const uint32_t t = (uint32_t)(((end + 15) & ~(uintptr_t)15) - end);
					if (t) c = mul_nib(c, KF + (1 + t) * kCrcNibTabWords);   // undo the trailing pad
				}
				uint64_t h = 0;
				for (int k = 0; k < 8; ++k) h = (h << 8) | D[9 + 8 * lane + k];
				bad = h != ~c;
			}
			const uint64_t bm = __ballot(bad);
			cst = bm & 1 ? 9 : (bm & 2 ? 10 : 0);
		}
		DPROF_ADD(DP_CRC_TAIL, tk2);
	}
	if (tid == 0) {
		a.status[i] = st ? st : cst;
		a.out_len[i] = st ? 0 : vsize;
	}
#ifdef DG_ONEPASS_PROF
	{
		DPROF_T(tw9);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		DPROF_ADD(DP_WAIT, tw9);
		dprof[DP_TOTAL] = __builtin_amdgcn_s_memtime() - t_start;
		if (tid == 0)
			for (int k = 0; k < kDecProfN; ++k) atomicAdd(&g_decode_prof[k], (unsigned long long)dprof[k]);
	}
#endif
}

hipError_t launch_decode(const DecodeArgs& a, hipStream_t st) {
	if (a.n) hipLaunchKernelGGL(decode_kernel, dim3(a.n), dim3(kDecBlock), 0, st, a);
	return hipGetLastError();
}

}  // namespace dg
