// dg_layout.h — the constants and plain-data records that the kernels and the
// host plan code share.  No HIP types: dg_plan.cpp includes this file and is
// compiled by a plain C++ compiler; dg_device.h adds the kernel argument
// structs and the launchers.
#pragma once
#include <stdint.h>

namespace dg {

constexpr uint64_t kMersenne = (1ULL << 61) - 1;   // src/c/delta.h:25
constexpr uint64_t kBase = 263;                    // src/c/delta.h:24
constexpr uint64_t kCrcPoly = 0xC96C5795D7870F42ULL;  // reflected, delta.h:303
constexpr uint32_t kSentinel = 0xFFFFFFFFu;        // "no slot" (q < 2^32 - 1)

// CRC segmentation: one wave64 per 64 KiB segment (dg_crc.h).  Segments tile
// a span from its (16-byte aligned-up) end backwards.
constexpr uint32_t kCrcSegBytes = 65536;
constexpr uint32_t kCrcWavesPerBlock = 4;

// Onepass register history: chunks of 64 steps kept in VGPRs before the
// epoch spills into the global table tier.  Round 3 A/B (same box, plain
// chain 90/94/96 VGPRs, no scratch, 5 waves/SIMD for 5/6/7): c3s 54 / 76 /
// 105 / 105 GiB/s at 4/5/6/7 chunks, C2 and C3 unchanged; 8 spills.
#ifndef DG_HIST_CHUNKS   // tuning knob (make variant)
#define DG_HIST_CHUNKS 6
#endif
constexpr int kHistChunks = DG_HIST_CHUNKS;

struct PairDev {          // == dg_pair_t
	uint64_t r_off, r_len, v_off, v_len;
};

struct PairPlanDev {
	uint64_t q;            // table size for this pair (onepass.c:61-62)
	uint64_t q_magic;      // floor((2^64-1)/q), Barrett
	uint64_t rec_base;     // first record slot
	uint32_t rec_cap;      // record capacity (>= #copies possible)
	uint32_t pad;
	// correcting only (correcting.c:116-136)
	uint64_t f_size, f_magic;  // |F| and floor((2^64-1)/|F|)
	uint64_t m, m_magic;       // checkpoint modulus and Barrett
	uint64_t tab_base;         // first entry of this pair's R index (correcting)
	// greedy (dg_greedy.hip) keeps its index geometry in the same words: q = 0,
	// f_size = bucket count (a power of two), tab_base = first word of the
	// pair's heads (f_size + 1 words), m = first of its |R| - p + 1 entries
	// onepass member mode (dg_members.hip)
	uint64_t mem_base;         // first member slot (n_chunks x kMemChunkSlots slots)
	uint32_t chunk_base;       // first chunk (index into the per-chunk member counts)
	uint32_t n_chunks;         // chunks of kMemChunk positions covering [0, min(|R|,|V|)]
	// correcting, CRC of R in the build: x^(-8 pad), pad = |R| rounded up to
	// 32 KiB minus |R| (the build's zero padding)
	uint64_t crc_unpad;
};

struct CrcSegDev {        // one wave's CRC segment
	uint32_t span;         // span index
	uint32_t j;            // segment index within the span (0 = first)
};

struct CrcSpanDev {
	uint64_t off, len;     // byte range in the arena
	uint32_t seg_base;     // first segment index
	uint32_t nseg;         // number of segments (0 for len < 8)
	uint32_t which;        // arena selector: 0 = reference arena, 1 = version arena
	uint32_t out;          // index of its CRC in CrcArgs::out
};

// Precomputed GF(2) constants for the CRC combine steps, as nibble tables:
// tab[c][16*j + n] = (n << 4j) * K_c mod P  (reflected), see crc_tables_build
// (dg_plan.cpp).
// Level l = x^(8 * 1024 * 2^l): 16 and 32 KiB are the decode kernel's segment
// combines, 32 KiB the correcting build's piece stride.
constexpr int kCrcLevels = 6;
constexpr int kCrcNibTabWords = 256;   // 16 nibbles x 16 values
// after the level tables (F): x^(8 kCrcSegBytes), x^(-8t) for t = 0..15,
// x^(8 kCrcSegBytes k) for k = 2..4, then for the decode kernel's 256-byte
// lanes x^(8 * 256), x^(8 * 512) (its first two tree levels) and x^(8 * 48 KiB)
constexpr int kCrcFinTabs = 1 + 16 + 3 + 3;
constexpr int kCrcFinX256 = 20, kCrcFinX512 = 21, kCrcFinX48K = 22;   // indices in F
// after F: the row-interleaved segment tables (dg_crc.h crc_seg_rows): for
// 16- and 8-byte pieces, U_j = T advanced by (64 PB - 1 - j) bytes (16 and 8
// tables of 256), then the per-lane constants x^(-8 PB l), l = 0..63, for PB
// = 16, 8; then the five-bit row tables F_k[v] = Z^n(v << 5k), k = 0..12, 32
// entries (256 B: one LDS row, so a 32-lane ds_read_b64 group never
// conflicts) -- for 8-byte pieces n = 512; for 16-byte pieces n = 1024 on
// (A ^ low 8 bytes), then 13 more with n = 1016 on the high 8 bytes
constexpr uint32_t kCrcRowsOff = 8 * 256 + (kCrcLevels + kCrcFinTabs) * kCrcNibTabWords;
constexpr uint32_t kCrcRows16 = kCrcRowsOff, kCrcRows8 = kCrcRowsOff + 16 * 256;
constexpr uint32_t kCrcRowK16 = kCrcRowsOff + 24 * 256, kCrcRowK8 = kCrcRowK16 + 64;
constexpr uint32_t kCrc5Tabs8 = 13, kCrc5Tabs16 = 26;
constexpr uint32_t kCrc5R8 = kCrcRowK8 + 64, kCrc5R16 = kCrc5R8 + 32 * kCrc5Tabs8;
constexpr uint32_t kCrcTabWords = kCrc5R16 + 32 * kCrc5Tabs16;

constexpr uint32_t kSegTail = 0xFFFFFFFFu;

// Speculative diagonal members of the onepass chain (dg_members.hip): one
// wave per chunk of kMemChunk positions, with kMemAhead bytes of look-ahead
// staged for the members that end past the chunk.  Members start >= p = 16
// bytes apart, so a chunk holds at most kMemChunk / 16 of them.
constexpr uint32_t kMemChunk = 2048;
constexpr uint32_t kMemAhead = 240;    // staged: [chunk - 16, chunk + 2048 + 240) = 2304 B
constexpr uint32_t kMemChunkSlots = kMemChunk / 16 + 1;

// COPY records: (v, r, len) u32 words, and for onepass a 4th word holding the
// first 4 bytes of V from the gap start (the end of the previous COPY), so a
// gap of <= 4 bytes serialises without reading V (at C2 nearly every ADD).
constexpr uint32_t kRecWordsOnepass = 4;
constexpr uint32_t kRecWordsCorrecting = 3;

struct SynthSpan {   // synthetic R stream: splitmix64(seed) words at off
	uint64_t off, len, seed;
};
struct SynthCopy {   // V[dst..+len) = R[src..+len)
	uint64_t dst, src, len;
};

}  // namespace dg
