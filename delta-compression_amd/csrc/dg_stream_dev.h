// dg_stream_dev.h — what the kernels that read and write whole delta streams
// share (decode, update, in-place, compose, invert): the stream magic, big-endian
// fields, unaligned access types, the lane-owned command header of the parser's
// window (dg_parse_chain.h), wave scans and shuffles, and the emit kernels' wave
// copy.  Device code only.
#pragma once
#include <stdint.h>

#include "dg_devutil.h"

namespace dg {

// unaligned dword / 16-byte accesses (gfx950 global memory allows them)
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));

constexpr uint32_t kSmallCopy = 64;   // emit: spans up to this many bytes are one thread's

// orders LDS and global memory between the lanes of a wave
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t be32(const uint8_t* p) {
	return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// not a DLT\x03 stream: shorter than the 25-byte header, or another magic
__device__ __forceinline__ bool bad_magic(const uint8_t* S, uint64_t len) {
	return len < 25 || S[0] != 'D' || S[1] != 'L' || S[2] != 'T' || S[3] != 3;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t x) {
	p[0] = (uint8_t)(x >> 24);
	p[1] = (uint8_t)(x >> 16);
	p[2] = (uint8_t)(x >> 8);
	p[3] = (uint8_t)x;
}

// exclusive prefix of x over the wave as 64 bits, and the wave's total
__device__ __forceinline__ uint64_t wave_excl_scan64(uint32_t x, uint64_t* total) {
	const uint32_t lo = wave_incl_scan(x & 0xFFFFu), hi = wave_incl_scan(x >> 16);
	*total = ((uint64_t)rdlane(hi, 63) << 16) + rdlane(lo, 63);
	return ((uint64_t)hi << 16) + lo - x;
}

// 1 + the nearest earlier lane whose flag is set, 0 when there is none
__device__ __forceinline__ uint32_t prev_set(bool f, uint32_t lane) {
	return wave_shr1z(wave_incl_max(f ? lane + 1u : 0u));
}
// 1 + the last lane whose flag is set, 0 when there is none (uniform)
__device__ __forceinline__ uint32_t last_set(bool f) {
	const uint64_t m = __ballot(f);
	return m ? 64u - (uint32_t)__builtin_clzll(m) : 0u;
}
__device__ __forceinline__ uint32_t shfl32(uint32_t x, uint32_t l) { return (uint32_t)__shfl((int)x, (int)(l & 63u), 64); }
__device__ __forceinline__ uint64_t shfl64(uint64_t x, uint32_t l) {
	return ((uint64_t)shfl32((uint32_t)(x >> 32), l) << 32) | shfl32((uint32_t)x, l);
}

// one command's fields, decoded from the parser's window by its lane
struct Hdr {
	uint32_t cx, kind, src, dst, len;
};
__device__ __forceinline__ Hdr decode_hdr(const uint8_t* win, const uint16_t* cmds, uint32_t k, bool mine) {
	Hdr h{0, 0, 0, 0, 0};
	if (mine) {
		h.cx = cmds[k];
		h.kind = win[h.cx];
		if (h.kind == 1) {
			h.src = be32(win + h.cx + 1);
			h.dst = be32(win + h.cx + 5);
			h.len = be32(win + h.cx + 9);
		} else {
			h.dst = be32(win + h.cx + 1);
			h.len = be32(win + h.cx + 5);
		}
	}
	return h;
}

// n bytes by one wave; src and dst do not overlap
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
	const uint32_t n16 = n >> 4;
	for (uint32_t j = lane; j < n16; j += 64)
		*reinterpret_cast<u32x4_u*>(dst + 16 * j) = *reinterpret_cast<const u32x4_u*>(src + 16 * j);
	const uint32_t t = 16 * n16 + lane;
	if (t < n) dst[t] = src[t];
}

// (The emit kernels' tail, "spans up to kSmallCopy by their lane, longer ones
// by the whole wave in ballot order", stays written out in both: as a function
// here it changes the instructions the compiler emits for them.)

}  // namespace dg
