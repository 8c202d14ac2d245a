// The bit buffer of the two Huffman coders that write JPEG entropy-coded segments (ITU-T T.81 F.1.2.3): jpeg.hip (baseline DCT) and dng.hip
// (lossless, process 14).  One wave owns one buffer in LDS.  A lane holds up to 59 bits of code, MSB first; a wave prefix sum of the lengths
// gives every lane its bit offset; the lanes OR their bits into the buffer (ds_or_b32); the buffer's complete bytes are then taken 64 at a
// time -- __ballot(byte == 0xFF) and a population count give each byte its place behind the stuffed zeros -- and the (up to 7) bits left
// over start the next round.  The callers keep the barriers between the steps, which differ (jpeg.hip pads inside a round).
#pragma once
#include "common.hpp"

namespace rc {

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {     // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// The low n bits of `bits` (1 <= n <= 59; zero above them), MSB first, at bit `off` of the buffer bb[0 .. words).
__device__ __forceinline__ void bits_or(uint32_t* bb, int words, int off, uint64_t bits, int n) {
    const int w = off >> 5, s = off & 31;
    const uint64_t v = bits << (64 - n), v0 = v >> s;
    const uint32_t w0 = (uint32_t)(v0 >> 32), w1 = (uint32_t)v0, w2 = s ? (uint32_t)v << (32 - s) : 0u;
    if (w + 2 < words) {
        if (w0) atomicOr(&bb[w], w0);
        if (w1) atomicOr(&bb[w + 1], w1);
        if (w2) atomicOr(&bb[w + 2], w2);
    }
}

// The segment ends behind `total` bits: 1-bits up to the next byte.  Returns the new total.
__device__ __forceinline__ int bits_pad_ones(uint32_t* bb, int total, int lane) {
    if (total & 7) {
        const int pad = 8 - (total & 7);
        if (lane == 0) atomicOr(&bb[total >> 5], ((1u << pad) - 1u) << (32 - (total & 31) - pad));
        total += pad;
    }
    return total;
}

// After a barrier behind the ORs: the complete bytes of the `total` bits leave the buffer -- with WRITE, to frame[base + out ..) clipped to
// cap, each 0xFF followed by a zero byte; `out` counts them either way -- and the incomplete byte moves to the front of the zeroed buffer.
// Returns the bits it holds (the next round's carry).  Ends with a barrier.
template <bool WRITE>
__device__ __forceinline__ int bits_flush(uint32_t* bb, int words, int total, int lane, uint8_t* frame, uint64_t cap, uint64_t base, uint32_t& out) {
    const uint64_t below = (1ull << lane) - 1ull;
    const int nb = total >> 3;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane;
        const bool act = j < nb;
        const uint32_t byte = act ? (bb[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu : 0u;
        const bool ff = byte == 0xffu;
        const uint64_t fm = __ballot(ff);
        if (WRITE && act) {
            const uint64_t pos = base + out + (uint32_t)lane + (uint32_t)__popcll(fm & below);
            if (pos < cap) frame[pos] = (uint8_t)byte;
            if (ff && pos + 1 < cap) frame[pos + 1] = 0;
        }
        out += (uint32_t)min(64, nb - j0) + (uint32_t)__popcll(fm);
    }
    const uint32_t left = (bb[nb >> 2] >> (24 - 8 * (nb & 3))) & 0xffu;        // the incomplete byte (zero bits behind its carry bits)
    __syncthreads();
    for (int i = lane; i <= (total >> 5) && i < words; i += 64) bb[i] = i == 0 ? left << 24 : 0u;
    __syncthreads();
    return total & 7;
}

}  // namespace rc
