// The map and the integer tail of the two pyramid kernels -- motion.hip's motion_pyramid_kernel (the luma code of the planar result) and
// temporal_mc.hip's raw_pyramid_kernel (the luma proxy of a mosaic's Bayer cells).  A lane owns a 4 x 4 tile of level-0 pixels: sixteen
// level-0 bytes, four level-1 bytes, one level-2 byte; a wave is 16 x 4 lanes (64 x 16 pixels), so the level-3 byte of a 2 x 2 group of
// lanes is two lane exchanges (lane ^ 1, lane ^ 16) and the lane with both bits clear stores it.  A block is four waves side by side
// (256 x 16 pixels).  Level 0 goes out as one dword per row and lane, level 1 as one 16-bit store per row where the level's rows keep that
// alignment, bytes otherwise.  A kernel forms its sixteen codes and calls pyramid_tail; everything from there on is integer.
#pragma once
#include "common.hpp"

namespace rc {

constexpr int kPyrWaves = 4, kPyrThreads = 64 * kPyrWaves, kPyrLanesX = 16, kPyrTile = 4;
constexpr int kPyrBlockW = kPyrWaves * kPyrLanesX * kPyrTile, kPyrBlockH = (64 / kPyrLanesX) * kPyrTile;   // pixels per block

// The tile (tx, ty) of a lane: where a block's waves and a wave's lanes lie.
__device__ __forceinline__ int pyramid_tx(int lane) { return (blockIdx.x * kPyrWaves + (threadIdx.x >> 6)) * kPyrLanesX + (lane & (kPyrLanesX - 1)); }
__device__ __forceinline__ int pyramid_ty(int lane) { return blockIdx.y * (64 / kPyrLanesX) + (lane >> 4); }

// Levels 0 .. a.levels - 1 of tile (tx, ty) of frame `frame` from its level-0 codes q (0 outside the frame: never stored).  A: a kernel's
// arguments -- lv[k] (B, h >> k, w >> k), levels, h, w, and vec0 / vec1: every row of level 0 starts on a dword, of level 1 on a 16-bit
// boundary.  The last thing a kernel does: the returns on `levels` are wave-uniform, so every lane reaches the exchanges.
template <typename A>
__device__ __forceinline__ void pyramid_tail(const A& a, int frame, int lane, int tx, int ty, const uint32_t (&q)[kPyrTile][kPyrTile]) {
    const int x0 = tx * kPyrTile, y0 = ty * kPyrTile, cnt = a.w - x0;                           // cnt <= 0: the tile is right of the frame
    {   // level 0: (B, h, w)
        uint8_t* o = a.lv[0] + ((size_t)frame * a.h + y0) * a.w + x0;
#pragma unroll
        for (int r = 0; r < kPyrTile; ++r) {
            if (y0 + r < a.h && cnt > 0) {
                uint8_t* p = o + (size_t)r * a.w;
                if (a.vec0 && cnt >= kPyrTile) {
                    *reinterpret_cast<uint32_t*>(p) = q[r][0] | (q[r][1] << 8) | (q[r][2] << 16) | (q[r][3] << 24);
                } else {
#pragma unroll
                    for (int k = 0; k < kPyrTile; ++k)
                        if (k < cnt) p[k] = (uint8_t)q[r][k];
                }
            }
        }
    }
    if (a.levels < 2) return;
    uint32_t q1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) q1[r][k] = (q[2 * r][2 * k] + q[2 * r][2 * k + 1] + q[2 * r + 1][2 * k] + q[2 * r + 1][2 * k + 1] + 2u) >> 2;
    {   // level 1: (B, h >> 1, w >> 1); a pixel that exists has its four sources inside the frame
        const int h1 = a.h >> 1, w1 = a.w >> 1, c1 = w1 - 2 * tx;
        uint8_t* o = a.lv[1] + ((size_t)frame * h1 + 2 * ty) * w1 + 2 * tx;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (2 * ty + r < h1 && c1 > 0) {
                uint8_t* p = o + (size_t)r * w1;
                if (a.vec1 && c1 >= 2) {
                    *reinterpret_cast<uint16_t*>(p) = (uint16_t)(q1[r][0] | (q1[r][1] << 8));
                } else {
                    p[0] = (uint8_t)q1[r][0];
                    if (c1 >= 2) p[1] = (uint8_t)q1[r][1];
                }
            }
        }
    }
    if (a.levels < 3) return;
    const uint32_t q2 = (q1[0][0] + q1[0][1] + q1[1][0] + q1[1][1] + 2u) >> 2;
    {
        const int h2 = a.h >> 2, w2 = a.w >> 2;
        if (ty < h2 && tx < w2) a.lv[2][((size_t)frame * h2 + ty) * w2 + tx] = (uint8_t)q2;
    }
    if (a.levels < 4) return;                                                                   // wave-uniform: every lane reaches the exchanges
    uint32_t s = q2 + (uint32_t)__shfl_xor((int)q2, 1);
    s += (uint32_t)__shfl_xor((int)s, kPyrLanesX);
    {
        const int h3 = a.h >> 3, w3 = a.w >> 3;
        if (!(lane & 1) && !(lane & kPyrLanesX) && (ty >> 1) < h3 && (tx >> 1) < w3)
            a.lv[3][((size_t)frame * h3 + (ty >> 1)) * w3 + (tx >> 1)] = (uint8_t)((s + 2u) >> 2);
    }
}

}  // namespace rc
