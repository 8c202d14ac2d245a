// Frame statistics (include/realcam_hip.h, rc_frame_stats): the planar result (B,3,H,W), cropped to the frame (h,w), read once ->
// hist (B,4,2^bits) and zones (B,gy,gx,8), int64: the R / G / B / Y code histograms and the 3A zone grid (valid / clipped / dark counts,
// colour sums, luma sum, focus energy) of a region of interest.  The one stage of the family that is a reduction, not a map.
//
// frame_stats_kernel: persistent blocks, grid (blocks per frame, frames).  A tile is 256 columns x 64 rows of the ROI; a block walks
// tiles t = blockIdx.x, + gridDim.x, ...; wave v of the block owns the tile's rows 16 v .. 16 v + 15 and walks DOWN them, a lane owning 4
// consecutive pixels of each row (one 8- or 16-byte load per plane and row where the source allows it).
//   codes     every sample is turned into its integer code once per row it is needed for: a wave computes row y + 1 before it accounts for
//             row y (dy needs qY below) and keeps it as the next row, so only the row under a wave's last one is computed twice (1 / 16,
//             out of L2: no second pass over HBM).  dx: qY of the pixel to the right is the lane's own next pixel, the next lane's first
//             (one DPP shuffle) or, for lane 63, three more samples of the tile to the right.
//   zones     a lane's 4 zone columns are fixed while it walks a tile (found once per tile by bisecting the 65 boundaries that the block
//             computes into LDS when it starts: no division per pixel); the zone ROW is wave-uniform and walked.  A lane sums its pixels'
//             8 slots in 4 x 8 32-bit registers down the rows; when the zone row changes or the tile ends the wave flushes: equal columns
//             of a lane merged, LDS 64-bit adds into the wave's own row of gx x 8 slots, then that row is swapped out (exchange with 0)
//             and its non-zero slots added to global memory with 64-bit atomics.
//   hist      one 4 x 2^bits table of 32-bit counters per block in LDS.  A lane run-length codes each channel across its pixels, tiles
//             included: an LDS add is issued only when the code changes, so a flat frame issues none until the end; flushed once per
//             block, non-zero bins only, with 64-bit global atomics.
// Widths (the bound of every partial is written where it is declared): everything after the codes is integer, so the order of the adds
// does not matter and the result is bit-exact and the same from run to run.
#include "rgb_strip.hpp"

namespace rc {

constexpr int kStatsPx = kRgbPx, kStatsWaves = 4, kStatsRows = 16, kStatsThreads = 64 * kStatsWaves;
constexpr int kStatsTileW = 64 * kStatsPx, kStatsTileH = kStatsWaves * kStatsRows;
constexpr int kStatsMaxBins = 1024, kStatsSlots = RC_STATS_SLOTS, kStatsGrid = RC_STATS_MAX_GRID;

struct StatsArgs {
    int W, plane;              // the source plane's row and its samples (< 2^29: three planes' offsets fit 32 bits)
    int org, rh, rw;           // the ROI inside it: its first sample y0 W + x0 and its size
    int gy, gx;
    int nbins, dark, clip;
    float fS;                  // float(S)
    Luma k;
    int ntx, ntiles, nblk;     // tiles per ROI row of tiles, tiles per frame, blocks per frame
    int vec;                   // every lane's 4 samples start on a 4-sample boundary of the source
};

struct StatsRow {
    uint32_t rgb[kStatsPx];    // qR | qG << 10 | qB << 20
    int y[kStatsPx];
    int yr;                    // qY of the pixel right of the lane's last one (meaningful where that pixel is inside the ROI)
};

__device__ __forceinline__ int stats_code(float v, float fS) {
    const float q = rintf(__fmul_rn(v, fS));                    // round half to even; v is in [0, 1 + a few ulp] and never NaN here
    return (int)__builtin_amdgcn_fmed3f(q, 0.f, fS);            // the clamp as one median: 16 codes' compare pairs would crowd the scalar registers
}

// float(S) and the luma coefficients
struct StatsCoef { float fS; Luma k; };

__device__ __forceinline__ int stats_luma(const StatsCoef& a, float r, float g, float b) {
    return stats_code(rgb_luma(a.k, r, g, b), a.fS);
}

// The codes of ROI row y for the lane's pixels px0 .. px0 + 3 (cnt = rw - px0 of them are inside the ROI; <= 0: none, and nothing is read).
// Called by the whole wave: the shuffle needs every lane.
template <typename TI>
__device__ __forceinline__ void stats_row(const StatsArgs& a, const StatsCoef& cf, const TI* __restrict__ frame, int y, int px0, int cnt, int cnt63, StatsRow& o) {
    const uint32_t plane = (uint32_t)a.plane, at = (uint32_t)a.org + (uint32_t)y * (uint32_t)a.W + (uint32_t)px0;
    float px[3][kStatsPx];
    // One branch for the three planes, and the element path written out with its index formed in 32 bits: through rgb_load the offsets
    // k fold into the loads' immediates, the whole kernel is scheduled differently (95 / 96 VGPRs, 77 instructions fewer) and runs 14 to
    // 19 % slower on 4K frames (profiles/output_strip_refactor.md).
    if (cnt >= kStatsPx && a.vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb_load<TI>(frame + c * plane + at, true, kStatsPx, px[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < kStatsPx; ++k) px[c][k] = k < cnt ? to_f32(frame[c * plane + at + k]) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kStatsPx; ++k) {
        const float r = rgb_unit(px[0][k]), g = rgb_unit(px[1][k]), b = rgb_unit(px[2][k]);
        o.rgb[k] = (uint32_t)stats_code(r, cf.fS) | ((uint32_t)stats_code(g, cf.fS) << 10) | ((uint32_t)stats_code(b, cf.fS) << 20);
        o.y[k] = stats_luma(cf, r, g, b);
    }
    int yr = __shfl_down(o.y[0], 1);                            // the next lane's first pixel: px0 + 4
    if (cnt63 > kStatsPx)                                       // ... which for the last lane (cnt63 = cnt there, 0 elsewhere) belongs to the tile to the right
        yr = stats_luma(cf, rgb_unit(to_f32(frame[at + kStatsPx])), rgb_unit(to_f32(frame[plane + at + kStatsPx])), rgb_unit(to_f32(frame[2 * plane + at + kStatsPx])));
    o.yr = yr;
}

// The zone of position p along an axis of n zones: the number of boundaries bd[1 .. n] that are <= p (bd[0] = 0 <= p < bd[n]).  A loop on
// purpose: it runs once per tile, and unrolled its invariants crowd the scalar registers.
__device__ __forceinline__ int stats_zone(const int* bd, int n, int p) {
    int lo = 0;                                                 // bd[lo] <= p throughout
#pragma unroll 1
    for (int step = kStatsGrid / 2; step; step >>= 1) {         // n <= 64: lo reaches at most 63
        const int c = lo + step;
        if (c < n && bd[c] <= p) lo = c;
    }
    return lo;
}

// The wave's register partials -> its LDS row -> zone row j of the frame in global memory.  Wave-uniform call.
__device__ __forceinline__ void stats_flush(uint32_t (&acc)[kStatsPx][kStatsSlots], const int* zc, uint32_t own, unsigned long long* zr, unsigned long long* gz, int n, int lane) {
#pragma unroll
    for (int k = 0; k < kStatsPx; ++k) {
        // bit k of `own`: pixel k is inside the ROI and is the last of its zone among the lane's pixels; a pixel that is not has its partials
        // carried to the next one (4 x 16 pixels at most: the bounds at acc hold x 4) or, outside the ROI, has none.  Mask arithmetic, no
        // compare: the masks of 4 pixels would otherwise live in scalar pairs across the whole tile.
        const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe(own, k, 1);          // 0 or ~0
#pragma unroll
        for (int s = 0; s < kStatsSlots; ++s) {
            const uint32_t v = acc[k][s] & m;
            if (k + 1 < kStatsPx) acc[k + 1 < kStatsPx ? k + 1 : k][s] += acc[k][s] & ~m;
            acc[k][s] = 0u;
            if (v) atomicAdd(&zr[zc[k] * kStatsSlots + s], (unsigned long long)v);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the wave's LDS adds are done before any lane swaps a slot out
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) {
        const unsigned long long v = atomicExch(&zr[i], 0ull);
        if (v) atomicAdd(&gz[i], v);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

template <typename TI>
__global__ void __launch_bounds__(kStatsThreads) frame_stats_kernel(StatsArgs a, const TI* __restrict__ src, unsigned long long* __restrict__ ghist,
                                                                    unsigned long long* __restrict__ gzones) {
    __shared__ uint32_t hist[4 * kStatsMaxBins];                                  // a count is at most the plane's samples, < 2^29
    __shared__ unsigned long long zrow[kStatsWaves][kStatsGrid * kStatsSlots];    // 64 bit: no bound needed
    __shared__ int xb[kStatsGrid + 1], yb[kStatsGrid + 1];                        // zone i is [b[i], b[i + 1]): b[i] = ceil(i side / zones)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), frame = blockIdx.y;
    for (int i = tid; i < 4 * a.nbins; i += kStatsThreads) hist[i] = 0u;
    for (int i = tid; i < kStatsWaves * kStatsGrid * kStatsSlots; i += kStatsThreads) (&zrow[0][0])[i] = 0ull;
    {   // ceil(i side / n) = i q + ceil(i r / n) with side = q n + r: 32-bit divisions only (i r < 64 x 64)
        const unsigned gx = a.gx, gy = a.gy, qx = (unsigned)a.rw / gx, rx = (unsigned)a.rw - qx * gx, qy = (unsigned)a.rh / gy, ry = (unsigned)a.rh - qy * gy;
        const unsigned i = tid & 127;
        if (tid < 128 && i <= gx) xb[i] = (int)(i * qx + (i * rx + gx - 1) / gx);
        if (tid >= 128 && i <= gy) yb[i] = (int)(i * qy + (i * ry + gy - 1) / gy);
    }
    __syncthreads();

    const TI* fsrc = src + (size_t)frame * 3 * (size_t)a.plane;
    unsigned long long* zr = zrow[wv];
    unsigned long long* gzf = gzones + (size_t)frame * a.gy * a.gx * kStatsSlots;
    unsigned long long* gh = ghist + (size_t)frame * 4 * a.nbins;
    const int zn = a.gx * kStatsSlots;
    int last[4] = {0, 0, 0, 0};                                                   // per channel: the code of the current run ...
    uint32_t run[4] = {0u, 0u, 0u, 0u};                                           // ... and its length, at most the lane's pixels < 2^29

    StatsCoef cf = {a.fS, a.k};
    int dark = a.dark, clip = a.clip;
    int ty = 0, tx = blockIdx.x;                                                  // tile t = ty ntx + tx, walked without a division
    for (int t = blockIdx.x; t < a.ntiles; t += a.nblk, tx += a.nblk) {
        while (tx >= a.ntx) {
            tx -= a.ntx;
            ++ty;
        }
        const int r0 = ty * kStatsTileH + wv * kStatsRows;
        if (r0 >= a.rh) continue;                                                 // wave-uniform; no block barrier inside the loop
        const int r1 = min(r0 + kStatsRows, a.rh);
        const int px0 = tx * kStatsTileW + lane * kStatsPx;
        int cnt = a.rw - px0;                                                     // the lane's pixels inside the ROI: >= 4 all, <= 0 none
        int cnt63 = lane == 63 ? cnt : 0;
        int zc[kStatsPx];
#pragma unroll
        for (int k = 0; k < kStatsPx; ++k)                                        // a zone is never empty: the next pixel is in the same or the next one
            zc[k] = k >= cnt ? 0 : k == 0 ? stats_zone(xb, a.gx, px0) : zc[k > 0 ? k - 1 : 0] + (px0 + k >= xb[zc[k > 0 ? k - 1 : 0] + 1] ? 1 : 0);
        uint32_t own = 0u;                                                        // see stats_flush
#pragma unroll
        for (int k = 0; k < kStatsPx; ++k)
            own |= (k < cnt && (k + 1 >= kStatsPx || k + 1 >= cnt || zc[k] != zc[k + 1 < kStatsPx ? k + 1 : k])) ? 1u << k : 0u;
        asm volatile("" : "+v"(own));                                             // opaque: stays a bit field, not four compare pairs
        int j = __builtin_amdgcn_readfirstlane(stats_zone(yb, a.gy, r0));
        // slot partials of at most 16 rows (x 4 when merged in stats_flush): counts <= 64, code sums <= 64 x 1023, focus <= 64 x 2 x 1023^2 < 2^28
        uint32_t acc[kStatsPx][kStatsSlots] = {};
        StatsRow cur = {};
        for (int yy = r0; yy <= r1; ++yy) {                                       // yy: the row whose codes are made; row yy - 1 is accounted for
            asm volatile("" : "+v"(cnt), "+v"(cnt63));                                         // opaque: the edge compares are remade per row, not kept in scalar pairs
            StatsRow nxt = cur;                                                   // yy = rh: the ROI's last row's lower neighbour is itself
            if (yy < a.rh) stats_row<TI>(a, cf, fsrc, yy, px0, cnt, cnt63, nxt);
            if (yy > r0) {
#pragma unroll
                for (int k = 0; k < kStatsPx; ++k) {
                    if (k < cnt) {
                        const int qr = cur.rgb[k] & 1023u, qg = (cur.rgb[k] >> 10) & 1023u, qb = cur.rgb[k] >> 20, qy = cur.y[k];
                        const int right = k + 1 < kStatsPx ? cur.y[k + 1 < kStatsPx ? k + 1 : k] : cur.yr;
                        const int dx = k + 1 < cnt ? right - qy : 0, dy = nxt.y[k] - qy;
                        const bool clipped = max(max(qr, qg), qb) >= clip, isdark = !clipped && qy <= dark, valid = !clipped && !isdark;
                        acc[k][0] += valid ? 1u : 0u;
                        acc[k][1] += valid ? (uint32_t)qr : 0u;
                        acc[k][2] += valid ? (uint32_t)qg : 0u;
                        acc[k][3] += valid ? (uint32_t)qb : 0u;
                        acc[k][4] += (uint32_t)qy;
                        acc[k][5] += clipped ? 1u : 0u;
                        acc[k][6] += isdark ? 1u : 0u;
                        acc[k][7] += (uint32_t)(dx * dx + dy * dy);
                        const int q[4] = {qr, qg, qb, qy};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (q[c] == last[c]) {
                                ++run[c];
                            } else {
                                if (run[c]) atomicAdd(&hist[c * a.nbins + last[c]], run[c]);
                                last[c] = q[c];
                                run[c] = 1u;
                            }
                        }
                    }
                }
                const bool band_ends = yy >= yb[j + 1];                           // row yy starts the next zone row (j + 1 <= gy, yb[gy] = rh)
                if (band_ends || yy == r1) stats_flush(acc, zc, own, zr, gzf + (size_t)j * zn, zn, lane);
                j += band_ends ? 1 : 0;
            }
            cur = nxt;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (run[c]) atomicAdd(&hist[c * a.nbins + last[c]], run[c]);
    __syncthreads();
    for (int i = tid; i < 4 * a.nbins; i += kStatsThreads) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&gh[i], (unsigned long long)v);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_stats_desc_size(void) { return sizeof(rc_stats_desc); }

int rc_frame_stats(const void* d_src, int src_dtype, const rc_stats_desc* desc, long long* d_hist, long long* d_zones,
                   int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && desc && d_hist && d_zones, "rc_frame_stats: null pointer");
    RgbSide src;
    if (int e = rgb_source("rc_frame_stats", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    RC_REQUIRE(batch <= 65535, "rc_frame_stats: bad shape (more than 65535 frames)");
    RC_REQUIRE((long long)H * W < (1LL << 29), "rc_frame_stats: bad shape (a source plane of 2^29 samples or more)");
    RC_REQUIRE(desc->bits == 8 || desc->bits == 10, "rc_frame_stats: bits must be 8 or 10");
    RC_REQUIRE(desc->matrix >= RC_MATRIX_BT601 && desc->matrix <= RC_MATRIX_BT2020, "rc_frame_stats: unknown matrix");
    RC_REQUIRE(!desc->reserved[0] && !desc->reserved[1] && !desc->reserved[2] && !desc->reserved[3], "rc_frame_stats: reserved fields must be zero");
    int y0 = desc->roi[0], x0 = desc->roi[1], rh = desc->roi[2], rw = desc->roi[3];
    if (rh == 0 && rw == 0) {
        RC_REQUIRE(y0 == 0 && x0 == 0, "rc_frame_stats: a roi of size (0, 0) is the whole crop and starts at (0, 0)");
        rh = h; rw = w;
    }
    RC_REQUIRE(y0 >= 0 && x0 >= 0 && rh >= 1 && rw >= 1 && y0 <= h - rh && x0 <= w - rw, "rc_frame_stats: the roi (y0, x0, rh, rw) is empty on one side or lies outside the crop");
    const int gy = desc->grid[0], gx = desc->grid[1], nbins = 1 << desc->bits;
    RC_REQUIRE(gy >= 1 && gy <= RC_STATS_MAX_GRID && gy <= rh && gx >= 1 && gx <= RC_STATS_MAX_GRID && gx <= rw, "rc_frame_stats: the grid must lie in 1 .. min(64, roi side) per axis");
    RC_REQUIRE(desc->clip >= 1 && desc->clip <= nbins, "rc_frame_stats: clip must lie in 1 .. 2^bits");
    RC_REQUIRE(desc->dark >= -1 && desc->dark <= nbins - 1, "rc_frame_stats: dark must lie in -1 .. 2^bits - 1");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_hist) % 8 == 0 && reinterpret_cast<uintptr_t>(d_zones) % 8 == 0, "rc_frame_stats: the outputs must be 8-byte aligned");

    StatsArgs a;
    a.W = W; a.plane = H * W; a.org = y0 * W + x0; a.rh = rh; a.rw = rw; a.gy = gy; a.gx = gx;
    a.nbins = nbins; a.dark = desc->dark; a.clip = desc->clip;
    a.fS = (float)(nbins - 1);
    a.k = rgb_coef(desc->matrix).k;
    a.ntx = ceil_div(rw, kStatsTileW);
    a.ntiles = a.ntx * ceil_div(rh, kStatsTileH);                                         // < 2^29 / 256 + 2^29 / 64
    a.vec = src.vec && x0 % kStatsPx == 0;                                                // then every lane, too, starts on a 4-sample boundary
    // persistent blocks: 4 per CU fit (33 KB of LDS, <= 128 VGPRs) shared among the frames, and no more than a third of the tiles, so
    // that a block's one histogram flush is paid by at least three tiles
    const int cap = std::max(1, 4 * device_cu_count() / batch);
    const int nblk = a.nblk = std::max(1, std::min(cap, a.ntiles / 3));
    const hipStream_t st = as_stream(stream);
    RC_HIP_CHECK(hipMemsetAsync(d_hist, 0, (size_t)batch * 4 * nbins * sizeof(long long), st));
    RC_HIP_CHECK(hipMemsetAsync(d_zones, 0, (size_t)batch * gy * gx * kStatsSlots * sizeof(long long), st));
    const dim3 grid((unsigned)nblk, (unsigned)batch), block(kStatsThreads);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(d_hist);
    unsigned long long* zones = reinterpret_cast<unsigned long long*>(d_zones);
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        hipLaunchKernelGGL(frame_stats_kernel<TI>, grid, block, 0, st, a, static_cast<const TI*>(d_src), hist, zones);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
