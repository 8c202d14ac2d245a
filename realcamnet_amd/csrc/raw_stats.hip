// RAW-domain 3A statistics (include/realcam_hip.h, rc_raw_stats): the sensor mosaic (B, 2h, 2w) as rc_raw_format describes it (any storage,
// padded lines, any cfa), read once -> hist (B,4,2^hist_bits) and zones (B,gy,gx,8), int64: per CFA colour the code histogram, and the 3A
// zone grid (valid / saturated / dark cell counts, the four colour sums, the green focus energy) of a region of interest given in Bayer
// CELLS.  Linear, black-subtracted and in front of every gain: what an AE / AWB / AF loop reads.  The second reduction of the family; the
// plan is frame_stats.hip's, with the cell in the place of the pixel and raw_row.hpp's reader in the place of the planar one.
//
// raw_stats_kernel: persistent blocks, grid (blocks per frame, frames).  A tile is 128 cell columns (256 samples) x 64 cell rows; tile
// columns start at the even cell column at or left of the ROI, so that every lane's 4 samples start on a multiple of 4 as row_load wants
// them.  A block walks tiles t = blockIdx.x, + gridDim.x, ...; wave v owns the tile's cell rows 16 v .. 16 v + 15 and walks DOWN them; a
// lane's 4 samples of mosaic rows 2 cy and 2 cy + 1 are two whole cells (two row_load per cell row).
//   codes     the 8 samples become integer codes once; everything is kept in CFA-POSITION order inside the kernel (the blacks and scales
//             are per position, a lane's samples alternate between two positions per row) and turned into slot order R, G1, G2, B only
//             where a partial leaves the block: slot = position ^ swz.  A wave computes cell row cy + 1 before it accounts for row cy (dy
//             needs the green code below) and keeps it as the next row, so only the row under a wave's last one is decoded twice (1 / 16,
//             out of L2: no second pass over HBM).  dx: the green code of the cell to the right is the lane's own second cell, the next
//             lane's first (one DPP shuffle) or, for lane 63, one more load per mosaic row from the tile to the right.
//   zones     a lane's 2 zone columns are fixed while it walks a tile (bisected once per tile in the 65 boundaries the block computes into
//             LDS when it starts: no division per cell); the zone ROW is wave-uniform and walked.  A lane sums its cells' 8 slots in 2 x 8
//             32-bit registers down the rows; when the zone row changes or the tile ends the wave flushes: equal columns of a lane merged,
//             LDS 64-bit adds into the wave's own row of gx x 8 slots, then that row is swapped out (exchange with 0) and its non-zero
//             slots added to global memory with 64-bit atomics.
//   hist      one 4 x 2^hist_bits table of 32-bit counters per block in LDS.  A lane run-length codes each position's bin across its
//             cells, tiles included: an LDS add is issued only when the bin changes; flushed once per block, non-zero bins only, with
//             64-bit global atomics.
// Vector loads, LDS atomics and vector global atomics only.  Everything after the codes is integer, so the order of the adds does not
// matter: bit-exact and the same from run to run.  The bound of every partial is written where it is declared.
#include "raw_row.hpp"

#include <cmath>
#include <type_traits>

namespace rc {

constexpr int kRsCells = 2, kRsWaves = 4, kRsRows = 16, kRsThreads = 64 * kRsWaves;
constexpr int kRsTileW = 64 * kRsCells, kRsTileH = kRsWaves * kRsRows;            // in cells
constexpr int kRsMaxBins = 1 << RC_RAW_STATS_MAX_HIST_BITS, kRsSlots = RC_RAW_STATS_SLOTS, kRsGrid = RC_RAW_STATS_MAX_GRID;
static_assert(2 * kRsCells == kRowPx, "a lane's 4 samples of a row are two cells");

struct RsArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    int H, W;                  // the mosaic's rows and columns (2h, 2w)
    int line_bytes, vec;       // vec: every lane's 4 samples start on a 4-sample boundary of the source
    int cy0, cx0, rh, rw;      // the ROI, in cells
    int tx0;                   // cx0 rounded down to even: the first tile's first cell column
    int gy, gx;
    int hbits, hshift, gshift; // log2 of the bins; bits - hist_bits; bits - 7
    int sat, dark;
    int swz, gdiag;            // slot = position ^ swz; gdiag: the greens are positions 0 and 3 (GRBG, GBRG), else 1 and 2
    float fS, black[4], k[4];  // float(S); CFA-position order
    int ntx, ntiles, nblk;     // tiles per row of tiles, tiles per frame, blocks per frame
};

struct RsCoef { float fS, black[4], k[4]; int gshift, gdiag; };

struct RsRow {
    uint32_t q01[kRsCells], q23[kRsCells];     // the codes of positions 0 | 1 << 16 and 2 | 3 << 16 (a code is at most 65535)
    int g[kRsCells];                           // (qG1 + qG2) >> (bits - 7): 0 .. 255
    int gr;                                    // g of the cell right of the lane's second one (meaningful where that cell is inside the ROI)
};

// Steps 1 and 2 of the header.  max / min, not a median: they return the other operand for a NaN, so no sample makes a code leave 0 .. S
// (the entry refuses the one way to a NaN here, a scale that is not finite); +-inf clamp like any other value.
template <typename TI>
__device__ __forceinline__ uint32_t rs_code(float v, float black, float k, float fS) {
    if constexpr (!std::is_integral<TI>::value) v = v != v ? 0.f : v;
    const float q = rintf(__fmul_rn(__fsub_rn(v, black), k));                      // round half to even
    return (uint32_t)(int)fminf(fmaxf(q, 0.f), fS);
}

// The codes of one cell from its samples a0, a1 (row 2 cy) and b0, b1 (row 2 cy + 1), and its green figure.
template <typename TI>
__device__ __forceinline__ void rs_cell(const RsCoef& cf, float a0, float a1, float b0, float b1, uint32_t& q01, uint32_t& q23, int& g) {
    const uint32_t q0 = rs_code<TI>(a0, cf.black[0], cf.k[0], cf.fS), q1 = rs_code<TI>(a1, cf.black[1], cf.k[1], cf.fS);
    const uint32_t q2 = rs_code<TI>(b0, cf.black[2], cf.k[2], cf.fS), q3 = rs_code<TI>(b1, cf.black[3], cf.k[3], cf.fS);
    q01 = q0 | (q1 << 16);
    q23 = q2 | (q3 << 16);
    g = (int)((cf.gdiag ? q0 + q3 : q1 + q2) >> cf.gshift);
}

// The codes of cell row cy (absolute) for the lane's cells at mosaic columns x0 .. x0 + 3 (n of them inside the frame).  `live`: one of the
// two cells is inside the ROI (else nothing is read); `edge`: the lane is lane 63 and needs the tile to the right.  Called by the whole
// wave: the shuffle needs every lane.
template <int ST, typename TI>
__device__ __forceinline__ void rs_row(const RsArgs& a, const RsCoef& cf, const uint8_t* __restrict__ frame, int cy, int x0, int n, bool live, bool edge, RsRow& o) {
    const uint8_t* ra = frame + (size_t)(2 * cy) * (size_t)a.line_bytes;           // wave-uniform; a frame may exceed 2 GiB
    const uint8_t* rb = ra + a.line_bytes;
    if (live) {
        const bool full = n == kRowPx && a.vec;
        const RowRaw A = row_load<ST, TI>(ra, x0, n, full), B = row_load<ST, TI>(rb, x0, n, full);
        float va[kRowPx], vb[kRowPx];
        row_decode<ST, TI>(A, n, full, va);
        row_decode<ST, TI>(B, n, full, vb);
#pragma unroll
        for (int k = 0; k < kRsCells; ++k) rs_cell<TI>(cf, va[2 * k], va[2 * k + 1], vb[2 * k], vb[2 * k + 1], o.q01[k], o.q23[k], o.g[k]);
    }
    int gr = __shfl_down(o.g[0], 1);                                               // the next lane's first cell
    if (edge) {                                                                    // ... which for lane 63 belongs to the tile to the right: inside the ROI, so inside the frame
        const int x1 = x0 + kRowPx, n1 = min(a.W - x1, kRowPx);
        const bool full = n1 == kRowPx && a.vec;
        const RowRaw A = row_load<ST, TI>(ra, x1, n1, full), B = row_load<ST, TI>(rb, x1, n1, full);
        float va[kRowPx], vb[kRowPx];
        row_decode<ST, TI>(A, n1, full, va);
        row_decode<ST, TI>(B, n1, full, vb);
        uint32_t q01, q23;
        rs_cell<TI>(cf, va[0], va[1], vb[0], vb[1], q01, q23, gr);
    }
    o.gr = gr;
}

// The zone of position p along an axis of n zones: the number of boundaries bd[1 .. n] that are <= p (bd[0] = 0 <= p < bd[n]).  A loop on
// purpose: it runs once per tile.
__device__ __forceinline__ int rs_zone(const int* bd, int n, int p) {
    int lo = 0;                                                 // bd[lo] <= p throughout
#pragma unroll 1
    for (int step = kRsGrid / 2; step; step >>= 1) {            // n <= 64: lo reaches at most 63
        const int c = lo + step;
        if (c < n && bd[c] <= p) lo = c;
    }
    return lo;
}

// The wave's register partials -> its LDS row -> zone row j of the frame in global memory.  Wave-uniform call.  The colour sums leave
// position order here: partial 1 + p goes to slot 1 + (p ^ swz).
__device__ __forceinline__ void rs_flush(uint32_t (&acc)[kRsCells][kRsSlots], const int* zc, uint32_t own, int swz, unsigned long long* zr, unsigned long long* gz, int n, int lane) {
#pragma unroll
    for (int k = 0; k < kRsCells; ++k) {
        // bit k of `own`: cell k is inside the ROI and is the last of its zone among the lane's cells; a cell that is not has its partials
        // carried to the next one (2 x 16 cells at most: the bounds at acc hold x 2) or, outside the ROI, has none.
        const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe(own, k, 1);          // 0 or ~0
#pragma unroll
        for (int s = 0; s < kRsSlots; ++s) {
            const uint32_t v = acc[k][s] & m;
            if (k + 1 < kRsCells) acc[k + 1 < kRsCells ? k + 1 : k][s] += acc[k][s] & ~m;
            acc[k][s] = 0u;
            const int slot = s >= 1 && s <= 4 ? 1 + ((s - 1) ^ swz) : s;
            if (v) atomicAdd(&zr[zc[k] * kRsSlots + slot], (unsigned long long)v);
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

// Both outputs are zeroed by this small launch on the stream, not by hipMemsetAsync, as tone.hip zeroes its histograms: a
// captured graph that held nothing but the two memsets and the kernel below did not replay to the eager result.
__global__ void __launch_bounds__(kRsThreads) raw_stats_zero_kernel(unsigned long long* __restrict__ hist, size_t nhist, unsigned long long* __restrict__ zones, size_t nzones) {
    const size_t first = (size_t)blockIdx.x * kRsThreads + threadIdx.x, step = (size_t)gridDim.x * kRsThreads;
    for (size_t i = first; i < nhist; i += step) hist[i] = 0ull;
    for (size_t i = first; i < nzones; i += step) zones[i] = 0ull;
}

template <int ST, typename TI>
__global__ void __launch_bounds__(kRsThreads) raw_stats_kernel(RsArgs a, unsigned long long* __restrict__ ghist, unsigned long long* __restrict__ gzones) {
    __shared__ uint32_t hist[4 * kRsMaxBins];                                     // position-major; a count is at most the frame's cells, < 2^29
    __shared__ unsigned long long zrow[kRsWaves][kRsGrid * kRsSlots];             // 64 bit: no bound needed
    __shared__ int xb[kRsGrid + 1], yb[kRsGrid + 1];                              // zone i is [b[i], b[i + 1]): b[i] = ceil(i side / zones), ROI-relative cells
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), frame = blockIdx.y;
    const int nbins = 1 << a.hbits;
    for (int i = tid; i < 4 * nbins; i += kRsThreads) hist[i] = 0u;
    for (int i = tid; i < kRsWaves * kRsGrid * kRsSlots; i += kRsThreads) (&zrow[0][0])[i] = 0ull;
    {   // ceil(i side / n) = i q + ceil(i r / n) with side = q n + r: 32-bit divisions only (i r < 64 x 64)
        const unsigned gx = a.gx, gy = a.gy, qx = (unsigned)a.rw / gx, rx = (unsigned)a.rw - qx * gx, qy = (unsigned)a.rh / gy, ry = (unsigned)a.rh - qy * gy;
        const unsigned i = tid & 127;
        if (tid < 128 && i <= gx) xb[i] = (int)(i * qx + (i * rx + gx - 1) / gx);
        if (tid >= 128 && i <= gy) yb[i] = (int)(i * qy + (i * ry + gy - 1) / gy);
    }
    __syncthreads();

    const uint8_t* fsrc = a.src + (size_t)frame * (size_t)a.H * (size_t)a.line_bytes;
    unsigned long long* zr = zrow[wv];
    unsigned long long* gzf = gzones + (size_t)frame * a.gy * a.gx * kRsSlots;
    unsigned long long* gh = ghist + (size_t)frame * 4 * nbins;
    const int zn = a.gx * kRsSlots;
    uint32_t last[4] = {0u, 0u, 0u, 0u};                                          // per position: the bin of the current run ...
    uint32_t run[4] = {0u, 0u, 0u, 0u};                                           // ... and its length, at most the lane's cells < 2^29

    RsCoef cf;
    cf.fS = a.fS; cf.gshift = a.gshift; cf.gdiag = a.gdiag;
#pragma unroll
    for (int p = 0; p < 4; ++p) { cf.black[p] = a.black[p]; cf.k[p] = a.k[p]; }
    const int sat = a.sat, dark = a.dark, hshift = a.hshift;
    int ty = 0, tx = blockIdx.x;                                                  // tile t = ty ntx + tx, walked without a division
    for (int t = blockIdx.x; t < a.ntiles; t += a.nblk, tx += a.nblk) {
        while (tx >= a.ntx) {
            tx -= a.ntx;
            ++ty;
        }
        const int r0 = ty * kRsTileH + wv * kRsRows;                              // ROI-relative cell rows r0 .. r1 - 1
        if (r0 >= a.rh) continue;                                                 // wave-uniform; no block barrier inside the loop
        const int r1 = min(r0 + kRsRows, a.rh);
        const int c0 = a.tx0 + tx * kRsTileW + lane * kRsCells;                   // the lane's first cell column (even); its samples start at 2 c0
        const int x0 = 2 * c0, n = min(a.W - x0, kRowPx);                         // n <= 0: the lane is right of the frame
        const int rel = c0 - a.cx0;                                               // ROI-relative: -1 where the ROI starts on an odd column
        // bit k of `inm`: cell k is inside the ROI (then it is inside the frame, and n >= 2 (k + 1) samples are)
        uint32_t inm = (rel >= 0 && rel < a.rw ? 1u : 0u) | (rel + 1 < a.rw ? 2u : 0u);
        const bool right1 = rel + 2 < a.rw;                                       // the cell right of cell 1 is inside the ROI
        int zc[kRsCells];
        zc[0] = (inm & 1u) ? rs_zone(xb, a.gx, rel) : 0;                          // a zone is never empty: the next cell is in the same or the next one
        zc[1] = (inm & 2u) && (inm & 1u) ? zc[0] + (rel + 1 >= xb[zc[0] + 1] ? 1 : 0) : 0;     // cell 1 alone: ROI column 0
        uint32_t own = ((inm & 1u) && (!(inm & 2u) || zc[0] != zc[1]) ? 1u : 0u) | (inm & 2u);       // see rs_flush
        uint32_t edge = lane == 63 && (inm & 2u) && right1 ? 1u : 0u;
        asm volatile("" : "+v"(own));                                             // opaque: stays a bit field, not compare pairs
        int j = __builtin_amdgcn_readfirstlane(rs_zone(yb, a.gy, r0));
        // slot partials of at most 16 rows (x 2 when merged in rs_flush): counts <= 32, code sums <= 32 x 65535 < 2^21, focus <= 32 x 2 x 255^2 < 2^22
        uint32_t acc[kRsCells][kRsSlots] = {};
        RsRow cur = {};
        for (int yy = r0; yy <= r1; ++yy) {                                       // yy: the row whose codes are made; row yy - 1 is accounted for
            asm volatile("" : "+v"(inm), "+v"(edge));                             // opaque: the edge tests are remade per row, not kept in scalar pairs
            RsRow nxt = cur;                                                      // yy = rh: the ROI's last row's lower neighbour is itself
            if (yy < a.rh) rs_row<ST, TI>(a, cf, fsrc, a.cy0 + yy, x0, n, inm != 0u, edge != 0u, nxt);
            if (yy > r0) {
#pragma unroll
                for (int k = 0; k < kRsCells; ++k) {
                    if (inm & (1u << k)) {
                        const uint32_t q[4] = {cur.q01[k] & 0xffffu, cur.q01[k] >> 16, cur.q23[k] & 0xffffu, cur.q23[k] >> 16};
                        const int g = cur.g[k];
                        const int dx = k + 1 < kRsCells ? ((inm & 2u) ? cur.g[k + 1 < kRsCells ? k + 1 : k] - g : 0) : (right1 ? cur.gr - g : 0);
                        const int dy = nxt.g[k] - g;
                        const int m = (int)max(max(q[0], q[1]), max(q[2], q[3]));
                        const bool issat = m >= sat, isdark = !issat && m <= dark, valid = !issat && !isdark;
                        acc[k][0] += valid ? 1u : 0u;
#pragma unroll
                        for (int p = 0; p < 4; ++p) acc[k][1 + p] += valid ? q[p] : 0u;
                        acc[k][5] += issat ? 1u : 0u;
                        acc[k][6] += isdark ? 1u : 0u;
                        acc[k][7] += (uint32_t)(dx * dx + dy * dy);
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            const uint32_t bin = q[p] >> hshift;
                            if (bin == last[p]) {
                                ++run[p];
                            } else {
                                if (run[p]) atomicAdd(&hist[(p << a.hbits) + last[p]], run[p]);
                                last[p] = bin;
                                run[p] = 1u;
                            }
                        }
                    }
                }
                const bool band_ends = yy >= yb[j + 1];                           // row yy starts the next zone row (j + 1 <= gy, yb[gy] = rh)
                if (band_ends || yy == r1) rs_flush(acc, zc, own, a.swz, zr, gzf + (size_t)j * zn, zn, lane);
                j += band_ends ? 1 : 0;
            }
            cur = nxt;
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
        if (run[p]) atomicAdd(&hist[(p << a.hbits) + last[p]], run[p]);
    __syncthreads();
    for (int i = tid; i < 4 * nbins; i += kRsThreads) {                           // position p's table is colour slot p ^ swz's
        const uint32_t v = hist[i];
        if (v) atomicAdd(&gh[(((i >> a.hbits) ^ a.swz) << a.hbits) + (i & (nbins - 1))], (unsigned long long)v);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_raw_stats_desc_size(void) { return sizeof(rc_raw_stats_desc); }

int rc_raw_stats(const void* d_src, const rc_raw_format* fmt, const rc_raw_stats_desc* desc, void* d_hist, void* d_zones, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_hist && d_zones, "rc_raw_stats: null pointer");
    if (const int e = raw_frames("rc_raw_stats", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_stats", d_src, fmt, w, &rs)) return e;
    if (const int e = raw_blacks_finite("rc_raw_stats", fmt)) return e;
    RC_REQUIRE(4LL * h * w < (1LL << 31), "rc_raw_stats: bad shape (a mosaic of 2^31 samples or more)");
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_stats: reserved fields must be zero");
    const int bits = desc->bits, hbits = desc->hist_bits;
    RC_REQUIRE(bits >= 8 && bits <= 16, "rc_raw_stats: bits must lie in 8 .. 16");
    RC_REQUIRE(hbits >= 6 && hbits <= std::min(bits, RC_RAW_STATS_MAX_HIST_BITS), "rc_raw_stats: hist_bits must lie in 6 .. min(bits, 10)");
    const int S = (1 << bits) - 1;
    RC_REQUIRE(std::isfinite(desc->top), "rc_raw_stats: top must be finite");
    float k[4];
    for (int p = 0; p < 4; ++p) {
        RC_REQUIRE(desc->top > fmt->black[p], "rc_raw_stats: top must exceed every black level");
        k[p] = (float)((double)S / ((double)desc->top - (double)fmt->black[p]));
        RC_REQUIRE(std::isfinite(k[p]), "rc_raw_stats: top is too close to a black level (the scale S / (top - black) is not finite)");
    }
    RC_REQUIRE(desc->sat >= 1 && desc->sat <= S + 1, "rc_raw_stats: sat must lie in 1 .. 2^bits");
    RC_REQUIRE(desc->dark >= -1 && desc->dark <= S, "rc_raw_stats: dark must lie in -1 .. 2^bits - 1");
    int cy0 = desc->roi[0], cx0 = desc->roi[1], rh = desc->roi[2], rw = desc->roi[3];
    if (rh == 0 && rw == 0) {
        RC_REQUIRE(cy0 == 0 && cx0 == 0, "rc_raw_stats: a roi of size (0, 0) is the whole frame and starts at (0, 0)");
        rh = h; rw = w;
    }
    RC_REQUIRE(cy0 >= 0 && cx0 >= 0 && rh >= 1 && rw >= 1 && cy0 <= h - rh && cx0 <= w - rw,
               "rc_raw_stats: the roi (cy0, cx0, rh, rw) is empty on one side or lies outside the frame of (h, w) cells");
    const int gy = desc->grid[0], gx = desc->grid[1];
    RC_REQUIRE(gy >= 1 && gy <= RC_RAW_STATS_MAX_GRID && gy <= rh && gx >= 1 && gx <= RC_RAW_STATS_MAX_GRID && gx <= rw,
               "rc_raw_stats: the grid must lie in 1 .. min(64, roi side) per axis");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_hist) % 8 == 0 && reinterpret_cast<uintptr_t>(d_zones) % 8 == 0, "rc_raw_stats: the outputs must be 8-byte aligned");

    RsArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)rs.line_bytes; a.vec = rs.vec;
    a.cy0 = cy0; a.cx0 = cx0; a.rh = rh; a.rw = rw; a.tx0 = cx0 & ~1;
    a.gy = gy; a.gx = gx;
    a.hbits = hbits; a.hshift = bits - hbits; a.gshift = bits - 7;
    a.sat = desc->sat; a.dark = desc->dark;
    // position -> slot (R, G of the R row, G of the B row, B): every cfa's map is an exclusive-or (raw_format.py, SLOT_POS)
    a.swz = fmt->cfa == RC_CFA_RGGB ? 0 : fmt->cfa == RC_CFA_BGGR ? 3 : fmt->cfa == RC_CFA_GRBG ? 1 : 2;
    a.gdiag = fmt->cfa == RC_CFA_GRBG || fmt->cfa == RC_CFA_GBRG;
    a.fS = (float)S;
    for (int p = 0; p < 4; ++p) { a.black[p] = fmt->black[p]; a.k[p] = k[p]; }
    a.ntx = ceil_div(cx0 - a.tx0 + rw, kRsTileW);
    a.ntiles = a.ntx * ceil_div(rh, kRsTileH);                                             // < 2^29 / 128 + 2^29 / 64
    // persistent blocks: 4 per CU fit (33 KB of LDS, <= 128 VGPRs) shared among the frames, and no more than half of the tiles, so that
    // a block's one histogram flush is paid by at least two tiles (a mosaic has a third of the bytes of the planar frame rc_frame_stats
    // reads: at a third of the tiles 8 x 4K would fill 2.7 of the 4 blocks per CU, and the kernel is bound by the latency of its row loads)
    const int cap = std::max(1, 4 * device_cu_count() / batch);
    const int nblk = a.nblk = std::max(1, std::min(cap, a.ntiles / 2));
    const hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)nblk, (unsigned)batch), block(kRsThreads);
    unsigned long long* hist = static_cast<unsigned long long*>(d_hist);
    unsigned long long* zones = static_cast<unsigned long long*>(d_zones);
    const size_t nhist = (size_t)batch * 4 * ((size_t)1 << hbits), nzones = (size_t)batch * gy * gx * kRsSlots;
    const unsigned zblocks = (unsigned)std::min<size_t>((std::max(nhist, nzones) + kRsThreads - 1) / kRsThreads, 1024);
    hipLaunchKernelGGL(raw_stats_zero_kernel, dim3(zblocks), block, 0, st, hist, nhist, zones, nzones);
    by_storage(fmt->storage, [&](auto sg) {
        hipLaunchKernelGGL((raw_stats_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, block, 0, st, a, hist, zones);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
