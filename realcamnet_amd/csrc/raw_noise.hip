// RAW noise measurement (include/realcam_hip.h, rc_raw_noise): the sensor mosaic (B, 2h, 2w) as rc_raw_format describes it (any storage,
// padded lines, any cfa), read once -> hist (B,4,L,320) int32 and level (B,4,L) int64: per CFA colour and per level bin the histogram of the
// pair-difference energy of the region's T x T-cell tiles, and the sum of the tiles' code sums.  A photon-transfer curve from ordinary frames:
// the low quantile of a level bin's energies is the energy of its flat tiles, whose expectation is 2 sigma^2 per pair.  The third reduction
// of the family; the plan is raw_stats.hip's with the tile in the place of the zone, and registers in the place of its LDS partials.
//
// raw_noise_kernel: grid (blocks per frame, frames), 4 waves per block.  A wave's unit of work is a strip of 128 cell columns (one lane: 2
// cells, raw_row.hpp's 4 samples of the two mosaic rows of a cell row) by 32 cell rows; strips start at the ROI's even cx0, so every lane's
// 4 samples start on a multiple of 4 and a tile (T = 4, 8 or 16 cells: T/2 adjacent lanes, T rows) never straddles a wave or a unit.
//   rows      the wave walks DOWN its cell rows; the two row loads of row r + 1 are issued before row r is decoded, so a wave always has a
//             row in flight while it computes (rc_raw_stats waits for each row with nothing else in flight: DESIGN.md 4.i).  The loop body
//             has no branch around a load -- whether a lane's 4 samples are one vector load is a template parameter, a lane beyond the
//             last tile and the row behind the last one re-read valid samples -- so the wait in front of the decode counts loads.
//   codes     the 8 samples become signed codes -S .. S in CFA-POSITION order (the blacks and scales are per position); a position's
//             pair is the lane's own two cells: d = q(cell 0) - q(cell 1).  Per position a lane keeps s1 (|s1| <= 2 x 16 x 65535 < 2^21), e =
//             sum d^2 (64 bit: d^2 < 2^35) and one bit "a code reached sat or floor" down the T rows of a tile row.
//   tiles     after the T-th row the T/2 lanes of a tile add their partials with log2(T/2) butterfly steps (lane ^ 1, 2, 4: inside a row of
//             16 lanes), and the first lane of each tile commits, per valid position: one count into the histogram (slot = position ^
//             swz) and one 64-bit add of s1 into the block's 4 x L level sums in LDS (2 KB).
//   sums      both tables are pre-summed per block, because a frame's tiles share a handful of addresses -- a grey card or a dark frame
//             puts every tile of a colour into ONE level bin and a dozen energy bins, and global atomics on one address are served one
//             after the other (measured: DESIGN.md 4.h).  The level sums are small enough to be held whole.  Of the histogram a block
//             holds a WINDOW in LDS (20 KB): per position the 4 level bins around the level of the first cell it reads; a tile inside the
//             window is an LDS add, any other one a returnless 32-bit global atomic.  The block adds its non-zero sums to global memory when
//             it ends.
// Vector loads, LDS atomics and vector global atomics only.  Everything after the codes is integer, so the order of the adds does not
// matter: bit-exact and the same from run to run.
#include "raw_row.hpp"

#include <cmath>
#include <type_traits>

namespace rc {

constexpr int kRnWaves = 4, kRnThreads = 64 * kRnWaves;
constexpr int kRnStripW = 128, kRnRows = 32;                                       // a wave's unit, in cells
constexpr int kRnEbins = RC_RAW_NOISE_EBINS, kRnMaxLevels = 1 << RC_RAW_NOISE_MAX_LEVEL_BITS;
constexpr int kRnWin = 4;                                                          // level bins per position a block counts in LDS (L >= 8)
static_assert(kRowPx == 4 && kRnStripW == 64 * 2, "a lane's 4 samples of a row are two cells: one pair per CFA position");
static_assert(kRnRows % 16 == 0 && kRnStripW % 16 == 0, "a tile of 4, 8 or 16 cells never straddles a unit");

struct RnArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    int H;                     // the mosaic's rows (2h)
    int line_bytes, vec;       // vec: every lane's 4 samples start on a 4-sample boundary of the source
    int cy0, cx0;              // the ROI's first cell; cx0 even
    int rows, cols;            // the measured cells: (rh div T) T and (rw div T) T
    int tlog;                  // log2 T
    int lbits, lshift;         // log2 L; 2 log2 T + bits - level_bits
    int sat, floor;
    int swz;                   // slot = position ^ swz
    float fS, black[4], k[4];  // float(S); CFA-position order
    int nstrips, nunits;       // strips per row of units; units per frame
};

// Step 1 of the header.  fmaxf / fminf return the other operand for a NaN, and the one way to a NaN here (a scale that is not finite) is
// refused by the entry: no sample makes a code leave -S .. S; +-inf clamp like any other value.
template <typename TI>
__device__ __forceinline__ int rn_code(float v, float black, float k, float fS) {
    if constexpr (!std::is_integral<TI>::value) v = v != v ? 0.f : v;
    const float q = rintf(__fmul_rn(__fsub_rn(v, black), k));                      // round half to even
    return (int)fminf(fmaxf(q, -fS), fS);
}

// Step 5: e < 2^41, so the bin is at most 8 x 37 + 15 = 311.
__device__ __forceinline__ int rn_ebin(unsigned long long e) {
    if (e < 16ull) return (int)e;
    const int k = 63 - __clzll((long long)e);
    return 8 * (k - 3) + (int)(e >> (k - 3));
}

// Both outputs are zeroed by this small launch on the stream, not by hipMemsetAsync, as raw_stats.hip and tone.hip zero theirs.
__global__ void __launch_bounds__(kRnThreads) raw_noise_zero_kernel(int* __restrict__ hist, size_t nhist, unsigned long long* __restrict__ level, size_t nlevel) {
    const size_t first = (size_t)blockIdx.x * kRnThreads + threadIdx.x, step = (size_t)gridDim.x * kRnThreads;
    for (size_t i = first; i < nhist; i += step) hist[i] = 0;
    for (size_t i = first; i < nlevel; i += step) level[i] = 0ull;
}

// VEC: an element storage whose every lane reads its 4 samples of a row with one vector load (RnArgs::vec); packed rows: false.
template <int ST, typename TI, bool VEC>
__global__ void __launch_bounds__(kRnThreads) raw_noise_kernel(RnArgs a, int* __restrict__ ghist, unsigned long long* __restrict__ glevel) {
    __shared__ unsigned long long lev[4 * kRnMaxLevels];                          // position-major; two's complement sums, |sum| < 2^45
    __shared__ uint32_t win[4 * kRnWin * kRnEbins];                               // position-major: level bins base[p] .. + kRnWin - 1; a count is at most the block's tiles
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), frame = blockIdx.y;
    const int nl = 4 << a.lbits;
    for (int i = tid; i < nl; i += kRnThreads) lev[i] = 0ull;
    for (int i = tid; i < 4 * kRnWin * kRnEbins; i += kRnThreads) win[i] = 0u;
    __syncthreads();

    const uint8_t* fsrc = a.src + (size_t)frame * (size_t)a.H * (size_t)a.line_bytes;
    int* gh = ghist + (size_t)frame * nl * kRnEbins;
    const int T = 1 << a.tlog, half = T >> 1;
    const bool leader = (lane & (half - 1)) == 0;
    const float fS = a.fS;
    float black[4], k[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) { black[p] = a.black[p]; k[p] = a.k[p]; }
    const int sat = a.sat, floor = a.floor;
    const size_t lb = (size_t)a.line_bytes;
    // The window: the level bins around those of the first cell of the block's first unit (every thread reads the same 8 samples: a block's
    // units are neighbours, and a scene is mostly smooth).  A tile inside it is counted in LDS, any other one in global memory.
    int base[4];
    {
        const int u0 = blockIdx.x * kRnWaves, g0 = u0 / a.nstrips, s0 = u0 - g0 * a.nstrips;      // u0 < nunits: the entry launches no idle block
        const int x0 = 2 * (a.cx0 + s0 * kRnStripW);
        const uint8_t* ra = fsrc + (size_t)(2 * (a.cy0 + g0 * kRnRows)) * lb;
        const RowRaw A = row_load<ST, TI>(ra, x0, kRowPx, VEC), B = row_load<ST, TI>(ra + lb, x0, kRowPx, VEC);
        float va[kRowPx], vb[kRowPx];
        row_decode<ST, TI>(A, kRowPx, VEC, va);
        row_decode<ST, TI>(B, kRowPx, VEC, vb);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int q = max(rn_code<TI>((p < 2 ? va : vb)[p & 1], black[p], k[p], fS), 0);     // T^2 q stands for the tile's s1
            const int l = (q << (2 * a.tlog)) >> a.lshift;                                        // q <= S: 0 .. L - 1
            base[p] = __builtin_amdgcn_readfirstlane(min(max(l - 1, 0), (1 << a.lbits) - kRnWin));
        }
    }

    for (int u = blockIdx.x * kRnWaves + wv; u < a.nunits; u += gridDim.x * kRnWaves) {      // wave-uniform; no block barrier inside
        const int g = u / a.nstrips, s = u - g * a.nstrips;
        const int rel = s * kRnStripW + 2 * lane;                                 // ROI-relative column of the lane's first cell (even)
        const bool live = rel < a.cols;                                           // cols is even: both cells are measured, or neither
        const int x0 = 2 * (a.cx0 + (live ? rel : 0));                            // a multiple of 4; x0 + 3 < 2w.  A lane beyond the last tile reads the
                                                                                  // ROI's first cells again and commits nothing: no branch around a load
        const int row0 = g * kRnRows, nrows = min(kRnRows, a.rows - row0);        // a multiple of T rows
        const uint8_t* ra = fsrc + (size_t)(2 * (a.cy0 + row0)) * lb;             // wave-uniform; a frame may exceed 2 GiB
        RowRaw A = row_load<ST, TI>(ra, x0, kRowPx, VEC), B = row_load<ST, TI>(ra + lb, x0, kRowPx, VEC);
        int s1[4] = {0, 0, 0, 0};
        unsigned long long e[4] = {0ull, 0ull, 0ull, 0ull};
        int bad = 0;                                                              // bit p: a code of position p reached sat or floor
#pragma unroll 1
        for (int r = 0; r < nrows; ++r) {
            // the next row is in flight while this one is reduced (the last row is asked for twice: the loop body has no branch, so the
            // compiler waits for the two older loads only)
            ra += r + 1 < nrows ? 2 * lb : 0;
            const RowRaw An = row_load<ST, TI>(ra, x0, kRowPx, VEC), Bn = row_load<ST, TI>(ra + lb, x0, kRowPx, VEC);
            float va[kRowPx], vb[kRowPx];
            row_decode<ST, TI>(A, kRowPx, VEC, va);
            row_decode<ST, TI>(B, kRowPx, VEC, vb);
#pragma unroll
            for (int p = 0; p < 4; ++p) {                                         // position p: row p >> 1, column p & 1 of both cells
                const float* v = p < 2 ? va : vb;
                const int q0 = rn_code<TI>(v[p & 1], black[p], k[p], fS), q1 = rn_code<TI>(v[2 + (p & 1)], black[p], k[p], fS);
                const int d = q0 - q1;                                            // |d| <= 2 S < 2^17
                s1[p] += q0 + q1;
                e[p] += (unsigned long long)((long long)d * (long long)d);
                bad |= (max(q0, q1) >= sat || min(q0, q1) <= floor) ? 1 << p : 0;
            }
            if (((r + 1) & (T - 1)) == 0) {                                       // the tile row is complete: wave-uniform
                for (int m = 1; m < half; m <<= 1) {                              // every lane takes part
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        s1[p] += __shfl_xor(s1[p], m);
                        e[p] += __shfl_xor(e[p], m);
                    }
                    bad |= __shfl_xor(bad, m);
                }
                if (leader && live) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        if (!((bad >> p) & 1)) {
                            const int l = max(s1[p], 0) >> a.lshift;              // 0 .. L - 1: s1 <= T^2 S < 2^(2 log2 T + bits)
                            const int eb = rn_ebin(e[p]), wl = l - base[p];
                            if ((unsigned)wl < (unsigned)kRnWin) atomicAdd(&win[(p * kRnWin + wl) * kRnEbins + eb], 1u);
                            else atomicAdd(&gh[((((p ^ a.swz) << a.lbits) + l) * kRnEbins) + eb], 1);
                            atomicAdd(&lev[(p << a.lbits) + l], (unsigned long long)(long long)s1[p]);
                        }
                    }
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) { s1[p] = 0; e[p] = 0ull; }
                bad = 0;
            }
            A = An;
            B = Bn;
        }
    }
    __syncthreads();
    unsigned long long* gl = glevel + (size_t)frame * nl;
    for (int i = tid; i < nl; i += kRnThreads) {                                  // position p's sums are colour slot p ^ swz's
        const unsigned long long v = lev[i];
        if (v) atomicAdd(&gl[(((i >> a.lbits) ^ a.swz) << a.lbits) + (i & ((1 << a.lbits) - 1))], v);
    }
    for (int i = tid; i < 4 * kRnWin * kRnEbins; i += kRnThreads) {
        const uint32_t v = win[i];
        if (v) {
            const int p = i / (kRnWin * kRnEbins), rest = i - p * (kRnWin * kRnEbins), wl = rest / kRnEbins, eb = rest - wl * kRnEbins;
            const int l = (p == 0 ? base[0] : p == 1 ? base[1] : p == 2 ? base[2] : base[3]) + wl;
            atomicAdd(&gh[((((p ^ a.swz) << a.lbits) + l) * kRnEbins) + eb], (int)v);
        }
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_raw_noise_desc_size(void) { return sizeof(rc_raw_noise_desc); }

int rc_raw_noise(const void* d_src, const rc_raw_format* fmt, const rc_raw_noise_desc* desc, void* d_hist, void* d_level, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_hist && d_level, "rc_raw_noise: null pointer");
    if (const int e = raw_frames("rc_raw_noise", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_noise", d_src, fmt, w, &rs)) return e;
    if (const int e = raw_blacks_finite("rc_raw_noise", fmt)) return e;
    RC_REQUIRE(4LL * h * w < (1LL << 31), "rc_raw_noise: bad shape (a mosaic of 2^31 samples or more)");
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_noise: reserved fields must be zero");
    const int T = desc->tile, bits = desc->bits, lbits = desc->level_bits;
    RC_REQUIRE(T == 4 || T == 8 || T == 16, "rc_raw_noise: tile must be 4, 8 or 16");
    RC_REQUIRE(bits >= 8 && bits <= 16, "rc_raw_noise: bits must lie in 8 .. 16");
    RC_REQUIRE(lbits >= 3 && lbits <= RC_RAW_NOISE_MAX_LEVEL_BITS, "rc_raw_noise: level_bits must lie in 3 .. 6");
    const int S = (1 << bits) - 1;
    RC_REQUIRE(std::isfinite(desc->top), "rc_raw_noise: top must be finite");
    float k[4];
    for (int p = 0; p < 4; ++p) {
        RC_REQUIRE(desc->top > fmt->black[p], "rc_raw_noise: top must exceed every black level");
        k[p] = (float)((double)S / ((double)desc->top - (double)fmt->black[p]));
        RC_REQUIRE(std::isfinite(k[p]), "rc_raw_noise: top is too close to a black level (the scale S / (top - black) is not finite)");
    }
    RC_REQUIRE(desc->sat >= 1 && desc->sat <= S + 1, "rc_raw_noise: sat must lie in 1 .. 2^bits");
    RC_REQUIRE(desc->floor >= -S - 1 && desc->floor <= S - 1, "rc_raw_noise: floor must lie in -2^bits .. 2^bits - 2");
    int cy0 = desc->roi[0], cx0 = desc->roi[1], rh = desc->roi[2], rw = desc->roi[3];
    if (rh == 0 && rw == 0) {
        RC_REQUIRE(cy0 == 0 && cx0 == 0, "rc_raw_noise: a roi of size (0, 0) is the whole frame and starts at (0, 0)");
        rh = h; rw = w;
    }
    RC_REQUIRE(cy0 >= 0 && cx0 >= 0 && rh >= 1 && rw >= 1 && cy0 <= h - rh && cx0 <= w - rw,
               "rc_raw_noise: the roi (cy0, cx0, rh, rw) is empty on one side or lies outside the frame of (h, w) cells");
    RC_REQUIRE(cx0 % 2 == 0, "rc_raw_noise: the roi must start on an even cell column (cx0)");
    RC_REQUIRE(rh >= T && rw >= T, "rc_raw_noise: the roi holds no whole tile (fewer than `tile` cell rows or columns)");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_hist) % 4 == 0, "rc_raw_noise: d_hist must be 4-byte aligned");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_level) % 8 == 0, "rc_raw_noise: d_level must be 8-byte aligned");

    RnArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.H = 2 * h;
    a.line_bytes = (int)rs.line_bytes; a.vec = rs.vec;
    a.cy0 = cy0; a.cx0 = cx0;
    a.tlog = T == 4 ? 2 : T == 8 ? 3 : 4;
    a.rows = (rh >> a.tlog) << a.tlog; a.cols = (rw >> a.tlog) << a.tlog;
    a.lbits = lbits; a.lshift = 2 * a.tlog + bits - lbits;
    a.sat = desc->sat; a.floor = desc->floor;
    // position -> slot (R, G of the R row, G of the B row, B): every cfa's map is an exclusive-or (raw_format.py, SLOT_POS)
    a.swz = fmt->cfa == RC_CFA_RGGB ? 0 : fmt->cfa == RC_CFA_BGGR ? 3 : fmt->cfa == RC_CFA_GRBG ? 1 : 2;
    a.fS = (float)S;
    for (int p = 0; p < 4; ++p) { a.black[p] = fmt->black[p]; a.k[p] = k[p]; }
    a.nstrips = ceil_div(a.cols, kRnStripW);
    a.nunits = a.nstrips * ceil_div(a.rows, kRnRows);                                      // < 2^29 / 128 + 2^29 / 32
    // 2 KB of LDS and few registers: 8 blocks per CU fit, shared among the frames; a block that is not needed is not launched
    const int cap = std::max(1, 8 * device_cu_count() / batch);
    const int nblk = std::max(1, std::min(cap, ceil_div(a.nunits, kRnWaves)));
    const hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)nblk, (unsigned)batch), block(kRnThreads);
    int* hist = static_cast<int*>(d_hist);
    unsigned long long* level = static_cast<unsigned long long*>(d_level);
    const size_t nlevel = (size_t)batch * 4 * ((size_t)1 << lbits), nhist = nlevel * kRnEbins;
    const unsigned zblocks = (unsigned)std::min<size_t>((nhist + kRnThreads - 1) / kRnThreads, 1024);
    hipLaunchKernelGGL(raw_noise_zero_kernel, dim3(zblocks), block, 0, st, hist, nhist, level, nlevel);
    by_storage(fmt->storage, [&](auto sg) {
        constexpr int ST = decltype(sg)::ST;
        typedef typename decltype(sg)::type TI;
        if constexpr (ST == kElem) {
            if (a.vec) {
                hipLaunchKernelGGL((raw_noise_kernel<ST, TI, true>), grid, block, 0, st, a, hist, level);
                return;
            }
        }
        hipLaunchKernelGGL((raw_noise_kernel<ST, TI, false>), grid, block, 0, st, a, hist, level);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
