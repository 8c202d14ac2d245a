// Local tone mapping between the scaler and the look (include/realcam_hip.h, rc_tone_*): CLAHE on the 8-bit luma code of the planar
// result (B,3,H,W), cropped to (h,w), applied as one gain to R, G and B.  Three launches: the tiles' histograms, histograms -> gain tables,
// and the map itself, which gathers a gain per pixel from the tables of the four nearest tile centres.
//
// tone_hist_kernel: grid (slabs of 32 rows of a tile, tiles, frames), four waves per block.
//   A block owns (tile, slab).  Wave v takes the slab's rows v, v + 4, ...; along a row it walks the tile's columns in pieces of 256, a
//   lane holding the 4 pixels x0 .. x0 + 3 with x0 a multiple of 4 (the first piece starts at the tile's first column rounded DOWN to 4,
//   so that a lane's load is one 8- or 16-byte vector whatever column the tile starts at; pixels left of the tile or right of it are
//   masked).  One 256-bin table of 32-bit counters per block in LDS.  A lane run-length codes its pixels, rows and pieces included: an LDS
//   add is issued only when the code changes, so a flat tile issues one per lane.  Flushed once per block, non-zero bins only, with
//   32-bit global atomics (a count is at most a plane's samples, < 2^29).  The histograms are zeroed by tone_zero_kernel on the stream
//   in front of it: a launch, not a memset node, replayed correctly under a captured graph.
// tone_gains_kernel: one block of 256 threads per tile, thread k owns bin k; the sums and the prefix sum are a Hillis-Steele scan in LDS,
//   in 64-bit integers.  Off the hot path.
// tone_apply_kernel: grid (strips of 256 columns, bands of 64 rows, frames), four waves per block, dynamic LDS.
//   lane map   lane l holds the 4 pixels xs + 4 l .. + 3 of a row of each plane (rgb_strip.hpp's loads and stores); ix / ux of these columns
//              are the lane's constants for the whole band.  Wave v takes rows v, v + 4, ... of a segment.
//   segments   the band is cut where iy changes: inside a segment jy and jy' are fixed, so the block stages the gain tables of tile rows
//              jy and jy', tile columns jx_lo .. jx_hi (what the strip can touch: at most ceil(256 / min tile width) + 3 of them, 1 KiB
//              each) into LDS once and every pixel gathers its 8 values from there.  iy / uy are wave-uniform per row.
//   gathers    G_t[i] and G_t[i + 1] are neighbours: one two-dword LDS read per tile and pixel, 4 per pixel.  The index i comes from the
//              pixel's luma alone (0 .. 254), the tile offsets from ix / iy clamped to the staged range: nothing is indexed by a gain.
// 32-bit element offsets below a 64-bit frame base (the entry points check).  The arithmetic is step for step the header's: every product,
// sum, difference and quotient rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn), so the vector path, the element path
// and a plain elementwise restatement give the same bits.  Nothing outside the crop is ever read.
#include "rgb_strip.hpp"

#include <cmath>

namespace rc {

constexpr int kTonePx = 4, kToneWaves = 4, kToneThreads = 64 * kToneWaves;
static_assert(kTonePx == kRgbPx, "a lane holds one rgb_strip.hpp strip");
constexpr int kToneSpan = 64 * kTonePx;           // columns of a piece (hist) and of a strip (apply)
constexpr int kToneHistRows = 32;                 // rows of a hist slab
constexpr int kToneBand = 64;                     // rows of an apply band
constexpr int kToneBins = RC_TONE_BINS, kToneGrid = RC_TONE_MAX_GRID;

// a_i = ceil(i side / g) for i <= g <= 16 and side < 2^29: i side < 2^33, so 64 bits
__host__ __device__ inline int tone_bound(int i, int side, int g) { return (int)(((long long)i * side + g - 1) / g); }

// The histograms start from zero: a launch on the stream, so that a captured graph replays it with the rest.
__global__ void __launch_bounds__(kToneThreads) tone_zero_kernel(unsigned int* __restrict__ p, size_t n) {
    const size_t i = (size_t)blockIdx.x * kToneThreads + threadIdx.x;
    if (i < n) p[i] = 0u;
}

struct ToneHistArgs {
    int H, W, h, w;            // source plane, crop
    int gy, gx;
    int vec;                   // every 4-sample group of every row starts on a vector boundary
    Luma k;
};

template <typename TI>
__global__ void __launch_bounds__(kToneThreads) tone_hist_kernel(ToneHistArgs a, const TI* __restrict__ src, unsigned int* __restrict__ ghist) {
    __shared__ unsigned int hist[kToneBins];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.y, ty = tile / a.gx, tx = tile - ty * a.gx, frame = blockIdx.z;
    const int ya = tone_bound(ty, a.h, a.gy), yb = tone_bound(ty + 1, a.h, a.gy);
    const int xa = tone_bound(tx, a.w, a.gx), xb = tone_bound(tx + 1, a.w, a.gx);
    const int r0 = ya + blockIdx.x * kToneHistRows;
    if (r0 >= yb) return;                                                          // block-uniform: this tile has fewer slabs
    const int r1 = min(r0 + kToneHistRows, yb);
    hist[tid] = 0u;
    __syncthreads();

    const uint32_t plane = (uint32_t)a.H * (uint32_t)a.W;
    const TI* s = src + (size_t)frame * 3 * (size_t)plane;
    int last = 0;                                                                  // the code of the current run ...
    uint32_t run = 0u;                                                             // ... and its length, at most 32 rows of the tile's columns
    for (int y = r0 + wv; y < r1; y += kToneWaves) {
        for (int x0 = (xa & ~(kTonePx - 1)) + lane * kTonePx; x0 < xb; x0 += kToneSpan) {
            const int cnt = min(a.w - x0, kTonePx);                                // the lane's pixels inside the crop: > 0 here (xb <= w)
            const uint32_t o = (uint32_t)y * (uint32_t)a.W + (uint32_t)x0;
            const bool vec = a.vec && cnt == kTonePx;
            float c[3][kTonePx];
#pragma unroll
            for (int p = 0; p < 3; ++p) rgb_load<TI>(s + (p * plane + o), vec, cnt, c[p]);
#pragma unroll
            for (int k = 0; k < kTonePx; ++k) {
                if (x0 + k >= xa && x0 + k < xb) {
                    const float Y = rgb_luma(a.k, rgb_unit(c[0][k]), rgb_unit(c[1][k]), rgb_unit(c[2][k]));
                    const int q = (int)__builtin_amdgcn_fmed3f(rintf(__fmul_rn(Y, 255.f)), 0.f, 255.f);
                    if (q == last) {
                        ++run;
                    } else {
                        if (run) atomicAdd(&hist[last], run);
                        last = q;
                        run = 1u;
                    }
                }
            }
        }
    }
    if (run) atomicAdd(&hist[last], run);
    __syncthreads();
    const unsigned int v = hist[tid];
    if (v) atomicAdd(&ghist[((size_t)frame * gridDim.y + tile) * kToneBins + tid], v);
}

struct ToneGainArgs {
    long long clip_q8;
    float strength, max_gain;
};

// The inclusive prefix sum of one value per thread over the block's 256 threads (Hillis-Steele in LDS).  Every thread calls it.
__device__ __forceinline__ long long tone_scan(long long* buf, int tid, long long v) {
    buf[tid] = v;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < kToneBins; d <<= 1) {
        const long long add = tid >= d ? buf[tid - d] : 0ll;
        __syncthreads();
        v += add;
        buf[tid] = v;
        __syncthreads();
    }
    return v;
}

__global__ void __launch_bounds__(kToneBins) tone_gains_kernel(ToneGainArgs a, const int* __restrict__ ghist, float* __restrict__ gains) {
    __shared__ long long buf[kToneBins];
    __shared__ float g1;
    const int k = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kToneBins;
    const long long hk = (long long)ghist[base + k];
    tone_scan(buf, k, hk);
    const long long total = buf[kToneBins - 1];
    __syncthreads();
    const long long n = total > 1 ? total : 1;
    long long limit = (n * a.clip_q8) >> 16;
    limit = limit > 1 ? limit : 1;
    long long c = hk < limit ? hk : limit;
    tone_scan(buf, k, c);
    const long long E = n - buf[kToneBins - 1];
    __syncthreads();
    const long long lowbits = E & 255;
    c += (E >> 8) + ((((long long)(k + 1) * lowbits) >> 8) - (((long long)k * lowbits) >> 8));
    const long long C = tone_scan(buf, k, c);
    const float T = __fdiv_rn((float)C, (float)n);                                 // int64 -> fp32: round to nearest even
    float G = 0.f;
    if (k >= 1) {
        const float y = __fdiv_rn((float)k, 255.f);
        const float m = __fadd_rn(y, __fmul_rn(a.strength, __fsub_rn(T, y)));
        G = fminf(__fdiv_rn(m, y), a.max_gain);
    }
    if (k == 1) g1 = G;
    __syncthreads();
    gains[base + k] = k == 0 ? g1 : G;
}

struct ToneApplyArgs {
    int H, W, h, w;            // source plane, cropped / output plane
    int gy, gx;
    int shared_gains;          // one set of tables for every frame
    int ncmax;                 // tile columns the LDS holds per tile row
    int vec_src, vec_dst;
    Luma k;
};

template <typename TI, typename TO>
__global__ void __launch_bounds__(kToneThreads) tone_apply_kernel(ToneApplyArgs a, const TI* __restrict__ src, TO* __restrict__ dst, const float* __restrict__ gains,
                                                                  const int* __restrict__ iy, const float* __restrict__ uy, const int* __restrict__ ix, const float* __restrict__ ux) {
    extern __shared__ __attribute__((aligned(16))) float tab[];                                                 // [2][ncmax][256]: tile rows jy, jy' of the segment
    __shared__ int siy[kToneBand];
    __shared__ float suy[kToneBand];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xs = blockIdx.x * kToneSpan, frame = blockIdx.z;
    const int r0 = blockIdx.y * kToneBand, r1 = min(r0 + kToneBand, a.h);          // r0 < h: the grid has ceil(h / kToneBand) bands
    if (tid < r1 - r0) {
        siy[tid] = min(max(iy[r0 + tid], 0), a.gy - 1);
        suy[tid] = uy[r0 + tid];
    }
    // the tile columns this strip can touch: ix is non-decreasing, so those of its first column up to the right neighbour of its last one
    const int xe = min(xs + kToneSpan, a.w) - 1;
    const int jx_lo = min(max(ix[xs], 0), a.gx - 1);
    const int jx_hi = min(min(max(ix[xe], 0), a.gx - 1) + 1, a.gx - 1);
    const int nc = min(max(jx_hi - jx_lo + 1, 1), a.ncmax);

    const int x0 = xs + lane * kTonePx;
    const int n = x0 < a.w ? min(a.w - x0, kTonePx) : 0;
    const bool vin = n == kTonePx && a.vec_src, vout = n == kTonePx && a.vec_dst;
    int c0[kTonePx], c1[kTonePx];                                                  // the LDS offsets of the pixel's two tile columns
    float u[kTonePx];
#pragma unroll
    for (int k = 0; k < kTonePx; ++k) {
        const int x = min(x0 + k, a.w - 1);
        const int jx = min(max(ix[x], 0), a.gx - 1), jxn = min(jx + 1, a.gx - 1);
        c0[k] = min(max(jx - jx_lo, 0), nc - 1) * kToneBins;
        c1[k] = min(max(jxn - jx_lo, 0), nc - 1) * kToneBins;
        u[k] = ux[x];
    }
    const uint32_t splane = (uint32_t)a.H * (uint32_t)a.W, dplane = (uint32_t)a.h * (uint32_t)a.w;
    const TI* s = src + (size_t)frame * 3 * (size_t)splane;
    TO* d = dst + (size_t)frame * 3 * (size_t)dplane;
    const float* gf = gains + (a.shared_gains ? (size_t)0 : (size_t)frame * a.gy * a.gx * kToneBins);
    const int row1 = a.ncmax * kToneBins;                                          // where tile row jy' starts in tab
    __syncthreads();

    int ys = r0;
    while (ys < r1) {                                                              // block-uniform: one segment of constant iy per turn
        const int jy = siy[ys - r0], jyn = min(jy + 1, a.gy - 1);
        int ye = ys + 1;
        while (ye < r1 && siy[ye - r0] == jy) ++ye;
        {   // stage nc tables of each of the two tile rows: nc x 64 float4 per row, contiguous in global memory
            const float4* g0 = reinterpret_cast<const float4*>(gf + ((size_t)jy * a.gx + jx_lo) * kToneBins);
            const float4* g1 = reinterpret_cast<const float4*>(gf + ((size_t)jyn * a.gx + jx_lo) * kToneBins);
            float4* t0 = reinterpret_cast<float4*>(tab);
            float4* t1 = reinterpret_cast<float4*>(tab + row1);
            for (int i = tid; i < nc * (kToneBins / 4); i += kToneThreads) {
                t0[i] = g0[i];
                t1[i] = g1[i];
            }
        }
        __syncthreads();
        for (int y = ys + wv; y < ye; y += kToneWaves) {
            if (n > 0) {
                const float v = suy[y - r0];
                const uint32_t o = (uint32_t)y * (uint32_t)a.W + (uint32_t)x0;
                float c[3][kTonePx], out[3][kTonePx];
#pragma unroll
                for (int p = 0; p < 3; ++p) rgb_load<TI>(s + (p * splane + o), vin, n, c[p]);
#pragma unroll
                for (int k = 0; k < kTonePx; ++k) {
                    const float r = rgb_unit(c[0][k]), g = rgb_unit(c[1][k]), b = rgb_unit(c[2][k]);
                    const float Y = rgb_luma(a.k, r, g, b);
                    const float p = __fmul_rn(Y, 255.f);                           // in [0, 255 + a few ulp], never NaN
                    const int i = min((int)floorf(p), kToneBins - 2);
                    const float f = fminf(__fsub_rn(p, (float)i), 1.f);
                    const float* t00 = tab + c0[k] + i;
                    const float* t01 = tab + c1[k] + i;
                    const float a00 = t00[0], b00 = t00[1], a01 = t01[0], b01 = t01[1];
                    const float a10 = t00[row1], b10 = t00[row1 + 1], a11 = t01[row1], b11 = t01[row1 + 1];
                    const float g00 = __fadd_rn(a00, __fmul_rn(f, __fsub_rn(b00, a00)));
                    const float g01 = __fadd_rn(a01, __fmul_rn(f, __fsub_rn(b01, a01)));
                    const float g10 = __fadd_rn(a10, __fmul_rn(f, __fsub_rn(b10, a10)));
                    const float g11 = __fadd_rn(a11, __fmul_rn(f, __fsub_rn(b11, a11)));
                    const float top = __fadd_rn(g00, __fmul_rn(u[k], __fsub_rn(g01, g00)));
                    const float bot = __fadd_rn(g10, __fmul_rn(u[k], __fsub_rn(g11, g10)));
                    const float gn = __fadd_rn(top, __fmul_rn(v, __fsub_rn(bot, top)));
                    out[0][k] = fminf(__fmul_rn(r, gn), 1.f);
                    out[1][k] = fminf(__fmul_rn(g, gn), 1.f);
                    out[2][k] = fminf(__fmul_rn(b, gn), 1.f);
                }
                const uint32_t off = (uint32_t)y * (uint32_t)a.w + (uint32_t)x0;
#pragma unroll
                for (int p = 0; p < 3; ++p) rgb_store<TO>(d + (p * dplane + off), vout, n, out[p]);
            }
        }
        __syncthreads();                                                           // every wave is done with the tables before the next segment's replace them
        ys = ye;
    }
}

// The refusals the three entries share; the message names the entry.
static int tone_check_desc(const rc_tone_desc* d, const char* who) {
    const std::string w(who);
    if (!d) return fail(RC_ERR_INVALID, w + ": null pointer");
    if (!(d->grid[0] >= 1 && d->grid[0] <= kToneGrid && d->grid[1] >= 1 && d->grid[1] <= kToneGrid)) return fail(RC_ERR_INVALID, w + ": the grid must lie in 1 .. 16 per axis");
    if (!(d->matrix >= RC_MATRIX_BT601 && d->matrix <= RC_MATRIX_BT2020)) return fail(RC_ERR_INVALID, w + ": unknown matrix");
    if (!(d->clip_q8 >= 256 && d->clip_q8 <= 65536)) return fail(RC_ERR_INVALID, w + ": clip_q8 must lie in 256 .. 65536");
    if (!(std::isfinite(d->strength) && d->strength >= 0.f && d->strength <= 1.f)) return fail(RC_ERR_INVALID, w + ": strength must be finite and lie in [0, 1]");
    if (!(std::isfinite(d->max_gain) && d->max_gain >= 1.f && d->max_gain <= 64.f)) return fail(RC_ERR_INVALID, w + ": max_gain must be finite and lie in [1, 64]");
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return fail(RC_ERR_INVALID, w + ": reserved fields must be zero");
    return RC_OK;
}

static int tone_check_frame(const rc_tone_desc* d, const void* d_src, int src_dtype, int batch, int H, int W, int h, int w, const char* who, RgbSide* src) {
    const std::string n(who);
    if (int e = rgb_source(who, d_src, src_dtype, batch, H, W, h, w, src)) return e;
    if (!(batch <= 65535)) return fail(RC_ERR_INVALID, n + ": bad shape (more than 65535 frames)");
    if (!((long long)H * W < (1LL << 29))) return fail(RC_ERR_INVALID, n + ": bad shape (a source plane of 2^29 samples or more)");
    if (!(d->grid[0] <= h && d->grid[1] <= w)) return fail(RC_ERR_INVALID, n + ": the grid has more tiles than the frame has rows or columns");
    return RC_OK;
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_tone_desc_size(void) { return sizeof(rc_tone_desc); }

int rc_tone_axis(int n, int g, int* idx, float* wt) {
    RC_REQUIRE(idx && wt, "rc_tone_axis: null pointer");
    RC_REQUIRE(n >= 1 && g >= 1 && g <= kToneGrid && g <= n, "rc_tone_axis: n must be positive and g lie in 1 .. min(16, n)");
    long long s[kToneGrid];                                                        // twice the centre of tile i
    for (int i = 0; i < g; ++i) s[i] = (((long long)i * n + g - 1) / g) + (((long long)(i + 1) * n + g - 1) / g);
    int i = 0;
    for (int x = 0; x < n; ++x) {
        const long long q = 2LL * x + 1;
        if (q <= s[0]) {
            idx[x] = 0; wt[x] = 0.f;
        } else if (q >= s[g - 1]) {
            idx[x] = g - 1; wt[x] = 0.f;
        } else {
            while (i + 1 < g && s[i + 1] <= q) ++i;                                // q only grows: the largest i with s_i <= q
            idx[x] = i;
            wt[x] = (float)((double)(q - s[i]) / (double)(s[i + 1] - s[i]));
        }
    }
    return RC_OK;
}

int rc_tone_hist(const void* d_src, int src_dtype, const rc_tone_desc* desc, int* d_hist, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && desc && d_hist, "rc_tone_hist: null pointer");
    if (int e = tone_check_desc(desc, "rc_tone_hist")) return e;
    RgbSide src;
    if (int e = tone_check_frame(desc, d_src, src_dtype, batch, H, W, h, w, "rc_tone_hist", &src)) return e;
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_hist) % 4 == 0, "rc_tone_hist: misaligned pointer");

    ToneHistArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w; a.gy = desc->grid[0]; a.gx = desc->grid[1];
    a.vec = src.vec;
    a.k = rgb_coef(desc->matrix).k;
    const int tiles = a.gy * a.gx, tall = ceil_div(h, a.gy);                              // the tallest tile's rows
    const hipStream_t st = as_stream(stream);
    const size_t words = (size_t)batch * tiles * kToneBins;                               // < 2^32: 65535 frames of 256 tiles
    hipLaunchKernelGGL(tone_zero_kernel, dim3((unsigned)((words + kToneThreads - 1) / kToneThreads)), dim3(kToneThreads), 0, st, reinterpret_cast<unsigned int*>(d_hist), words);
    const dim3 grid((unsigned)ceil_div(tall, kToneHistRows), (unsigned)tiles, (unsigned)batch), block(kToneThreads);
    unsigned int* hist = reinterpret_cast<unsigned int*>(d_hist);
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        hipLaunchKernelGGL(tone_hist_kernel<TI>, grid, block, 0, st, a, static_cast<const TI*>(d_src), hist);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_tone_gains(const int* d_hist, const rc_tone_desc* desc, float* d_gains, int batch, void* stream) {
    RC_REQUIRE(d_hist && desc && d_gains, "rc_tone_gains: null pointer");
    if (int e = tone_check_desc(desc, "rc_tone_gains")) return e;
    RC_REQUIRE(batch >= 1 && batch <= 65535, "rc_tone_gains: bad shape (empty or more than 65535 frames)");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_hist) % 4 == 0 && reinterpret_cast<uintptr_t>(d_gains) % 4 == 0, "rc_tone_gains: misaligned pointer");
    ToneGainArgs a;
    a.clip_q8 = desc->clip_q8; a.strength = desc->strength; a.max_gain = desc->max_gain;
    const dim3 grid((unsigned)(batch * desc->grid[0] * desc->grid[1])), block(kToneBins);
    hipLaunchKernelGGL(tone_gains_kernel, grid, block, 0, as_stream(stream), a, d_hist, d_gains);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_tone_apply(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const rc_tone_desc* desc, const float* d_gains, int gains_batch,
                  const int* d_iy, const float* d_uy, const int* d_ix, const float* d_ux, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && d_dst && desc && d_gains && d_iy && d_uy && d_ix && d_ux, "rc_tone_apply: null pointer");
    if (int e = tone_check_desc(desc, "rc_tone_apply")) return e;
    RgbSide src, dst;
    if (int e = tone_check_frame(desc, d_src, src_dtype, batch, H, W, h, w, "rc_tone_apply", &src)) return e;
    if (int e = rgb_dest("rc_tone_apply", d_dst, dst_dtype, src_dtype, w, &dst)) return e;
    RC_REQUIRE(gains_batch == 1 || gains_batch == batch, "rc_tone_apply: gains_batch must be 1 or batch");
    const long long ss = (long long)src.esize, ds = (long long)dst.esize;
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_gains) % 16 == 0, "rc_tone_apply: the gains must be 16-byte aligned");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_iy) % 4 == 0 && reinterpret_cast<uintptr_t>(d_uy) % 4 == 0 && reinterpret_cast<uintptr_t>(d_ix) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(d_ux) % 4 == 0, "rc_tone_apply: misaligned axis table");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + (uintptr_t)(3LL * H * W * ss * batch);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_dst), o1 = o0 + (uintptr_t)(3LL * h * w * ds * batch);
    RC_REQUIRE(s1 <= o0 || o1 <= s0, "rc_tone_apply: dst overlaps src");

    ToneApplyArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w; a.gy = desc->grid[0]; a.gx = desc->grid[1];
    a.shared_gains = gains_batch == 1 && batch > 1;
    a.ncmax = std::min(a.gx, ceil_div(kToneSpan, w / a.gx) + 3);                          // w / gx: the narrowest tile, >= 1
    a.vec_src = src.vec; a.vec_dst = dst.vec;
    a.k = rgb_coef(desc->matrix).k;
    const dim3 grid((unsigned)ceil_div(w, kToneSpan), (unsigned)ceil_div(h, kToneBand), (unsigned)batch), block(kToneThreads);
    RC_REQUIRE(grid.y <= 65535u, "rc_tone_apply: more than 4194240 rows");
    const size_t lds = (size_t)2 * a.ncmax * kToneBins * sizeof(float);                   // at most 32 KiB: below the default limit
    const hipStream_t st = as_stream(stream);
    by_source_dest(src_dtype, dst_dtype, [&](auto ti, auto to) {
        typedef typename decltype(ti)::type TI;
        typedef typename decltype(to)::type TO;
        hipLaunchKernelGGL((tone_apply_kernel<TI, TO>), grid, block, lds, st, a, static_cast<const TI*>(d_src), static_cast<TO*>(d_dst), d_gains, d_iy, d_uy, d_ix, d_ux);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
