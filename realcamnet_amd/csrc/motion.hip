// Motion estimation behind the network (include/realcam_hip.h, rc_motion_pyramid and rc_motion_search): hierarchical block matching on the
// 8-bit luma code of the planar result.  Two kernels; everything after the level-0 codes is integer.
//
// motion_pyramid_kernel: one launch, the frame read once.  A lane forms the sixteen level-0 codes of its 4 x 4 tile of pixels; the map and
// the levels' reductions and stores are pyramid_tail.hpp's.
//
// motion_search_kernel<N>: one wave per matching block of N x N, four waves (four matching blocks) per workgroup, each with its own LDS.
//   stage     the block's N x N bytes of `cur`, and the window of `ref` the candidates touch, every index clamped into the plane: rows
//             py - R .. py + R + N - 1 and 4 (N / 4 + Gx) columns from px - R on, Gx = ceil((2R + 1) / 4).  The window's left edge is a dword
//             boundary of LDS, so candidate column group gx (ox = -R + 4 gx .. + 3) of block column dword k reads window dwords k + gx and
//             k + gx + 1 as they lie: v_qsad_pk_u16_u8 needs no byte alignment step.
//   cost      work items (candidate row, column group, slice of RS block rows) are spread over the lanes; an item accumulates four u16 sums
//             with one v_qsad_pk_u16_u8 per 4 block pixels (RS N <= 256 pixels: at most 65 280 per sum) and adds them to the candidates'
//             32-bit LDS sums.
//   texture   v_sad_u8 of each block dword against itself moved one byte (the last byte against itself: 0) and against the dword below.
//   winner    every lane packs its candidates' keys (cost, |oy| + |ox|, oy + R, ox + R) into 18 + 5 + 5 + 5 bits and keeps the smallest;
//             six lane exchanges give the wave's.  Lane 0 stores the four ints as one 16-byte store.
#include "pyramid_tail.hpp"
#include "ycc_code.hpp"

namespace rc {

// ---- pyramid ------------------------------------------------------------------------------------------------------------------------------
struct PyramidArgs {
    uint8_t* lv[RC_MOTION_MAX_LEVELS];
    int levels;
    int H, W, h, w;
    int vec_src;               // rgb_strip.hpp's vec of the source
    int vec0, vec1;            // level 0: every row starts on a dword; level 1: every row starts on a 16-bit boundary
    LumaChroma c;
};

template <typename TI>
__global__ void __launch_bounds__(kPyrThreads) motion_pyramid_kernel(PyramidArgs a, const TI* __restrict__ src) {
    const int lane = threadIdx.x & 63, frame = blockIdx.z;
    const int tx = pyramid_tx(lane), ty = pyramid_ty(lane);                                     // the lane's tile: pixels 4 tx .., 4 ty ..
    const int x0 = tx * kPyrTile, y0 = ty * kPyrTile, cnt = a.w - x0;                           // cnt <= 0: the tile is right of the crop
    const size_t plane = (size_t)a.H * a.W;
    const TI* s0 = src + (size_t)frame * 3 * plane + x0;
    const bool vec = a.vec_src && cnt >= kPyrTile;

    uint32_t q[kPyrTile][kPyrTile];                                                             // level-0 codes; 0 outside the crop (never stored)
#pragma unroll
    for (int r = 0; r < kPyrTile; ++r) {
        float px[3][kPyrTile];
        const bool inside = y0 + r < a.h && cnt > 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (inside) rgb_load<TI>(s0 + c * plane + (size_t)(y0 + r) * a.W, vec, cnt, px[c]);
            else
#pragma unroll
                for (int k = 0; k < kPyrTile; ++k) px[c][k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < kPyrTile; ++k) {
            float y, cb, cr;
            ycc(a.c, px[0][k], px[1][k], px[2][k], y, cb, cr);
            q[r][k] = code(y, 255.f, 0.f, 0.f, 255.f);
        }
    }
    pyramid_tail(a, frame, lane, tx, ty, q);
}

// ---- search -------------------------------------------------------------------------------------------------------------------------------
constexpr int kMsWaves = 4, kMsThreads = 64 * kMsWaves;
constexpr int kMsMaxR = RC_MOTION_MAX_RANGE, kMsMaxGx = (2 * kMsMaxR + 1 + 3) / 4;               // 5 column groups of 4 candidates
constexpr int kMsCostWords = (2 * kMsMaxR + 1) * 4 * kMsMaxGx;                                  // 17 rows x 20 columns

struct SearchArgs {
    int hs, ws, by, bx, nblk;  // the planes, the grid of matching blocks and blocks per frame
    int R, gx, ginv;           // range; column groups; ceil(65536 / gx): g / gx = g ginv >> 16 for g < 2^12
    int rs_log2;               // an item sums 1 << rs_log2 block rows
    int pred_by, pred_bx, shift;
    int vec;                   // both planes start on a dword: whole dwords may be loaded where they lie inside the batch's bytes
    unsigned long long total;  // bytes of a plane set: batch hs ws
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Bytes at columns x .. x + 3 of row `row` (a pointer to its first byte) of a plane whose rows hold ws bytes: every column clamped.
__device__ __forceinline__ uint32_t ms_gather(const uint8_t* row, int x, int ws) {
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= (uint32_t)row[clampi(x + k, 0, ws - 1)] << (8 * k);
    return v;
}

// The same where the four bytes lie inside the row and both aligned dwords that hold them lie inside the batch's bytes (`off`: the first
// byte's offset from the 4-byte aligned base).
__device__ __forceinline__ uint32_t ms_dword(const uint8_t* base, size_t off) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + (off & ~(size_t)3));
    const uint32_t lo = p[0], hi = p[1];
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)off & 3u);
}
__device__ __forceinline__ bool ms_whole(const SearchArgs& a, size_t off) { return a.vec && (off & ~(size_t)3) + 8 <= a.total; }

template <int N>
__global__ void __launch_bounds__(kMsThreads) motion_search_kernel(SearchArgs a, const uint8_t* __restrict__ cur, const uint8_t* __restrict__ ref,
                                                                   const int* __restrict__ pred, int4* __restrict__ out) {
    constexpr int ND = N / 4, kMaxWd = ND + kMsMaxGx, kMaxRows = N + 2 * kMsMaxR;
    __shared__ uint32_t s_win[kMsWaves][kMaxRows * kMaxWd];
    __shared__ uint32_t s_cur[kMsWaves][N * ND];
    __shared__ uint32_t s_cost[kMsWaves][kMsCostWords];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), frame = blockIdx.y;
    const int blk = blockIdx.x * kMsWaves + wv;
    const bool live = blk < a.nblk;                                                   // a wave past the last block works on the last one and stores nothing
    const int bi = min(blk, a.nblk - 1), j = bi / a.bx, i = bi - j * a.bx;
    uint32_t* win = s_win[wv];
    uint32_t* cb = s_cur[wv];
    uint32_t* cost = s_cost[wv];
    const int R = a.R, D = 2 * R + 1, wd = ND + a.gx, rows = N + 2 * R, cw = 4 * a.gx;

    int px = 0, py = 0;
    if (pred) {                                                                       // device data is not trusted: clamped before it is used
        const int pj = min(j >> a.shift, a.pred_by - 1), pi = min(i >> a.shift, a.pred_bx - 1);
        const int* p = pred + (((size_t)frame * a.pred_by + pj) * a.pred_bx + pi) * 4;
        px = clampi(p[0], -32768, 32767) << a.shift;
        py = clampi(p[1], -32768, 32767) << a.shift;
    }
    px = __builtin_amdgcn_readfirstlane(px);
    py = __builtin_amdgcn_readfirstlane(py);

    const size_t fo = (size_t)frame * a.hs * a.ws;                                    // < 2^29 x 65535: size_t
    const uint8_t* fcur = cur + fo;
    const uint8_t* fref = ref + fo;
    const int bx0 = i * N, by0 = j * N;
    for (int t = lane; t < N * ND; t += 64) {                                         // the block lies inside the plane
        const int y = t / ND, k = t - y * ND;
        const size_t off = fo + (size_t)(by0 + y) * a.ws + (bx0 + 4 * k);
        uint32_t v;
        if (ms_whole(a, off)) v = ms_dword(cur, off);
        else v = ms_gather(fcur + (size_t)(by0 + y) * a.ws, bx0 + 4 * k, a.ws);
        cb[t] = v;
    }
    for (int t = lane; t < rows * wd; t += 64) {
        const int r = t / wd, k = t - r * wd;
        const int yy = clampi(by0 - R + py + r, 0, a.hs - 1), x = bx0 - R + px + 4 * k;
        const size_t off = fo + (size_t)yy * a.ws + (size_t)max(x, 0);
        uint32_t v;
        if (x >= 0 && x + 3 < a.ws && ms_whole(a, off)) v = ms_dword(ref, off);
        else v = ms_gather(fref + (size_t)yy * a.ws, x, a.ws);
        win[t] = v;
    }
    for (int t = lane; t < D * cw; t += 64) cost[t] = 0u;
    __syncthreads();

    {   // cost: item = ((gy gx + g) slices + s); slices = N >> rs_log2
        const int sl_log2 = (N == 8 ? 3 : N == 16 ? 4 : 5) - a.rs_log2, nitems = (D * a.gx) << sl_log2, RS = 1 << a.rs_log2;
        for (int t = lane; t < nitems; t += 64) {
            const int g = t >> sl_log2, s = t & ((1 << sl_log2) - 1);
            const int gy = (g * a.ginv) >> 16, gxi = g - gy * a.gx;
            unsigned long long acc = 0ull;
            for (int y = s * RS; y < (s + 1) * RS; ++y) {
                const uint32_t* wrow = win + (y + gy) * wd + gxi;
                const uint32_t* crow = cb + y * ND;
#pragma unroll
                for (int k = 0; k < ND; ++k) {
                    const unsigned long long w2 = (unsigned long long)wrow[k] | ((unsigned long long)wrow[k + 1] << 32);
                    acc = __builtin_amdgcn_qsad_pk_u16_u8(w2, crow[k], acc);
                }
            }
            uint32_t* c = cost + gy * cw + 4 * gxi;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * gxi + e < D) atomicAdd(&c[e], (uint32_t)(acc >> (16 * e)) & 0xffffu);
        }
    }
    uint32_t tex = 0u;
    for (int t = lane; t < N * ND; t += 64) {
        const int y = t / ND, k = t - y * ND;
        const uint32_t d = cb[t];
        const uint32_t nxt = k + 1 < ND ? cb[t + 1] : d >> 24;                        // the byte right of the dword; the last one's own: |b3 - b3| = 0
        tex = __builtin_amdgcn_sad_u8(d, __builtin_amdgcn_alignbyte(nxt, d, 1), tex);
        if (y + 1 < N) tex = __builtin_amdgcn_sad_u8(d, cb[t + ND], tex);
    }
    __syncthreads();

    unsigned long long best = ~0ull;
    for (int t = lane; t < D * cw; t += 64) {
        const int q4 = t >> 2, oyi = (q4 * a.ginv) >> 16, oxi = t - oyi * cw;
        if (oxi < D) {
            const int oy = oyi - R, ox = oxi - R;
            const unsigned long long key = ((unsigned long long)cost[t] << 15) | (unsigned long long)(((abs(oy) + abs(ox)) << 10) | (oyi << 5) | oxi);
            best = key < best ? key : best;
        }
    }
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        best = o < best ? o : best;
        tex += (uint32_t)__shfl_xor((int)tex, m);
    }
    if (live && lane == 0) {
        const int oxi = (int)(best & 31u), oyi = (int)((best >> 5) & 31u);
        out[(size_t)frame * a.nblk + bi] = make_int4(px + oxi - R, py + oyi - R, (int)(best >> 15), (int)tex);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_motion_desc_size(void) { return sizeof(rc_motion_desc); }

int rc_motion_pyramid(const void* d_src, int src_dtype, int matrix, int levels, void* const* d_levels, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && d_levels, "rc_motion_pyramid: null pointer");
    RgbSide src;
    if (int e = rgb_source("rc_motion_pyramid", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    RC_REQUIRE(batch <= 65535, "rc_motion_pyramid: bad shape (more than 65535 frames)");
    RC_REQUIRE((long long)H * W < (1LL << 29), "rc_motion_pyramid: bad shape (a source plane of 2^29 samples or more)");
    RC_REQUIRE(matrix >= RC_MATRIX_BT601 && matrix <= RC_MATRIX_BT2020, "rc_motion_pyramid: unknown matrix");
    RC_REQUIRE(levels >= 1 && levels <= RC_MOTION_MAX_LEVELS, "rc_motion_pyramid: levels must lie in 1 .. 4");
    RC_REQUIRE((h >> (levels - 1)) >= 1 && (w >> (levels - 1)) >= 1, "rc_motion_pyramid: the coarsest level is empty (h >> (levels - 1) or w >> (levels - 1) is 0)");
    PyramidArgs a = {};
    for (int k = 0; k < levels; ++k) {
        RC_REQUIRE(d_levels[k], "rc_motion_pyramid: null level pointer");
        a.lv[k] = static_cast<uint8_t*>(d_levels[k]);
    }
    a.levels = levels; a.H = H; a.W = W; a.h = h; a.w = w;
    a.vec_src = src.vec;
    a.vec0 = reinterpret_cast<uintptr_t>(a.lv[0]) % 4 == 0 && w % 4 == 0;
    a.vec1 = levels > 1 && reinterpret_cast<uintptr_t>(a.lv[1]) % 2 == 0 && (w >> 1) % 2 == 0;
    a.c = rgb_coef(matrix);
    const dim3 grid((unsigned)ceil_div(w, kPyrBlockW), (unsigned)ceil_div(h, kPyrBlockH), (unsigned)batch), block(kPyrThreads);
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        hipLaunchKernelGGL(motion_pyramid_kernel<TI>, grid, block, 0, as_stream(stream), a, static_cast<const TI*>(d_src));
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_motion_search(const uint8_t* d_cur, const uint8_t* d_ref, const rc_motion_desc* desc, const int* d_pred, int pred_by, int pred_bx,
                     int* d_out, int batch, int hs, int ws, void* stream) {
    RC_REQUIRE(d_cur && d_ref && desc && d_out, "rc_motion_search: null pointer");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_out) % 16 == 0, "rc_motion_search: the output must be 16-byte aligned");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_pred) % 16 == 0, "rc_motion_search: the predictor must be 16-byte aligned");
    const int N = desc->block, R = desc->range;
    RC_REQUIRE(N == 8 || N == 16 || N == 32, "rc_motion_search: block must be 8, 16 or 32");
    RC_REQUIRE(R >= 0 && R <= RC_MOTION_MAX_RANGE, "rc_motion_search: range must lie in 0 .. 8");
    RC_REQUIRE(desc->pred_shift == 0 || desc->pred_shift == 1, "rc_motion_search: pred_shift must be 0 or 1");
    for (int k = 0; k < 5; ++k) RC_REQUIRE(!desc->reserved[k], "rc_motion_search: reserved fields must be zero");
    RC_REQUIRE(batch >= 1 && hs >= 1 && ws >= 1, "rc_motion_search: bad shape (an empty plane)");
    RC_REQUIRE(batch <= 65535, "rc_motion_search: bad shape (more than 65535 frames)");
    RC_REQUIRE((long long)hs * ws < (1LL << 29), "rc_motion_search: bad shape (a plane of 2^29 samples or more)");
    const int by = hs / N, bx = ws / N;
    RC_REQUIRE(by >= 1 && bx >= 1, "rc_motion_search: the plane is smaller than one block");
    RC_REQUIRE(!d_pred || (pred_by >= 1 && pred_bx >= 1), "rc_motion_search: a predictor grid needs pred_by, pred_bx >= 1");

    SearchArgs a = {};
    a.hs = hs; a.ws = ws; a.by = by; a.bx = bx; a.nblk = by * bx;
    a.R = R; a.gx = (2 * R + 1 + 3) / 4; a.ginv = (65536 + a.gx - 1) / a.gx;
    // an item sums RS rows: as many as keep 64 items or more per wave, RS N <= 256 (the u16 sums), at most N
    const int groups = (2 * R + 1) * a.gx;
    int rs = 0;
    while ((2 << rs) * N <= 256 && (2 << rs) <= N && groups * (N >> (rs + 1)) >= 64) ++rs;
    a.rs_log2 = rs;
    a.pred_by = pred_by; a.pred_bx = pred_bx; a.shift = desc->pred_shift;
    a.total = (unsigned long long)batch * hs * ws;
    a.vec = reinterpret_cast<uintptr_t>(d_cur) % 4 == 0 && reinterpret_cast<uintptr_t>(d_ref) % 4 == 0;
    const dim3 grid((unsigned)ceil_div(a.nblk, kMsWaves), (unsigned)batch), block(kMsThreads);
    int4* out = reinterpret_cast<int4*>(d_out);
    const hipStream_t st = as_stream(stream);
    if (N == 8) hipLaunchKernelGGL(motion_search_kernel<8>, grid, block, 0, st, a, d_cur, d_ref, d_pred, out);
    else if (N == 16) hipLaunchKernelGGL(motion_search_kernel<16>, grid, block, 0, st, a, d_cur, d_ref, d_pred, out);
    else hipLaunchKernelGGL(motion_search_kernel<32>, grid, block, 0, st, a, d_cur, d_ref, d_pred, out);
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
