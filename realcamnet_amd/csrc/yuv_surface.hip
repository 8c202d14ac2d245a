// The professional video surfaces of rc_yuv_encode (include/realcam_hip.h, the layouts from RC_YUV_NV16 on): the network's planar sRGB
// result (B,3,H,W) -> one Y'CbCr 4:2:2 / 4:4:4 / planar 10-bit 4:2:0 surface per frame -- planar, semi-planar, packed YUYV / UYVY or V210
// -- with the caller's row pitch and plane offsets, in one launch that reads the result once.
//
// yuv_surface_kernel keeps yuv420_kernel's shape (yuv_encode.hip): one item = a strip of P pixels of one row (of a row pair for 4:2:0);
// P = 16 / 8 for the 8- / 16-bit layouts (always 16 bytes of a Y row) and 24 for V210 (four groups: 64 bytes out, and 96 / 48 bytes of an
// fp32 / 16-bit source row, whole 16-byte accesses both).  The strips of a row tile the whole PITCH and the rows the allocated rows, so the
// lanes that own pitch / height padding write it as zero in the same launch.  A block row is a wave of strips (half a wave for V210), so for
// LEFT siting the chroma of column x0 - 1 comes from the lane to the left; only the first lane of a block row reloads it.  Arithmetic: ycc() / code() of
// ycc_code.hpp and __fmul_rn / __fadd_rn, as the header states it.
#include "ycc_code.hpp"
#include "yuv_surface.hpp"

namespace rc {

enum SurfContainer { kPlanar = 0, kSemi = 1, kYuyv = 2, kUyvy = 3, kV210 = 4 };

constexpr int kSurfThreads = 256;
// A block: 64 strips (one wave) x 4 rows (row pairs); V210: 32 strips x 8 rows, a wave being two rows of 32 -- a 3840-pixel row is 160 strips,
// five whole blocks (measured against 64 and 16: DESIGN 4.j).  The strips of a block row divide the wave, so lane - 1 is the strip to the left.
constexpr int surf_strips(int cont) { return cont == kV210 ? 32 : 64; }

struct SurfArgs {
    int H, W, h, w;
    int pitch, cpitch;         // bytes of a row of the first plane and of a chroma plane
    int rows;                  // allocated rows of the first plane (>= h)
    int nrow;                  // row items: rows, or ceil(rows / 2) row pairs for 4:2:0 (the allocated chroma rows)
    int nstrip;                // strips per row: ceil(pitch / bytes a strip writes to the first plane)
    int vec_src, vec_dst;      // every source row segment / every destination strip is 16-byte aligned (8 for a half-width chroma strip)
    long long off_c0, off_c1;  // byte offsets of the CbCr (or Cb) plane and of the Cr plane in a frame
    long long frame;           // bytes from one frame to the next
    LumaChroma c;
    float ys, yo, ylo, yhi, cs, co, clo, chi;
};

// Element k of ES bytes into the dwords of a strip.
template <int ES>
__device__ __forceinline__ void put(uint32_t* wd, int k, uint32_t c) {
    if constexpr (ES == 1) wd[k >> 2] |= c << (8 * (k & 3));
    else wd[k >> 1] |= c << (16 * (k & 1));
}

// NB bytes (8, 16, 32 or 64) at byte `at` of a row of `row_bytes` bytes: 16-byte (8-byte) stores, or elements of E bytes one by one.  Both
// stop at the row's end.
template <int NB, int E>
__device__ __forceinline__ void store_bytes(uint8_t* row, int at, int row_bytes, const uint32_t* wd, bool vec) {
    if (vec) {
        if constexpr (NB == 8) {
            if (at < row_bytes) *reinterpret_cast<uint2*>(row + at) = make_uint2(wd[0], wd[1]);
        } else {
#pragma unroll
            for (int i = 0; i < NB / 16; ++i)
                if (at + 16 * i < row_bytes) *reinterpret_cast<uint4*>(row + at + 16 * i) = make_uint4(wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NB / E; ++k) {
            if (at + k * E < row_bytes) {
                if constexpr (E == 1) row[at + k] = (uint8_t)(wd[k >> 2] >> (8 * (k & 3)));
                else if constexpr (E == 2) *reinterpret_cast<uint16_t*>(row + at + 2 * k) = (uint16_t)(wd[k >> 1] >> (16 * (k & 1)));
                else *reinterpret_cast<uint32_t*>(row + at + 4 * k) = wd[k];
            }
        }
    }
}

// The row step of the chroma filter at an even column: l, c0, c1 = c[x-1], c[x], c[x+1].  4:2:0 CENTER leaves the 0.25 to the vertical step,
// as yuv420_kernel does.
template <int SUB, int SITING>
__device__ __forceinline__ float chroma_row(float l, float c0, float c1) {
    if constexpr (SITING == RC_SITING_LEFT) return __fmul_rn(__fadd_rn(__fadd_rn(l, c1), __fadd_rn(c0, c0)), 0.25f);
    else if constexpr (SUB == 420) return __fadd_rn(c0, c1);
    else return __fmul_rn(__fadd_rn(c0, c1), 0.5f);
}

// SUB 420 / 422 / 444; BITS 8 / 10; CONT a SurfContainer; SHIFT 6 for the layouts with the code in the high bits.
template <typename TI, int SUB, int BITS, int CONT, int SHIFT, int SITING>
__global__ void __launch_bounds__(kSurfThreads) yuv_surface_kernel(SurfArgs a, const TI* __restrict__ src, uint8_t* __restrict__ dst) {
    constexpr int ES = BITS == 8 ? 1 : 2;                             // bytes of a stored sample (a V210 row is stored by dwords)
    constexpr int P = CONT == kV210 ? 24 : 16 / ES, R = SUB == 420 ? 2 : 1, SX = SUB == 444 ? 1 : 2, C = P / SX, V = 16 / sizeof(TI);
    constexpr bool kLeft = SUB != 444 && SITING == RC_SITING_LEFT;
    const size_t plane = (size_t)a.H * a.W;
    constexpr int BS = surf_strips(CONT), BR = kSurfThreads / BS;
    const int s = blockIdx.x * BS + threadIdx.x, j = blockIdx.y * BR + threadIdx.y, b = blockIdx.z;
    const bool item = s < a.nstrip && j < a.nrow;
    const int x0 = s * P, y0 = R * j;
    const bool inside = item && y0 < a.h && x0 < a.w;                 // 4:2:0: h is even, both rows are inside
    uint32_t yc[R][P], qb[C], qr[C];                                  // the codes; zero where there is no sample
    float hb[R][C], hr[R][C];
#pragma unroll
    for (int q = 0; q < C; ++q) qb[q] = qr[q] = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float cb[P], cr[P];
#pragma unroll
        for (int k = 0; k < P; ++k) { yc[r][k] = 0u; cb[k] = cr[k] = 0.f; }
        const TI* s0 = src + (size_t)b * 3 * plane + (size_t)(y0 + r) * a.W + x0;
        if (inside) {
            float px[3][P];
            if (a.vec_src && x0 + P <= a.W) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < P / V; ++k) Vec16<TI>::unpack(*reinterpret_cast<const uint4*>(s0 + c * plane + k * V), &px[c][k * V]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < P; ++k) px[c][k] = x0 + k < a.w ? to_f32(s0[c * plane + k]) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < P; ++k) {
                float y;
                ycc(a.c, px[0][k], px[1][k], px[2][k], y, cb[k], cr[k]);
                if (x0 + k < a.w) yc[r][k] = code(y, a.ys, a.yo, a.ylo, a.yhi) << SHIFT;
            }
        }
        if constexpr (kLeft) {
            // column x0 - 1: the last pixel of the lane to the left, which is inside whenever this lane is.  Every lane of the wave takes part.
            float lb = __shfl_up(cb[P - 1], 1), lr = __shfl_up(cr[P - 1], 1);
            if (inside) {
                if (x0 == 0) {                                        // clamped to column 0
                    lb = cb[0]; lr = cr[0];
                } else if (threadIdx.x == 0) {                        // no lane to the left in this block row: one element per plane
                    float y;
                    ycc(a.c, to_f32(s0[-1]), to_f32(s0[plane - 1]), to_f32(s0[2 * plane - 1]), y, lb, lr);
                }
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    hb[r][q] = chroma_row<SUB, SITING>(q ? cb[2 * q - 1] : lb, cb[2 * q], cb[2 * q + 1]);
                    hr[r][q] = chroma_row<SUB, SITING>(q ? cr[2 * q - 1] : lr, cr[2 * q], cr[2 * q + 1]);
                }
            }
        } else if constexpr (SUB != 444) {
#pragma unroll
            for (int q = 0; q < C; ++q) {
                hb[r][q] = chroma_row<SUB, SITING>(0.f, cb[2 * q], cb[2 * q + 1]);
                hr[r][q] = chroma_row<SUB, SITING>(0.f, cr[2 * q], cr[2 * q + 1]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < C; ++q) { hb[r][q] = cb[q]; hr[r][q] = cr[q]; }
        }
    }
    if (inside) {
#pragma unroll
        for (int q = 0; q < C; ++q) {
            if (x0 + SX * q < a.w) {
                float vb = hb[0][q], vr = hr[0][q];
                if constexpr (SUB == 420) {
                    const float vs = SITING == RC_SITING_LEFT ? 0.5f : 0.25f;
                    vb = __fmul_rn(__fadd_rn(hb[0][q], hb[R - 1][q]), vs);
                    vr = __fmul_rn(__fadd_rn(hr[0][q], hr[R - 1][q]), vs);
                }
                qb[q] = code(vb, a.cs, a.co, a.clo, a.chi) << SHIFT;
                qr[q] = code(vr, a.cs, a.co, a.clo, a.chi) << SHIFT;
            }
        }
    }
    if (!item) return;
    uint8_t* frame = dst + (size_t)b * (size_t)a.frame;
    if constexpr (CONT == kPlanar || CONT == kSemi) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < P; ++k) put<ES>(wd, k, yc[r][k]);
            if (y0 + r < a.rows) store_bytes<16, ES>(frame + (size_t)(y0 + r) * a.pitch, x0 * ES, a.pitch, wd, a.vec_dst);
        }
        uint8_t* c0 = frame + a.off_c0 + (size_t)j * a.cpitch;        // the chroma row: j is the row, or the row pair for 4:2:0
        if constexpr (CONT == kSemi) {
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < C; ++q) { put<ES>(wd, 2 * q, qb[q]); put<ES>(wd, 2 * q + 1, qr[q]); }
            store_bytes<16, ES>(c0, x0 * ES, a.cpitch, wd, a.vec_dst);
        } else {
            uint32_t wb[4] = {0u, 0u, 0u, 0u}, wr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < C; ++q) { put<ES>(wb, q, qb[q]); put<ES>(wr, q, qr[q]); }
            store_bytes<16 / SX, ES>(c0, x0 / SX * ES, a.cpitch, wb, a.vec_dst);
            store_bytes<16 / SX, ES>(frame + a.off_c1 + (size_t)j * a.cpitch, x0 / SX * ES, a.cpitch, wr, a.vec_dst);
        }
    } else if constexpr (CONT == kYuyv || CONT == kUyvy) {
        constexpr int YO = CONT == kYuyv ? 0 : 1;                     // where Y stands in a sample pair
        uint32_t wd[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < C; ++q) {
            put<ES>(wd, 4 * q + YO, yc[0][2 * q]);
            put<ES>(wd, 4 * q + 1 - YO, qb[q]);
            put<ES>(wd, 4 * q + 2 + YO, yc[0][2 * q + 1]);
            put<ES>(wd, 4 * q + 3 - YO, qr[q]);
        }
        store_bytes<32, ES>(frame + (size_t)y0 * a.pitch, 2 * x0 * ES, a.pitch, wd, a.vec_dst);
    } else {
        uint32_t wd[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t* y = &yc[0][6 * g];
            const uint32_t *cb = &qb[3 * g], *cr = &qr[3 * g];
            wd[4 * g] = cb[0] | y[0] << 10 | cr[0] << 20;
            wd[4 * g + 1] = y[1] | cb[1] << 10 | y[2] << 20;
            wd[4 * g + 2] = cr[1] | y[3] << 10 | cb[2] << 20;
            wd[4 * g + 3] = y[4] | cr[2] << 10 | y[5] << 20;
        }
        store_bytes<64, 4>(frame + (size_t)y0 * a.pitch, s * 64, a.pitch, wd, a.vec_dst);
    }
}

// ---- host: the surface plan and the launch ------------------------------------------------------------------------------------------
struct SurfLayout { int sub, bits, cont, shift; };

static SurfLayout surf_layout(int layout) {
    switch (layout) {
        case RC_YUV_NV16: return {422, 8, kSemi, 0};
        case RC_YUV_P210: return {422, 10, kSemi, 6};
        case RC_YUV_I422: return {422, 8, kPlanar, 0};
        case RC_YUV_I210: return {422, 10, kPlanar, 0};
        case RC_YUV_I010: return {420, 10, kPlanar, 0};
        case RC_YUV_I444: return {444, 8, kPlanar, 0};
        case RC_YUV_I410: return {444, 10, kPlanar, 0};
        case RC_YUV_YUY2: return {422, 8, kYuyv, 0};
        case RC_YUV_UYVY: return {422, 8, kUyvy, 0};
        case RC_YUV_Y210: return {422, 10, kYuyv, 6};
        default: return {422, 10, kV210, 0};
    }
}

struct SurfPlan {
    long long pitch, cpitch, rows, crows, off_c0, off_c1, frame;
    int esize, strip_bytes;    // bytes of a sample; bytes a strip writes to the first plane
};

// nullptr, or what is wrong with the format for an (h, w) frame.
static const char* surf_plan(const rc_out_format* f, int h, int w, SurfPlan* p) {
    if (!f) return "null format";
    if (!yuv_surface_layout(f->layout)) return "unknown layout";
    if (f->matrix < RC_MATRIX_BT601 || f->matrix > RC_MATRIX_BT2020) return "unknown matrix";
    if (f->range != RC_RANGE_LIMITED && f->range != RC_RANGE_FULL) return "unknown range";
    if (f->siting != RC_SITING_LEFT && f->siting != RC_SITING_CENTER) return "unknown siting";
    if (f->reserved[0] || f->reserved[1] || f->reserved[2] || f->reserved[3]) return "reserved fields must be zero";
    const SurfLayout l = surf_layout(f->layout);
    if (l.sub == 420 && (h < 2 || w < 2 || (h & 1) || (w & 1))) return "4:2:0 needs an even height and width (h, w >= 2)";
    if (l.sub == 422 && (h < 1 || w < 2 || (w & 1))) return "4:2:2 needs an even width (w >= 2, h >= 1)";
    if (h < 1 || w < 1) return "an empty frame";
    const bool planar = l.cont == kPlanar, semi = l.cont == kSemi, half = planar && l.sub != 444;      // half: the chroma pitch is pitch / 2
    p->esize = l.bits == 8 ? 1 : 2;
    const long long row_bytes = l.cont == kV210 ? (long long)((w + 5) / 6) * 16 : (long long)w * p->esize * (planar || semi ? 1 : 2);
    const int unit = l.cont == kV210 ? 4 : (half ? 2 * p->esize : p->esize);
    p->strip_bytes = l.cont == kV210 ? 64 : (planar || semi ? 16 : 32);
    if (f->pitch < 0 || f->rows < 0 || f->chroma_offset[0] < 0 || f->chroma_offset[1] < 0) return "negative pitch, rows or chroma offset";
    p->pitch = f->pitch ? f->pitch : row_bytes;
    if (p->pitch < row_bytes) return "pitch shorter than one row";
    if (p->pitch % unit) return "pitch must be a multiple of the sample size (twice it where the chroma pitch is pitch / 2; 4 for V210)";
    p->rows = f->rows ? f->rows : h;
    if (p->rows < h) return "rows below the frame height";
    p->crows = l.sub == 420 ? (p->rows + 1) / 2 : p->rows;
    p->cpitch = half ? p->pitch / 2 : p->pitch;
    const long long y_end = p->pitch * p->rows, c_bytes = p->cpitch * p->crows;
    p->off_c0 = p->off_c1 = 0;
    if (!planar && !semi) {
        if (f->chroma_offset[0] || f->chroma_offset[1]) return "chroma_offset must be zero for a one-plane layout (YUY2 / UYVY / Y210 / V210)";
        p->frame = y_end;
    } else {
        p->off_c0 = f->chroma_offset[0] ? f->chroma_offset[0] : y_end;
        if (semi && f->chroma_offset[1]) return "chroma_offset[1] is a planar layout's Cr plane: zero for NV16 / P210";
        if (planar) p->off_c1 = f->chroma_offset[1] ? f->chroma_offset[1] : p->off_c0 + c_bytes;
        if (p->off_c0 % p->esize || p->off_c1 % p->esize) return "chroma offset must be a multiple of the sample size";
        if (p->off_c0 < y_end || (planar && p->off_c1 < y_end)) return "planes overlap: a chroma plane starts inside the Y plane";
        if (planar && !(p->off_c1 >= p->off_c0 + c_bytes || p->off_c0 >= p->off_c1 + c_bytes)) return "planes overlap: Cb and Cr";
        p->frame = (planar && p->off_c1 > p->off_c0 ? p->off_c1 : p->off_c0) + c_bytes;
    }
    if (p->frame > 0x7fffffffLL) return "frame larger than 2 GiB";
    return nullptr;
}

const char* yuv_surface_plan(const rc_out_format* f, int h, int w, long long* frame_bytes) {
    SurfPlan p;
    const char* err = surf_plan(f, h, w, &p);
    if (!err) *frame_bytes = p.frame;
    return err;
}

template <typename TI, int SUB, int BITS, int CONT, int SHIFT>
static void surf_launch(bool left, hipStream_t stream, const SurfArgs& a, int batch, const void* d_src, void* d_dst) {
    constexpr int BS = surf_strips(CONT), BR = kSurfThreads / BS;
    const dim3 grid((a.nstrip + BS - 1) / BS, (a.nrow + BR - 1) / BR, batch);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(BS, BR), 0, stream, a, static_cast<const TI*>(d_src), static_cast<uint8_t*>(d_dst)); };
    if constexpr (SUB == 444) launch(yuv_surface_kernel<TI, SUB, BITS, CONT, SHIFT, RC_SITING_CENTER>);      // no chroma step: one instantiation
    else launch(left ? yuv_surface_kernel<TI, SUB, BITS, CONT, SHIFT, RC_SITING_LEFT> : yuv_surface_kernel<TI, SUB, BITS, CONT, SHIFT, RC_SITING_CENTER>);
}

int yuv_surface_encode(const void* d_src, int src_dtype, const rc_out_format* fmt, void* d_dst, int batch, int H, int W, int h, int w, void* stream) {
    SurfPlan p;
    const char* err = surf_plan(fmt, h, w, &p);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_yuv_encode: ") + err);
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_dst) % 16 == 0, "rc_yuv_encode: dst must be 16-byte aligned");
    const SurfLayout l = surf_layout(fmt->layout);

    SurfArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w;
    a.pitch = (int)p.pitch; a.cpitch = (int)p.cpitch; a.rows = (int)p.rows; a.nrow = (int)p.crows;
    a.nstrip = (int)((p.pitch + p.strip_bytes - 1) / p.strip_bytes);
    a.off_c0 = p.off_c0; a.off_c1 = p.off_c1; a.frame = p.frame;
    a.vec_src = reinterpret_cast<uintptr_t>(d_src) % 16 == 0 && ((size_t)W * dtype_size(src_dtype)) % 16 == 0;     // a strip's P elements are whole 16-byte words: every plane and row starts on 16 bytes
    const long long calign = p.cpitch == p.pitch ? 16 : 8;           // a half-width chroma strip is 8 bytes
    a.vec_dst = p.pitch % 16 == 0 && p.cpitch % calign == 0 && p.off_c0 % calign == 0 && p.off_c1 % calign == 0 && p.frame % 16 == 0;
    a.c = rgb_coef(fmt->matrix);
    const float k = (float)(1 << (l.bits - 8)), top = (float)((1 << l.bits) - 1);
    if (fmt->range == RC_RANGE_LIMITED) {
        a.ys = 219.f * k; a.yo = 16.f * k; a.ylo = 16.f * k; a.yhi = 235.f * k;
        a.cs = 224.f * k; a.co = 128.f * k; a.clo = 16.f * k; a.chi = 240.f * k;
    } else {
        a.ys = top; a.yo = 0.f; a.ylo = 0.f; a.yhi = top;
        a.cs = top; a.co = (float)(1 << (l.bits - 1)); a.clo = 0.f; a.chi = top;
    }
    RC_REQUIRE(a.nrow <= 4 * 65535 && batch <= 65535, "rc_yuv_encode: more than 65535 frames or 262140 rows");
    const bool left = fmt->siting == RC_SITING_LEFT;
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        const hipStream_t st = as_stream(stream);
        switch (fmt->layout) {
            case RC_YUV_NV16: surf_launch<TI, 422, 8, kSemi, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_P210: surf_launch<TI, 422, 10, kSemi, 6>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_I422: surf_launch<TI, 422, 8, kPlanar, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_I210: surf_launch<TI, 422, 10, kPlanar, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_I010: surf_launch<TI, 420, 10, kPlanar, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_I444: surf_launch<TI, 444, 8, kPlanar, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_I410: surf_launch<TI, 444, 10, kPlanar, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_YUY2: surf_launch<TI, 422, 8, kYuyv, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_UYVY: surf_launch<TI, 422, 8, kUyvy, 0>(left, st, a, batch, d_src, d_dst); break;
            case RC_YUV_Y210: surf_launch<TI, 422, 10, kYuyv, 6>(left, st, a, batch, d_src, d_dst); break;
            default: surf_launch<TI, 422, 10, kV210, 0>(left, st, a, batch, d_src, d_dst); break;
        }
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // namespace rc
