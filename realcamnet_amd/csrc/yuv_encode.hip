// Video-encoder output at the back of the path (include/realcam_hip.h, rc_yuv_encode): the network's planar sRGB result
// (B,3,H,W) -> one Y'CbCr 4:2:0 surface per frame -- NV12 (u8), P010 (u16, the 10-bit code in the high bits) or I420 (u8) -- with the
// caller's row pitch and plane offsets, in one launch that reads the result once.
//
// yuv420_kernel: one item = a strip of P pixels x 2 rows (P = 16 for the 8-bit layouts, 8 for P010: always 16 bytes of a Y row).  The
// strips of a row pair tile the whole PITCH, not just the image, and the row pairs tile the allocated rows, so the lanes that own
// pitch / height padding write it as zero in the same launch.  Arithmetic: fp32, every product and every sum rounded on its own in
// the order the header states (__fmul_rn / __fadd_rn: no contraction whatever the compile flags say), so the vector path, the
// element path and a plain elementwise restatement give the same bits.
#include "ycc_code.hpp"
#include "yuv_surface.hpp"

namespace rc {

constexpr int kYuvStrips = 64, kYuvPairs = 4, kYuvThreads = kYuvStrips * kYuvPairs;     // a block: 64 strips (one wave) x 4 row pairs

template <int LAYOUT> struct YuvOut { typedef uint8_t T; static constexpr int P = 16, SHIFT = 0; };
template <> struct YuvOut<RC_YUV_P010> { typedef uint16_t T; static constexpr int P = 8, SHIFT = 6; };

struct YuvArgs {
    int batch, H, W, h, w;
    int pitch;                 // bytes of a Y row (and of an NV12 / P010 chroma row); an I420 chroma row has pitch / 2
    int rows, crows;           // allocated rows of the Y plane (>= h) and of a chroma plane (ceil(rows / 2))
    int nstrip;                // ceil(pitch / 16): strips per row pair
    int vec_src, vec_dst;      // every source row segment / every destination strip is 16-byte aligned
    long long off_c0, off_c1;  // byte offsets of the CbCr (or Cb) plane and of the Cr plane in a frame
    long long frame;           // bytes from one frame to the next
    LumaChroma c;
    float ys, yo, ylo, yhi, cs, co, clo, chi;
};

__device__ __forceinline__ void ycc(const YuvArgs& a, float r, float g, float b, float& y, float& cb, float& cr) { ycc(a.c, r, g, b, y, cb, cr); }

// P codes of TO into the four dwords of a strip.
template <typename TO>
__device__ __forceinline__ void put(uint32_t* wd, int k, uint32_t c) {
    if constexpr (sizeof(TO) == 1) wd[k >> 2] |= c << (8 * (k & 3));
    else wd[k >> 1] |= c << (16 * (k & 1));
}
template <typename TO>
__device__ __forceinline__ TO get(const uint32_t* wd, int k) {
    if constexpr (sizeof(TO) == 1) return (TO)(wd[k >> 2] >> (8 * (k & 3)));
    else return (TO)(wd[k >> 1] >> (16 * (k & 1)));
}

// n elements of TO (16 bytes when n == P, 8 for an I420 chroma strip) at element e0 of a row of `row_elems` elements.
template <typename TO, int N>
__device__ __forceinline__ void store_strip(uint8_t* row, int e0, int row_elems, const uint32_t* wd, bool vec) {
    TO* o = reinterpret_cast<TO*>(row) + e0;
    if (vec) {
        if constexpr (N * sizeof(TO) == 16) *reinterpret_cast<uint4*>(o) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        else *reinterpret_cast<uint2*>(o) = make_uint2(wd[0], wd[1]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (e0 + k < row_elems) o[k] = get<TO>(wd, k);
    }
}

template <typename TI, int LAYOUT, int SITING>
__global__ void __launch_bounds__(kYuvThreads) yuv420_kernel(YuvArgs a, const TI* __restrict__ src, uint8_t* __restrict__ dst) {
    typedef typename YuvOut<LAYOUT>::T TO;
    constexpr int P = YuvOut<LAYOUT>::P, C = P / 2, SH = YuvOut<LAYOUT>::SHIFT, V = 16 / sizeof(TI);
    const size_t plane = (size_t)a.H * a.W;
    const int pitch_elems = a.pitch / (int)sizeof(TO);
    const int s = blockIdx.x * kYuvStrips + threadIdx.x, j = blockIdx.y * kYuvPairs + threadIdx.y, b = blockIdx.z;
    if (s < a.nstrip && j < a.crows) {
        const int x0 = s * P, y0 = 2 * j;
        uint32_t yw[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        uint32_t cw[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};     // NV12 / P010: cw[0] = the interleaved strip; I420: cw[0] Cb, cw[1] Cr (2 dwords each)
        if (y0 < a.h && x0 < a.w) {                                   // h and w are even: both rows and at least one pixel pair are inside
            float hb[2][C], hr[2][C];                                 // per row: the horizontal step of the chroma filter
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const TI* s0 = src + (size_t)b * 3 * plane + (size_t)(y0 + r) * a.W + x0;
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
                float cb[P + 1], cr[P + 1];                           // [k + 1]: pixel x0 + k; [0]: pixel x0 - 1, clamped to column 0
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    float y;
                    ycc(a, px[0][k], px[1][k], px[2][k], y, cb[k + 1], cr[k + 1]);
                    if (x0 + k < a.w) put<TO>(yw[r], k, code(y, a.ys, a.yo, a.ylo, a.yhi) << SH);
                }
                if constexpr (SITING == RC_SITING_LEFT) {
                    cb[0] = cb[1]; cr[0] = cr[1];
                    if (x0 > 0) {                                     // one element per plane, out of the line the lane to the left loads
                        float y;
                        ycc(a, to_f32(s0[-1]), to_f32(s0[plane - 1]), to_f32(s0[2 * plane - 1]), y, cb[0], cr[0]);
                    }
#pragma unroll
                    for (int q = 0; q < C; ++q) {
                        hb[r][q] = __fmul_rn(__fadd_rn(__fadd_rn(cb[2 * q], cb[2 * q + 2]), __fadd_rn(cb[2 * q + 1], cb[2 * q + 1])), 0.25f);
                        hr[r][q] = __fmul_rn(__fadd_rn(__fadd_rn(cr[2 * q], cr[2 * q + 2]), __fadd_rn(cr[2 * q + 1], cr[2 * q + 1])), 0.25f);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < C; ++q) {
                        hb[r][q] = __fadd_rn(cb[2 * q + 1], cb[2 * q + 2]);
                        hr[r][q] = __fadd_rn(cr[2 * q + 1], cr[2 * q + 2]);
                    }
                }
            }
            const float vs = SITING == RC_SITING_LEFT ? 0.5f : 0.25f;
#pragma unroll
            for (int q = 0; q < C; ++q) {
                if (x0 + 2 * q < a.w) {
                    const uint32_t ub = code(__fmul_rn(__fadd_rn(hb[0][q], hb[1][q]), vs), a.cs, a.co, a.clo, a.chi) << SH;
                    const uint32_t ur = code(__fmul_rn(__fadd_rn(hr[0][q], hr[1][q]), vs), a.cs, a.co, a.clo, a.chi) << SH;
                    if constexpr (LAYOUT == RC_YUV_I420) {
                        put<TO>(cw[0], q, ub);
                        put<TO>(cw[1], q, ur);
                    } else {
                        put<TO>(cw[0], 2 * q, ub);
                        put<TO>(cw[0], 2 * q + 1, ur);
                    }
                }
            }
        }
        uint8_t* frame = dst + (size_t)b * (size_t)a.frame;
        store_strip<TO, P>(frame + (size_t)y0 * a.pitch, x0, pitch_elems, yw[0], a.vec_dst);
        if (y0 + 1 < a.rows) store_strip<TO, P>(frame + (size_t)(y0 + 1) * a.pitch, x0, pitch_elems, yw[1], a.vec_dst);
        if constexpr (LAYOUT == RC_YUV_I420) {
            const int cpitch = a.pitch / 2;
            if (x0 / 2 < cpitch) {
                store_strip<TO, C>(frame + a.off_c0 + (size_t)j * cpitch, x0 / 2, cpitch, cw[0], a.vec_dst);
                store_strip<TO, C>(frame + a.off_c1 + (size_t)j * cpitch, x0 / 2, cpitch, cw[1], a.vec_dst);
            }
        } else {
            store_strip<TO, P>(frame + a.off_c0 + (size_t)j * a.pitch, x0, pitch_elems, cw[0], a.vec_dst);
        }
    }
}

// ---- host: the surface plan shared by rc_yuv_frame_bytes and rc_yuv_encode -----------------------------------------------------
struct YuvPlan {
    long long pitch, rows, crows, cpitch, off_c0, off_c1, frame;
    int esize;
};

// nullptr, or what is wrong with the format for an (h, w) frame.
static const char* yuv_plan(const rc_out_format* f, int h, int w, YuvPlan* p) {
    if (!f) return "null format";
    if (f->layout < RC_YUV_NV12 || f->layout > RC_YUV_I420) return "unknown layout";
    if (f->matrix < RC_MATRIX_BT601 || f->matrix > RC_MATRIX_BT2020) return "unknown matrix";
    if (f->range != RC_RANGE_LIMITED && f->range != RC_RANGE_FULL) return "unknown range";
    if (f->siting != RC_SITING_LEFT && f->siting != RC_SITING_CENTER) return "unknown siting";
    if (f->reserved[0] || f->reserved[1] || f->reserved[2] || f->reserved[3]) return "reserved fields must be zero";
    if (h < 2 || w < 2 || (h & 1) || (w & 1)) return "4:2:0 needs an even height and width (h, w >= 2)";
    const bool i420 = f->layout == RC_YUV_I420;
    p->esize = f->layout == RC_YUV_P010 ? 2 : 1;
    const long long row_bytes = (long long)w * p->esize;
    if (f->pitch < 0 || f->rows < 0 || f->chroma_offset[0] < 0 || f->chroma_offset[1] < 0) return "negative pitch, rows or chroma offset";
    p->pitch = f->pitch ? f->pitch : row_bytes;
    if (p->pitch < row_bytes) return "pitch shorter than one row";
    if (p->pitch % (i420 ? 2 : p->esize)) return "pitch must be a multiple of the sample size (I420: even, the chroma pitch is pitch / 2)";
    p->rows = f->rows ? f->rows : h;
    if (p->rows < h) return "rows below the frame height";
    p->crows = (p->rows + 1) / 2;
    p->cpitch = i420 ? p->pitch / 2 : p->pitch;
    const long long y_end = p->pitch * p->rows, c_bytes = p->cpitch * p->crows;
    p->off_c0 = f->chroma_offset[0] ? f->chroma_offset[0] : y_end;
    p->off_c1 = i420 ? (f->chroma_offset[1] ? f->chroma_offset[1] : p->off_c0 + c_bytes) : 0;
    if (!i420 && f->chroma_offset[1]) return "chroma_offset[1] is the I420 Cr plane: zero for NV12 / P010";
    if (p->off_c0 % p->esize || p->off_c1 % p->esize) return "chroma offset must be a multiple of the sample size";
    if (p->off_c0 < y_end || (i420 && p->off_c1 < y_end)) return "planes overlap: a chroma plane starts inside the Y plane";
    if (i420 && !(p->off_c1 >= p->off_c0 + c_bytes || p->off_c0 >= p->off_c1 + c_bytes)) return "planes overlap: Cb and Cr";
    p->frame = (i420 && p->off_c1 > p->off_c0 ? p->off_c1 : p->off_c0) + c_bytes;
    if (p->frame > 0x7fffffffLL) return "frame larger than 2 GiB";
    return nullptr;
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_out_format_size(void) { return sizeof(rc_out_format); }

size_t rc_yuv_frame_bytes(const rc_out_format* fmt, int h, int w) {
    YuvPlan p;
    const bool surface = fmt && yuv_surface_layout(fmt->layout);     // the layouts of yuv_surface.hip
    const char* err = surface ? yuv_surface_plan(fmt, h, w, &p.frame) : yuv_plan(fmt, h, w, &p);
    if (err) {
        fail(RC_ERR_INVALID, std::string("rc_yuv_frame_bytes: ") + err);
        return 0;
    }
    return (size_t)p.frame;
}

int rc_yuv_encode(const void* d_src, int src_dtype, const rc_out_format* fmt, void* d_dst, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && d_dst, "rc_yuv_encode: null pointer");
    RgbSide src;
    if (int e = rgb_source("rc_yuv_encode", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    if (yuv_surface_layout(fmt->layout)) return yuv_surface_encode(d_src, src_dtype, fmt, d_dst, batch, H, W, h, w, stream);
    YuvPlan p;
    const char* err = yuv_plan(fmt, h, w, &p);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_yuv_encode: ") + err);
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_dst) % 16 == 0, "rc_yuv_encode: dst must be 16-byte aligned");

    YuvArgs a;
    a.batch = batch; a.H = H; a.W = W; a.h = h; a.w = w;
    a.pitch = (int)p.pitch; a.rows = (int)p.rows; a.crows = (int)p.crows;
    a.nstrip = (int)((p.pitch + 15) / 16);
    a.off_c0 = p.off_c0; a.off_c1 = p.off_c1; a.frame = p.frame;
    a.vec_src = reinterpret_cast<uintptr_t>(d_src) % 16 == 0 && ((size_t)W * src.esize) % 16 == 0;        // a strip here is 16 bytes, not 4 pixels: every plane and row starts on 16 bytes
    a.vec_dst = p.pitch % 16 == 0 && p.off_c0 % 16 == 0 && p.off_c1 % 8 == 0 && p.frame % 16 == 0;
    a.c = rgb_coef(fmt->matrix);
    const int n = fmt->layout == RC_YUV_P010 ? 10 : 8;
    const float k = (float)(1 << (n - 8)), top = (float)((1 << n) - 1);
    if (fmt->range == RC_RANGE_LIMITED) {
        a.ys = 219.f * k; a.yo = 16.f * k; a.ylo = 16.f * k; a.yhi = 235.f * k;
        a.cs = 224.f * k; a.co = 128.f * k; a.clo = 16.f * k; a.chi = 240.f * k;
    } else {
        a.ys = top; a.yo = 0.f; a.ylo = 0.f; a.yhi = top;
        a.cs = top; a.co = (float)(1 << (n - 1)); a.clo = 0.f; a.chi = top;
    }
    const dim3 grid((a.nstrip + kYuvStrips - 1) / kYuvStrips, (a.crows + kYuvPairs - 1) / kYuvPairs, batch);
    RC_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "rc_yuv_encode: more than 65535 frames or 524280 rows");
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kYuvStrips, kYuvPairs), 0, as_stream(stream), a, static_cast<const TI*>(d_src), static_cast<uint8_t*>(d_dst)); };
        const bool left = fmt->siting == RC_SITING_LEFT;
        if (fmt->layout == RC_YUV_NV12) launch(left ? yuv420_kernel<TI, RC_YUV_NV12, RC_SITING_LEFT> : yuv420_kernel<TI, RC_YUV_NV12, RC_SITING_CENTER>);
        else if (fmt->layout == RC_YUV_P010) launch(left ? yuv420_kernel<TI, RC_YUV_P010, RC_SITING_LEFT> : yuv420_kernel<TI, RC_YUV_P010, RC_SITING_CENTER>);
        else launch(left ? yuv420_kernel<TI, RC_YUV_I420, RC_SITING_LEFT> : yuv420_kernel<TI, RC_YUV_I420, RC_SITING_CENTER>);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
