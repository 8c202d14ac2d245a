// Sensor RAW formats at the front and back of the path (include/realcam_hip.h, rc_raw_ingest_fmt / rc_rgb_encode).
//
// raw_ingest_fmt_kernel: rc_raw_ingest (pointwise.hip) generalised to the frames a camera stack delivers -- any Bayer phase,
// per-CFA-position black levels, and the sample storages float / uint16 / uint8 / MIPI CSI-2 RAW10 / RAW12 with a padded line
// stride.  Same item split, same arithmetic, same stores: with an RGGB phase and four equal black levels it computes, value
// for value, what raw_ingest_kernel computes from the same counts.
// rgb_encode_kernel: planar (B,3,H,W) float result -> interleaved (B,h,w,3) uint8 / uint16, round-half-even and clamped.
#include "raw_row.hpp"

namespace rc {

constexpr int kRfThreads = 256;

static inline int rf_grid(size_t n_items, int cap = 1 << 22) {
    size_t g = (n_items + kRfThreads - 1) / kRfThreads;
    if (g < 1) g = 1;
    if (g > (size_t)cap) g = cap;
    return (int)g;
}

struct IngestArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * 2h + r) * line_bytes
    int batch, h, w, hp, wp, ch, cw;
    int line_bytes;
    int pos;                   // cell position (2 bits, (row << 1) | col) that packed slot k reads: (pos >> 2k) & 3
    float black[4], inv[4];    // per packed slot: the black level of that slot's position and 1 / (white - black), fp32 on the host
    float scale_y, scale_x;
};

// One sample of a mosaic row (the cond image's random taps: scalar byte reads, B*4*ch*cw*4 of them).
template <int ST, typename TI>
__device__ __forceinline__ float sample(const uint8_t* row, int x) {
    if constexpr (ST == kElem) {
        return to_f32(reinterpret_cast<const TI*>(row)[x]);
    } else if constexpr (ST == kMipi10) {
        const uint8_t* g = row + (size_t)(x >> 2) * 5;
        return raw10_value(g[x & 3], g[4], x & 3);
    } else {
        const uint8_t* g = row + (size_t)(x >> 1) * 3;
        return raw12_value(g[x & 1], g[2], x & 1);
    }
}

// Samples x0 .. x0 + n - 1 (n = 2 or 4, x0 % 4 == 0) of a mosaic row into v[0..3] (v[2], v[3] = 0 when n == 2).  A wave covers
// 64 consecutive 4-sample quads of one row: 320 contiguous bytes of a RAW10 line, 384 of a RAW12 line.
template <int ST, typename TI>
__device__ __forceinline__ void load_quad(const uint8_t* row, size_t row_off, int x0, int n, float* v) {
    if constexpr (ST == kElem) {
        const TI* p = reinterpret_cast<const TI*>(row + row_off) + x0;
        v[0] = to_f32(p[0]); v[1] = to_f32(p[1]);
        v[2] = n == 4 ? to_f32(p[2]) : 0.f; v[3] = n == 4 ? to_f32(p[3]) : 0.f;
    } else {
        const uint64_t g = window_at(row, row_off + packed_offset<ST, size_t>(x0), packed_bytes<ST>(n));
        if constexpr (ST == kMipi10) unpack_raw10(g, v);
        else unpack_raw12(g, n, v);
    }
}

template <typename TO>
__device__ __forceinline__ void store_px(TO* o, const float* v) {
    if constexpr (sizeof(TO) == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        uint2 p;
        p.x = Vec16<TO>::rne2(v[0], v[1]);
        p.y = Vec16<TO>::rne2(v[2], v[3]);
        *reinterpret_cast<uint2*>(o) = p;
    }
}

// Items [0, B*hp*ceil(wp/2)): two horizontally adjacent packed pixels each (4 samples of mosaic rows 2y and 2y+1); items
// [.., + B*ch*cw): one cond pixel each, all 4 slots, with raw_ingest_kernel's F.interpolate(bilinear, align_corners=False) taps.
template <int ST, typename TI, typename TO>
__global__ void __launch_bounds__(kRfThreads) raw_ingest_fmt_kernel(IngestArgs a, TO* __restrict__ packed, TO* __restrict__ cond) {
    const int h = a.h, w = a.w, hp = a.hp, wp = a.wp;
    const int wq = (wp + 1) >> 1;
    const size_t n_packed = (size_t)a.batch * hp * wq, n_cond = (size_t)a.batch * a.ch * a.cw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_packed + n_cond; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n_packed) {
            const int q = (int)(i % wq);
            const int y = (int)((i / wq) % hp);
            const int b = (int)(i / ((size_t)wq * hp));
            float px[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            if (y < h && 2 * q < w) {
                const int n = 2 * q + 1 < w ? 4 : 2;
                float r[2][4];
                const size_t off0 = ((size_t)b * 2 * h + 2 * y) * (size_t)a.line_bytes;
                load_quad<ST, TI>(a.src, off0, 4 * q, n, r[0]);
                load_quad<ST, TI>(a.src, off0 + (size_t)a.line_bytes, 4 * q, n, r[1]);
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int pos = (a.pos >> (2 * k)) & 3;
                        px[p][k] = (r[pos >> 1][2 * p + (pos & 1)] - a.black[k]) * a.inv[k];
                    }
                if (n == 2) px[1][0] = px[1][1] = px[1][2] = px[1][3] = 0.f;
            }
            TO* o = packed + (((size_t)b * hp + y) * wp + 2 * q) * 4;
            store_px<TO>(o, px[0]);
            if (2 * q + 1 < wp) store_px<TO>(o + 4, px[1]);
        } else {
            const size_t j = i - n_packed;
            const int ox = (int)(j % a.cw);
            const int oy = (int)((j / a.cw) % a.ch);
            const int b = (int)(j / ((size_t)a.cw * a.ch));
            float sy = a.scale_y * ((float)oy + 0.5f) - 0.5f; sy = sy < 0.f ? 0.f : sy;
            float sx = a.scale_x * ((float)ox + 0.5f) - 0.5f; sx = sx < 0.f ? 0.f : sx;
            int y0 = (int)sy, x0 = (int)sx;
            y0 = y0 < h - 1 ? y0 : h - 1; x0 = x0 < w - 1 ? x0 : w - 1;
            const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
            const float ly1 = sy - (float)y0, ly0 = 1.f - ly1, lx1 = sx - (float)x0, lx0 = 1.f - lx1;
            const uint8_t* img = a.src + (size_t)b * 2 * h * (size_t)a.line_bytes;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int pos = (a.pos >> (2 * k)) & 3, di = pos >> 1, dj = pos & 1;
                const uint8_t* r0 = img + (size_t)(2 * y0 + di) * a.line_bytes;
                const uint8_t* r1 = img + (size_t)(2 * y1 + di) * a.line_bytes;
                const float v00 = (sample<ST, TI>(r0, 2 * x0 + dj) - a.black[k]) * a.inv[k];
                const float v01 = (sample<ST, TI>(r0, 2 * x1 + dj) - a.black[k]) * a.inv[k];
                const float v10 = (sample<ST, TI>(r1, 2 * x0 + dj) - a.black[k]) * a.inv[k];
                const float v11 = (sample<ST, TI>(r1, 2 * x1 + dj) - a.black[k]) * a.inv[k];
                const float r = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
                cond[(((size_t)b * 4 + k) * a.ch + oy) * a.cw + ox] = from_f32<TO>(r);
            }
        }
    }
}

// ---- rgb_encode: planar (B,3,H,W) -> interleaved (B,h,w,3) uint8 / uint16 -------------------------------------------
// One item = P consecutive output pixels (16 for 8 bits, 8 for 16 bits: 48 bytes, three 16-byte stores).  The output is
// dense, so items are cut from the flat pixel index; an item inside one source row whose plane segments are 16-byte aligned
// reads them as 16-byte vectors, any other item (ragged widths, the last partial item) goes sample by sample.
template <int BITS> struct RgbOut;
template <> struct RgbOut<8> { typedef uint8_t T; static constexpr int P = 16; static constexpr float S = 255.f; };
template <> struct RgbOut<16> { typedef uint16_t T; static constexpr int P = 8; static constexpr float S = 65535.f; };

template <int BITS>
__device__ __forceinline__ uint32_t quantise(float v) {
    const float S = RgbOut<BITS>::S;
    float q = rintf(v * S);                    // round half to even, as torch.round
    q = q > 0.f ? (q < S ? q : S) : 0.f;       // NaN compares false: 0
    return (uint32_t)q;
}

template <typename TI, int BITS>
__global__ void __launch_bounds__(kRfThreads) rgb_encode_kernel(const TI* __restrict__ src, typename RgbOut<BITS>::T* __restrict__ dst,
                                                                int batch, int H, int W, int h, int w) {
    typedef typename RgbOut<BITS>::T TO;
    constexpr int P = RgbOut<BITS>::P, V = 16 / sizeof(TI);          // V: samples per 16-byte load
    const size_t total = (size_t)batch * h * w, n_items = (total + P - 1) / P;
    const size_t plane = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p0 = i * P;
        const int x0 = (int)(p0 % w);
        const size_t by = p0 / w;
        const int y = (int)(by % h), b = (int)(by / h);
        const TI* s0 = src + (size_t)b * 3 * plane + (size_t)y * W + x0;
        if (p0 + P <= total && x0 + P <= w && (reinterpret_cast<uintptr_t>(s0) & 15) == 0 && ((plane * sizeof(TI)) & 15) == 0) {
            float v[3][P];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < P / V; ++k)
                    Vec16<TI>::unpack(*reinterpret_cast<const uint4*>(s0 + c * plane + k * V), &v[c][k * V]);
            uint32_t o[12];
#pragma unroll
            for (int d = 0; d < 12; ++d) o[d] = 0u;
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = 3 * p + c;
                    if constexpr (BITS == 8) o[e >> 2] |= quantise<8>(v[c][p]) << (8 * (e & 3));
                    else o[e >> 1] |= quantise<16>(v[c][p]) << (16 * (e & 1));
                }
            uint4* d4 = reinterpret_cast<uint4*>(dst + p0 * 3);
            d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
        } else {
            const size_t pe = p0 + P < total ? p0 + P : total;
            for (size_t p = p0; p < pe; ++p) {
                const int x = (int)(p % w);
                const size_t pby = p / w;
                const int py = (int)(pby % h), pb = (int)(pby / h);
                const TI* s = src + (size_t)pb * 3 * plane + (size_t)py * W + x;
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[p * 3 + c] = (TO)quantise<BITS>(to_f32(s[c * plane]));
            }
        }
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_raw_format_size(void) { return sizeof(rc_raw_format); }

int rc_raw_ingest_fmt(const void* d_src, const rc_raw_format* fmt, void* d_packed, void* d_cond, int out_dtype, int batch, int h, int w,
                      int hp, int wp, int cond_h, int cond_w, void* stream) {
    RC_REQUIRE(d_src && fmt && d_packed && d_cond, "rc_raw_ingest_fmt: null pointer");
    RC_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && hp >= h && wp >= w && cond_h >= 1 && cond_w >= 1, "rc_raw_ingest_fmt: bad shape");
    RC_REQUIRE(out_dtype == RC_F32 || out_dtype == RC_BF16 || out_dtype == RC_F16, "rc_raw_ingest_fmt: bad dtype");
    RawSource rs;
    if (const int e = raw_source("rc_raw_ingest_fmt", d_src, fmt, w, &rs)) return e;
    for (int k = 0; k < 4; ++k) RC_REQUIRE(fmt->white > fmt->black[k], "rc_raw_ingest_fmt: white must exceed every black level");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_packed) % 16 == 0, "rc_raw_ingest_fmt: packed must be 16-byte aligned");

    // packed slot k (0 R, 1 G of the R row, 2 G of the B row, 3 B) <- cell position of that colour in the 2x2 cell
    static const int kSlotPos[4][4] = {{0, 1, 2, 3} /* RGGB */, {3, 2, 1, 0} /* BGGR */, {1, 0, 3, 2} /* GRBG */, {2, 3, 0, 1} /* GBRG */};
    IngestArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.batch = batch; a.h = h; a.w = w; a.hp = hp; a.wp = wp; a.ch = cond_h; a.cw = cond_w;
    a.line_bytes = (int)rs.line_bytes;
    a.pos = 0;
    for (int k = 0; k < 4; ++k) {
        const int pos = kSlotPos[fmt->cfa][k];
        a.pos |= pos << (2 * k);
        a.black[k] = fmt->black[pos];
        a.inv[k] = 1.f / (fmt->white - fmt->black[pos]);        // rc_raw_ingest's order: (v - black) * (1 / (white - black))
    }
    a.scale_y = (float)h / (float)cond_h; a.scale_x = (float)w / (float)cond_w;
    const size_t total = (size_t)batch * hp * ((wp + 1) / 2) + (size_t)batch * cond_h * cond_w;
    by_storage(fmt->storage, [&](auto sg) {
        by_dtype(out_dtype, [&](auto to) {
            typedef typename decltype(to)::type TO;
            hipLaunchKernelGGL((raw_ingest_fmt_kernel<decltype(sg)::ST, typename decltype(sg)::type, TO>), dim3(rf_grid(total)), dim3(kRfThreads), 0,
                               as_stream(stream), a, static_cast<TO*>(d_packed), static_cast<TO*>(d_cond));
        });
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_rgb_encode(const void* d_src, int src_dtype, void* d_dst, int out_bits, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && d_dst, "rc_rgb_encode: null pointer");
    RC_REQUIRE(src_dtype == RC_F32 || src_dtype == RC_BF16 || src_dtype == RC_F16, "rc_rgb_encode: bad dtype");
    RC_REQUIRE(out_bits == 8 || out_bits == 16, "rc_rgb_encode: out_bits must be 8 or 16");
    RC_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && h <= H && w <= W, "rc_rgb_encode: bad shape");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_dst) % 16 == 0, "rc_rgb_encode: dst must be 16-byte aligned");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % dtype_size(src_dtype) == 0, "rc_rgb_encode: src misaligned");
    const size_t total = (size_t)batch * h * w;
    by_dtype(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        const TI* src = static_cast<const TI*>(d_src);
        const dim3 block(kRfThreads);
        const hipStream_t s = as_stream(stream);
        if (out_bits == 8)
            hipLaunchKernelGGL((rgb_encode_kernel<TI, 8>), dim3(rf_grid((total + RgbOut<8>::P - 1) / RgbOut<8>::P)), block, 0, s, src, static_cast<uint8_t*>(d_dst), batch, H, W, h, w);
        else
            hipLaunchKernelGGL((rgb_encode_kernel<TI, 16>), dim3(rf_grid((total + RgbOut<16>::P - 1) / RgbOut<16>::P)), block, 0, s, src, static_cast<uint16_t*>(d_dst), batch, H, W, h, w);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
