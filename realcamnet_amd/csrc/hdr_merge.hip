// Multi-exposure HDR merge on the mosaic (include/realcam_hip.h, rc_raw_hdr_merge): E = 2 .. 4 exposures of one scene as the sensor delivers
// them (any storage, padded lines, whole frames or line-interleaved) -> one linear fp32 mosaic (B, 2h, 2w) in the shortest exposure's code
// units.  Pointwise across the exposures: no halo, no LDS, no atomics.
//
// raw_hdr_merge_kernel: grid (pairs of strips, bands of 16 rows, frames), four waves per block -- calibrate.hip's map.
//   lane map   a STRIP is 256 columns.  Lane l of a wave holds the 4 consecutive samples 256 s + 4 l .. + 3 of a row, of each of the E
//              exposures: E loads of 4 / 8 / 16 bytes per lane and row for u8 / 16-bit / fp32 samples, 5 bytes of a RAW10 line, 6 of a RAW12
//              line, one 16-byte store; ragged frames (a base, pitch or stride that is no multiple of 4 samples, the last two columns of a
//              width that is 2 mod 4) go sample by sample.
//   rows       waves 0, 2 of a block walk the even rows of the band downwards, waves 1, 3 the odd rows (waves 0, 1: the block's first
//              strip; 2, 3: its second), so a wave sees two CFA positions only: its blacks are two values read once.  The raw bytes of the
//              wave's next row, of all E exposures, are in flight while it works on this one.
//   times      host times ride in the argument block with their quotients q_e = t_0 / t_e; device times are read per frame (wave-uniform)
//              and the kernel forms the same quotients with the same correctly rounded division.
//   E          a template parameter: the E rows in flight and the E rows at work are registers, and the exposure loop unrolls.
// One correctly rounded division per sample (num / den: v_div_scale / v_rcp / v_div_fmas / v_div_fixup, denormals on), no 64-bit address
// arithmetic per sample (a frame's offsets over all its exposures fit 32 bits: the entry point checks), no scratch.  The arithmetic is step
// for step the header's: every product, sum and quotient rounded on its own.
#include "raw_row.hpp"

#include <cmath>

namespace rc {

constexpr int kHdrPx = 4, kHdrWaves = 4, kHdrThreads = 64 * kHdrWaves;
constexpr int kHdrSpan = 64 * kHdrPx;             // columns of a strip
constexpr int kHdrStrips = kHdrWaves / 2;         // strips per block
constexpr int kHdrRows = 16;                      // rows per block
constexpr int kHdrMaxE = 4;
static_assert(kHdrPx == kRowPx, "a lane holds the row reader's 4 samples");

struct HdrArgs {
    const uint8_t* src;        // row r of exposure e of frame b starts at src + b * frame_stride + e * exp_stride + r * line_bytes
    const float* times;        // (1 or B, E) on the device, or null: t[] / q[] below
    uint8_t* dst;
    long long frame_stride;
    int H, W;                  // one exposure's rows and columns (2h, 2w)
    int line_bytes, exp_stride, dst_pitch;
    int vec_in, vec_out;       // every lane's 4 samples start on a 4-sample boundary of the source / the destination
    int times_stride;          // 0 (one row for every frame) or E
    int motion;
    float black[4];            // CFA-position order
    float t[kHdrMaxE], q[kHdrMaxE];    // host times and t[0] / t[e]
    float lo, hi, ik;          // the knee and 1 / (hi - lo)
    float m_abs, m_rel;
};

template <int ST, typename TI, int E>
__global__ void __launch_bounds__(kHdrThreads) raw_hdr_merge_kernel(HdrArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int par = wv & 1, strip = blockIdx.x * kHdrStrips + (wv >> 1), frame = blockIdx.z;
    const int x0 = strip * kHdrSpan + lane * kHdrPx;
    if (x0 >= a.W) return;                                                         // no barrier and no lane exchange below
    const int n = min(a.W - x0, kHdrPx);                                           // W is even and x0 a multiple of 4: 2 or 4
    const bool full_in = n == kHdrPx && a.vec_in, full_out = n == kHdrPx && a.vec_out;
    const int r0 = blockIdx.y * kHdrRows, r1 = min(r0 + kHdrRows, a.H);
    const uint8_t* src = a.src + (size_t)frame * (size_t)a.frame_stride;
    uint8_t* dst = a.dst + (size_t)frame * (size_t)a.H * (size_t)a.dst_pitch;
    // r0 is even: y & 1 = par; x0 % 4 = 0: x & 1 = k & 1.  The wave's two positions are 2 par and 2 par + 1
    const float black[2] = {a.black[2 * par], a.black[2 * par + 1]};
    float t[E], q[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { t[e] = a.t[e]; q[e] = a.q[e]; }
    if (a.times) {                                                                 // wave-uniform
        const float* row = a.times + frame * a.times_stride;
#pragma unroll
        for (int e = 0; e < E; ++e) t[e] = row[e];
#pragma unroll
        for (int e = 0; e < E; ++e) q[e] = __fdiv_rn(t[0], t[e]);
    }

    int y = r0 + par;
    if (y >= r1) return;
    const uint32_t line_bytes = (uint32_t)a.line_bytes, exp_stride = (uint32_t)a.exp_stride;
    RowRaw ahead[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ahead[e] = row_load<ST, TI>(src + ((uint32_t)e * exp_stride + (uint32_t)y * line_bytes), x0, n, full_in);
    for (; y < r1; y += 2) {
        float v[E][kHdrPx];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const RowRaw raw = ahead[e];
            if (y + 2 < r1) ahead[e] = row_load<ST, TI>(src + ((uint32_t)e * exp_stride + (uint32_t)(y + 2) * line_bytes), x0, n, full_in);     // in flight while this row is worked on
            row_decode<ST, TI>(raw, n, full_in, v[e]);
        }
        float o[kHdrPx];
#pragma unroll
        for (int s = 0; s < kHdrPx; ++s) {
            const float b = black[s & 1];
            const float l0 = __fmul_rn(__fsub_rn(v[0][s], b), q[0]);
            float den = t[0];                                                      // w_0 = u_0 t_0, u_0 = 1
            float num = __fmul_rn(den, l0);
            const float tol = __fadd_rn(a.m_abs, __fmul_rn(a.m_rel, fabsf(l0)));
#pragma unroll
            for (int e = 1; e < E; ++e) {
                const float c = v[e][s];
                const float l = __fmul_rn(__fsub_rn(c, b), q[e]);
                float u = c <= a.lo ? 1.f : c >= a.hi ? 0.f : __fmul_rn(__fsub_rn(a.hi, c), a.ik);
                if (a.motion) u = fabsf(__fsub_rn(l, l0)) > tol ? 0.f : u;         // wave-uniform
                const float w = __fmul_rn(u, t[e]);
                num = __fadd_rn(num, __fmul_rn(w, l));
                den = __fadd_rn(den, w);
            }
            o[s] = __fadd_rn(b, __fdiv_rn(num, den));
        }
        row_store<float>(reinterpret_cast<float*>(dst + (uint32_t)y * (uint32_t)a.dst_pitch) + x0, o, n, full_out);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_hdr_desc_size(void) { return sizeof(rc_hdr_desc); }

int rc_raw_hdr_merge(const void* d_src, const rc_raw_format* fmt, const rc_hdr_desc* desc, const float* d_times, int times_batch, void* d_dst,
                     int dst_pitch_bytes, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_dst, "rc_raw_hdr_merge: null pointer");
    if (const int e = raw_frames("rc_raw_hdr_merge", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_hdr_merge", d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    if (const int e = raw_blacks_finite("rc_raw_hdr_merge", fmt)) return e;
    const int E = desc->exposures;
    RC_REQUIRE(E >= 2 && E <= kHdrMaxE, "rc_raw_hdr_merge: 2 to 4 exposures");
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_hdr_merge: reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~RC_HDR_MOTION) == 0, "rc_raw_hdr_merge: unknown flags");
    // the times
    if (d_times) {
        RC_REQUIRE(times_batch == 1 || times_batch == batch, "rc_raw_hdr_merge: times_batch must be 1 or the batch");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(d_times) % 4 == 0, "rc_raw_hdr_merge: the times must be 4-byte aligned");
    } else {
        RC_REQUIRE(times_batch == 0, "rc_raw_hdr_merge: times_batch without d_times must be 0");
        for (int e = 0; e < E; ++e)
            RC_REQUIRE(std::isfinite(desc->times[e]) && desc->times[e] > 0.f && (e == 0 || desc->times[e] > desc->times[e - 1]),
                       "rc_raw_hdr_merge: times must be finite, positive and strictly increasing (the shortest exposure first)");
    }
    RC_REQUIRE(std::isfinite(desc->knee_lo) && std::isfinite(desc->knee_hi) && desc->knee_lo < desc->knee_hi, "rc_raw_hdr_merge: the knee needs finite lo < hi");
    const bool motion = (desc->flags & RC_HDR_MOTION) != 0;
    if (motion)
        RC_REQUIRE(std::isfinite(desc->motion_abs) && std::isfinite(desc->motion_rel) && desc->motion_abs >= 0.f && desc->motion_rel >= 0.f,
                   "rc_raw_hdr_merge: motion thresholds must be finite and >= 0");
    // the strides
    const long long es = desc->exposure_stride_bytes ? desc->exposure_stride_bytes : 2LL * h * lb;
    const long long fs = desc->frame_stride_bytes ? desc->frame_stride_bytes : (long long)E * 2LL * h * lb;
    const int unit = rs.packed ? 4 : rs.esize;
    RC_REQUIRE(es > 0 && fs > 0, "rc_raw_hdr_merge: strides must be positive (0: whole frames, dense)");
    RC_REQUIRE(es % unit == 0 && fs % unit == 0, "rc_raw_hdr_merge: strides misaligned (MIPI: 4 bytes, else one sample)");
    // the destination
    long long dp;
    if (const int e = raw_pitch("rc_raw_hdr_merge", "dst", d_dst, dst_pitch_bytes, 2LL * w * 4, 4, &dp)) return e;
    // a frame's byte offsets, over all its exposures, are formed in 32 bits
    RC_REQUIRE(es <= 0x7fffffffLL && (E - 1) * es + 2LL * h * lb <= 0x7fffffffLL && 2LL * h * dp <= 0x7fffffffLL,
               "rc_raw_hdr_merge: a frame (all its exposures: strides, rows x pitch) must stay below 2 GiB");

    HdrArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.times = d_times;
    a.dst = static_cast<uint8_t*>(d_dst);
    a.frame_stride = fs;
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.exp_stride = (int)es; a.dst_pitch = (int)dp;
    const long long quad = (long long)kHdrPx * rs.esize;
    a.vec_in = rs.vec && es % quad == 0 && fs % quad == 0;
    a.vec_out = raw_vec(d_dst, dp, 4);
    a.times_stride = d_times && times_batch > 1 ? E : 0;
    a.motion = motion;
    for (int p = 0; p < 4; ++p) a.black[p] = fmt->black[p];
    for (int e = 0; e < kHdrMaxE; ++e) {
        const bool live = e < E && !d_times;
        a.t[e] = live ? desc->times[e] : 1.f;
        a.q[e] = live ? desc->times[0] / desc->times[e] : 1.f;                     // one fp32 division: the kernel's own for device times
    }
    a.lo = desc->knee_lo; a.hi = desc->knee_hi;
    a.ik = (float)(1.0 / ((double)desc->knee_hi - (double)desc->knee_lo));
    a.m_abs = motion ? desc->motion_abs : 0.f; a.m_rel = motion ? desc->motion_rel : 0.f;
    const hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)ceil_div(ceil_div(a.W, kHdrSpan), kHdrStrips), (unsigned)ceil_div(a.H, kHdrRows), (unsigned)batch), block(kHdrThreads);
    by_storage(fmt->storage, [&](auto sg) {
        constexpr int ST = decltype(sg)::ST;
        typedef typename decltype(sg)::type TI;
        if (E == 2) hipLaunchKernelGGL((raw_hdr_merge_kernel<ST, TI, 2>), grid, block, 0, s, a);
        else if (E == 3) hipLaunchKernelGGL((raw_hdr_merge_kernel<ST, TI, 3>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((raw_hdr_merge_kernel<ST, TI, 4>), grid, block, 0, s, a);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
