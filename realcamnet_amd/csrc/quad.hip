// Quad-Bayer sensors on the mosaic (include/realcam_hip.h, rc_raw_quad): the frame as delivered (any storage, padded lines), whose colours
// come in 2x2 blocks, -> an ordinary Bayer mosaic: REMOSAIC (B, H, W) in the unpacked storage rc_raw_defects writes, or BIN (B, H/2, W/2)
// fp32.  The first box of the input side.  No LDS, no atomics, no scratch.
//
// raw_quad_remosaic_kernel: grid (pairs of strips, bands of 32 rows, frames), four waves per block.
//   lane map   defects.hip's: a STRIP is 248 columns, lane l of a wave holds the 4 consecutive samples 248 s - 4 + 4 l .. + 3 of a row -- one
//              quad period, so x & 3 is the lane element and every site's recipe is chosen at compile time.  Lanes 1 .. 62 produce and store,
//              lanes 0 and 63 only load (the halo: 8 of 256 columns are read twice, out of L2).  W is a multiple of 4: a lane holds 4
//              samples of the frame or none.
//   columns    the stencil reaches x - 2 .. x + 2, but from a lane's 4 samples only x0 - 1 and x0 + 4 lie outside it (near is at x + sx,
//              far at x - 2 sx): two lane shifts per row.  At the frame's edges they are the lane's own samples 2 and 1 (the reflection).
//   rows       waves 0, 1 of a block take its first strip, 2, 3 its second; waves 0, 2 the upper 16 rows of the band, 1, 3 the lower.  A
//              wave walks DOWNWARDS four rows at a time (y0 a multiple of 4: y & 3 is compile-time too).  Rows y0 .. y0 + 3 read the rows
//              y0 - 1 .. y0 + 4 and no others (near is row y + sy, far y - 2 sy), so a wave keeps that six-row window, decoded, in
//              registers (6 x 6 floats), carries its last two rows into the next step and loads four: 18 rows read for 16 produced (the
//              height was chosen by timing: 32 and 64 rows re-read less and are slower, 8 rows gains on bf16 what it loses on RAW10).  The
//              bytes of the next four rows are in flight while these are worked on.  A row outside the frame is fetched as the row it
//              reflects to: no tap tests its bounds.
// raw_quad_bin_kernel: a lane reads 4 samples of rows 2y and 2y + 1 and stores 2 results; four output rows per block row.
// The arithmetic is step for step the header's; the two G positions decide everything (R and B swap roles, not recipes), so the kernel is
// built for "G on the anti-diagonal" (RGGB, BGGR) and "G on the diagonal" (GRBG, GBRG).
#include "raw_row.hpp"

namespace rc {

constexpr int kQdPx = 4, kQdWaves = 4, kQdThreads = 64 * kQdWaves;
constexpr int kQdSpan = 62 * kQdPx;             // columns a wave produces
constexpr int kQdStrips = 2;                    // strips per block
constexpr int kQdWaveRows = 16;                 // rows a wave walks
constexpr int kQdRows = 2 * kQdWaveRows;        // rows per block
constexpr int kQbRows = 4;                      // bin: output rows per block row
static_assert(kQdPx == kRowPx, "a lane holds the row reader's 4 samples");
static_assert(kQdWaveRows % 4 == 0, "a wave starts on a multiple of 4: y & 3 is the row of its step");

struct QuadArgs {
    const uint8_t* src;        // row r of frame b starts at src + (b * H + r) * line_bytes
    uint8_t* dst;
    int H, W;
    int line_bytes, dst_pitch;
    int vec_in, vec_out;       // every lane's samples start on a vector boundary of the source / the destination
};

struct QdRow { float v[6]; };                    // columns x0 - 1 .. x0 + 4

__device__ __forceinline__ int qd_reflect(int y, int H) { return y < 0 ? 1 - y : y >= H ? 2 * H - 3 - y : y; }

__device__ __forceinline__ float qd_axis(float near, float far, float* d) {
    const float diff = __fsub_rn(far, near);
    if (d) *d = fabsf(diff);
    return __fadd_rn(near, __fdiv_rn(diff, 3.f));
}

// Site (y & 3, x & 3) = (J, K) of a tile; R[i] is row y0 - 1 + i.  GA: G sits on the cell's anti-diagonal (positions 1, 2).
template <bool GA, int J, int K>
__device__ __forceinline__ float qd_site(const QdRow (&R)[6]) {
    constexpr int by = J >> 1, bx = K >> 1, ty = J & 1, tx = K & 1;               // the sensor's block, the wanted cell position
    constexpr int sy = ty ? 1 : -1, sx = tx ? 1 : -1;
    constexpr bool s_g = ((by ^ bx) == 1) == GA, t_g = ((ty ^ tx) == 1) == GA;
    constexpr int c = K + 1;
    const QdRow& cu = R[J + 1];
    if constexpr ((by == ty && bx == tx) || (s_g && t_g)) {                        // 1. S = T
        return cu.v[c];
    } else {
        const QdRow& rn = R[J + 1 + sy];
        const QdRow& rf = R[J + 1 - 2 * sy];
        if constexpr (!s_g && t_g) {                                               // 3. G at an R or B site
            float dh, dv;
            const float eh = qd_axis(cu.v[c + sx], cu.v[c - 2 * sx], &dh);
            const float ev = qd_axis(rn.v[c], rf.v[c], &dv);
            return dh < dv ? eh : dv < dh ? ev : __fmul_rn(__fadd_rn(eh, ev), 0.5f);
        } else if constexpr (!s_g) {                                               // 5. R at a B site, B at an R site
            const float r_near = qd_axis(rn.v[c + sx], rn.v[c - 2 * sx], nullptr);
            const float r_far = qd_axis(rf.v[c + sx], rf.v[c - 2 * sx], nullptr);
            return qd_axis(r_near, r_far, nullptr);
        } else if constexpr (by == ty) {                                           // 4. the row's other block is T
            return qd_axis(cu.v[c + sx], cu.v[c - 2 * sx], nullptr);
        } else {                                                                   // 4. the column's
            return qd_axis(rn.v[c], rf.v[c], nullptr);
        }
    }
}

template <bool GA, int J>
__device__ __forceinline__ void qd_out_row(const QdRow (&R)[6], float* o) {
    o[0] = qd_site<GA, J, 0>(R); o[1] = qd_site<GA, J, 1>(R); o[2] = qd_site<GA, J, 2>(R); o[3] = qd_site<GA, J, 3>(R);
}

template <int ST, typename TI, typename TO, bool GA>
__global__ void __launch_bounds__(kQdThreads) raw_quad_remosaic_kernel(QuadArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int strip = blockIdx.x * kQdStrips + (wv >> 1), frame = blockIdx.z;
    const int r0 = blockIdx.y * kQdRows + (wv & 1) * kQdWaveRows, r1 = min(r0 + kQdWaveRows, a.H);
    if (strip * kQdSpan >= a.W || r0 >= a.H) return;                               // wave-uniform
    const int x0 = strip * kQdSpan + (lane - 1) * kQdPx;
    const bool act = x0 >= 0 && x0 < a.W;                                          // W % 4 == 0: all 4 samples inside, or none
    const bool writer = act && lane >= 1 && lane <= 62;
    const bool first = x0 == 0, last = x0 + kQdPx == a.W;
    const bool full_in = a.vec_in, full_out = a.vec_out;
    const size_t frame_row = (size_t)frame * (size_t)a.H;
    auto load = [&](int y) {                                                       // row y, reflected into the frame
        RowRaw r = {{0u, 0u, 0u, 0u}};
        if (act) r = row_load<ST, TI>(a.src, (frame_row + (size_t)qd_reflect(y, a.H)) * (size_t)a.line_bytes, x0, kQdPx, full_in);
        return r;
    };
    auto decode = [&](const RowRaw& raw, QdRow& o) {                               // every lane of the wave runs this: the shifts need them all
        float v[kQdPx];
        row_decode<ST, TI>(raw, kQdPx, full_in, v);
        const float l = __shfl_up(v[3], 1), r = __shfl_down(v[0], 1);
        o.v[0] = first ? v[2] : l;                                                 // column -1 reflects to 2, column W to W - 3
        o.v[5] = last ? v[1] : r;
#pragma unroll
        for (int k = 0; k < kQdPx; ++k) o.v[1 + k] = v[k];
    };

    QdRow R[6];
    {
        const RowRaw ra = load(r0 - 1), rb = load(r0);
        decode(ra, R[4]);
        decode(rb, R[5]);
    }
    RowRaw ahead[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ahead[i] = load(r0 + 1 + i);
    for (int y0 = r0; y0 < r1; y0 += 4) {                                          // H % 4 == 0: whole steps
        R[0] = R[4];
        R[1] = R[5];
        RowRaw raw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) raw[i] = ahead[i];
        if (y0 + 4 < r1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ahead[i] = load(y0 + 5 + i);               // in flight while these rows are worked on
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) decode(raw[i], R[2 + i]);
        float o[4][kQdPx];
        qd_out_row<GA, 0>(R, o[0]);
        qd_out_row<GA, 1>(R, o[1]);
        qd_out_row<GA, 2>(R, o[2]);
        qd_out_row<GA, 3>(R, o[3]);
        if (writer) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                TO* dst = reinterpret_cast<TO*>(a.dst + (frame_row + (size_t)(y0 + j)) * (size_t)a.dst_pitch) + x0;
                row_store<TO>(dst, o[j], kQdPx, full_out);
            }
        }
    }
}

// H here is the SOURCE's; the result has H / 2 rows of W / 2 floats.
template <int ST, typename TI>
__global__ void __launch_bounds__(kQdThreads) raw_quad_bin_kernel(QuadArgs a) {
    const int x0 = (blockIdx.x * kQdThreads + threadIdx.x) * kQdPx, frame = blockIdx.z;
    if (x0 >= a.W) return;
    const int oh = a.H >> 1, y0 = blockIdx.y * kQbRows;
    const bool full_in = a.vec_in;
    const size_t frame_row = (size_t)frame * (size_t)a.H;
    RowRaw raw[kQbRows][2] = {};
#pragma unroll
    for (int j = 0; j < kQbRows; ++j) {
        if (y0 + j < oh) {                                                         // block-uniform
            raw[j][0] = row_load<ST, TI>(a.src, (frame_row + (size_t)(2 * (y0 + j))) * (size_t)a.line_bytes, x0, kQdPx, full_in);
            raw[j][1] = row_load<ST, TI>(a.src, (frame_row + (size_t)(2 * (y0 + j) + 1)) * (size_t)a.line_bytes, x0, kQdPx, full_in);
        }
    }
#pragma unroll
    for (int j = 0; j < kQbRows; ++j) {
        if (y0 + j < oh) {
            float t[kQdPx], b[kQdPx];
            row_decode<ST, TI>(raw[j][0], kQdPx, full_in, t);
            row_decode<ST, TI>(raw[j][1], kQdPx, full_in, b);
            const float o0 = __fmul_rn(__fadd_rn(__fadd_rn(t[0], t[1]), __fadd_rn(b[0], b[1])), 0.25f);
            const float o1 = __fmul_rn(__fadd_rn(__fadd_rn(t[2], t[3]), __fadd_rn(b[2], b[3])), 0.25f);
            float* dst = reinterpret_cast<float*>(a.dst + ((size_t)frame * (size_t)oh + (size_t)(y0 + j)) * (size_t)a.dst_pitch) + (x0 >> 1);
            if (a.vec_out) {
                *reinterpret_cast<float2*>(dst) = make_float2(o0, o1);
            } else {
                dst[0] = o0;
                dst[1] = o1;
            }
        }
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_quad_desc_size(void) { return sizeof(rc_quad_desc); }

int rc_raw_quad(const void* d_src, const rc_raw_format* fmt, const rc_quad_desc* desc, void* d_dst, int dst_pitch_bytes,
                int batch, int H, int W, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_dst, "rc_raw_quad: null pointer");
    RC_REQUIRE(batch >= 1 && batch <= 65535 && H >= 4 && W >= 4 && H <= (1 << 21) && W <= (1 << 25), "rc_raw_quad: bad shape (below 4, more than 65535 frames, or too large)");
    RC_REQUIRE(H % 4 == 0 && W % 4 == 0, "rc_raw_quad: H and W must be multiples of 4 (the quad tile)");
    RawSource rs;
    if (const int e = raw_source("rc_raw_quad", d_src, fmt, W / 2, &rs)) return e;
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_quad: reserved fields must be zero");
    RC_REQUIRE(desc->mode == RC_QUAD_REMOSAIC || desc->mode == RC_QUAD_BIN, "rc_raw_quad: unknown mode");
    const bool bin = desc->mode == RC_QUAD_BIN;
    const int osize = bin ? 4 : rs.usize;
    long long dp;
    if (const int e = raw_pitch("rc_raw_quad", "dst", d_dst, dst_pitch_bytes, (bin ? W / 2 : W) * (long long)osize, osize, &dp)) return e;

    QuadArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.dst = static_cast<uint8_t*>(d_dst);
    a.H = H; a.W = W;
    a.line_bytes = (int)rs.line_bytes; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec;
    a.vec_out = raw_vec(d_dst, dp, bin ? osize / 2 : osize);                       // bin: a lane stores two floats, half a vector of four
    const bool ga = fmt->cfa == RC_CFA_RGGB || fmt->cfa == RC_CFA_BGGR;            // G on the cell's anti-diagonal
    const hipStream_t s = as_stream(stream);
    const dim3 block(kQdThreads);
    const dim3 grid = bin ? dim3((unsigned)ceil_div(W / kQdPx, kQdThreads), (unsigned)ceil_div(H / 2, kQbRows), (unsigned)batch)
                          : dim3((unsigned)ceil_div(ceil_div(W, kQdSpan), kQdStrips), (unsigned)ceil_div(H, kQdRows), (unsigned)batch);
    by_storage(fmt->storage, [&](auto sg) {
        constexpr int ST = decltype(sg)::ST;
        typedef typename decltype(sg)::type TI;
        if (bin) hipLaunchKernelGGL((raw_quad_bin_kernel<ST, TI>), grid, block, 0, s, a);
        else if (ga) hipLaunchKernelGGL((raw_quad_remosaic_kernel<ST, TI, unpacked_t<TI>, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((raw_quad_remosaic_kernel<ST, TI, unpacked_t<TI>, false>), grid, block, 0, s, a);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
