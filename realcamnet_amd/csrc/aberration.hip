// Lateral chromatic aberration correction on the mosaic (include/realcam_hip.h, rc_raw_aberration): the sensor frame as rc_raw_calibrate
// reads it (any storage, padded lines, any cfa) -> a dense fp32 mosaic (B, 2h, 2w) whose G samples are the decoded input and whose R and B
// samples are resampled inside their own colour's h x w plane through a coarse mesh of shifts.  One launch, no atomics, no device state.
//
// aberration_kernel: grid (tiles of 64 mosaic columns, tiles of 64 mosaic rows, frames), four waves per block.
//   tile       32 x 32 Bayer cells.  The block stages the R plane and the B plane of its tile plus a halo of reach + 2 (bicubic) or
//              reach + 1 (bilinear) plane samples in LDS as fp32; the halo comes from the descriptor, so a lens with a reach of 1 or 2
//              stages little more than its tile.  Plane rows and columns outside the frame are staged as the clamped ones: the gather has
//              no bounds test, and the guard of step 2 keeps every tap inside what was staged whatever the mesh holds.
//   stage      a task is 4 samples of a mosaic row that start on a multiple of 4 (row_load / row_decode of raw_row.hpp): two samples of
//              the row's colour, written to that colour's plane.  The staged columns start on an even plane column (the halo is rounded
//              up to an even number there), so a task is one group of 4.  A clamped column lies in another group, which is loaded instead.
//   barrier    one.
//   gather     a lane owns 4 output samples of a row: 16 lanes cover the tile's 64 columns, lanes 16 .. 31 the next row of the SAME colour
//              (two mosaic rows down), lanes 32 .. 63 the two after.  ds_read_b32 banks are (a / 4) % 32 per 32-lane half: the 16 lanes
//              of a row read every second float (their plane columns 2 l + c, displaced by a nearly common shift) and so touch 16 banks of
//              one parity; the plane's row stride is odd (kCaStride), which puts the other 16 lanes on the other parity.  The lane's own
//              row was loaded before the barrier; its two G samples stay in registers.  One 16-byte store.
// Row offsets are formed in 64 bits once per row.  The arithmetic is step for step the header's: every product, sum and difference
// rounded on its own.
#include "raw_row.hpp"

#include <cmath>

namespace rc {

constexpr int kCaThreads = 256;
constexpr int kCaCells = 32;                      // Bayer cells per tile side: 64 mosaic rows and columns
constexpr int kCaLanesX = kCaCells / 2;           // lanes across a tile row (4 samples = 2 cells each)
constexpr int kCaMaxReach = 8;
constexpr int kCaMaxHalo = kCaMaxReach + 2;
constexpr int kCaMaxSide = kCaCells + 2 * kCaMaxHalo;      // 52 staged plane rows / columns at the most
constexpr int kCaStride = kCaMaxSide + 1;         // odd: see the bank rule above
constexpr int kCaRowsPerThread = 2 * kCaCells * kCaLanesX / kCaThreads;    // 4 gather tasks per thread
static_assert(kCaStride % 2 == 1 && kCaMaxHalo % 2 == 0, "odd row stride; the largest halo is even");
static_assert(2 * kCaMaxSide * kCaStride * 4 <= 65536, "static LDS");

struct CaArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    const float2* mesh;        // (2, Gh, Gw) nodes of (dx, dy): plane 0 R, plane 1 B
    uint8_t* dst;
    int H, W;                  // the mosaic's rows and columns (2h, 2w)
    int line_bytes, dst_pitch;
    int vec_in, vec_out;
    int cell_log2, Gw, plane;  // log2(cell), nodes per mesh row, nodes per colour
    int halo;                  // plane samples staged around the tile: reach + 2 or reach + 1
    int rpos;                  // CFA position 2 (y & 1) + (x & 1) of R; B is at 3 - rpos
    float reach;
};

__device__ __forceinline__ float ca_c1(float x) { return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, x), 2.25f), x), x), 1.f); }
__device__ __forceinline__ float ca_c2(float x) {
    return __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(-0.75f, x), 3.75f), x), 6.f), x), 3.f);
}

// Steps 3 and 4 of one axis: the first tap's index and the NT weights.
template <int NT>
__device__ __forceinline__ int ca_axis(float s, float* wt) {
    const float fl = floorf(s);
    const float t = __fsub_rn(s, fl);
    if constexpr (NT == 2) {
        wt[0] = __fsub_rn(1.f, t);
        wt[1] = t;
        return (int)fl;
    } else {
        wt[0] = ca_c2(__fadd_rn(t, 1.f));
        wt[1] = ca_c1(t);
        wt[2] = ca_c1(__fsub_rn(1.f, t));
        wt[3] = ca_c2(__fsub_rn(2.f, t));
        return (int)fl - 1;
    }
}

// Sample i of a lane's 4, without an indexed read of registers.
__device__ __forceinline__ float ca_pick(const float* v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// Step 2: NaN -> 0, then into [-reach, reach].
__device__ __forceinline__ float ca_guard(float d, float reach) {
    d = d == d ? d : 0.f;
    return fminf(fmaxf(d, -reach), reach);
}

template <int ST, typename TI, int INTERP>
__global__ void __launch_bounds__(kCaThreads) aberration_kernel(CaArgs a) {
    constexpr int NT = INTERP == RC_WARP_BICUBIC ? 4 : 2;
    __shared__ float tile[2][kCaMaxSide * kCaStride];                              // [colour: 0 R, 1 B][staged row * kCaStride + staged column]
    const int tid = threadIdx.x, frame = blockIdx.z;
    const int h = a.H >> 1, w = a.W >> 1;
    const int X0 = blockIdx.x * kCaCells, Y0 = blockIdx.y * kCaCells;              // the tile's first plane column and row
    const int halo = a.halo, halo_x = (halo + 1) & ~1;                             // block-uniform; the staged columns start on an even plane column
    const int sw = kCaCells + 2 * halo_x, sh = kCaCells + 2 * halo;                // staged plane columns and rows: <= kCaMaxSide
    const int px0 = X0 - halo_x, py0 = Y0 - halo;                                  // plane coordinates of staged (0, 0)
    const size_t frame_off = (size_t)frame * (size_t)a.H * (size_t)a.line_bytes;
    const int rrow = a.rpos >> 1;                                                  // the row parity that holds R

    // ---- the lane's own rows: in flight across the staging ----
    const int lane = tid & 63, wv = tid >> 6, lx = lane & (kCaLanesX - 1), q = lane >> 4;
    const int par = wv & 1;                                                        // wave-uniform: the wave's rows hold one colour
    const int x0 = 2 * X0 + lx * kRowPx;
    const int n = min(a.W - x0, kRowPx);
    const bool full_in = n == kRowPx && a.vec_in, full_out = n == kRowPx && a.vec_out;
    RowRaw own[kCaRowsPerThread];
#pragma unroll
    for (int it = 0; it < kCaRowsPerThread; ++it) {
        const int y = 2 * (Y0 + it * 8 + (wv >> 1) * 4 + q) + par;
        own[it] = RowRaw{{0u, 0u, 0u, 0u}};
        if (x0 < a.W && y < a.H) own[it] = row_load<ST, TI>(a.src, frame_off + (size_t)y * (size_t)a.line_bytes, x0, n, full_in);
    }

    // ---- stage ----
    const int per_row = sw >> 1;                                                   // tasks of a staged mosaic row
    for (int t = tid; t < 2 * sh * per_row; t += kCaThreads) {
        const int sr = t / per_row, sc = 2 * (t - sr * per_row);                   // staged mosaic row (2 per plane row), staged plane column (even)
        const int rp = sr & 1, sy = sr >> 1;                                       // the mosaic row's parity; the staged plane row
        const int colour = rp == rrow ? 0 : 1;
        const int cpar = (colour == 0 ? a.rpos : 3 - a.rpos) & 1;                  // the column parity of the row's colour
        const int Yc = min(max(py0 + sy, 0), h - 1);
        const size_t off = frame_off + (size_t)(2 * Yc + rp) * (size_t)a.line_bytes;
        const int Xa = min(max(px0 + sc, 0), w - 1), Xb = min(max(px0 + sc + 1, 0), w - 1);
        const int ma = 2 * Xa + cpar, mb = 2 * Xb + cpar;                          // the mosaic columns of the two samples
        const int ga = ma & ~3, gb = mb & ~3;
        float v[kRowPx];
        const int na = min(a.W - ga, kRowPx);
        const bool fa = na == kRowPx && a.vec_in;
        row_decode<ST, TI>(row_load<ST, TI>(a.src, off, ga, na, fa), na, fa, v);
        const float va = ca_pick(v, ma & 3);
        if (gb != ga) {                                                            // only where a column was clamped
            const int nb = min(a.W - gb, kRowPx);
            const bool fb = nb == kRowPx && a.vec_in;
            row_decode<ST, TI>(row_load<ST, TI>(a.src, off, gb, nb, fb), nb, fb, v);
        }
        const float vb = ca_pick(v, mb & 3);
        float* p = &tile[colour][sy * kCaStride + sc];
        p[0] = va;
        p[1] = vb;
    }
    __syncthreads();

    // ---- gather and store ----
    if (x0 >= a.W) return;
    const int colour = par == rrow ? 0 : 1;
    const int cpar = (colour == 0 ? a.rpos : 3 - a.rpos) & 1;
    const float* plane = tile[colour];
    const int k = a.cell_log2, cmask = (1 << k) - 1;
    const float step = __uint_as_float((uint32_t)(127 - k) << 23);                 // 2^-k
    const int X = x0 >> 1;                                                         // even: X and X + 1 lie in one mesh cell
    const float fx[2] = {__fmul_rn((float)(X & cmask), step), __fmul_rn((float)((X + 1) & cmask), step)};
    const float2* node = a.mesh + ((size_t)colour * (size_t)a.plane + (size_t)(X >> k));
    uint8_t* dst = a.dst + (size_t)frame * (size_t)a.H * (size_t)a.dst_pitch;
#pragma unroll
    for (int it = 0; it < kCaRowsPerThread; ++it) {
        const int Y = Y0 + it * 8 + (wv >> 1) * 4 + q, y = 2 * Y + par;
        if (y >= a.H) continue;
        float o[kRowPx];
        row_decode<ST, TI>(own[it], n, full_in, o);
        // step 1
        const float2* g = node + (size_t)(Y >> k) * (size_t)a.Gw;
        const float2 g00 = g[0], g01 = g[1], g10 = g[a.Gw], g11 = g[a.Gw + 1];
        const float fy = __fmul_rn((float)(Y & cmask), step);
        const float dtx = __fsub_rn(g01.x, g00.x), dbx = __fsub_rn(g11.x, g10.x), dty = __fsub_rn(g01.y, g00.y), dby = __fsub_rn(g11.y, g10.y);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (2 * c + cpar >= n) continue;                                       // the last two columns of a width that is 2 mod 4
            const float topx = __fadd_rn(g00.x, __fmul_rn(fx[c], dtx)), botx = __fadd_rn(g10.x, __fmul_rn(fx[c], dbx));
            const float topy = __fadd_rn(g00.y, __fmul_rn(fx[c], dty)), boty = __fadd_rn(g10.y, __fmul_rn(fx[c], dby));
            const float dx = ca_guard(__fadd_rn(topx, __fmul_rn(fy, __fsub_rn(botx, topx))), a.reach);
            const float dy = ca_guard(__fadd_rn(topy, __fmul_rn(fy, __fsub_rn(boty, topy))), a.reach);
            // steps 3 and 4
            float wx[NT], wy[NT];
            const int ix = ca_axis<NT>(__fadd_rn((float)(X + c), dx), wx) - px0;   // staged coordinates of the first tap: inside by the guard
            const int iy = ca_axis<NT>(__fadd_rn((float)Y, dy), wy) - py0;
            const float* s = plane + iy * kCaStride + ix;
            // step 5
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < NT; ++r) {
                float rr = 0.f;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const float p = __fmul_rn(wx[i], s[r * kCaStride + i]);
                    rr = i == 0 ? p : __fadd_rn(rr, p);
                }
                const float p = __fmul_rn(wy[r], rr);
                acc = r == 0 ? p : __fadd_rn(acc, p);
            }
            o[2 * c] = cpar ? o[2 * c] : acc;
            o[2 * c + 1] = cpar ? acc : o[2 * c + 1];
        }
        row_store<float>(reinterpret_cast<float*>(dst + (size_t)y * (size_t)a.dst_pitch) + x0, o, n, full_out);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_ca_desc_size(void) { return sizeof(rc_ca_desc); }

int rc_raw_aberration(const void* d_src, const rc_raw_format* fmt, const rc_ca_desc* desc, const float* d_shift, float* d_dst, int dst_pitch_bytes,
                      int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_shift && d_dst, "rc_raw_aberration: null pointer");
    if (const int e = raw_frames("rc_raw_aberration", batch, h, w)) return e;
    RC_REQUIRE(h <= RC_WARP_MAX_DIM && w <= RC_WARP_MAX_DIM, "rc_raw_aberration: h and w must not exceed 2^23 (plane coordinates are exact in fp32)");
    RawSource rs;
    if (const int e = raw_source("rc_raw_aberration", d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    RC_REQUIRE(desc->interp == RC_WARP_BILINEAR || desc->interp == RC_WARP_BICUBIC, "rc_raw_aberration: bad interp (RC_WARP_BILINEAR or RC_WARP_BICUBIC)");
    const int cell = desc->cell;
    RC_REQUIRE(cell == 8 || cell == 16 || cell == 32 || cell == 64 || cell == 128, "rc_raw_aberration: cell must be 8, 16, 32, 64 or 128");
    RC_REQUIRE(desc->reach >= 1 && desc->reach <= RC_CA_MAX_REACH, "rc_raw_aberration: reach must lie in 1 .. 8");
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_aberration: reserved fields must be zero");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_shift) % 8 == 0, "rc_raw_aberration: the shift mesh must be 8-byte aligned");
    long long dp;
    if (const int e = raw_pitch("rc_raw_aberration", "dst", d_dst, dst_pitch_bytes, 2LL * w * 4, 4, &dp)) return e;
    RC_REQUIRE(2LL * h * lb <= 0x7fffffffLL && 2LL * h * dp <= 0x7fffffffLL, "rc_raw_aberration: a frame (rows x pitch) must stay below 2 GiB");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + (uintptr_t)(2LL * h * lb * batch);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_dst), o1 = o0 + (uintptr_t)(2LL * h * dp * batch);
    RC_REQUIRE(s1 <= o0 || o1 <= s0, "rc_raw_aberration: dst overlaps src (a sample's neighbours are read after it is written)");

    CaArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.mesh = reinterpret_cast<const float2*>(d_shift);
    a.dst = reinterpret_cast<uint8_t*>(d_dst);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec; a.vec_out = raw_vec(d_dst, dp, 4);
    a.cell_log2 = 0;
    while ((1 << a.cell_log2) < cell) ++a.cell_log2;
    a.Gw = ceil_div(w, cell) + 1;
    a.plane = (ceil_div(h, cell) + 1) * a.Gw;
    a.halo = desc->reach + (desc->interp == RC_WARP_BICUBIC ? 2 : 1);
    a.rpos = fmt->cfa == RC_CFA_RGGB ? 0 : fmt->cfa == RC_CFA_BGGR ? 3 : fmt->cfa == RC_CFA_GRBG ? 1 : 2;
    a.reach = (float)desc->reach;
    const hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)ceil_div(w, kCaCells), (unsigned)ceil_div(h, kCaCells), (unsigned)batch), block(kCaThreads);
    RC_REQUIRE(grid.y <= 65535u, "rc_raw_aberration: too many rows");
    const bool cubic = desc->interp == RC_WARP_BICUBIC;
    by_storage(fmt->storage, [&](auto sg) {
        if (cubic) hipLaunchKernelGGL((aberration_kernel<decltype(sg)::ST, typename decltype(sg)::type, RC_WARP_BICUBIC>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((aberration_kernel<decltype(sg)::ST, typename decltype(sg)::type, RC_WARP_BILINEAR>), grid, block, 0, s, a);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
