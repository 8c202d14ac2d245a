// Raw stills (include/realcam_hip.h, rc_dng_*): the sensor mosaic (B, h2, w2) as rc_raw_format describes it (u16 / u8 / RAW10 / RAW12, padded
// lines) -> one DNG file per frame: the caller's TIFF header, then the image in tiles, each a lossless JPEG stream (ITU-T T.81 process 14,
// predictor 1, one fixed Huffman table).  Three launches and no host sync, the plan of jpeg.hip with the tile in the place of the restart
// interval; the bit buffer, the 0xFF stuffing and the flush are bitpack.hpp's, shared with it.
//
// dng_tile_kernel<ST, TI, VEC, WRITE>: one wave (a 64-thread block) per tile, walking its lines; nothing but the source samples and the
// stuffed bytes touches memory.
//   samples   a lane holds raw_row.hpp's 4 consecutive samples of a line, so a step of the wave is 256 samples; a tile wider than that takes
//             several steps per line.  Beyond the frame the last sample of the same colour repeats: the lane reads the frame's last group
//             and picks from it.  The load of the next step is issued before this one is coded; the last step is asked for twice, so the
//             loop body has no branch around a load.
//   predict   with components = 2 a lane's samples 2, 3 are predicted by its samples 0, 1, and those by samples 2, 3 of the lane to the
//             left (with components = 1: each by the sample in front of it), which come by a wave shift, not through LDS.  Lane 0 takes
//             them from lane 63 of the step before (a readlane, kept in a register), or, at a line's first step, from the line above: every
//             lane keeps its samples 0, 1 of the first step of the previous line.
//   code      d -> SSSS by a leading-zero count, the Huffman word from a 17-entry LDS table, the extra bits behind it: at most 27 bits per
//             sample, so a pair is one word of at most 54 bits; a wave prefix sum of the lanes' lengths; two ORs of pairs into the LDS bit
//             buffer (a step is at most 7 carried + 256 x 27 = 6919 bits).
//   stuff     after each step the buffer's complete bytes are taken 64 at a time (ballot of 0xFF, population count); the (up to 7) bits left
//             over start the next step's buffer; the tile's last byte is padded with 1-bits.
// WRITE = false stores only the tile's stuffed byte count (4 bytes of scratch per tile); dng_scan_kernel turns the counts of a frame into the
// tiles' even offsets in the file (in place), copies the header, fills TileOffsets / TileByteCounts in it and writes `lengths`; WRITE = true
// codes again and stores the tile's header, its bytes, EOI and the pad byte at the final offset.  Every store to the frame is clipped to
// `capacity`.  No workgroup waits on another.
#include <atomic>
#include <cstring>
#include <type_traits>

#include "bitpack.hpp"
#include "raw_row.hpp"

namespace rc {

// ---- the constants of the format -----------------------------------------------------------------------------------------------------------
constexpr uint8_t kDngBits[16] = {0, 0, 5, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0};            // codes per length 1 .. 16
constexpr uint8_t kDngVals[17] = {1, 2, 3, 4, 5, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};   // SSSS in code order
constexpr int kDngStepPx = 64 * kRowPx;                     // samples of a line per step of the wave
constexpr int kDngBitWords = 224;                           // 7 carried + 256 x 27 + 7 pad bits = 6926 bits < 217 words
constexpr int kDngTileHeaderMax = 68, kDngTileHeaderWords = kDngTileHeaderMax / 4;
static_assert(7 + kDngStepPx * 27 + 7 <= 32 * (kDngBitWords - 3), "a step's bits, and the three words an OR may touch, fit the buffer");

struct DngConst { uint32_t tab[17]; };                      // (length << 16) | code at [SSSS]
constexpr DngConst dng_const() {
    DngConst c{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < kDngBits[len - 1]; ++i) c.tab[kDngVals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
    return c;
}
__device__ const DngConst kDngDev = dng_const();

struct DngArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    int H, W;                  // the mosaic's rows and columns (h2, w2)
    int line_bytes;
    int tw, th, nc, half;      // the tile, the components, 2^(P-1)
    int tiles_x, ntiles;
    int thb;                   // the tile header's bytes
    long long capacity;
    uint32_t thdr[kDngTileHeaderWords];     // the tile header, little-endian words
};

// One sample's Huffman word with its extra bits behind it, and the bit count (header: code).
__device__ __forceinline__ void dng_code(const uint32_t* tab, int v, int pred, uint32_t& word, int& n) {
    const int d = (int)(int16_t)(uint16_t)(v - pred);
    const int ssss = 32 - __clz(d < 0 ? -d : d);           // 0 for d = 0; 16 for -32768
    const uint32_t e = tab[ssss];
    const int nx = ssss == 16 ? 0 : ssss;
    word = ((e & 0xffffu) << nx) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << nx) - 1u));
    n = (int)(e >> 16) + nx;
}

template <int ST, typename TI, bool VEC, bool WRITE>
__global__ void __launch_bounds__(64) dng_tile_kernel(DngArgs a, uint32_t* __restrict__ scratch, uint8_t* __restrict__ dst) {
    __shared__ uint32_t tab[17];
    __shared__ uint32_t hdr[kDngTileHeaderWords];
    __shared__ uint32_t bb[kDngBitWords];
    const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    if (lane < 17) tab[lane] = kDngDev.tab[lane];
#pragma unroll
    for (int i = 0; i < kDngTileHeaderWords; ++i)
        if (lane == i) hdr[i] = a.thdr[i];
    for (int i = lane; i < kDngBitWords; i += 64) bb[i] = 0u;

    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int H = a.H, W = a.W, nc = a.nc;
    const size_t lb = (size_t)a.line_bytes;
    const uint8_t* fsrc = a.src + (size_t)b * (size_t)H * lb;
    uint8_t* frame = dst + (size_t)b * (size_t)a.capacity;
    const uint64_t cap = (uint64_t)a.capacity;
    const size_t slot = (size_t)b * a.ntiles + t;
    const uint64_t base = WRITE ? (uint64_t)scratch[slot] : 0ull;
    const int nsteps = (a.tw + kDngStepPx - 1) / kDngStepPx;
    const int last_group = (W - 2) & ~3;                   // where the frame's last group of 4 (or, for W = 2 mod 4, of 2) samples starts
    __syncthreads();

    if (WRITE) {
        for (int i = lane; i < a.thb; i += 64) {
            const uint64_t pos = base + (uint32_t)i;
            if (pos < cap) frame[pos] = (uint8_t)(hdr[i >> 2] >> (8 * (i & 3)));
        }
    }
    const uint64_t dbase = base + (uint32_t)a.thb;

    // the lane's group of line y, step s: always inside the frame
    auto load = [&](int y, int s) {
        const int gy0 = ty * a.th + y, gy = gy0 < H ? gy0 : H - 2 + (gy0 & 1);
        const int xb = min(tx * a.tw + s * kDngStepPx + kRowPx * lane, last_group), n = min(kRowPx, W - xb);
        return row_load<ST, TI>(fsrc + (size_t)gy * lb, xb, n, VEC && n == kRowPx);
    };

    uint32_t out = 0u;                   // stuffed bytes of this tile so far
    int carry = 0;                       // bits of the last incomplete byte, at the top of bb[0]
    int above0 = 0, above1 = 0;          // this lane's samples 0, 1 of the first step of the line above
    int left2 = 0, left3 = 0;            // lane 63's samples 2, 3 of the step before
    int y = 0, s = 0;
    RowRaw cur = load(0, 0);
#pragma unroll 1
    for (int q = 0, nq = a.th * nsteps; q < nq; ++q) {
        int y1 = y, s1 = s + 1;
        if (s1 == nsteps) { s1 = 0; ++y1; }
        const bool last = y1 == a.th;
        const RowRaw nxt = load(last ? y : y1, last ? s : s1);
        // ---- samples ----
        const int x = s * kDngStepPx + kRowPx * lane, gx0 = tx * a.tw + x;
        const int xb = min(gx0, last_group), n = min(kRowPx, W - xb);
        float f[kRowPx];
        row_decode<ST, TI>(cur, n, VEC && n == kRowPx, f);
        int v0 = (int)f[0], v1 = (int)f[1], v2 = (int)f[2], v3 = (int)f[3];
        if (gx0 >= W) {                                     // beyond the frame: its last two samples, by colour
            const bool hi = W - 2 - xb != 0;
            v0 = hi ? v2 : v0; v1 = hi ? v3 : v1;
            v2 = v0; v3 = v1;
        } else if (n == 2) {
            v2 = v0; v3 = v1;
        }
        // ---- predict ----
        int p2 = __shfl_up(v2, 1), p3 = __shfl_up(v3, 1);
        if (lane == 0) {
            if (s == 0) {
                p2 = y == 0 ? a.half : above0;
                p3 = y == 0 ? a.half : (nc == 2 ? above1 : above0);
            } else {
                p2 = left2; p3 = left3;
            }
        }
        if (s == 0) { above0 = v0; above1 = v1; }
        left2 = __shfl(v2, 63); left3 = __shfl(v3, 63);
        // ---- code ----
        uint32_t w0, w1, w2, w3;
        int n0, n1, n2, n3;
        dng_code(tab, v0, nc == 2 ? p2 : p3, w0, n0);
        dng_code(tab, v1, nc == 2 ? p3 : v0, w1, n1);
        dng_code(tab, v2, nc == 2 ? v0 : v1, w2, n2);
        dng_code(tab, v3, nc == 2 ? v1 : v2, w3, n3);
        const bool act = x < a.tw;                          // tw is a multiple of 16: all four samples of a lane, or none
        const int na = act ? n0 + n1 : 0, nb = act ? n2 + n3 : 0;
        const int incl = wave_scan_incl(na + nb, lane);
        int total = carry + __shfl(incl, 63);
        const int off = carry + incl - na - nb;
        if (na) bits_or(bb, kDngBitWords, off, ((uint64_t)w0 << n1) | w1, na);
        if (nb) bits_or(bb, kDngBitWords, off + na, ((uint64_t)w2 << n3) | w3, nb);
        if (q == nq - 1) total = bits_pad_ones(bb, total, lane);
        __syncthreads();
        // ---- stuff and store ----
        carry = bits_flush<WRITE>(bb, kDngBitWords, total, lane, frame, cap, dbase, out);
        cur = nxt;
        y = y1; s = s1;
    }
    if (lane == 0) {
        if (!WRITE) {
            scratch[slot] = out;
        } else {
            const uint64_t end = dbase + out;
            if (end < cap) frame[end] = 0xff;
            if (end + 1 < cap) frame[end + 1] = 0xd9;
            if (((a.thb + out) & 1u) && end + 2 < cap) frame[end + 2] = 0;      // the stream has an odd length: the next one starts on an even offset
        }
    }
}

// One block per frame: the header; the tiles' byte counts -> their even offsets in the file (in place, saturated at 2^32 - 1: a store beyond
// `capacity` is dropped anyway); the two LONG arrays of the header; the file's length.
constexpr int kDngScanThreads = 256;
__global__ void __launch_bounds__(kDngScanThreads) dng_scan_kernel(int ntiles, int thb, int hdr_bytes, int offsets_at, int counts_at, long long capacity,
                                                                   const uint8_t* __restrict__ hdr, uint32_t* __restrict__ scratch, uint8_t* __restrict__ dst,
                                                                   long long* __restrict__ lengths) {
    __shared__ unsigned long long wave_sum[kDngScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    uint32_t* cnt = scratch + (size_t)b * ntiles;
    uint8_t* frame = dst + (size_t)b * (size_t)capacity;
    const unsigned long long cap = (unsigned long long)capacity;
    for (int i = tid; i < hdr_bytes && (unsigned long long)i < cap; i += kDngScanThreads) frame[i] = hdr[i];
    __syncthreads();                                        // the two arrays are written over the header's zeros
    auto put32 = [&](unsigned long long at, uint32_t v) {   // little-endian; a frame need not start on a dword
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (at + k < cap) frame[at + k] = (uint8_t)(v >> (8 * k));
    };
    unsigned long long run = (unsigned long long)hdr_bytes;
    for (int i0 = 0; i0 < ntiles; i0 += kDngScanThreads) {
        const int i = i0 + tid;
        const unsigned long long size = i < ntiles ? (unsigned long long)cnt[i] + (unsigned)thb + 2ull : 0ull;     // header, data, EOI
        const unsigned long long c = (size + 1ull) & ~1ull;
        unsigned long long v = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wave_sum[wv] = v;
        __syncthreads();
        unsigned long long before = 0ull, chunk = 0ull;
#pragma unroll
        for (int k = 0; k < kDngScanThreads / 64; ++k) {
            const unsigned long long sk = wave_sum[k];
            if (k < wv) before += sk;
            chunk += sk;
        }
        if (i < ntiles) {
            const unsigned long long start = run + before + v - c;
            const uint32_t start32 = start > 0xffffffffull ? 0xffffffffu : (uint32_t)start;
            cnt[i] = start32;
            put32((unsigned long long)offsets_at + 4ull * i, start32);
            put32((unsigned long long)counts_at + 4ull * i, size > 0xffffffffull ? 0xffffffffu : (uint32_t)size);
        }
        run += chunk;
        __syncthreads();
    }
    if (tid == 0) lengths[b] = (long long)run;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static std::atomic<int> g_dng_passes{7};        // rc_debug_dng_passes: measurement only

static int dng_precision(int storage) { return storage == RC_RAW_U8 ? 8 : storage == RC_RAW_MIPI10 ? 10 : storage == RC_RAW_MIPI12 ? 12 : storage == RC_RAW_U16 ? 16 : 0; }

static const char* dng_desc_check(const rc_dng_desc* d, const rc_raw_format* fmt) {
    if (!d || !fmt) return "null pointer";
    if (fmt->storage == RC_RAW_F32 || fmt->storage == RC_RAW_BF16 || fmt->storage == RC_RAW_F16)
        return "a float storage: a DNG holds sensor codes (u16, u8, RAW10 or RAW12)";
    if (!dng_precision(fmt->storage)) return "unknown storage";
    if (d->tile_w < 16 || d->tile_w > 65520 || d->tile_w % 16 || d->tile_h < 16 || d->tile_h > 65520 || d->tile_h % 16)
        return "tile_w and tile_h must be multiples of 16 in 16 .. 65520";
    if (d->components != 1 && d->components != 2) return "components must be 1 or 2";
    for (int r : d->reserved)
        if (r) return "reserved fields must be zero";
    return nullptr;
}

static const char* dng_plan(const rc_dng_desc* d, const rc_raw_format* fmt, int h2, int w2, long long header_bytes, long long offsets_at, long long counts_at,
                            rc_dng_plan_info* p) {
    if (const char* err = dng_desc_check(d, fmt)) return err;
    if (h2 < 2 || w2 < 2 || h2 % 2 || w2 % 2) return "the mosaic's height and width must be even and at least 2";
    if (header_bytes < 8 || header_bytes % 2 || header_bytes > 0x7fffffffLL) return "header_bytes must be even and at least 8";
    p->tile_header_bytes = 58 + 5 * d->components;
    p->tiles_x = ((long long)w2 + d->tile_w - 1) / d->tile_w;
    p->tiles_y = ((long long)h2 + d->tile_h - 1) / d->tile_h;
    const long long tiles = p->tiles_x * p->tiles_y, per_tile = p->tile_header_bytes + 2 + 4LL * d->tile_w * d->tile_h;
    if (tiles > 0x7fffffffLL / per_tile || header_bytes + tiles * per_tile > 0x7fffffffLL) return "the file's default capacity must stay below 2^31 bytes";
    p->capacity = header_bytes + tiles * per_tile;
    p->scratch_bytes = 4 * tiles;
    const long long arr = 4 * tiles;
    if (offsets_at < 0 || counts_at < 0 || offsets_at % 2 || counts_at % 2 || offsets_at + arr > header_bytes || counts_at + arr > header_bytes)
        return "offsets_at and counts_at must be even and their arrays (4 bytes per tile) must lie inside the header";
    if (offsets_at < counts_at + arr && counts_at < offsets_at + arr) return "the arrays at offsets_at and counts_at overlap";
    return nullptr;
}

static int dng_tile_header(const rc_dng_desc* d, int storage, uint8_t* o) {
    uint8_t* o0 = o;
    const int nc = d->components;
    auto put = [&](int v) { *o++ = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 0xff); };
    put16(0xffd8);                                                                   // SOI
    put16(0xffc3); put16(8 + 3 * nc); put(dng_precision(storage)); put16(d->tile_h); put16(d->tile_w / nc); put(nc);      // SOF3
    for (int c = 0; c < nc; ++c) { put(c + 1); put(0x11); put(0); }
    put16(0xffc4); put16(2 + 1 + 16 + 17); put(0x00);                                // DHT: class 0, id 0
    for (int i = 0; i < 16; ++i) put(kDngBits[i]);
    for (int i = 0; i < 17; ++i) put(kDngVals[i]);
    put16(0xffda); put16(6 + 2 * nc); put(nc);                                       // SOS
    for (int c = 0; c < nc; ++c) { put(c + 1); put(0x00); }
    put(1); put(0); put(0);                                                          // predictor 1; Se; Ah / Al
    return (int)(o - o0);
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_dng_desc_size(void) { return sizeof(rc_dng_desc); }

int rc_debug_dng_passes(int mask) {
    g_dng_passes.store(mask & 7, std::memory_order_relaxed);
    return RC_OK;
}

int rc_dng_plan(const rc_dng_desc* desc, const rc_raw_format* fmt, int h2, int w2, long long header_bytes, long long offsets_at, long long counts_at,
                rc_dng_plan_info* plan) {
    RC_REQUIRE(plan, "rc_dng_plan: null pointer");
    const char* err = dng_plan(desc, fmt, h2, w2, header_bytes, offsets_at, counts_at, plan);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_dng_plan: ") + err);
    return RC_OK;
}

int rc_dng_tile_header(const rc_dng_desc* desc, const rc_raw_format* fmt, uint8_t* buf, size_t cap, size_t* len) {
    RC_REQUIRE(buf && len, "rc_dng_tile_header: null pointer");
    const char* err = dng_desc_check(desc, fmt);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_dng_tile_header: ") + err);
    RC_REQUIRE(cap >= (size_t)(58 + 5 * desc->components), "rc_dng_tile_header: the buffer is shorter than the header (rc_dng_plan's tile_header_bytes)");
    *len = (size_t)dng_tile_header(desc, fmt->storage, buf);
    return RC_OK;
}

int rc_dng_encode(const void* d_src, const rc_raw_format* fmt, const rc_dng_desc* desc, const void* d_header, long long header_bytes, long long offsets_at,
                  long long counts_at, void* d_scratch, void* d_dst, void* d_lengths, int batch, int h2, int w2, long long capacity, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_header && d_scratch && d_dst && d_lengths, "rc_dng_encode: null pointer");
    rc_dng_plan_info p;
    const char* err = dng_plan(desc, fmt, h2, w2, header_bytes, offsets_at, counts_at, &p);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_dng_encode: ") + err);
    if (const int e = raw_frames("rc_dng_encode", batch, h2 / 2, w2 / 2)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_dng_encode", d_src, fmt, w2 / 2, &rs)) return e;
    RC_REQUIRE(capacity >= 1 && capacity <= 0xffffffffLL, "rc_dng_encode: capacity must be 1 .. 2^32 - 1 bytes (TIFF offsets are LONG)");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_scratch) % 4 == 0 && reinterpret_cast<uintptr_t>(d_lengths) % 8 == 0, "rc_dng_encode: scratch or lengths misaligned");

    DngArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.H = h2; a.W = w2;
    a.line_bytes = (int)rs.line_bytes;
    a.tw = desc->tile_w; a.th = desc->tile_h; a.nc = desc->components; a.half = 1 << (dng_precision(fmt->storage) - 1);
    a.tiles_x = (int)p.tiles_x; a.ntiles = (int)(p.tiles_x * p.tiles_y);
    a.capacity = capacity;
    uint8_t th[kDngTileHeaderMax] = {};
    a.thb = dng_tile_header(desc, fmt->storage, th);
    std::memcpy(a.thdr, th, sizeof(th));
    const dim3 grid((unsigned)a.ntiles, (unsigned)batch);
    hipStream_t s = as_stream(stream);
    uint32_t* scratch = static_cast<uint32_t*>(d_scratch);
    uint8_t* dst = static_cast<uint8_t*>(d_dst);
    const int passes = g_dng_passes.load(std::memory_order_relaxed);
    by_storage(fmt->storage, [&](auto sg) {
        constexpr int ST = decltype(sg)::ST;
        typedef typename decltype(sg)::type TI;
        if constexpr (std::is_integral<TI>::value) {
            const bool vec = ST == kElem && rs.vec;
            auto pass = [&](auto plain, auto vector) {
                if (vec) hipLaunchKernelGGL(vector, grid, dim3(64), 0, s, a, scratch, dst);
                else hipLaunchKernelGGL(plain, grid, dim3(64), 0, s, a, scratch, dst);
            };
            constexpr bool V = ST == kElem;                // a packed row has no vector form
            if (passes & 1) pass(dng_tile_kernel<ST, TI, false, false>, dng_tile_kernel<ST, TI, V, false>);
            if (passes & 2)
                hipLaunchKernelGGL(dng_scan_kernel, dim3(batch), dim3(kDngScanThreads), 0, s, a.ntiles, a.thb, (int)header_bytes, (int)offsets_at, (int)counts_at,
                                   capacity, static_cast<const uint8_t*>(d_header), scratch, dst, static_cast<long long*>(d_lengths));
            if (passes & 4) pass(dng_tile_kernel<ST, TI, false, true>, dng_tile_kernel<ST, TI, V, true>);
        }
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
