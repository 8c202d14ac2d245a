// How a sensor mosaic row is stored, and nothing else: the one reader of the rc_raw_storage forms for the six entry points that read a frame
// as rc_raw_format describes it -- rc_raw_ingest_fmt (raw_format.hip), rc_raw_defects (defects.hip), rc_raw_calibrate (calibrate.hip),
// rc_raw_hdr_merge (hdr_merge.hip), rc_raw_temporal (temporal.hip) and rc_raw_quad (quad.hip).  A row is either one TI per sample (fp32 /
// bf16 / fp16 / uint16 / uint8) or MIPI CSI-2 packed bytes: RAW10 = groups of 5 bytes (bytes 0-3: bits [9:2] of samples 0-3, byte 4: their
// bits [1:0], sample k at bits 2k+1..2k), RAW12 = groups of 3 bytes (bytes 0, 1: bits [11:4] of samples 0, 1, byte 2: their bits [3:0],
// sample 1 high).  A lane works on kRowPx consecutive samples that start on a multiple of kRowPx: one RAW10 group, two RAW12 groups.  The
// host half is here too: by_storage for an entry's launch, and the checks the entries share (raw_frames, raw_source, raw_pitch ...).  A
// further storage is added in this header alone: the window, its unpack, row_load / row_decode, and by_storage and raw_source on the host.
#pragma once
#include <cmath>

#include "common.hpp"

namespace rc {

enum { kElem = 0, kMipi10 = 1, kMipi12 = 2 };   // how a mosaic row is stored: one TI per sample, or MIPI CSI-2 packed bytes
constexpr int kRowPx = 4;                        // samples of a row per lane

// ---- packed rows: the 64-bit window ---------------------------------------------------------------------------------------------------------
// Bytes [sh, sh + nb) (sh < 4, nb <= 6) of the dwords at d as a little-endian 64-bit window: only the dwords that hold at least one wanted
// byte are loaded, so nothing past the dword holding the buffer's last byte is touched.
__device__ __forceinline__ uint64_t window_dwords(const uint32_t* d, int sh, int nb) {
    const int ndw = (sh + nb + 3) >> 2;
    const uint32_t w0 = d[0];
    const uint32_t w1 = ndw > 1 ? d[1] : 0u;
    const uint32_t w2 = ndw > 2 ? d[2] : 0u;
    const uint64_t lo = ((uint64_t)w1 << 32) | w0;
    return sh ? (lo >> (8 * sh)) | ((uint64_t)w2 << (64 - 8 * sh)) : lo;
}

// The two ways a kernel names those bytes.  Byte s of a 4-byte aligned buffer (any line stride): the address stays (uniform base, offset).
__device__ __forceinline__ uint64_t window_at(const uint8_t* base, size_t s, int nb) {
    return window_dwords(reinterpret_cast<const uint32_t*>(base + (s & ~(size_t)3)), (int)(s & 3), nb);
}

// Any pointer (a frame of a batch need not start on a dword): read from the 4-byte boundary below it.
__device__ __forceinline__ uint64_t window_ptr(const uint8_t* p, int nb) {
    const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
    return window_dwords(reinterpret_cast<const uint32_t*>(ad & ~(uintptr_t)3), (int)(ad & 3), nb);
}

// Sample k of a group from its high byte and the group's byte of low bits.
__device__ __forceinline__ float raw10_value(uint32_t high, uint32_t low_bits, int k) { return (float)((high << 2) | ((low_bits >> (2 * k)) & 3u)); }
__device__ __forceinline__ float raw12_value(uint32_t high, uint32_t low_bits, int k) { return (float)((high << 4) | ((low_bits >> (4 * k)) & 15u)); }

__device__ __forceinline__ void unpack_raw10(uint64_t g, float* v) {               // 2w % 4 == 0: always a whole 5-byte group
    const uint32_t low_bits = (uint32_t)(g >> 32) & 0xffu;
#pragma unroll
    for (int k = 0; k < kRowPx; ++k) v[k] = (float)((((uint32_t)(g >> (8 * k)) & 0xffu) << 2) | ((low_bits >> (2 * k)) & 3u));
}

__device__ __forceinline__ void unpack_raw12(uint64_t g, int n, float* v) {        // n == 2 (the end of a row of 2 mod 4 samples): v[2] = v[3] = 0
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t b0 = (uint32_t)(g >> (24 * j)) & 0xffu, b1 = (uint32_t)(g >> (24 * j + 8)) & 0xffu, b2 = (uint32_t)(g >> (24 * j + 16)) & 0xffu;
        const bool live = j == 0 || n == 4;
        v[2 * j] = live ? (float)((b0 << 4) | (b2 & 15u)) : 0.f;
        v[2 * j + 1] = live ? (float)((b1 << 4) | (b2 >> 4)) : 0.f;
    }
}

// Where the group that holds sample x0 >= 0 starts in a packed row, in the type the caller forms its offsets in (it fits 32 bits: a line is
// below 2 GiB), and how many bytes the groups of n = 2 or 4 samples from a multiple of 4 are.
template <int ST, typename T> __device__ __forceinline__ T packed_offset(int x0) { return ST == kMipi10 ? (T)(x0 >> 2) * 5 : (T)(x0 >> 1) * 3; }
template <int ST> __device__ __forceinline__ int packed_bytes(int n) { return ST == kMipi10 ? 5 : n == 4 ? 6 : 3; }

// ---- a lane's 4 samples of a row, as loaded and as floats -----------------------------------------------------------------------------------
struct RowRaw { uint32_t d[4]; };                // a row's bytes as loaded (or, sample by sample, its 4 values)

// `full`: n == 4 and the lane may use one vector load (p on a 4-sample boundary); otherwise sample by sample, n of them.
template <typename TI>
__device__ __forceinline__ RowRaw elem_load(const TI* p, int n, bool full) {
    RowRaw r = {{0u, 0u, 0u, 0u}};
    if (full) {
        if constexpr (sizeof(TI) == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            r.d[0] = q.x; r.d[1] = q.y; r.d[2] = q.z; r.d[3] = q.w;
        } else if constexpr (sizeof(TI) == 2) {
            const uint2 q = *reinterpret_cast<const uint2*>(p);
            r.d[0] = q.x; r.d[1] = q.y;
        } else {
            r.d[0] = *reinterpret_cast<const uint32_t*>(p);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRowPx; ++k) r.d[k] = k < n ? __float_as_uint(to_f32(p[k])) : 0u;
    }
    return r;
}

__device__ __forceinline__ RowRaw packed_row(uint64_t g) { return {{(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u}}; }

// Columns x0 .. x0 + 3 (n of them inside the frame) of the row at `row`, any pointer.
template <int ST, typename TI>
__device__ __forceinline__ RowRaw row_load(const uint8_t* row, int x0, int n, bool full) {
    if constexpr (ST == kElem) return elem_load(reinterpret_cast<const TI*>(row) + x0, n, full);
    else return packed_row(window_ptr(row + packed_offset<ST, uint32_t>(x0), packed_bytes<ST>(n)));
}

// The same of the row that starts `off` bytes into the buffer at `base` (4-byte aligned when packed).
template <int ST, typename TI>
__device__ __forceinline__ RowRaw row_load(const uint8_t* base, size_t off, int x0, int n, bool full) {
    if constexpr (ST == kElem) return elem_load(reinterpret_cast<const TI*>(base + off) + x0, n, full);
    else return packed_row(window_at(base, off + packed_offset<ST, size_t>(x0), packed_bytes<ST>(n)));
}

template <int ST, typename TI>
__device__ __forceinline__ void row_decode(const RowRaw& r, int n, bool full, float* v) {
    if constexpr (ST == kMipi10) {
        unpack_raw10(((uint64_t)r.d[1] << 32) | r.d[0], v);
    } else if constexpr (ST == kMipi12) {
        unpack_raw12(((uint64_t)r.d[1] << 32) | r.d[0], n, v);
    } else if (!full) {
#pragma unroll
        for (int k = 0; k < kRowPx; ++k) v[k] = __uint_as_float(r.d[k]);
    } else if constexpr (__is_same(TI, float)) {
#pragma unroll
        for (int k = 0; k < kRowPx; ++k) v[k] = __uint_as_float(r.d[k]);
    } else if constexpr (__is_same(TI, bf16_t)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { v[2 * j] = __uint_as_float(r.d[j] << 16); v[2 * j + 1] = __uint_as_float(r.d[j] & 0xffff0000u); }
    } else if constexpr (__is_same(TI, f16_t)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { v[2 * j] = Vec16<f16_t>::lo(r.d[j]); v[2 * j + 1] = Vec16<f16_t>::hi(r.d[j]); }
    } else if constexpr (sizeof(TI) == 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { v[2 * j] = (float)(r.d[j] & 0xffffu); v[2 * j + 1] = (float)(r.d[j] >> 16); }
    } else {
#pragma unroll
        for (int k = 0; k < kRowPx; ++k) v[k] = (float)((r.d[0] >> (8 * k)) & 0xffu);
    }
}

// ---- a lane's 4 results of a row ------------------------------------------------------------------------------------------------------------
template <typename TO>
__device__ __forceinline__ uint32_t row_bits(float v) {                            // the stored value, as the low bits of a word
    if constexpr (__is_same(TO, uint16_t)) return (uint32_t)rintf(v);              // half to even; the caller keeps v in 0 .. 65535
    else if constexpr (__is_same(TO, float)) return __float_as_uint(v);
    else return (uint32_t)__builtin_bit_cast(uint16_t, from_f32<TO>(v));           // round to nearest even
}

// `full`: n == 4 and o on a 4-sample boundary: one 8- or 16-byte store.
template <typename TO>
__device__ __forceinline__ void row_store(TO* o, const float* v, int n, bool full) {
    if (full) {
        if constexpr (sizeof(TO) == 4) {
            *reinterpret_cast<uint4*>(o) = make_uint4(row_bits<TO>(v[0]), row_bits<TO>(v[1]), row_bits<TO>(v[2]), row_bits<TO>(v[3]));
        } else {
            *reinterpret_cast<uint2*>(o) = make_uint2(row_bits<TO>(v[0]) | (row_bits<TO>(v[1]) << 16), row_bits<TO>(v[2]) | (row_bits<TO>(v[3]) << 16));
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRowPx; ++k) {
            if (k < n) {
                if constexpr (sizeof(TO) == 4) reinterpret_cast<uint32_t*>(o)[k] = row_bits<TO>(v[k]);
                else reinterpret_cast<uint16_t*>(o)[k] = (uint16_t)row_bits<TO>(v[k]);
            }
        }
    }
}

// ---- the host half: the launch ---------------------------------------------------------------------------------------------------------------
// The one map from rc_raw_storage to how a kernel reads it: f(Stored<ST, TI>()) for a checked storage; its result is returned.  The choices
// that belong to one stage (a destination type: common.hpp's by_dtype; hdr's E, quad's mode) are made inside f.
template <int S, typename T> struct Stored { static constexpr int ST = S; typedef T type; };

template <typename F>
inline auto by_storage(int storage, F&& f) {
    switch (storage) {
        case RC_RAW_F32: return f(Stored<kElem, float>());
        case RC_RAW_BF16: return f(Stored<kElem, bf16_t>());
        case RC_RAW_F16: return f(Stored<kElem, f16_t>());
        case RC_RAW_U16: return f(Stored<kElem, uint16_t>());
        case RC_RAW_U8: return f(Stored<kElem, uint8_t>());
        case RC_RAW_MIPI10: return f(Stored<kMipi10, uint8_t>());
        default: return f(Stored<kMipi12, uint8_t>());
    }
}

// What a stage that keeps the storage writes: a float storage as itself, counts (u16 / u8 / RAW10 / RAW12) as uint16 (RawSource::usize bytes).
template <typename TI> using unpacked_t = typename std::conditional<std::is_integral<TI>::value, uint16_t, TI>::type;

// ---- the host half: the checks ---------------------------------------------------------------------------------------------------------------
// Each returns RC_OK, or the error as RC_REQUIRE reports it; `who` names the entry point in the messages.
template <typename T, size_t N>
inline bool all_zero(const T (&v)[N]) {                                            // reserved fields
    for (size_t i = 0; i < N; ++i)
        if (v[i] != 0) return false;
    return true;
}

// Every lane's kRowPx samples of `bytes` each are one vector access: the base and the pitch are multiples of it.
inline bool raw_vec(const void* p, long long pitch, int bytes) { return reinterpret_cast<uintptr_t>(p) % (kRowPx * bytes) == 0 && pitch % (kRowPx * bytes) == 0; }

// `batch` frames of a mosaic (2h, 2w): the grid's z takes 65535, and rows and columns stay far inside an int.
inline int raw_frames(const char* who, int batch, int h, int w) {
    RC_REQUIRE(batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && h <= (1 << 20) && w <= (1 << 24), std::string(who) + ": bad shape (empty, more than 65535 frames, or too large)");
    return RC_OK;
}

struct RawSource {
    long long line_bytes;      // the frame's line stride (fmt->line_bytes, or one dense row): fits an int
    int esize;                 // bytes per sample of an element storage (2 for the packed ones: what they unpack to)
    int usize;                 // bytes per sample of unpacked_t
    bool packed;               // MIPI RAW10 / RAW12
    bool vec;                  // an element storage whose base and lines are multiples of kRowPx samples
};

// What every entry point that reads a sensor frame (B, 2h, 2w) at d_src as `fmt` describes it requires of the two.
inline int raw_source(const char* who, const void* d_src, const rc_raw_format* fmt, int w, RawSource* out) {
    const std::string at = std::string(who) + ": ";
    const int st = fmt->storage;
    RC_REQUIRE(st >= RC_RAW_F32 && st <= RC_RAW_MIPI12, at + "unknown storage");
    RC_REQUIRE(fmt->cfa >= RC_CFA_RGGB && fmt->cfa <= RC_CFA_GBRG, at + "unknown cfa");
    RC_REQUIRE(all_zero(fmt->reserved), at + "the format's reserved fields must be zero");
    RC_REQUIRE(fmt->width == 0 || fmt->width == 2 * w, at + "width must be 0 or the mosaic width 2w");
    const bool packed = st == RC_RAW_MIPI10 || st == RC_RAW_MIPI12;
    RC_REQUIRE(st != RC_RAW_MIPI10 || (2 * w) % 4 == 0, at + "RAW10 needs a mosaic width 2w divisible by 4");
    const int esize = st == RC_RAW_F32 ? 4 : st == RC_RAW_U8 ? 1 : 2;
    const long long need = st == RC_RAW_MIPI10 ? 2LL * w * 10 / 8 : st == RC_RAW_MIPI12 ? 2LL * w * 12 / 8 : 2LL * w * esize;
    const long long lb = fmt->line_bytes ? fmt->line_bytes : need;
    RC_REQUIRE(lb >= need && lb <= 0x7fffffffLL, at + "line_bytes shorter than one mosaic row");
    RC_REQUIRE(packed || lb % esize == 0, at + "line_bytes must be a multiple of the sample size");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % (packed ? 4 : esize) == 0, at + "source misaligned (MIPI: 4 bytes, else one sample)");
    *out = {lb, esize, st == RC_RAW_F32 ? 4 : 2, packed, !packed && raw_vec(d_src, lb, esize)};
    return RC_OK;
}

inline int raw_blacks_finite(const char* who, const rc_raw_format* fmt) {
    for (int p = 0; p < 4; ++p) RC_REQUIRE(std::isfinite(fmt->black[p]), std::string(who) + ": black levels must be finite");
    return RC_OK;
}

// A destination or state buffer (`name`: "dst", "prev") at p, rows of row_bytes, samples of esize bytes: its pitch (0: dense) into *out.
inline int raw_pitch(const char* who, const char* name, const void* p, int pitch_bytes, long long row_bytes, int esize, long long* out) {
    const long long pitch = pitch_bytes ? pitch_bytes : row_bytes;
    RC_REQUIRE(pitch >= row_bytes && pitch <= 0x7fffffffLL && pitch % esize == 0,
               std::string(who) + ": " + name + " pitch shorter than one row or no multiple of the sample size");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(p) % esize == 0, std::string(who) + ": " + name + " misaligned");
    *out = pitch;
    return RC_OK;
}

// A gain given on the host (`host_gain`: it is; `how` names that way in the message) or as (gain_batch) floats on the device, not both.
inline int raw_gain(const char* who, const char* how, bool host_gain, float host_value, const float* d_gain, int gain_batch, int batch) {
    const std::string at = std::string(who) + ": ";
    RC_REQUIRE(!(host_gain && d_gain), at + "the gain is given both ways (" + how + " and d_gain)");
    if (d_gain) {
        RC_REQUIRE(gain_batch == 1 || gain_batch == batch, at + "gain_batch must be 1 or the batch");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(d_gain) % 4 == 0, at + "the gain must be 4-byte aligned");
    } else {
        RC_REQUIRE(gain_batch == 0, at + "gain_batch without d_gain must be 0");
        if (host_gain) RC_REQUIRE(std::isfinite(host_value) && host_value > 0.f, at + "the gain must be finite and > 0");
    }
    return RC_OK;
}

}  // namespace rc
