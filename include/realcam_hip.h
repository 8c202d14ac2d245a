/*
 * realcam_hip.h -- C ABI of librealcam_hip.so: the MI355X (gfx950) RAW->sRGB hot path.
 *
 * Drop-in boundary.  The upstream project (kepengxu/RealCamNet) has no FFI
 * layer: its hot path is a chain of stock ATen calls made from nn.Module.forward().  Each entry
 * point below replaces one such call site; the citation gives the reference file:line (paths
 * relative to the upstream repo).  The Python modules in realcamnet_amd/ keep the reference class
 * names / state_dict keys / forward() signatures and reach these symbols through ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer named d_* / in desc structs is DEVICE memory on
 *     the current HIP device unless the comment says "host".
 *   - activations are NHWC ("pixel-major"): element (b,y,x,c) at ((b*H + y)*W + x)*C + c.
 *   - dtype: RC_F32 (float) or RC_BF16 (bfloat16 storage, fp32 accumulate).  (ABI 15) RC_F16 (IEEE half storage, fp32
 *     accumulate, values beyond +-65504 become inf) wherever the ISP path accepts RC_BF16: the bayer / ingest / layout
 *     plumbing, rc_conv2d (not ksize 2, not the 32x32x16 forms) and its packers, the DWT, tail-fold, gate / FiLM / SFT,
 *     resampling and colour-prior entry points.  Entry points off that path (codecs, GroupMix, Winograd, rc_conv_pair,
 *     the register-resident layer chains) return RC_ERR_UNSUPPORTED / RC_ERR_INVALID ("bad dtype") for it.
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*); no host sync, no
 *     allocation -> HIP-graph capturable.
 *   - return value: 0 on success, negative rc_status otherwise; rc_last_error() gives the text.
 *     Shape / alignment violations are reported, never silently "fixed".
 */
#ifndef REALCAM_HIP_H
#define REALCAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 15

typedef enum rc_status {
    RC_OK = 0,
    RC_ERR_INVALID = -1,     /* bad argument (shape, alignment, null pointer, unsupported combination) */
    RC_ERR_HIP = -2,         /* a HIP runtime call failed */
    RC_ERR_UNSUPPORTED = -3  /* valid request, but no kernel instantiation covers it */
} rc_status;

typedef enum rc_dtype { RC_F32 = 0, RC_BF16 = 1, RC_U16 = 2 /* sensor counts: rc_raw_ingest's mosaic only */,
                        RC_F16 = 3 /* (ABI 15) IEEE binary16 storage, fp32 accumulate: the ISP path's entry points only */ } rc_dtype;

typedef enum rc_act { RC_ACT_NONE = 0, RC_ACT_RELU = 1, RC_ACT_LEAKY = 2 /* slope in act_slope */,
                      RC_ACT_GELU = 3 /* exact erf GELU: nn.GELU() in groupmix.Mlp */,
                      RC_ACT_RELU_POST = 4 /* ReLU applied LAST, after the residual add: relu(conv(x) + residual), the
                                              ResidualUnit of CompressAI's AttentionBlock (models/tcm.py:270 SWAtten) */ } rc_act;

typedef enum rc_out_mode {
    RC_OUT_NHWC = 0,           /* out[b][y][x][cout]                                             */
    RC_OUT_PIXEL_SHUFFLE2 = 1, /* nn.PixelShuffle(2) folded into the store:
                                  out[b][2y+i][2x+j][c] <- conv channel 4c+2i+j; out is NHWC (2H,2W,cout/4) */
    RC_OUT_NCHW = 2,           /* planar out[b][cout][y][x], cropped to (out_h,out_w); the network's
                                  final tensor (reference forward returns NCHW)                   */
    RC_OUT_PIXEL_SHUFFLE2_NCHW = 3, /* nn.PixelShuffle(2) + planar store: out[b][c][2y+i][2x+j] <- conv channel 4c+2i+j, cropped to
                                  (out_h,out_w) <= (2 height, 2 width); out_dtype fp32 or the activation dtype.  The folded tail's store
                                  (rc_tail_fold_weights)                                          */
    RC_OUT_NHWC_DWT = 4        /* (ABI 14) the convolution followed by networks.DWTForward (models/networks.py:224-235, the `conv -> DWT`
                                  end of LiteISP's down1, models/LiteISP.py:1950-1953) in ONE launch: out is NHWC (height/2, width/2, 4 cout),
                                  out[b][y][x][4c+k] = sum_ij haar[k][i][j] * bf16(conv[b][2y+i][2x+j][c]) with the reference's frozen taps
                                  haar = .5 * {++++, ++--, +-+-, +--+}; the full-resolution map is never written.  Bit-identical to rc_conv2d
                                  (RC_OUT_NHWC) + rc_dwt_forward with those taps.  bf16 or fp16 (rounded to that type), ksize 3, one Cin chunk and one cout tile of 32 or
                                  48 channels (the layers of the wave-autonomous kernel), even height / width, act NONE / RELU / LEAKY, or act NONE with a
                                  residual (NHWC, the conv's own shape: an RCAGroup's closing conv + group skip in front of the DWT, LiteISP down2);
                                  no film / mul_plus1 / gate / chan_sums: anything else is RC_ERR_UNSUPPORTED */
} rc_out_mode;

/* ---- library -------------------------------------------------------------------------------- */
int rc_abi_version(void);
const char* rc_last_error(void);           /* thread-local, host string */
const char* rc_build_info(void);           /* "gfx950 <compiler>" */
/* Device query used by the host mirror to fail loudly on a wrong GPU: writes the gcnArchName. */
int rc_device_arch(char* buf, size_t buflen);

/* ---- a1/a2: Bayer pixel-unshuffle + zero pad -------------------------------------------------
 * Replaces: the "Unpixel shuffle" box of assets/networkarch.png (README.md:33-38; upstream has no
 * code for it, every model already takes the packed tensor, models/LiteISP.py:2670) fused with
 * pad_to_multiple_of_16 (models/LiteISP.py:84-105).
 * mosaic: (B, 2*h, 2*w) one plane, dtype `in_dtype`; packed: NHWC (B, hp, wp, 4), hp>=h, wp>=w,
 * channel k = 2*i + j <- mosaic pixel (2y+i, 2x+j); rows/cols beyond (h,w) are written as zero. */
int rc_bayer_unshuffle(const void* d_mosaic, int in_dtype, void* d_packed, int out_dtype,
                       int batch, int h, int w, int hp, int wp, void* stream);

/* ---- f4: RAW ingest in front of the path ----------------------------------
 * The "Unpixel shuffle" and "Resize" boxes of assets/networkarch.png with the sensor normalisation upstream leaves to
 * the data loader: v' = (v - black_level) / (white_level - black_level); packed as rc_bayer_unshuffle (zero padded to
 * hp x wp); cond (B,4,cond_h,cond_w) NCHW = bilinear resize of the un-padded normalised packed RAW (h x w) with
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False) semantics -- the colour prior's input
 * (models/LiteISP.py:2016, x[1]).  One launch.  in_dtype may also be RC_U16 (sensor counts, e.g. black 64 / white 1023). */
int rc_raw_ingest(const void* d_mosaic, int in_dtype, void* d_packed, void* d_cond, int out_dtype, int batch, int h, int w,
                  int hp, int wp, int cond_h, int cond_w, float black_level, float white_level, void* stream);

/* ---- sensor RAW formats (ABI 15, additive) -----------------------------------------------------
 * rc_raw_ingest for the frames a camera stack delivers.  Still the "Unpixel shuffle" and "Resize" boxes of
 * assets/networkarch.png in front of pad_to_multiple_of_16 (models/LiteISP.py:84-105), one launch. */
typedef enum rc_raw_storage {
    RC_RAW_F32 = 0, RC_RAW_BF16 = 1, RC_RAW_U16 = 2, RC_RAW_F16 = 3,   /* one sample per element (the rc_dtype values; U16: LSB-aligned counts) */
    RC_RAW_U8 = 4,                                                      /* one count per byte */
    RC_RAW_MIPI10 = 5,  /* MIPI CSI-2 RAW10: 4 samples in 5 bytes; bytes 0-3 = bits [9:2] of samples 0-3, byte 4 bits 2k+1..2k = bits [1:0] of
                           sample k.  The mosaic width 2w must be a multiple of 4 */
    RC_RAW_MIPI12 = 6   /* MIPI CSI-2 RAW12: 2 samples in 3 bytes; byte 0 = s0[11:4], byte 1 = s1[11:4], byte 2 = s1[3:0] << 4 | s0[3:0] */
} rc_raw_storage;

/* Colour of the mosaic cell positions (0,0), (0,1), (1,0), (1,1).  The packed map keeps the RGGB slot meaning (slot 0 R, 1 G of the
 * R row, 2 G of the B row, 3 B); each slot reads the position of its colour in the same 2x2 cell (pack_raw convention). */
typedef enum rc_cfa { RC_CFA_RGGB = 0, RC_CFA_BGGR = 1, RC_CFA_GRBG = 2, RC_CFA_GBRG = 3 } rc_cfa;

typedef struct rc_raw_format {
    int storage;      /* rc_raw_storage */
    int cfa;          /* rc_cfa */
    int line_bytes;   /* bytes from one mosaic row to the next, >= the packed / element size of 2w samples; 0: exactly that.  The bytes past
                         the row's samples are ignored (a V4L2 bytesperline) */
    int width;        /* mosaic width 2w in samples, or 0 */
    float black[4];   /* black level per CFA position (0,0), (0,1), (1,0), (1,1) (DNG BlackLevel order) */
    float white;      /* white level, > every black level */
    int reserved[4];  /* zero */
} rc_raw_format;
size_t rc_raw_format_size(void);

/* d_src: B frames of 2h rows of fmt->line_bytes bytes (4-byte aligned for MIPI storage).  packed NHWC (B,hp,wp,4) zero padded and cond
 * (B,4,cond_h,cond_w) NCHW exactly as rc_raw_ingest, with v' = (v - black[pos]) * (1 / (white - black[pos])) (fp32, the divisor
 * computed on the host) for the CFA position pos each packed slot reads.  RGGB with four equal black levels gives rc_raw_ingest's
 * bits.  out_dtype RC_F32 / RC_BF16 / RC_F16. */
int rc_raw_ingest_fmt(const void* d_src, const rc_raw_format* fmt, void* d_packed, void* d_cond, int out_dtype, int batch, int h, int w,
                      int hp, int wp, int cond_h, int cond_w, void* stream);

/* ---- RGB out: the network's planar result (models/LiteISP.py:2032-2035, the sRGB tensor `out`) as interleaved 8- or 16-bit RGB ----------
 * src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16, cropped to (h,w); dst (B,h,w,3) uint8 (out_bits 8) or uint16 (out_bits 16), 16-byte
 * aligned: q = clamp(rint(float(y) * S), 0, S), S = 255 or 65535, round half to even, NaN -> 0. */
int rc_rgb_encode(const void* d_src, int src_dtype, void* d_dst, int out_bits, int batch, int H, int W, int h, int w, void* stream);

/* ---- video-encoder out (ABI 15, additive): the same planar result as one Y'CbCr 4:2:0 surface per frame -------------------------------
 * What hardware and software video encoders take: NV12 / I420 (8 bit) and P010 (10 bit), with the caller's row pitch and plane
 * offsets.  One launch that reads the result once; pitch and height padding is written as zero by the same launch. */
typedef enum rc_yuv_layout {
    RC_YUV_NV12 = 0,   /* uint8: Y plane, then one plane of interleaved Cb,Cr pairs at half size, same pitch */
    RC_YUV_P010 = 1,   /* NV12's planes as uint16, the 10-bit code in the HIGH bits (code << 6); pitch and offsets still in bytes */
    RC_YUV_I420 = 2,   /* uint8: Y, Cb, Cr planes; the chroma pitch is pitch / 2 */
    /* 3..15 are not layouts.  The professional video surfaces (additive; see rc_yuv_encode): */
    RC_YUV_NV16 = 16,  /* 4:2:2  8 bit: uint8 Y plane, then an interleaved CbCr plane of as many rows, same pitch */
    RC_YUV_P210 = 17,  /* 4:2:2 10 bit: NV16's planes as uint16, code << 6 */
    RC_YUV_I422 = 18,  /* 4:2:2  8 bit: uint8 Y, Cb, Cr planes; the chroma pitch is pitch / 2 (yuv422p) */
    RC_YUV_I210 = 19,  /* 4:2:2 10 bit: I422's planes as uint16, the code in the LOW bits (yuv422p10le) */
    RC_YUV_I010 = 20,  /* 4:2:0 10 bit: I420's planes as uint16, the code in the LOW bits (yuv420p10le) */
    RC_YUV_I444 = 21,  /* 4:4:4  8 bit: three uint8 planes, all at `pitch` (yuv444p) */
    RC_YUV_I410 = 22,  /* 4:4:4 10 bit: the same as uint16, the code in the LOW bits (yuv444p10le) */
    RC_YUV_YUY2 = 23,  /* 4:2:2  8 bit, one plane: bytes Y0 Cb Y1 Cr per pixel pair */
    RC_YUV_UYVY = 24,  /* 4:2:2  8 bit, one plane: bytes Cb Y0 Cr Y1 */
    RC_YUV_Y210 = 25,  /* 4:2:2 10 bit, one plane: YUY2's order as uint16, code << 6 */
    RC_YUV_V210 = 26   /* 4:2:2 10 bit, one plane: six pixels in four little-endian dwords (below) */
} rc_yuv_layout;
typedef enum rc_yuv_matrix { RC_MATRIX_BT601 = 0, RC_MATRIX_BT709 = 1, RC_MATRIX_BT2020 = 2 /* its luma coefficients only: no gamut conversion */ } rc_yuv_matrix;
typedef enum rc_yuv_range { RC_RANGE_LIMITED = 0, RC_RANGE_FULL = 1 } rc_yuv_range;
typedef enum rc_chroma_siting { RC_SITING_LEFT = 0 /* co-sited with the even column, between the rows: MPEG-2 / H.264 / HEVC */,
                                RC_SITING_CENTER = 1 /* the middle of the 2x2 block: JPEG / MPEG-1 */ } rc_chroma_siting;

/* The one table of luma coefficients {Kr, Kb} per rc_yuv_matrix.  Kg = 1 - Kr - Kb, sb = 0.5 / (1 - Kb), sr = 0.5 / (1 - Kr) are
 * computed from it in double and rounded to fp32 once. */
#define RC_YUV_KR_KB {{0.299, 0.114}, {0.2126, 0.0722}, {0.2627, 0.0593}}

typedef struct rc_out_format {
    int layout;            /* rc_yuv_layout */
    int matrix;            /* rc_yuv_matrix */
    int range;             /* rc_yuv_range */
    int siting;            /* rc_chroma_siting */
    int pitch;             /* bytes from one Y row to the next, >= the row's bytes, a multiple of the sample size (I420: even; V210: 4); 0: exactly the
                              row's bytes.  A multiple of 16 (with 16-byte aligned offsets) takes the 16-byte store path */
    int rows;              /* allocated rows of the Y plane, >= h; 0: h.  A chroma plane has ceil(rows / 2) allocated rows */
    int chroma_offset[2];  /* bytes from the frame's start to the CbCr plane (NV12 / P010) or the Cb and Cr planes (I420); 0: packed behind
                              the plane before.  Planes must not overlap */
    int reserved[4];       /* zero */
} rc_out_format;
size_t rc_out_format_size(void);

/* Bytes of one frame of (h, w) pixels: the end of its last plane, allocated rows included (frame b of a batch starts at b times this).
 * 0 and rc_last_error() for a format rc_yuv_encode would refuse. */
size_t rc_yuv_frame_bytes(const rc_out_format* fmt, int h, int w);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w), both even; d_dst 16-byte aligned, batch * rc_yuv_frame_bytes.
 * fp32, every product and every sum rounded on its own in the order written (no fused multiply-add):
 *   r,g,b = float(src), NaN -> 0, clamped to [0,1];  Y = ((Kr r) + (Kg g)) + (Kb b);  Cb = (b - Y) sb;  Cr = (r - Y) sr
 *   4:2:0 of the unquantised Cb, Cr, for block rows 2j, 2j+1 and columns 2i, 2i+1:
 *     CENTER  ((c[2j][2i] + c[2j][2i+1]) + (c[2j+1][2i] + c[2j+1][2i+1])) 0.25
 *     LEFT    per row t = ((c[x-1] + c[x+1]) + (c[x] + c[x])) 0.25 with x = 2i, x-1 clamped to column 0; then (t[2j] + t[2j+1]) 0.5
 *   code = clamp(rint(v S + O), lo, hi), round half to even; n = 8 or 10 bits, k = 2^(n-8):
 *     LIMITED  Y: S 219k, O 16k, [16k, 235k]; chroma: S 224k, O 128k, [16k, 240k].  FULL  S 2^n - 1, O 0 (Y) / 2^(n-1) (chroma), [0, 2^n - 1]
 * Every byte of the Y plane's rows x pitch and of the chroma planes' ceil(rows / 2) x pitch that is not a sample is written as zero.
 * Odd h / w, a pitch below the row's bytes, overlapping planes, a misaligned d_dst: RC_ERR_INVALID before any launch.
 *
 * The layouts from RC_YUV_NV16 on (4:2:2, 4:4:4, planar 10 bit, packed, V210) share the steps above -- clamp, Y / Cb / Cr, code at
 * n = 8 or 10 -- and differ in the chroma step and in the storage:
 *   4:2:2 of the unquantised Cb, Cr, per row, for columns 2i, 2i+1:
 *     CENTER  (c[2i] + c[2i+1]) 0.5
 *     LEFT    ((c[x-1] + c[x+1]) + (c[x] + c[x])) 0.25 with x = 2i, x-1 clamped to column 0: the row step t of the 4:2:0 LEFT rule
 *   4:4:4: no chroma step, `siting` is not used (it must still be a valid value).  I010: the 4:2:0 rule above at n = 10.
 *   Sizes: I010 needs an even h and w; every 4:2:2 layout an even w, any h; 4:4:4 any size.
 *   chroma_offset[]: the CbCr plane (NV16 / P210, [1] zero), the Cb and Cr planes (I422 / I210 / I010 / I444 / I410); both zero for the
 *   one-plane layouts YUY2 / UYVY / Y210 / V210.  A chroma plane of 4:2:2 / 4:4:4 has `rows` allocated rows; the chroma pitch is
 *   pitch / 2 for I422 / I210 / I010 (pitch a multiple of twice the sample size) and pitch for the others.
 *   pitch 0 is the tight row: w samples (planar, semi-planar), 2 w samples (YUY2 / UYVY / Y210), ceil(w / 6) 16 bytes (V210).
 *   V210: each group of six pixels Y0..Y5, Cb0..Cb2, Cr0..Cr2 is four dwords, bits 30-31 zero, the 10-bit codes unshifted:
 *     w0 = Cb0 | Y0 << 10 | Cr0 << 20;  w1 = Y1 | Cb1 << 10 | Y2 << 20;  w2 = Cr1 | Y3 << 10 | Cb2 << 20;  w3 = Y4 | Cr2 << 10 | Y5 << 20
 *     The fields of samples a last group does not have are zero.  Any pitch >= ceil(w / 6) 16 that is a multiple of 4 is taken.
 *   As above, every byte of the allocated rows x pitch of every plane that is not a sample is written as zero by the one launch. */
int rc_yuv_encode(const void* d_src, int src_dtype, const rc_out_format* fmt, void* d_dst, int batch, int H, int W, int h, int w, void* stream);

/* ---- JPEG out (ABI 15, additive): the same planar result as one baseline JFIF file per frame, coded on the device ------------------------
 * The one compressed still of the output side: 8-bit baseline sequential DCT, Huffman coded with the typical tables of ITU-T T.81
 * Annex K.3.3, three components, 4:2:0 or 4:4:4, restart intervals.  Three launches per call and no host sync: every restart interval is
 * coded by one wave, twice -- once to count its bytes, once, after a scan of the counts, straight to its place in the file. */
typedef enum rc_jpeg_subsampling { RC_JPEG_420 = 0 /* MCU 16x16: Y00 Y01 Y10 Y11 Cb Cr */, RC_JPEG_444 = 1 /* MCU 8x8: Y Cb Cr */ } rc_jpeg_subsampling;

typedef struct rc_jpeg_desc {
    int quality;           /* 1 .. 100: the IJG scaling of the Annex K.1 / K.2 tables (rc_jpeg_tables) */
    int subsampling;       /* rc_jpeg_subsampling */
    int restart;           /* MCUs per restart interval, 1 .. 65535 (the DRI segment's 16 bits) */
    int reserved[5];       /* zero */
} rc_jpeg_desc;
size_t rc_jpeg_desc_size(void);

/* What a (h, w) frame needs, 1 <= h, w <= 65535 (the SOF0 segment's 16 bits).  hp, wp = h, w rounded up to the MCU. */
typedef struct rc_jpeg_plan_info {
    long long header_bytes;    /* SOI .. the end of SOS (rc_jpeg_header) */
    long long mcu_cols, mcu_rows;
    long long intervals;       /* ceil(mcu_cols mcu_rows / restart) */
    long long capacity;        /* the default bytes per frame: header_bytes + 3 hp wp (4:4:4) or 3 hp wp / 2 (4:2:0) + 2 intervals + 2 */
    long long scratch_bytes;   /* per frame of the batch: 4 per interval */
} rc_jpeg_plan_info;

/* Host only.  The two 8-bit quantisation tables of `quality` in natural (row-major) order: the Annex K.1 (luma) and K.2 (chroma) tables
 * scaled by the IJG rule, in integers: s = quality < 50 ? 5000 / quality : 200 - 2 quality; entry = clamp((base s + 50) / 100, 1, 255). */
int rc_jpeg_tables(int quality, uint8_t* luma, uint8_t* chroma);
/* Host only.  RC_ERR_INVALID for a description or a size outside the limits above. */
int rc_jpeg_plan(const rc_jpeg_desc* desc, int h, int w, rc_jpeg_plan_info* plan);
/* Host only.  The file's bytes from SOI to the end of SOS into buf[0 .. cap), *len = header_bytes: JFIF APP0 (version 1.01, aspect 1:1,
 * no thumbnail); one DQT with both 8-bit tables (0 luma, 1 chroma) in zigzag order; SOF0 (8 bit, h, w, Y id 1 sampling 2x2 or 1x1 table 0,
 * Cb id 2 and Cr id 3 sampling 1x1 table 1); one DHT with the four Annex K.3.3 tables (DC 0, DC 1, AC 0, AC 1); DRI (restart); SOS. */
int rc_jpeg_header(const rc_jpeg_desc* desc, int h, int w, uint8_t* buf, size_t cap, size_t* len);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w); d_header: rc_jpeg_header(desc, h, w) on the device (the
 * quantiser reads the very tables the decoder will); d_scratch: batch * scratch_bytes, 4-byte aligned, no state between calls; d_dst:
 * batch * capacity bytes, frame b at b * capacity; d_lengths (batch) int64: the bytes each complete file NEEDS, whether or not they fit.
 * Frame b is d_dst[b capacity .. b capacity + lengths[b]) when lengths[b] <= capacity; otherwise its `capacity` bytes are unspecified.
 * Nothing outside a frame's `capacity` bytes is written, whatever the data.  The stream, bit for bit:
 *   1. samples: pixel (y, x) of the padded MCU grid is the crop's pixel (min(y, h-1), min(x, w-1)); r,g,b, Y', Cb, Cr exactly as
 *      rc_yuv_encode forms them for RC_MATRIX_BT601; codes as its RC_RANGE_FULL: Y clamp(rint(255 Y), 0, 255), chroma
 *      clamp(rint(255 c + 128), 0, 255) -- at 4:4:4 per pixel, at 4:2:0 of ((c00 + c01) + (c10 + c11)) 0.25 (RC_SITING_CENTER).  For even
 *      h, w the codes are the planes of rc_yuv_encode's I420 / BT601 / FULL / CENTER surface.
 *   2. DCT per 8x8 block, exact in int32: s = code - 128;  M[u][x] = rint(2^14 a(u) cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2;
 *      R[y][u] = sum_x M[u][x] s[y][x];  R' = (R + 2^8) >> 9 (arithmetic);  F[v][u] = sum_y M[v][y] R'[y][u]: the DCT times 2^19.
 *      |R'| <= 11586, |F| <= 536941584 < 2^30.
 *   3. quantise with the table entry Q of the coefficient: q = sign(F) ((|F| + (Q << 18)) div (Q << 19)).
 *   4. baseline Huffman, the K.3.3 tables; blocks in MCU order, MCUs in raster order; the DC predictor per component, 0 at the start of each
 *      interval; ZRL for every 16 zeros in front of a non-zero coefficient, EOB unless coefficient 63 is non-zero; bits MSB first; each
 *      interval padded with 1-bits to a byte; 0xFF -> 0xFF 0x00; RSTm, m = i mod 8, between intervals i and i + 1; EOI. */
int rc_jpeg_encode(const void* d_src, int src_dtype, const rc_jpeg_desc* desc, const void* d_header, void* d_scratch, void* d_dst, void* d_lengths,
                   int batch, int H, int W, int h, int w, long long capacity, void* stream);
/* Measurement only (tools/jpeg_bench.py times the launches one by one): which of rc_jpeg_encode's three launches run from now on -- bit 0 the
 * counting pass, bit 1 the scan, bit 2 the writing pass.  7, the default, is the only value that gives files; with another value the frames'
 * bytes are unspecified, and still nothing outside them is written. */
int rc_debug_jpeg_passes(int mask);

/* ---- scaled and cropped renditions (ABI 15, additive): a window of the same planar result, downscaled, between the tail and the encoders --
 * One network pass, any number of outputs: each is a window (ROI) of the cropped result, a size and -- through rc_rgb_encode /
 * rc_yuv_encode on what this stage returns -- a format.  The stage is separable and only ever downscales: per axis 1 <= ROI / out <= 8. */
typedef enum rc_resize_filter {
    RC_FILTER_AREA = 0,      /* fractional coverage of the output pixel's footprint (F.interpolate mode="area" at integer ratios) */
    RC_FILTER_BILINEAR = 1   /* the antialiased triangle of F.interpolate(mode="bilinear", antialias=True, align_corners=False) */
} rc_resize_filter;
#define RC_RESIZE_MAX_TAPS 20   /* the longest weight list of an axis (bilinear at ratio 7.5 needs 16) */
#define RC_RESIZE_MAX_RATIO 8

/* HOST function: the tables of ONE axis.  ROI length n at offset off in the source, output length m (m <= n <= 8 m), scale s = n / m.
 * Everything in double, no contraction; for output index i the source indices k (inside the ROI, 0 <= k < n) and raw weights are
 *   AREA      k = floor(i s) .. min(n, ceil((i + 1) s)) - 1;              max(0, min(k + 1, (i + 1) s) - max(k, i s))
 *   BILINEAR  c = s (i + 0.5); k = max(0, int(c - s + 0.5)) .. min(n, int(c + s + 0.5)) - 1;   max(0, 1 - |(k - c + 0.5) / s|)
 * Zero weights at either end are dropped, the rest are summed in list order and divided by that sum (double), then rounded to fp32 once.
 * first[i] = off + the first k kept.  weights: m * RC_RESIZE_MAX_TAPS floats of room; written as [m][*taps], each list padded with zeros
 * to *taps, the axis's longest list.  A list that would exceed RC_RESIZE_MAX_TAPS, m > n (upscaling) or n > 8 m: RC_ERR_INVALID. */
int rc_resize_taps(int filter, int n, int off, int m, int* first, float* weights, int* taps);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar; dst (B,3,h,w) RC_F32, or src_dtype (rounded to nearest even once, at the store).
 * d_first_y / d_wy ([h] / [h][taps_y]) and d_first_x / d_wx ([w] / [w][taps_x]): DEVICE copies of rc_resize_taps' tables, first indices
 * into the source plane.  fp32, every product and every sum rounded on its own, in list order (no fused multiply-add):
 *   t[y][j] = (..((wx[j][0] src[y][fx[j]]) + (wx[j][1] src[y][fx[j] + 1])) + ..)      for each source row y the output needs
 *   o[i][j] = (..((wy[i][0] t[fy[i]][j]) + (wy[i][1] t[fy[i] + 1][j])) + ..)
 * over the weights of a list that are not zero (the padding is skipped, never multiplied).  No clamp, no NaN rule: the weights are
 * non-negative and sum to 1.  One launch; taps_y, taps_x in 1 .. RC_RESIZE_MAX_TAPS; a list's rows must lie within 8 x 8 + 20 source
 * rows of the first row of its tile of 8 output rows (rc_resize_taps' tables do). */
int rc_resize(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, int batch, int H, int W, int h, int w, const int* d_first_y,
              const float* d_wy, int taps_y, const int* d_first_x, const float* d_wx, int taps_x, void* stream);

/* ---- colour looks (ABI 15, additive): the same planar result through a 3D LUT, between the scaler and the encoders ------------------------
 * A look is a table of n x n x n nodes (the .cube format's LUT_3D_SIZE n, unit domain), interpolated tetrahedrally. */
#define RC_LUT3D_MIN_SIZE 2
#define RC_LUT3D_MAX_SIZE 65

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w); dst (B,3,h,w) planar, RC_F32 or src_dtype.
 * d_lut: DEVICE table of n^3 entries of 4 floats -- R, G, B and one pad float that is ignored -- 16-byte aligned, so one vertex is one
 * 16-byte load; node (ir, ig, ib) is entry ir + n (ig + n ib): R varies fastest, the order of a .cube file's rows.  L[.] below is an entry.
 * fp32, every product and every sum rounded on its own (no fused multiply-add):
 *   1. r,g,b = float(src), NaN -> 0, clamped to [0,1]                                          (step 1 of rc_yuv_encode)
 *   2. per channel c:  p = c float(n-1);  i = min(int(floor(p)), n-2);  f = p - float(i)       (exact; c = 1 gives i = n-2, f = 1)
 *   3. the axes ordered by fraction, ties fixed:
 *        fr >= fg:  fg >= fb: (r,g,b);  else fr >= fb: (r,b,g);  else (b,r,g)
 *        else:      fb >= fg: (b,g,r);  else fb >= fr: (g,b,r);  else (g,r,b)
 *      ordered axes a1, a2, a3 with fractions f1 >= f2 >= f3, e_a the unit step along axis a:
 *        V0 = L[i],  V1 = L[i + e_a1],  V2 = L[i + e_a1 + e_a2],  V3 = L[i + (1,1,1)]
 *        w0 = 1 - f1,  w1 = f1 - f2,  w2 = f2 - f3,  w3 = f3
 *   4. per output channel  o = (((w0 V0) + (w1 V1)) + (w2 V2)) + (w3 V3)
 * No output clamp and no NaN rule: the table is finite, the weights lie in [0,1], and the encoders clamp.  o is stored as fp32, or
 * rounded to nearest even once into src_dtype.  Step 2 clamps the indices to [0, n-2] after the NaN rule: no input makes the kernel
 * read outside the table.  One launch.  n outside 2 .. 65, a bad dtype, h > H or w > W: RC_ERR_INVALID before any launch. */
int rc_lut3d(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const float* d_lut, int n, int batch, int H, int W, int h, int w, void* stream);

/* ---- output sharpening (ABI 15, additive): the same planar result with its luma detail amplified, between the look and the encoders --------
 * Replaces: F.conv2d on a luma plane, F.max_pool2d twice for the local range and half a dozen elementwise passes after the network.
 * An unsharp mask on the luma: a 3x3 (radius 1) or 5x5 (radius 2) binomial blur, the difference cored (detail below `core` is left
 * alone, so noise is not sharpened), scaled by `amount`, limited so that the sharpened luma leaves the range of its 3x3 neighbourhood by
 * at most `overshoot`, and added to R, G and B alike.  matrix: RC_MATRIX_* (the luma coefficients of RC_YUV_KR_KB). */
typedef struct rc_sharpen_desc {
    int radius;                 /* 1 or 2 */
    int matrix;                 /* RC_MATRIX_BT601 / BT709 / BT2020 */
    float amount;               /* [0, 8] */
    float core;                 /* [0, 1], in output units */
    float overshoot;            /* [0, 1], in output units */
} rc_sharpen_desc;
size_t rc_sharpen_desc_size(void);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w); dst (B,3,h,w) planar, RC_F32 or src_dtype; dst must not overlap src.
 * The taps of pixel (y, x) of the crop are taken at clamp(y + dy, 0, h-1) and clamp(x + dx, 0, w-1), each axis on its own: nothing outside
 * the crop is ever read (the source's rows and columns beyond (h, w) may hold anything).  X[dy][dx] below is X at such a tap.
 * fp32, every product, sum and difference rounded on its own (no fused multiply-add):
 *   1. r,g,b = float(src), NaN -> 0, clamped to [0,1]                                          (step 1 of rc_yuv_encode)
 *   2. L = ((Kr r) + (Kg g)) + (Kb b)         RC_YUV_KR_KB, Kg = 1 - Kr - Kb in double, each rounded to fp32 once   (rc_yuv_encode's Y)
 *   3. a separable binomial, along the row on L and then down the column on the row sums, in this order of additions:
 *        radius 1:  S = (L[-1] + L[+1]) + (2 L[0]);                                       T = (S[-1] + S[+1]) + (2 S[0]);    blur = T 2^-4
 *        radius 2:  S = (((L[-2] + L[+2]) + (2 L[0])) + (4 L[0])) + (4 (L[-1] + L[+1]));   T the same way on the rows of S;  blur = T 2^-8
 *      (on a constant neighbourhood every partial sum is a power of two times the value: blur == L exactly)
 *   4. d = L - blur;  a = |d|;  c = max(a - core, 0);  d1 = copysign(c, d);  e = amount d1
 *   5. lo, hi = the minimum and maximum of L over the 3x3 taps;
 *      t = L + e;  t = min(t, hi + overshoot);  t = max(t, lo - overshoot);  e2 = t - L
 *   6. per channel c of step 1:  o = min(max(c + e2, 0), 1), stored as fp32, or rounded to nearest even once into src_dtype
 * So a frame whose three planes are each constant, amount = 0 and core = 1 all return step 1's values, and every output is finite and lies
 * in [0,1] whatever the source holds.  One launch, no device state.  Null pointers, a bad dtype, radius or matrix, a non-finite or
 * out-of-range amount / core / overshoot, an empty frame, h > H or w > W, three planes of 2 GiB or more (the offsets inside a frame are
 * 32-bit), dst overlapping src: RC_ERR_INVALID before any launch. */
int rc_sharpen(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const rc_sharpen_desc* desc, int batch, int H, int W, int h, int w, void* stream);

/* ---- local tone mapping (ABI 15, additive): the same planar result with a scene-adaptive gain, between the scaler and the look -------------
 * Replaces: an fp32 copy of the frame, torch.bincount per tile, cumulative sums, eight gathers per pixel and the interpolation passes.
 * Contrast-limited adaptive histogram equalisation (CLAHE) on the 8-bit luma code, applied as ONE gain to R, G and B, so the hue is
 * kept.  A grid of gy x gx tiles; each tile owns a table of 256 gains, and a pixel interpolates bilinearly between the tables of the
 * four nearest tile centres.  Three launches, none keeps device state: rc_tone_hist (the tiles' histograms), rc_tone_gains (histograms
 * -> gain tables; a video caller may smooth the tables over time before the next step) and rc_tone_apply.
 *
 * Tiles follow rc_frame_stats' zones: tile column i is the columns a_i .. a_{i+1} - 1 with a_i = ceil(i w / gx), rows the same way with h
 * and gy.  The grid is 1 .. RC_TONE_MAX_GRID per axis and at most the side, so no tile is empty.
 * fp32 throughout, every product, sum, difference and quotient rounded on its own (no fused multiply-add; divisions correctly rounded):
 *  hist    1. r,g,b = float(src), NaN -> 0, clamped to [0,1]                                          (step 1 of rc_yuv_encode)
 *          2. Y = ((Kr r) + (Kg g)) + (Kb b)     RC_YUV_KR_KB, Kg = 1 - Kr - Kb in double, each rounded to fp32 once  (rc_sharpen's L)
 *          3. q = clamp(rint(Y 255), 0, 255), round half to even
 *          4. hist[tile][q] += 1            (integers: independent of the order of the adds, the same from run to run)
 *  gains   per tile, in 64-bit integers; n = max(sum of h[k], 1): the tile's pixels; clip_q8 = rint(clip 256) in 256 .. 65536
 *          1. limit = max(1, (n clip_q8) >> 16)
 *          2. c[k] = min(h[k], limit)
 *          3. E = n - sum c
 *          4. c[k] += (E >> 8) + ((((k + 1) (E & 255)) >> 8) - ((k (E & 255)) >> 8))       (the excess spread evenly, sum c = n again; one pass)
 *          5. C[k] = sum of c[j] over j <= k
 *          6. T_k = float(C[k]) / float(n), the conversions rounded to nearest even
 *          7. for k >= 1:  y_k = float(k) / 255;  m_k = y_k + strength (T_k - y_k);  G[k] = min(m_k / y_k, max_gain)
 *          8. G[0] = G[1]
 *  axis    rc_tone_axis, per column x (per row y the same way):  s_i = a_i + a_{i+1} (twice the centre of tile i), q = 2 x + 1;
 *          q <= s_0: idx = 0, wt = 0;  q >= s_{g-1}: idx = g - 1, wt = 0;  otherwise idx = the largest i with s_i <= q and
 *          wt = (float)((double)(q - s_i) / (double)(s_{i+1} - s_i))
 *  apply   steps 1 and 2 of hist, then  p = Y 255;  i = min(int(floor(p)), 254);  f = min(p - float(i), 1)
 *          jy = iy[y], v = uy[y], jx = ix[x], u = ux[x];  jy' = min(jy + 1, gy - 1), jx' = min(jx + 1, gx - 1)
 *          for each of the four tiles t = (jy | jy', jx | jx'):  g_t = G_t[i] + f (G_t[i + 1] - G_t[i])
 *          top = g00 + u (g01 - g00);  bot = g10 + u (g11 - g10);  g = top + v (bot - top)
 *          per channel c of step 1:  o = min(c g, 1), stored as fp32, or rounded to nearest even once into src_dtype
 * The form a + t (b - a) interpolates equal nodes exactly.  So strength = 0 (every gain 1) returns step 1's values, and a frame that
 * repeats one tile maps as that tile alone.  No index is formed from a gain; the gains on the device are not checked, and non-finite
 * gains are outside the contract.  The kernel clamps the indices it reads from iy / ix to the grid, so no table can make it read outside
 * the gains. */
#define RC_TONE_MAX_GRID 16       /* tiles per axis */
#define RC_TONE_BINS 256
typedef struct rc_tone_desc {
    int grid[2];                /* gy, gx: 1 .. RC_TONE_MAX_GRID and at most the frame's side */
    int matrix;                 /* RC_MATRIX_BT601 / BT709 / BT2020 */
    int clip_q8;                /* 256 .. 65536: the clip limit in 1/256 of a bin's mean count; 65536 = plain equalisation */
    float strength;             /* [0, 1] */
    float max_gain;             /* [1, 64] */
    int reserved[4];            /* zero */
} rc_tone_desc;
size_t rc_tone_desc_size(void);

/* Host function, no GPU: idx[n] and wt[n] of an axis of n positions and g tiles (the `axis` rules above).  n < 1, g outside
 * 1 .. min(RC_TONE_MAX_GRID, n), a null pointer: RC_ERR_INVALID. */
int rc_tone_axis(int n, int g, int* idx, float* wt);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w) -> d_hist (B,gy,gx,256) int32, zeroed on `stream` by the call
 * itself.  Null pointers, a bad dtype, matrix or grid, clip_q8 / strength / max_gain out of range or not finite, non-zero reserved, an
 * empty frame, h > H or w > W, a source plane of 2^29 samples or more (offsets inside a frame are 32-bit), more than 65535 frames, a
 * misaligned pointer: RC_ERR_INVALID before anything is enqueued.  The same holds for the two entries below. */
int rc_tone_hist(const void* d_src, int src_dtype, const rc_tone_desc* desc, int* d_hist, int batch, int H, int W, int h, int w, void* stream);

/* d_hist (tiles,256) int32 -> d_gains (tiles,256) fp32, tiles = batch gy gx.  One block per tile. */
int rc_tone_gains(const int* d_hist, const rc_tone_desc* desc, float* d_gains, int batch, void* stream);

/* src as rc_tone_hist takes it; d_gains (gains_batch,gy,gx,256) fp32, 16-byte aligned, gains_batch 1 (one set for every frame) or batch;
 * d_iy / d_uy (h) and d_ix / d_ux (w): the device copies of rc_tone_axis(h, gy) and rc_tone_axis(w, gx), 4-byte aligned; dst (B,3,h,w)
 * planar, RC_F32 or src_dtype, must not overlap src. */
int rc_tone_apply(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const rc_tone_desc* desc, const float* d_gains, int gains_batch,
                  const int* d_iy, const float* d_uy, const int* d_ix, const float* d_ux, int batch, int H, int W, int h, int w, void* stream);

/* ---- geometric correction (ABI 15, additive): the same planar result resampled through a coarse mesh, in front of the scaler --------------
 * Replaces: F.grid_sample(result.float(), dense (B, oh, ow, 2) grid, align_corners=True) after the network -- lens distortion correction,
 * a 90 degree orientation, a flip, per-frame stabilisation -- and with it the dense grid in HBM and the fp32 copy of the frame.
 * The mesh holds one source position per `cell` output pixels and is interpolated bilinearly; the source is sampled bilinearly or with
 * the bicubic kernel of A = -0.75 (F.grid_sample(mode="bicubic"), OpenCV INTER_CUBIC). */
typedef enum rc_warp_interp {
    RC_WARP_BILINEAR = 0,
    RC_WARP_BICUBIC = 1
} rc_warp_interp;
typedef enum rc_warp_border {
    RC_WARP_CLAMP = 0,       /* a tap outside the frame reads the nearest pixel of the frame (grid_sample padding_mode="border") */
    RC_WARP_CONSTANT = 1     /* a tap outside the frame is fill[channel] (padding_mode="zeros" when the fill is 0) */
} rc_warp_border;
#define RC_WARP_MIN_CELL_LOG2 3   /* cell = 8, 16, 32 or 64 output pixels */
#define RC_WARP_MAX_CELL_LOG2 6
#define RC_WARP_MAX_DIM 8388608   /* h, w, oh, ow <= 2^23: every coordinate and w + 1, h + 1 are exact in fp32 */

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar, cropped to the frame (h,w); dst (B,3,oh,ow) planar, RC_F32 or src_dtype; oh, ow >= 1
 * are free (upscaling is allowed).  cell = 1 << cell_log2.
 * d_mesh: DEVICE fp32, 8-byte aligned, mesh_batch (1: shared by every frame, or batch: one per frame) meshes of Gh x Gw nodes of two
 * floats, Gh = ceil(oh / cell) + 1, Gw = ceil(ow / cell) + 1, row-major; node (j, i) = (sx, sy) is the source position, in pixels of the
 * frame with an integer at a pixel's centre, that output pixel (x, y) = (i cell, j cell) samples.  Nodes need not be finite (step 2).
 * fp32, every product, sum and difference rounded on its own (no fused multiply-add); for output pixel (x, y), per frame:
 *   1. i = x >> cell_log2, u = float(x & (cell-1)) (1/cell);  j = y >> cell_log2, v = float(y & (cell-1)) (1/cell)       (all exact)
 *      per component (sx, then sy) with m00 = node(j,i), m10 = node(j,i+1), m01 = node(j+1,i), m11 = node(j+1,i+1):
 *        top = ((1-u) m00) + (u m10);  bot = ((1-u) m01) + (u m11);  s = ((1-v) top) + (v bot)
 *   2. guard: NaN -> -2; then sx = min(max(sx, -2), float(w+1)), sy = min(max(sy, -2), float(h+1)).  Every tap index below is also
 *      clamped into the frame or tested against it: no mesh -- NaN, +-inf, 1e30 -- makes the kernel read outside its buffer.
 *   3. x0 = int(floor(sx)), tx = sx - float(x0);  y0 = int(floor(sy)), ty = sy - float(y0)                               (exact)
 *   4. taps, per axis with t = tx or ty:
 *        BILINEAR  offsets 0, 1      weights 1-t, t
 *        BICUBIC   offsets -1, 0, 1, 2   weights c2(t+1), c1(t), c1(1-t), c2(2-t)
 *                  c1(x) = (((1.25 x) - 2.25) x) x + 1;   c2(x) = ((((-0.75 x) + 3.75) x) - 6) x + 3      (exactly 0, 1, 0, 0 at t = 0)
 *      a tap whose column x0 + offset lies outside [0, w) or whose row lies outside [0, h) reads the pixel at the index clamped into the
 *      frame (CLAMP) or is fill[channel] (CONSTANT); 16-bit samples are widened exactly.
 *   5. per tap row k:  r_k = (..((wx_0 s_k0) + (wx_1 s_k1)) + ..) in offset order;  o = (..((wy_0 r_0) + (wy_1 r_1)) + ..)
 * No output clamp and no NaN rule for samples (the look and the encoders have theirs).  o is stored as fp32, or rounded to nearest even
 * once into src_dtype.  An identity mesh returns the frame exactly (up to the sign of a zero).  One launch.
 * A bad dtype, interp, border or cell, mesh_batch other than 1 or batch, a non-finite fill, h > H, w > W, a dimension above
 * RC_WARP_MAX_DIM, a source plane of 2^29 samples or more, a null or misaligned pointer: RC_ERR_INVALID before any launch. */
int rc_warp(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const float* d_mesh, int mesh_batch, int cell_log2, int interp,
            int border, float fill_r, float fill_g, float fill_b, int batch, int H, int W, int h, int w, int oh, int ow, void* stream);

/* ---- frame statistics (ABI 15, additive): histograms and a 3A zone grid of the same planar result, the one stage that is a reduction ------
 * Replaces: y.float().clamp(0, 1).mul(255).round(), torch.bincount per channel and a pooling pass per sum -- an fp32 copy of the frame
 * and several passes over it.  What auto-exposure, auto white balance, autofocus, a scope and a scene-change detector read. */
#define RC_STATS_MAX_GRID 64      /* zones per axis */
#define RC_STATS_SLOTS 8          /* numbers per zone */
typedef struct rc_stats_desc {
    int roi[4];            /* y0, x0, rh, rw: the window of the crop (h,w) that is measured; rh = rw = 0: the whole crop */
    int grid[2];           /* gy, gx: zones per axis, 1 .. min(64, rh) and 1 .. min(64, rw) */
    int bits;              /* 8 or 10: codes 0 .. S, S = 2^bits - 1 */
    int matrix;            /* rc_yuv_matrix: the luma coefficients */
    int dark;              /* -1 .. S: a pixel that is not clipped is dark if qY <= dark; -1: nothing is dark */
    int clip;              /* 1 .. 2^bits: a pixel is clipped if max(qR, qG, qB) >= clip; 2^bits: nothing clips */
    int reserved[4];       /* zero */
} rc_stats_desc;
size_t rc_stats_desc_size(void);

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w); the ROI (y0, x0, rh, rw) lies inside the crop; pixel (x, y) below
 * is ROI-relative.  d_hist (B, 4, 2^bits) and d_zones (B, gy, gx, 8), both int64, 8-byte aligned.  Per frame:
 *   1. r,g,b = float(src), NaN -> 0, clamped to [0,1]                                                   (step 1 of rc_yuv_encode)
 *   2. Y = ((Kr r) + (Kg g)) + (Kb b) in fp32, every product and every sum rounded on its own (no fused multiply-add); Kr, Kb from
 *      RC_YUV_KR_KB, Kg = 1 - Kr - Kb in double, each rounded to fp32 once                               (rc_yuv_encode's Y)
 *   3. codes q(v) = clamp(rint(v S), 0, S), round half to even: integers qR, qG, qB, qY.
 *      At 8 bits qR, qG, qB are rc_rgb_encode(.., 8)'s bytes and qY is the Y plane of a full-range NV12 surface of the same matrix; at 10
 *      bits qY is full-range P010's Y code, sample >> 6.
 *   4. hist[c][k] = the number of ROI pixels whose code in channel c (R, G, B, Y) is k.
 *   5. pixel (x, y) belongs to zone (floor(y gy / rh), floor(x gx / rw)): zone column i is the columns ceil(i rw / gx) ..
 *      ceil((i+1) rw / gx) - 1, never empty; rows alike.
 *   6. a pixel is clipped if max(qR,qG,qB) >= clip; otherwise dark if qY <= dark; otherwise valid.
 *   7. focus f = dx^2 + dy^2, dx = qY[y][min(x+1, rw-1)] - qY[y][x], dy = qY[min(y+1, rh-1)][x] - qY[y][x]: the neighbour is clamped to the
 *      ROI, not to the crop or the plane.
 *   8. zones[j][i][0..7] = count of valid pixels; sum of qR, of qG, of qB over valid pixels; sum of qY over all pixels of the zone; count of
 *      clipped pixels; count of dark pixels; sum of f over all pixels of the zone.
 * Everything after step 3 is integer arithmetic: the result does not depend on the order of summation, so it is bit-exact and the same
 * from run to run although it is accumulated with atomics.  A plane holds fewer than 2^29 samples and f <= 2 * 1023^2, so every total
 * stays below 2^51.
 * Every element of both outputs is written: the entry point zeroes them on `stream` itself (the caller does not), then one launch adds.
 * It keeps no device buffer of its own and is capturable; a graph replay starts from zero again.
 * Null pointers, a bad dtype, bits or matrix, an ROI outside the crop or with one zero side only, a grid outside 1 .. min(64, side),
 * thresholds out of range, non-zero reserved, h > H or w > W, outputs not 8-byte aligned, a misaligned source, a plane of 2^29 samples or
 * more: RC_ERR_INVALID before any launch. */
int rc_frame_stats(const void* d_src, int src_dtype, const rc_stats_desc* desc, long long* d_hist, long long* d_zones,
                   int batch, int H, int W, int h, int w, void* stream);

/* ---- motion estimation (ABI 15, additive): hierarchical block matching on the luma code of the same planar result -----------------------
 * Replaces: copying frames to the host, or per candidate a shifted abs difference and a pooling pass in torch, each reading the frame
 * again.  What rc_warp's per-frame mesh (stabilisation), a scene-cut detector, a motion mask and an encoder hint read.  Two entries: the
 * luma pyramid of a frame (one launch) and the full search of one pyramid level of two frames (one launch per level).  Stateless and
 * capturable; no device buffer of their own. */
#define RC_MOTION_MAX_LEVELS 4
#define RC_MOTION_MAX_RANGE 8

/* src (B,3,H,W) RC_F32 / RC_BF16 / RC_F16 planar R,G,B, cropped to (h,w).  d_levels: a HOST array of `levels` (1 .. 4) device pointers;
 * level k is (B, h >> k, w >> k) uint8, contiguous; h >> (levels-1) and w >> (levels-1) must be >= 1.
 *   level 0      qY of rc_frame_stats steps 1 - 3 at bits = 8, exactly: NaN -> 0, clamp to [0,1], Y = ((Kr r) + (Kg g)) + (Kb b) with every
 *                product and sum rounded on its own, clamp(rint(255 Y), 0, 255) with half to even (the Y plane of a full-range NV12
 *                surface of the same matrix).
 *   level k+1    pixel (x, y) = (a + b + c + d + 2) >> 2 over level k's pixels (2x .. 2x+1, 2y .. 2y+1), which always exist
 *                (2 (n >> 1) <= n); a trailing odd row or column of level k feeds nothing.
 * One launch reads every source sample once and writes every element of every level.
 * Null pointers (a level's included), a bad dtype or matrix, levels outside 1 .. 4, an empty coarsest level, h > H or w > W, a misaligned
 * source, a source plane of 2^29 samples or more, more than 65535 frames: RC_ERR_INVALID before any launch. */
int rc_motion_pyramid(const void* d_src, int src_dtype, int matrix, int levels, void* const* d_levels, int batch, int H, int W, int h, int w,
                      void* stream);

typedef struct rc_motion_desc {
    int block;             /* 8, 16 or 32: a matching block is block x block pixels */
    int range;             /* R, 0 .. 8: offsets -R .. R per axis around the predictor */
    int pred_shift;        /* s, 0 or 1: the predictor grid is of the same level (0) or of the next coarser one (1) */
    int reserved[5];       /* zero */
} rc_motion_desc;
size_t rc_motion_desc_size(void);

/* cur, ref (B,hs,ws) uint8, contiguous: one pyramid level of two frames.  by = hs / block, bx = ws / block (floored, both >= 1); block
 * (j, i) covers rows j block .. and columns i block ..; pixels right of or under the last whole block belong to no block.
 * d_out (B,by,bx,4) int32, 16-byte aligned.  d_pred: null (the predictor is 0), or (B,pred_by,pred_bx,4) int32, 16-byte aligned -- a
 * coarser (s = 1) or equal (s = 0) level's output.  Per block, all in integers:
 *   1. predictor  (px, py) = slots 0 and 1 of node (min(j >> s, pred_by-1), min(i >> s, pred_bx-1)), each clamped to [-32768, 32767], then
 *                 shifted left by s.  Device data is never trusted.
 *   2. cost       for every offset (ox, oy) in [-R, R]^2, dx = px + ox, dy = py + oy:
 *                 cost = sum over the block's pixels (x, y) of |cur[y][x] - ref[clamp(y+dy, 0, hs-1)][clamp(x+dx, 0, ws-1)]|.
 *                 Every index is clamped: no predictor makes the kernel read outside its buffers.  cost <= 32 * 32 * 255 = 261120.
 *   3. winner     the offset with the lexicographically smallest key (cost, |oy| + |ox|, oy, ox): a flat frame returns its predictor.
 *   4. texture    sum of |c[y][x] - c[y][x+1]| over the block's horizontal neighbour pairs plus sum of |c[y][x] - c[y+1][x]| over its
 *                 vertical pairs, c = cur; both pixels of a pair lie inside the block.
 *   5. out        (dx, dy, cost, texture) of the winner.
 * Integer arithmetic throughout: the order of summation is free, the result bit-exact and the same from run to run.  Every element of
 * d_out is written.  One launch.
 * Null or misaligned pointers, a bad block, range or pred_shift, non-zero reserved, by or bx < 1, pred_by or pred_bx < 1 with a predictor,
 * hs ws >= 2^29, more than 65535 frames: RC_ERR_INVALID before any launch. */
int rc_motion_search(const uint8_t* d_cur, const uint8_t* d_ref, const rc_motion_desc* desc, const int* d_pred, int pred_by, int pred_bx,
                     int* d_out, int batch, int hs, int ws, void* stream);

/* ---- defective-pixel correction (ABI 15, additive): the first box of the input side, on the mosaic itself, before the ingest ------------
 * Replaces: unpacking the RAW10 / RAW12 lines into a tensor, eight shifted fp32 planes, masked min / max / direction selects -- a dozen
 * full-frame passes.  Here one launch over the bytes the ingest reads anyway; the one stage that is a stencil. */
#define RC_DEFECT_HOT 1           /* rc_defect_desc.flags: the dynamic hot test is on */
#define RC_DEFECT_COLD 2          /* ... the dynamic cold test is on */
typedef struct rc_defect_desc {
    int flags;             /* RC_DEFECT_HOT | RC_DEFECT_COLD, or 0 (then d_map is required: something must be enabled) */
    float hot_abs, hot_rel;    /* t = hot_abs + hot_rel max(hi - black, 0); both finite and >= 0; in the storage's own units, as the levels */
    float cold_abs, cold_rel;  /* t = cold_abs + cold_rel max(lo - black, 0) */
    int reserved[3];       /* zero */
} rc_defect_desc;
size_t rc_defect_desc_size(void);

/* src: the mosaic (B, 2h, 2w) as rc_raw_ingest_fmt reads it (fmt: storage, cfa, line_bytes, width, black; white is not looked
 * at).  d_map: NULL (no static map) or the defect bitmap, one bit per mosaic sample: sample (y, x) is bit x & 31 of dword
 * x >> 5 of row y, rows map_pitch_bytes apart (a multiple of 4, >= 4 ceil(2w / 32)); one map serves every frame of the batch.
 * d_dst (B, 2h, 2w), rows dst_pitch_bytes apart (0: dense), frames 2h rows apart: uint16 for RC_RAW_U16 / U8 / MIPI10 / MIPI12, the source
 * type for RC_RAW_F32 / BF16 / F16; unpacked.  d_counts: NULL or (B, 3) int64: samples replaced from the map, as hot, as cold.
 *
 * v(y,x) is the decoded sample as fp32 (counts are exact).  pos = 2 (y & 1) + (x & 1); black[pos] is fmt->black[pos].  The ring of (y,x)
 * is the eight positions (y + 2dy, x + 2dx), (dy,dx) in {-1,0,1}^2 \ (0,0): the nearest samples of the same colour.  A ring position is
 * GOOD if it lies inside the frame and is not set in the map.  Every product and every sum is rounded on its own (no fused multiply-add).
 *   1. a sample set in the map: the pairs, in the order H (x-2, x+2), V (y-2, y+2), D1 ((y-2,x-2), (y+2,x+2)), D2 ((y-2,x+2), (y+2,x-2));
 *      among the pairs with both ends good the one with the smallest |a - b| (a tie: the first in that order): out = (a + b) 0.5.
 *      No whole pair: out = the first good neighbour in the order W, E, N, S, NW, NE, SW, SE.  No good neighbour: out = v, not counted.
 *   2. a sample not set in the map with at least one good ring neighbour; hi = max, lo = min over the good ring:
 *      hot, if enabled:             t = hot_abs + hot_rel max(hi - black[pos], 0);   v - hi > t: out = hi, counted as hot;
 *      otherwise cold, if enabled:  t = cold_abs + cold_rel max(lo - black[pos], 0); lo - v > t: out = lo, counted as cold;
 *      otherwise out = v.  No good neighbour: out = v.
 *   3. count storages store rint(out), half to even, as uint16 (only step 1's .5 can round); float storages store out rounded to nearest
 *      even to the source type.  A sample that is not replaced keeps its exact value.
 * Single pass: neighbours are always source samples, never corrected ones, so the result does not depend on the traversal order and is the
 * same from run to run; the counts are integer atomics.  Frames holding NaN / Inf are outside this contract (no fault, any value).
 * d_counts, when given, is zeroed on `stream` by the entry point itself, then one launch adds: capturable, and a graph replay starts from
 * zero.  The library keeps no device buffer of its own.
 * Null d_src / fmt / desc / d_dst, an unknown storage or cfa, line_bytes shorter than a row or no multiple of the sample size, fmt->width
 * other than 0 or 2w, a RAW10 width not divisible by 4, a source misaligned for its sample (MIPI: 4 bytes), a map pitch that is too small
 * or no multiple of 4 or a map not 4-byte aligned, a dst pitch shorter than a row or no multiple of the sample size, dst misaligned,
 * d_counts not 8-byte aligned, a threshold that is negative or not finite, unknown flags, non-zero reserved (fmt's too), nothing enabled
 * (flags == 0 and no map), more than 65535 frames: RC_ERR_INVALID before anything is enqueued. */
int rc_raw_defects(const void* d_src, const rc_raw_format* fmt, const rc_defect_desc* desc, const void* d_map, int map_pitch_bytes,
                   void* d_dst, int dst_pitch_bytes, long long* d_counts, int batch, int h, int w, void* stream);

/* ---- sensor calibration (ABI 15, additive): linearisation, levels, flat-field gain map, white-balance gains, clip -- the second box of
 * the input side, between the repaired samples and the ingest.
 * Replaces: unpacking the lines into an fp32 tensor, bucketize + gather for the knee curve, F.interpolate of the gain map per CFA
 * position, and a multiply per step -- several full-frame fp32 passes.  Here one launch over the bytes as delivered. */
#define RC_CALIB_GAINS 1          /* rc_calib_desc.flags: gains[] holds the four gains */
#define RC_CALIB_CLIP 2           /* ... clip_lo / clip_hi are applied */
#define RC_CALIB_MAX_KNOTS 16
typedef struct rc_calib_desc {
    int flags;             /* RC_CALIB_GAINS | RC_CALIB_CLIP, or 0 */
    int knots;             /* K: 0 (no curve) or 2 .. 16 */
    int cell;              /* 0 (no gain map) or 8, 16, 32, 64, 128: a node every `cell` samples of a position's own h x w plane */
    float curve_x[RC_CALIB_MAX_KNOTS];   /* strictly increasing, in the storage's own units */
    float curve_y[RC_CALIB_MAX_KNOTS];   /* non-decreasing, in linear units: with a curve, fmt->black / white are in these units */
    float gains[4];        /* CFA-position order, finite and >= 0 (RC_CALIB_GAINS) */
    float clip_lo, clip_hi;    /* finite, lo < hi (RC_CALIB_CLIP) */
    int reserved[3];       /* zero */
} rc_calib_desc;
size_t rc_calib_desc_size(void);

/* src: the mosaic (B, 2h, 2w) as rc_raw_defects reads it (fmt: storage, cfa, line_bytes, width, black, white).  d_gain_map: NULL, or
 * (4, Gh, Gw) fp32, dense, one plane per CFA position (0,0), (0,1), (1,0), (1,1), Gh = ceil(h / cell) + 1, Gw = ceil(w / cell) + 1; one map
 * serves every frame.  d_frame_gains: NULL, or (frame_gains_batch, 4) fp32 on the device, frame_gains_batch = 1 (one row for every frame)
 * or batch (one row per frame), read by the kernel when it runs: a loop that rewrites them needs no host sync, and a captured graph sees
 * the new values on replay.  d_dst (B, 2h, 2w) of dst_dtype RC_F32 / RC_BF16 / RC_F16, rows dst_pitch_bytes apart (0: dense), frames 2h rows
 * apart; unpacked.
 *
 * c is the decoded sample as fp32 (counts are exact).  pos = 2 (y & 1) + (x & 1); (Y, X) = (y >> 1, x >> 1); k = log2(cell).  Every product
 * and every sum is rounded on its own (no fused multiply-add).  A step that is not enabled is skipped; step 2 always runs.
 *   1. curve    j = the largest index <= K - 2 with x_j <= c, or 0 if c < x_0;  l = y_j + (c - x_j) s_j, where
 *               s_j = (y_{j+1} - y_j) / (x_{j+1} - x_j) is formed in double on the host and rounded to fp32 once.  The end segments
 *               extrapolate.  No curve: l = c.
 *   2. levels   n = (l - black[pos]) inv[pos], inv[pos] = 1.f / (white - black[pos]) in fp32 on the host: rc_raw_ingest_fmt's own.
 *   3. shading  j0 = Y >> k, i0 = X >> k; fy = (Y & (cell - 1)) 2^-k, fx = (X & (cell - 1)) 2^-k (exact); with g00, g01, g10, g11 the
 *               nodes (j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1) of plane pos:
 *               top = g00 + fx (g01 - g00);  bot = g10 + fx (g11 - g10);  g = top + fy (bot - top);  m = n g.
 *               top and bot depend on the column and the node row only.  A constant map multiplies by exactly that constant.
 *   4. gains    m = m wb[pos]: desc->gains, or row (frame_gains_batch == 1 ? 0 : frame) of d_frame_gains.
 *   5. clip     m = min(max(m, clip_lo), clip_hi).
 *   6. store    round to nearest even into dst_dtype.
 * Frames holding NaN / Inf are outside this contract (no fault, any value).  One launch, capturable; the library keeps no device buffer.
 * Null d_src / fmt / desc / d_dst, an unknown storage, cfa or dst dtype, line_bytes shorter than a row or no multiple of the sample size,
 * fmt->width other than 0 or 2w, a RAW10 width not divisible by 4, a source misaligned for its sample (MIPI: 4 bytes), a dst pitch shorter
 * than a row or no multiple of the sample size, dst misaligned, a frame of 2 GiB or more (rows x pitch, either side), white <= a black level,
 * a knot count other than 0 or 2 .. 16, knots out of order or not finite, a cell other than 0, 8 .. 128, a gain map pointer without a cell
 * or a cell without a pointer, frame_gains_batch other than 1 or batch (0 without d_frame_gains), gains given both ways, a gain that is
 * negative or not finite, clip_lo >= clip_hi or not finite, unknown flags, non-zero reserved (fmt's too), nothing enabled (no curve, map,
 * gains or clip), more than 65535 frames: RC_ERR_INVALID before anything is enqueued. */
int rc_raw_calibrate(const void* d_src, const rc_raw_format* fmt, const rc_calib_desc* desc, const float* d_gain_map, const float* d_frame_gains,
                     int frame_gains_batch, void* d_dst, int dst_dtype, int dst_pitch_bytes, int batch, int h, int w, void* stream);

/* ---- multi-exposure HDR merge (ABI 15, additive): E = 2 .. 4 exposures of one scene -> one linear mosaic, between the defects stage (run per
 * exposure) and the calibration.
 * Replaces: a float copy of every exposure (the packed lines unpacked first), and a dozen elementwise passes over the E frames -- weights,
 * masks, the sums and the quotient.  Here one launch over the bytes as delivered. */
#define RC_HDR_MOTION 1           /* rc_hdr_desc.flags: motion_abs / motion_rel cut a longer exposure that disagrees with the shortest */
typedef struct rc_hdr_desc {
    int exposures;                 /* E, 2 .. 4 */
    int flags;                     /* RC_HDR_MOTION, or 0 */
    float times[4];                /* t_0 < t_1 < ..: exposure times or ratios (only their quotients matter), finite and positive; not looked
                                      at when d_times is given */
    float knee_lo, knee_hi;        /* finite, lo < hi, in the storage's own units (codes) */
    float motion_abs, motion_rel;  /* finite and >= 0 (RC_HDR_MOTION) */
    long long exposure_stride_bytes;   /* bytes from row r of exposure e to row r of exposure e + 1; 0: 2h line_bytes (whole frames, dense) */
    long long frame_stride_bytes;      /* bytes from one frame of the batch (all its exposures) to the next; 0: E 2h line_bytes */
    int reserved[4];               /* zero */
} rc_hdr_desc;
size_t rc_hdr_desc_size(void);

/* src: B frames of E exposures of a mosaic (2h, 2w) as rc_raw_calibrate reads one (fmt: storage, cfa, line_bytes, width, black; white is not
 * looked at).  Row r of exposure e of frame f starts at d_src + f frame_stride_bytes + e exposure_stride_bytes + r line_bytes, where
 * fmt->line_bytes (0: one dense row) is the stride between rows of ONE exposure: whole frames (B, E, 2h, X) are the defaults above;
 * line-interleaved readout (B, E 2h, X), row r of exposure e at tensor row r E + e, is line_bytes = E X, exposure_stride_bytes = X.
 * Exposure 0 is the shortest.  d_times: NULL (desc->times), or (times_batch, E) fp32 on the device, times_batch = 1 (one row for every frame)
 * or batch, read by the kernel when it runs: a loop that rewrites them needs no host sync, and a captured graph sees the new values on
 * replay; device values are not checked (a value <= 0 or rows out of order: any result, no fault).  d_dst (B, 2h, 2w) fp32, rows
 * dst_pitch_bytes apart (0: dense), frames 2h rows apart.
 *
 * c_e is the decoded sample of exposure e as fp32 (counts are exact), at (y, x); pos = 2 (y & 1) + (x & 1); b = black[pos].  Every product,
 * every sum and every quotient is rounded to fp32 on its own (no fused multiply-add; both divisions correctly rounded).
 *   1. linear   d_e = c_e - b;  l_e = d_e q_e,  q_e = t_0 / t_e (one fp32 division: on the host for desc->times, in the kernel per frame for
 *               d_times -- the same bits).  l_e is in exposure 0's units.
 *   2. knee     u_0 = 1.  e >= 1: u_e = 1 if c_e <= knee_lo, 0 if c_e >= knee_hi, otherwise (knee_hi - c_e) ik,
 *               ik = (float)(1.0 / ((double)knee_hi - (double)knee_lo)) on the host.
 *   3. motion   (RC_HDR_MOTION) e >= 1: u_e = 0 where |l_e - l_0| > motion_abs + motion_rel |l_0|.
 *   4. sums     w_e = u_e t_e;  num = w_0 l_0, den = w_0;  then for e = 1 .. E - 1 in this order: num = num + w_e l_e, den = den + w_e.
 *   5. result   m = b + num / den  (den >= t_0 > 0).
 * m is in exposure 0's code units: fmt->black / white mean for it what they meant for exposure 0, and the range the longer exposures add
 * shows as fractional codes.  Non-finite samples of a float storage are outside this contract (no fault, any value).  One launch, capturable;
 * the library keeps no device buffer.
 * Null d_src / fmt / desc / d_dst, an unknown storage or cfa, line_bytes shorter than a row or no multiple of the sample size, fmt->width
 * other than 0 or 2w, a RAW10 width not divisible by 4, a source misaligned for its sample (MIPI: 4 bytes), a black level that is not finite,
 * E outside 2 .. 4, unknown flags, non-zero reserved (fmt's too), times_batch other than 1 or batch (0 without d_times), d_times not 4-byte
 * aligned, host times that are not finite, positive and strictly increasing, knee_lo >= knee_hi or not finite, a motion threshold that is
 * negative or not finite, a stride that is negative or no multiple of 4 bytes (MIPI) / of the sample size, a dst pitch shorter than a row or
 * no multiple of 4, dst misaligned, a frame whose extent over all its exposures (or whose destination) reaches 2 GiB, more than 65535
 * frames: RC_ERR_INVALID before anything is enqueued. */
int rc_raw_hdr_merge(const void* d_src, const rc_raw_format* fmt, const rc_hdr_desc* desc, const float* d_times, int times_batch,
                     void* d_dst, int dst_pitch_bytes, int batch, int h, int w, void* stream);

/* ---- temporal noise reduction (ABI 15, additive): a motion-adaptive recursive filter on the mosaic, between the repair / merge and the
 * calibration, where the samples are linear sensor codes and the noise depends on the level alone.
 * Replaces: fp32 copies of the frame and the state (the packed lines unpacked first), padded shifts for the nine taps, and a dozen
 * elementwise passes -- difference, activity, noise level, ratio, weight, blend.  Here one launch over the bytes as delivered. */
#define RC_TNR_RESET 1            /* rc_temporal_desc.flags: no state yet (or a scene cut): the result is the decoded frame */
#define RC_TNR_GAIN 2             /* rc_temporal_desc.flags: desc->gain scales the state about the black level */
typedef struct rc_temporal_desc {
    int flags;                     /* RC_TNR_RESET | RC_TNR_GAIN, or 0 */
    float noise_abs, noise_rel;    /* the noise level of a sample is noise_abs + noise_rel max(p - black, 0), in the storage's own units
                                      (codes): noise_abs finite and > 0, noise_rel finite and >= 0 */
    float alpha;                   /* in (0, 1]: the weight of the new frame where nothing moves */
    float ramp;                    /* finite and > 1: at an activity of ramp noise levels the new frame passes unchanged */
    float gain;                    /* RC_TNR_GAIN: this frame's exposure over the state's, finite and > 0 */
    int reserved[4];               /* zero */
} rc_temporal_desc;
size_t rc_temporal_desc_size(void);

/* src: B frames of a mosaic (2h, 2w) as rc_raw_calibrate reads them (fmt: storage, cfa, line_bytes, width, black; white is not looked at).
 * d_prev: the state, the last result (B, 2h, 2w) fp32, rows prev_pitch_bytes apart (0: dense), frames 2h rows apart; NULL with RC_TNR_RESET
 * (then it is not read).  d_gain: NULL, or (gain_batch) fp32 on the device, gain_batch = 1 (one value for every frame) or batch, read by the
 * kernel when it runs: an AE loop that rewrites it needs no host sync, and a captured graph sees the new value on replay; device values are
 * not checked (a value <= 0 or not finite: any result, no fault).  d_dst (B, 2h, 2w) fp32, rows dst_pitch_bytes apart (0: dense), frames 2h
 * rows apart; it must not overlap d_prev.  The B frames are B independent streams.
 *
 * c is the decoded sample as fp32 (counts are exact) and s the state's sample, at (y, x); pos = 2 (y & 1) + (x & 1); b = black[pos].  Every
 * product, every sum and every quotient is rounded to fp32 on its own (no fused multiply-add; the division correctly rounded).
 *   0. reset     (RC_TNR_RESET) out = c.  Nothing else is read.
 *   1. previous  p = s; with a gain g (desc->gain, or d_gain[gain_batch == 1 ? 0 : frame]): p = b + (s - b) g.
 *   2. diff      d = c - p, e = |d|, at every sample of the frame.
 *   3. activity  the taps (dy, dx) in the order (-2,-2), (-2,0), (-2,2), (0,-2), (0,0), (0,2), (2,-2), (2,0), (2,2): the same-colour 3x3
 *                neighbourhood.  A tap whose row y + dy is outside [0, 2h) takes row y; one whose column x + dx is outside [0, 2w) takes
 *                column x; each axis on its own.  A = the first tap's e, the others added one by one in this order; a = A (float)(1.0 / 9.0).
 *   4. noise     t = noise_abs + noise_rel max(p - b, 0)  (> 0).
 *   5. ratio     u = a / t.
 *   6. weight    u <= 1: k = alpha.  u >= ramp: out = c exactly, step 7 is skipped.  Otherwise k = alpha + (u - 1) slope,
 *                slope = (float)((1.0 - (double)alpha) / ((double)ramp - 1.0)) on the host.
 *   7. result    out = p + k d.
 * Hence, exactly: a reset returns c; a frame equal to its state (no gain) returns c; a frame that differs from its state by more than
 * ramp t everywhere returns c.  Non-finite samples or state are outside this contract (no fault, any value); no index is formed from a
 * value.  One launch, capturable; the library keeps no device buffer: the caller owns the state and swaps it with the result.
 * Null d_src / fmt / desc / d_dst, an unknown storage or cfa, line_bytes shorter than a row or no multiple of the sample size, fmt->width
 * other than 0 or 2w, a RAW10 width not divisible by 4, a source misaligned for its sample (MIPI: 4 bytes), a black level that is not finite,
 * a null d_prev without RC_TNR_RESET, d_dst overlapping d_prev, a prev or dst pitch shorter than a row or no multiple of 4, prev / dst /
 * d_gain not 4-byte aligned, a frame of 2 GiB or more (rows x pitch: source, state or destination), gain_batch other than 1 or batch (0
 * without d_gain), a gain given both ways (RC_TNR_GAIN and d_gain), noise_abs <= 0, noise_rel < 0, alpha outside (0, 1], ramp <= 1, a host
 * gain <= 0, any of them not finite, unknown flags, non-zero reserved (fmt's too), more than 65535 frames: RC_ERR_INVALID before anything is
 * enqueued. */
int rc_raw_temporal(const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                    const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w, void* stream);

/* ---- motion-compensated temporal noise reduction (ABI 15, additive): rc_raw_temporal against the state displaced by block vectors, and
 * the 8-bit luma proxy of a mosaic that rc_motion_search finds those vectors on.  On a pan every textured sample of rc_raw_temporal "moves"
 * and the frame passes unfiltered; with the state moved by its block's vector first, the filter works as on a static scene.
 * Replaces: a demosaic or an fp32 binning pass, a normalisation and a quantisation in torch to get a plane the matcher can read, and, for the
 * filter, an index gather of the whole state into an aligned copy (8 bytes per sample on top of a u16 frame's 10) in front of
 * rc_raw_temporal.  Here one launch for every level of a frame's pyramid and one launch for the filter; rc_motion_search is unchanged and
 * its vectors are in Bayer cells.  Stateless and capturable; no device buffer of their own.
 *
 * rc_raw_motion_pyramid.  src: B frames of a mosaic (2h, 2w) as rc_raw_temporal reads them (fmt: storage, cfa, line_bytes, width, black,
 * white); the fp32 state of the filter is the RC_RAW_F32 storage.  d_levels: a HOST array of `levels` (1 .. 4) device pointers; level k is
 * (B, h >> k, w >> k) uint8, contiguous: level 0 holds one code per Bayer cell.  c is the decoded sample as fp32; every product and every
 * sum is rounded to fp32 on its own.
 *   level 0      cell (cy, cx): d_pos = c[2cy + (pos >> 1)][2cx + (pos & 1)] - black[pos] for pos = 0 .. 3;  m = ((d0 + d1) + (d2 + d3)) 0.25;
 *                t = m inv, inv = (float)(1.0 / ((double)white - ((double)b0 + b1 + b2 + b3) / 4)) formed on the host;  with a gain g
 *                (`gain` when it is not 1, else d_gain[gain_batch == 1 ? 0 : frame]) t = t g;  NaN -> 0, clamp to [0, 1];
 *                q = (int)rint(65025 t), half to even;  code = floor(sqrt(q)) as an exact integer in 0 .. 255: r = (int)sqrtf((float)q), then
 *                r - 1 where r r > q, r + 1 where (r + 1)(r + 1) <= q, so no rounding of the float square root matters.  The square root is
 *                deliberate: linear sensor codes put the shadows into a handful of 8-bit levels, and it makes shot noise roughly uniform
 *                over the range.
 *   level k+1    pixel (x, y) = (a + b + c + d + 2) >> 2 over level k's pixels (2x .. 2x+1, 2y .. 2y+1): rc_motion_pyramid's rule; a trailing
 *                odd row or column of level k feeds nothing.
 * One launch reads every sample once and writes every element of every level.  The gain is what rc_raw_temporal applies to its state: the
 * proxy of a state taken with gain g matches the proxy of the frame across an exposure step (the black level is not re-added: the proxy
 * has none).  Device gain values are not checked (any code, no fault).
 * Null d_src / fmt / d_levels or a null level pointer, an unknown storage or cfa, line_bytes shorter than a row or no multiple of the sample
 * size, fmt->width other than 0 or 2w, a RAW10 width not divisible by 4, a source misaligned for its sample (MIPI: 4 bytes), a black level
 * that is not finite, a white level that is not finite or not above the mean black level, a gain given both ways (gain != 1 and d_gain), a
 * host gain <= 0 or not finite, gain_batch other than 1 or batch (0 without d_gain), d_gain not 4-byte aligned, levels outside 1 .. 4, an
 * empty coarsest level, a frame of 2 GiB or more, non-zero reserved, more than 65535 frames: RC_ERR_INVALID before any launch. */
int rc_raw_motion_pyramid(const void* d_src, const rc_raw_format* fmt, float gain, const float* d_gain, int gain_batch, int levels,
                          void* const* d_levels, int batch, int h, int w, void* stream);

/* rc_raw_temporal_mc.  Every argument up to w is rc_raw_temporal's and means what it means there.  d_vec: (B, by, bx, 4) int32, 16-byte
 * aligned -- what rc_motion_search wrote at level 0 of the two proxies; slots 0 and 1 (dx, dy) are used, in Bayer cells: the content of a
 * cell of the frame sits at (cx + dx, cy + dy) of the state.  block: 8, 16 or 32 cells per node and axis; by, bx >= 1 (a grid short of the
 * frame is continued by its last row and column, one beyond it is not read there).  One step goes in front of rc_raw_temporal's 1 - 7, which
 * stay word for word with this s:
 *   0'. displaced state   cy = y >> 1, cx = x >> 1; the node is (min(cy / block, by-1), min(cx / block, bx-1)); (dx, dy) are its slots 0 and
 *                1, each clamped to [-32768, 32767] (device data is never trusted);
 *                s = prev[2 clamp(cy + dy, 0, h-1) + (y & 1)][2 clamp(cx + dx, 0, w-1) + (x & 1)].
 * The displacement is in whole cells and the clamp is in cells, so a sample only ever meets a state sample of its own CFA position.  Step
 * 3's taps use e = |c - p| of each tap's own sample, displaced by that sample's own block.  With RC_TNR_RESET neither d_prev nor d_vec is
 * read (both may be null).  Hence, exactly: a zero field gives rc_raw_temporal's bits; any field gives the bits of rc_raw_temporal run on a
 * state gathered by step 0'.  Every index is clamped: no vector makes the kernel read outside its buffers.  One launch, capturable.
 * Every refusal of rc_raw_temporal, and: a null d_vec without RC_TNR_RESET, d_vec not 16-byte aligned, a block other than 8, 16 or 32,
 * by or bx < 1: RC_ERR_INVALID before anything is enqueued. */
int rc_raw_temporal_mc(const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                       const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w,
                       const int* d_vec, int by, int bx, int block, void* stream);

/* ---- Quad-Bayer (tetracell) sensors (ABI 15, additive): the new first box of the input side, in front of the defects stage.  Each colour of
 * the Bayer cell covers a 2x2 block of photosites, so the pattern repeats every 4x4; what leaves the stage is an ordinary Bayer mosaic with
 * the same cfa and the same levels.
 * Replaces: unpacking the RAW10 / RAW12 lines into a tensor and a dozen gather / select passes over fp32 copies of it.  Here one launch over
 * the bytes as delivered. */
#define RC_QUAD_REMOSAIC 0        /* rc_quad_desc.mode: the full-resolution quad mosaic -> a Bayer mosaic of the same size */
#define RC_QUAD_BIN 1             /* ... -> the 2x2 same-colour binned Bayer mosaic at half size */
typedef struct rc_quad_desc {
    int mode;              /* RC_QUAD_REMOSAIC or RC_QUAD_BIN */
    int reserved[3];       /* zero */
} rc_quad_desc;
size_t rc_quad_desc_size(void);

/* src: B frames (H, W) as rc_raw_defects reads them (fmt: storage, line_bytes, width = 0 or W; cfa is checked and names the colours of the
 * four 2x2 blocks of the 4x4 tile; black and white are not looked at).  H and W are the frame's rows and columns (not halves), multiples
 * of 4.  Sensor sample (y,x) has colour cfa[2 ((y>>1)&1) + ((x>>1)&1)]; the result has colour cfa[2 (y&1) + (x&1)] at (y,x).  The two G
 * of the cell are one colour.
 * d_dst, rows dst_pitch_bytes apart (0: dense):
 *   REMOSAIC  (B, H, W), frames H rows apart: uint16 for RC_RAW_U16 / U8 / MIPI10 / MIPI12, the source type for RC_RAW_F32 / BF16 / F16.
 *   BIN       (B, H/2, W/2) fp32 for every storage, frames H/2 rows apart.
 *
 * v(y,x) is the decoded sample as fp32 (counts are exact).  Every sum, difference and quotient is rounded to fp32 on its own (no fused
 * multiply-add); /3 is one correctly rounded fp32 division.  A coordinate outside the frame reflects so that the colour is kept:
 * y' = 1 - y for y < 0, y' = 2H - 3 - y for y >= H, the same in x (the stencil reaches 2 samples: one reflection suffices).
 * REMOSAIC, with T the wanted colour at (y,x), S the sensor's colour there, sy = +1 for odd y and -1 for even y, sx alike from x:
 *   1. S = T (6 of the 16 sites of a tile): out = v(y,x), unchanged.
 *   2. along a row or a column the colours come in pairs (A A B B ..).  If T occurs on that line its nearest samples to the two sides are
 *      near = the sample at distance 1 (x + sx, or y + sy) and far = the one at distance 2 on the other side (x - 2 sx, or y - 2 sy).
 *      The axis estimate is e = near + (far - near) / 3, the axis gradient d = |far - near|.
 *   3. T on both axes (G wanted at an R or B site): d_H < d_V: out = e_H;  d_V < d_H: out = e_V;  equal: out = (e_H + e_V) 0.5.
 *   4. T on one axis only (R or B wanted at a G site): out = that axis' e.
 *   5. T on neither axis (R wanted at a B site, or B at an R site): the diagonal neighbour (y + sy, x + sx) has colour T, and so have
 *      (y + sy, x - 2 sx), (y - 2 sy, x + sx), (y - 2 sy, x - 2 sx).  Per row:
 *        r_near = v(y+sy, x+sx) + (v(y+sy, x-2sx) - v(y+sy, x+sx)) / 3;   r_far the same on row y - 2 sy;
 *      then out = r_near + (r_far - r_near) / 3.
 *   6. count storages store rint(out), half to even, as uint16; float storages round to nearest even to the source type.  A kept sample
 *      keeps its exact value.
 * BIN:  out(y,x) = ((v(2y,2x) + v(2y,2x+1)) + (v(2y+1,2x) + v(2y+1,2x+1))) 0.25, stored as fp32 (the mean of four counts is exact).
 * Hence, exactly: per-colour flat fields come out unchanged; a plane affine in x and y with integer slopes comes out as the true Bayer
 * sampling wherever the stencil does not reflect (2 samples from every border).
 * Single pass over source samples only: the result does not depend on the traversal order and is the same from run to run.  No atomics, no
 * device state, one launch, capturable.  Frames holding NaN / Inf are outside this contract (no fault, any value).
 * Null d_src / fmt / desc / d_dst, an unknown storage or cfa, line_bytes shorter than a row or no multiple of the sample size, fmt->width
 * other than 0 or W, a source misaligned for its sample (MIPI: 4 bytes), a dst pitch shorter than a row or no multiple of the sample size,
 * dst misaligned, H or W below 4 or no multiple of 4, an unknown mode, non-zero reserved (fmt's too), more than 65535 frames:
 * RC_ERR_INVALID before anything is enqueued. */
int rc_raw_quad(const void* d_src, const rc_raw_format* fmt, const rc_quad_desc* desc, void* d_dst, int dst_pitch_bytes,
                int batch, int H, int W, void* stream);

/* ---- RAW-domain 3A statistics (ABI 15, additive): histograms and a zone grid of the sensor mosaic itself, per CFA colour --------------------
 * What an auto-exposure, auto-white-balance or autofocus loop reads: linear, black-subtracted, in front of every gain (rc_frame_stats measures
 * the network's result: sRGB-encoded, white-balanced by the gains the loop is looking for, clamped -- a clipped photosite can no longer be
 * told there).  The tap of forward_mosaic is behind rc_raw_quad / rc_raw_defects / rc_raw_hdr_merge / rc_raw_temporal and in front of
 * rc_raw_calibrate.
 * Replaces: rc_raw_calibrate to an fp32 copy of the frame, four strided slices, a bincount per colour and a pooling pass per sum.  Here one
 * launch over the bytes as delivered. */
#define RC_RAW_STATS_SLOTS 8
#define RC_RAW_STATS_MAX_GRID 64
#define RC_RAW_STATS_MAX_HIST_BITS 10
typedef struct rc_raw_stats_desc {
    int roi[4];      /* cy0, cx0, rh, rw in Bayer CELLS; rh = rw = 0: the whole frame */
    int grid[2];     /* gy, gx zones, 1 .. min(64, rh) and 1 .. min(64, rw) */
    int bits;        /* 8 .. 16: codes 0 .. S, S = 2^bits - 1 */
    int hist_bits;   /* 6 .. min(bits, 10): a histogram has 2^hist_bits bins */
    float top;       /* the sample value that maps to S; > every black level */
    int sat;         /* 1 .. 2^bits: a cell is saturated if max of its four codes >= sat; 2^bits: none */
    int dark;        /* -1 .. S: a cell that is not saturated is dark if that max <= dark; -1: none */
    int reserved[4]; /* zero */
} rc_raw_stats_desc;
size_t rc_raw_stats_desc_size(void);

/* d_src: B frames of a mosaic (2h, 2w) as rc_raw_calibrate reads them (fmt: every storage, cfa, line_bytes, width, black; white is not looked
 * at: `top` takes its place).  The ROI and the zones are in Bayer cells: cell (cy, cx) is the samples (2cy, 2cx), (2cy, 2cx+1), (2cy+1, 2cx),
 * (2cy+1, 2cx+1), CFA positions pos = 0 .. 3 in that order (black[]'s order).  d_hist (B, 4, 2^hist_bits) and d_zones (B, gy, gx, 8), both
 * int64, 8-byte aligned.  The colour index c is the packed map's slot order -- 0 R, 1 G of the R row (G1), 2 G of the B row (G2), 3 B; slot c
 * reads the position of its colour in the cell, as rc_raw_ingest_fmt's packed map does -- which is the order of rc_calib_desc.gains, not the
 * position order of black[].  Per frame, for the sample p at position pos with slot c:
 *   1. v = float(p), exact for every storage; NaN counts as 0.
 *   2. d = v - black[pos];  n = d k[pos], each rounded to fp32 on its own (no fused multiply-add), with
 *      k[pos] = float(double(S) / (double(top) - double(black[pos]))) formed once on the host;  q = clamp(rint(n), 0, S), round half to even.
 *      With top - black = S (black 0, white 1023, bits 10) q is the sensor's own code.  No value of p, +-inf included, makes an index leave a
 *      table: +inf gives S, -inf gives 0.
 *   3. hist[c][q >> (bits - hist_bits)] += 1 for every sample of the ROI.
 *   4. cell (cy, cx) has the four codes qR, qG1, qG2, qB and m = max of them: it is saturated if m >= sat; otherwise dark if m <= dark;
 *      otherwise valid.
 *   5. g = (qG1 + qG2) >> (bits - 7), 0 .. 255.  Focus f = dx^2 + dy^2, dx = g[cy][min(cx+1, rw-1)] - g[cy][cx], dy = g[min(cy+1, rh-1)][cx]
 *      - g[cy][cx] (ROI-relative indices): the neighbour is clamped to the ROI, not to the frame.
 *   6. cell (cy, cx) of the ROI belongs to zone (floor(cy gy / rh), floor(cx gx / rw)), as in rc_frame_stats (zone column i is the columns
 *      ceil(i rw / gx) .. ceil((i+1) rw / gx) - 1, never empty).  zones[j][i][0..7] = the valid cells; the sums of qR, of qG1, of qG2 and of
 *      qB over the valid cells; the saturated cells; the dark cells; the sum of f over all cells of the zone.
 * Everything after step 2 is integer arithmetic: the result does not depend on the order of summation, so it is bit-exact and the same from
 * run to run although it is accumulated with atomics.  A mosaic holds fewer than 2^31 samples, so fewer than 2^29 cells; a code is at most
 * 65535 and f at most 2 * 255^2, so every total stays below 2^46.
 * Every element of both outputs is written: the entry point zeroes them on `stream` itself (the caller does not), then one launch adds.
 * It keeps no device buffer of its own and is capturable; a graph replay starts from zero again.
 * Null pointers, an unknown storage or cfa, a bad line_bytes or width, a misaligned source, non-finite black levels, a bad shape (empty, more
 * than 65535 frames, a mosaic of 2^31 samples or more), bits, hist_bits, sat, dark or grid out of range, a top that is not finite, is at or
 * below a black level or so close to one that k is not finite, an ROI outside the frame or with one zero side only, non-zero reserved (fmt's
 * too), outputs not 8-byte aligned: RC_ERR_INVALID before anything is enqueued, with a message naming rc_raw_stats. */
int rc_raw_stats(const void* d_src, const rc_raw_format* fmt, const rc_raw_stats_desc* desc, void* d_hist, void* d_zones,
                 int batch, int h, int w, void* stream);

/* ---- RAW noise measurement (ABI 15, additive): a photon-transfer curve of the sensor mosaic itself, per CFA colour ---------------------------
 * What the noise models of rc_raw_temporal (noise_abs, noise_rel), rc_raw_defects (hot / cold) and rc_raw_hdr_merge (motion) are calibrated
 * from: variance against level, taken from the flat parts of ordinary frames.  The region is cut into tiles of T x T Bayer cells; per tile and
 * colour the energy of the differences of disjoint horizontal pairs is binned by the tile's level, and the low quantile of a level bin's
 * energies is the energy of its flat tiles (texture only ever adds energy).  The tap of forward_mosaic is behind rc_raw_quad /
 * rc_raw_defects / rc_raw_hdr_merge and IN FRONT of rc_raw_temporal: behind the filter the noise it is told about is gone.
 * Replaces: an fp32 copy of the frame, four strided slices, an unfold and a quantile per level bin.  Here one launch over the bytes as
 * delivered. */
#define RC_RAW_NOISE_EBINS 320
#define RC_RAW_NOISE_MAX_LEVEL_BITS 6
typedef struct rc_raw_noise_desc {
    int roi[4];      /* cy0, cx0, rh, rw in Bayer CELLS; rh = rw = 0: the whole frame.  cx0 even. */
    int tile;        /* 4, 8 or 16: a tile is tile x tile cells */
    int bits;        /* 8 .. 16: S = 2^bits - 1 */
    int level_bits;  /* 3 .. 6: L = 2^level_bits level bins */
    float top;       /* the sample value that maps to S; > every black level */
    int sat;         /* 1 .. S+1: a sample with code >= sat spoils its tile (for its colour); S+1: none */
    int floor;       /* -S-1 .. S-1: a sample with code <= floor spoils its tile; -S-1: none */
    int reserved[4]; /* zero */
} rc_raw_noise_desc;
size_t rc_raw_noise_desc_size(void);

/* d_src and fmt as rc_raw_stats reads them: B frames of a mosaic (2h, 2w), every storage, any cfa, padded lines, width, black; white is not
 * looked at: `top` takes its place.  Cells, CFA positions pos = 0 .. 3 (black[]'s order) and the colour index c = 0 R, 1 G1, 2 G2, 3 B (the
 * packed map's slot order, rc_calib_desc.gains' order) are rc_raw_stats'.  d_hist (B, 4, L, 320) int32, 4-byte aligned; d_level (B, 4, L)
 * int64, 8-byte aligned; T = tile.  Per frame:
 *   1. Code.  v = float(p), exact for every storage; NaN counts as 0.  d = v - black[pos];  n = d k[pos], each rounded to fp32 on its own (no
 *      fused multiply-add), with k[pos] = float(double(S) / (double(top) - double(black[pos]))) formed once on the host exactly as
 *      rc_raw_stats forms it;  q = clamp(rint(n), -S, S), rint rounding half to even.  The lower clamp is -S, NOT 0: samples below the black
 *      level are the lower half of the noise at black, and clamping them at 0 would halve the variance of the darkest bin.  +-inf clamp like
 *      any other value.
 *   2. Tiles.  Tile (ty, tx) is the cells cy0 + T ty .. + T - 1 by cx0 + T tx .. + T - 1, for ty < rh div T and tx < rw div T; the cells
 *      beyond the last whole tile are not measured.  Per tile and per CFA position, over that position's T^2 samples:  s1 = sum q;
 *      m = max q;  n = min q;  e = sum d^2 over the T^2 / 2 DISJOINT horizontal pairs of cells, d = q(y, 2j) - q(y, 2j+1) with tile-relative
 *      cell columns.  Disjoint pairs make the d independent: on a flat tile with noise variance sigma^2 (in codes), e / (2 sigma^2) is
 *      chi-squared with T^2 / 2 degrees of freedom.
 *   3. Validity.  The tile is valid for that colour if m < sat and n > floor.
 *   4. Level bin.  l = max(s1, 0) >> (2 log2 T + bits - level_bits), so 0 <= l <= L - 1 by construction.
 *   5. Energy bin, a 3-bit-mantissa code of e:  ebin(e) = e for e < 16;  else, with k = floor(log2 e), ebin(e) = 8 (k - 3) + (e >> (k - 3)).
 *      e <= 2 T^2 S^2 < 2^41, so ebin <= 311; e needs 64 bits above bits = 12.
 *   6. Accumulate.  For a valid tile:  hist[c][l][ebin(e)] += 1  and  level[c][l] += s1 (signed).
 * Everything after step 1 is integer arithmetic: the result does not depend on the order of summation, so it is bit-exact and the same from
 * run to run although it is accumulated with atomics.  A mosaic holds fewer than 2^31 samples, so a frame has fewer than 2^25 tiles (a
 * count fits int32) and |sum s1| < 2^29 x 2^16 = 2^45.
 * Every element of both outputs is written: the entry point zeroes them on `stream` itself (the caller does not), then one launch adds.
 * It keeps no device buffer of its own and is capturable; a graph replay starts from zero again.
 * Null pointers, an unknown storage or cfa, a bad line_bytes or width, a misaligned source, non-finite black levels, a bad shape (empty, more
 * than 65535 frames, a mosaic of 2^31 samples or more), a tile other than 4, 8 or 16, bits, level_bits, sat or floor out of range, a top that
 * is not finite, is at or below a black level or so close to one that k is not finite, an odd cx0, an ROI outside the frame, with one zero
 * side only or with fewer than T cell rows or columns, non-zero reserved (fmt's too), d_level not 8-byte or d_hist not 4-byte aligned:
 * RC_ERR_INVALID before anything is enqueued, with a message naming rc_raw_noise. */
int rc_raw_noise(const void* d_src, const rc_raw_format* fmt, const rc_raw_noise_desc* desc, void* d_hist, void* d_level,
                 int batch, int h, int w, void* stream);

/* ---- lateral chromatic aberration (ABI 15, additive): the R and B samples of the mosaic resampled inside their own colour's plane -- the last
 * box of the input side, between the calibration and the ingest.
 * A lens images red and blue at a slightly different magnification than green; towards the corners an edge lands on different photosites in
 * R, G and B.  The error has to leave the mosaic: once the planes are interpolated together the fringe is part of the picture, and rc_warp
 * moves the three output planes by one mesh.  DNG carries the calibration as WarpRectilinear radial terms per plane, chart tools as a coarse
 * grid of shifts; both become the mesh below.
 * Replaces: unpacking the lines into fp32, two strided slices, two dense grids and two F.grid_sample calls, and a scatter -- five full-frame
 * passes and two dense grids in HBM.  Here one launch over the bytes as delivered. */
#define RC_CA_MAX_REACH 8         /* the largest |shift| a mesh may ask for, in samples of a colour's plane */
typedef struct rc_ca_desc {
    int interp;            /* RC_WARP_BILINEAR | RC_WARP_BICUBIC */
    int cell;              /* 8, 16, 32, 64 or 128: a node every `cell` samples of a colour's own h x w plane (every 2 cell mosaic samples) */
    int reach;             /* 1 .. 8: every shift is clamped into [-reach, reach]; the kernel stages a halo of reach + 2 (bicubic) or + 1 */
    int reserved[5];       /* zero */
} rc_ca_desc;
size_t rc_ca_desc_size(void);

/* d_src: B frames of a mosaic (2h, 2w) as rc_raw_calibrate reads them (fmt: every storage, cfa, line_bytes, width; black and white are not
 * looked at: the interpolation is linear and R and B each have one black level, so the levels keep their meaning).  d_shift: DEVICE fp32,
 * 8-byte aligned, (2, Gh, Gw, 2): plane 0 belongs to R, plane 1 to B; node (j, i) of a plane holds (dx, dy) in samples of the colour's own
 * plane (one unit is two mosaic samples) for plane sample (j cell, i cell); Gh = ceil(h / cell) + 1, Gw = ceil(w / cell) + 1; one mesh serves
 * every frame.  Nodes need not be finite (step 2).  d_dst: (B, 2h, 2w) fp32, rows dst_pitch_bytes apart (0: dense), frames 2h rows apart.
 *
 * c is the decoded sample as fp32 (counts are exact).  Every product, sum and difference is rounded on its own (no fused multiply-add).
 * A G sample stores c.  The R sample -- and likewise the B sample, with its own mesh plane -- at position (Y, X) of its colour's plane
 * (mosaic sample (2Y + py, 2X + px), (py, px) the colour's place in the cell), with k = log2(cell):
 *   1. mesh     j0 = Y >> k, i0 = X >> k; fy = (Y & (cell - 1)) 2^-k, fx = (X & (cell - 1)) 2^-k (exact); with g00, g01, g10, g11 the nodes
 *               (j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1), per component (dx, then dy):
 *               top = g00 + fx (g01 - g00);  bot = g10 + fx (g11 - g10);  d = top + fy (bot - top)
 *               -- rc_raw_calibrate's step 3: a constant mesh shifts by exactly that constant.
 *   2. guard    NaN -> 0; then d = min(max(d, -float(reach)), float(reach)).  Whatever the device mesh holds -- NaN, +-inf, 1e30 -- no tap
 *               leaves what the kernel staged.
 *   3. source   sx = float(X) + dx, sy = float(Y) + dy;  x0 = int(floor(sx)), tx = sx - float(x0);  y0, ty likewise.
 *   4. taps     offsets and weights are rc_warp's step 4: BILINEAR 0, 1 with 1-t, t; BICUBIC -1, 0, 1, 2 with c2(t+1), c1(t), c1(1-t),
 *               c2(2-t) and its two polynomials.  A tap outside [0, w) x [0, h) reads the plane sample at the index clamped into the plane.
 *   5. sums     rc_warp's step 5: per tap row r_k = (..((wx_0 s_k0) + (wx_1 s_k1)) + ..), then o = (..((wy_0 r_0) + (wy_1 r_1)) + ..).
 *   6. store    fp32.
 * Consequences: a zero mesh returns the decoded frame exactly (up to the sign of a zero); a mesh of whole numbers returns the shifted plane
 * exactly wherever no tap was clamped; a zero R plane of the mesh leaves R exact while B moves.  Frames holding NaN / Inf are outside this
 * contract (no fault, any value).  One launch, capturable; the library keeps no device buffer.
 * Null pointers, an unknown storage, cfa or interp, a cell outside 8 .. 128, a reach outside 1 .. 8, non-zero reserved (fmt's too),
 * line_bytes shorter than a row or no multiple of the sample size, fmt->width other than 0 or 2w, a RAW10 width not divisible by 4, a source
 * misaligned for its sample (MIPI: 4 bytes), a mesh not 8-byte aligned, a dst pitch shorter than a row or no multiple of 4, dst misaligned or
 * overlapping src, a frame of 2 GiB or more (rows x pitch, either side), h or w above 2^23 (RC_WARP_MAX_DIM), more than 65535 frames:
 * RC_ERR_INVALID before anything is enqueued. */
int rc_raw_aberration(const void* d_src, const rc_raw_format* fmt, const rc_ca_desc* desc, const float* d_shift,
                      float* d_dst, int dst_pitch_bytes, int batch, int h, int w, void* stream);

/* ---- raw stills (ABI 15, additive): the sensor mosaic as delivered -> one DNG file per frame, coded on the device -----------------------------
 * The raw file next to rc_jpeg_encode's still: a little-endian TIFF whose one IFD holds the CFA image in tiles, each tile a lossless JPEG
 * stream (ITU-T T.81 process 14, DNG's Compression 7).  The library knows nothing of TIFF tags: the caller composes the header -- the TIFF
 * header, IFD 0 and its out-of-line values, header_bytes in all -- and names the two places in it where the TileOffsets and TileByteCounts
 * arrays (LONG, one entry per tile, raster order) stand; rc_dng_encode copies the header and fills the two arrays.
 * Replaces: a device-to-host copy of (B, 2h, 2w) uint16 and a host encoder.  Three launches per call and no host sync, as rc_jpeg_encode:
 * every tile is coded by one wave, twice -- once to count its bytes, once, after a scan of the counts, straight to its place in the file. */
typedef struct rc_dng_desc {
    int tile_w, tile_h;    /* in mosaic samples; multiples of 16 in 16 .. 65520 */
    int components;        /* 2: a tile is a frame of tile_w / 2 columns and 2 components, so a sample is predicted from the sample two to its
                              left, which has its own colour; 1: tile_w columns of one component */
    int reserved[5];       /* zero */
} rc_dng_desc;
size_t rc_dng_desc_size(void);

typedef struct rc_dng_plan_info {
    long long tile_header_bytes;   /* SOI .. the end of SOS of a tile (rc_dng_tile_header): 58 + 5 components */
    long long tiles_x, tiles_y;    /* ceil(w2 / tile_w), ceil(h2 / tile_h) */
    long long capacity;            /* the default bytes per frame: header_bytes + tiles (tile_header_bytes + 2 + 4 tile_w tile_h).  A sample is
                                      at most 27 bits, so only a frame full of stuffed 0xFF bytes can exceed it */
    long long scratch_bytes;       /* per frame of the batch: 4 per tile */
} rc_dng_plan_info;

/* Host only.  h2, w2: the mosaic's size in samples, both even.  fmt: only its storage is looked at -- RC_RAW_U16, RC_RAW_U8, RC_RAW_MIPI10 or
 * RC_RAW_MIPI12; a float storage is refused (a DNG holds sensor codes).  header_bytes must be even and at least 8; the two arrays
 * [offsets_at, offsets_at + 4 tiles) and [counts_at, ...) must start on even offsets, lie inside the header and not overlap; the default
 * capacity must stay below 2^31 (TIFF offsets are LONG, and a tile's stuffed byte count must fit 32 bits).  RC_ERR_INVALID otherwise. */
int rc_dng_plan(const rc_dng_desc* desc, const rc_raw_format* fmt, int h2, int w2, long long header_bytes, long long offsets_at, long long counts_at,
                rc_dng_plan_info* plan);
/* Host only.  SOI .. the end of SOS of a tile into buf[0 .. cap), *len = tile_header_bytes (the same for every tile of a file). */
int rc_dng_tile_header(const rc_dng_desc* desc, const rc_raw_format* fmt, uint8_t* buf, size_t cap, size_t* len);

/* d_src: B frames of a mosaic (h2, w2) as rc_raw_stats reads them (fmt: the four integer storages, any cfa -- it is not looked at --
 * line_bytes, width; black and white are not looked at).  d_header: the caller's header_bytes on the device.  d_scratch: batch *
 * scratch_bytes, 4-byte aligned, no state between calls.  d_dst: batch * capacity bytes, frame b at b * capacity.  d_lengths (batch) int64:
 * the bytes each complete file NEEDS, whether or not they fit.  Frame b is d_dst[b capacity .. b capacity + lengths[b]) when lengths[b] <=
 * capacity; otherwise its `capacity` bytes are unspecified.  Nothing outside a frame's `capacity` bytes is written, whatever the data.
 * The file, bit for bit:
 *   layout   the header's bytes, with entry t of the array at offsets_at = the offset of tile t's stream and entry t of the array at
 *            counts_at = its length, both little-endian LONG; then the tiles' streams in raster order of tiles, each on an even offset: a
 *            stream of odd length is followed by one zero byte (the last one too; lengths[b] counts it).
 *   samples  sample (y, x) of the tile grid is the frame's (y', x'): x' = x for x < w2, else w2 - 2 + (x & 1); y' = y for y < h2, else
 *            h2 - 2 + (y & 1) -- beyond the frame the last sample of the same colour repeats (TIFF tiles are whole).  v is the sample's code
 *            as stored (rc_raw_storage's bit layouts), an integer below 2^P, P = 8 / 10 / 12 / 16 for U8 / MIPI10 / MIPI12 / U16.
 *   stream   SOI; SOF3 (Lf = 8 + 3 Nf, precision P, tile_h lines, tile_w / components columns, Nf = components, component c: id c + 1,
 *            sampling 1x1, Tq 0); one DHT (Lh = 36, class 0, id 0, the table below); SOS (Ls = 6 + 2 Ns, Ns = components, component c:
 *            id c + 1, tables 0; Ss = 1: predictor 1; Se = 0; Ah = Al = 0); the entropy-coded data; EOI.  No restart markers.
 *   predict  with n = components, sample (y, x) of a tile is predicted by 2^(P-1) for y = 0 and x < n, by sample (y - 1, x) for y > 0
 *            and x < n, and by sample (y, x - n) otherwise.
 *   code     d = (v - prediction) mod 2^16 taken as signed; SSSS = 0 for d = 0, else the bit length of |d| (16 for d = -32768); the
 *            Huffman code of SSSS, then -- unless SSSS is 0 or 16 -- the low SSSS bits of d (d >= 0) or of d + 2^SSSS - 1 (d < 0).
 *            Samples in raster order of the tile; bits MSB first; the last byte padded with 1-bits; 0xFF -> 0xFF 0x00.
 *   table    fixed and canonical, built for the noise of 10 .. 12-bit sensors: BITS = 0,0,5,3,1,1,1,1,1,1,1,1,1,0,0,0; HUFFVAL =
 *            1,2,3,4,5, 0,6,7, 8,9,10,11,12,13,14,15,16.  The longest code with its extra bits is 12 + 15 = 27 bits.
 * Null pointers, a float or unknown storage, an unknown cfa, a bad line_bytes or width, a misaligned source, odd or non-positive h2 / w2,
 * more than 65535 frames, a tile or components outside the limits, non-zero reserved (fmt's too), header_bytes / offsets_at / counts_at
 * that rc_dng_plan refuses, a capacity below 1 or of 2^32 or more, scratch not 4-byte or lengths not 8-byte aligned: RC_ERR_INVALID before
 * anything is enqueued, with a message naming rc_dng_encode. */
int rc_dng_encode(const void* d_src, const rc_raw_format* fmt, const rc_dng_desc* desc, const void* d_header, long long header_bytes,
                  long long offsets_at, long long counts_at, void* d_scratch, void* d_dst, void* d_lengths, int batch, int h2, int w2,
                  long long capacity, void* stream);
/* Measurement only (tools/dng_bench.py times the launches one by one): as rc_debug_jpeg_passes, for rc_dng_encode's three launches. */
int rc_debug_dng_passes(int mask);

/* ---- layout plumbing at the nn.Module boundary (reference tensors are NCHW) ------------------
 * nchw (B,C,h,w) -> nhwc (B,hp,wp,C) with zero padding (hp>=h, wp>=w) and dtype conversion. */
int rc_nchw_to_nhwc(const void* d_src, int src_dtype, void* d_dst, int dst_dtype,
                    int batch, int c, int h, int w, int hp, int wp, void* stream);
/* nhwc (B,H,W,C) -> nchw (B,C,h,w) cropping to h<=H, w<=W. */
int rc_nhwc_to_nchw(const void* d_src, int src_dtype, void* d_dst, int dst_dtype,
                    int batch, int c, int H, int W, int h, int w, void* stream);

/* ---- a3/a4/a7/a9/a11: KxK convolution, stride 1, "same" zero padding, MFMA implicit GEMM ------
 * Replaces: nn.Conv2d as built by networks.conv mode 'C' (models/networks.py:146-160) and its
 * fused neighbours: ReLU / LeakyReLU (networks.py:189-200), the RCAB/RCAGroup/U-Net additive skips
 * (networks.py:311,335; models/LiteISP.py:2028-2031), Res_GFM's FiLM + LeakyReLU(0.01)
 * (models/LiteISP.py:553-558), head*(lsc+1) (models/LiteISP.py:2014), nn.PixelShuffle(2)
 * (models/LiteISP.py:1998) and the CALayer input/gate (networks.py:267-270).
 *
 * Weights are re-packed once (host side) into the MFMA fragment order with rc_conv_pack_weights.
 */
typedef struct rc_conv_desc {
    int32_t batch, height, width;   /* input spatial size == conv output size                     */
    int32_t cin, cout, ksize;       /* ksize: 1 or 3 (zero padding ksize/2); 5 (cout <= 16; bf16 / fp16 with cin % 48 == 0 or cin % 32 == 0, fp32 with cin % 16 == 0:
                                       the folded tail, rc_tail_fold_weights);
                                       2 (bf16 only, cin % 16 == 0, RC_OUT_NHWC only): the 2x2 window
                                       at pixel offsets {-1, 0}^2, weights (cout, cin, 2, 2) -- the non-zero taps of a stride-2 3x3
                                       convolution (compressai conv3x3(stride=2), ResidualBlockWithStride; models/tcm.py:336-345) taken
                                       over the rc_space_to_depth2 map of its input (9 of the 16 (tap, phase) weight blocks non-zero;
                                       the 3x3 embedding of the same convolution carries 36 blocks) */
    int32_t dtype;                  /* rc_dtype of activations + packed weights: RC_F32, RC_BF16, RC_F16 */
    /* input x.  in_gate==NULL: x = in0.
     * in_gate!=NULL (CALayer gate + RCAB skip, networks.py:270,311): x = in0*gate[b][c] + in1 and,
     * if in_store!=NULL, x is also written there (it is the next block's skip tensor).           */
    const void* in0;
    const void* in1;
    const float* in_gate;           /* (B, cin) fp32                                              */
    void* in_store;
    const void* wpacked;            /* device copy of rc_conv_pack_weights output                 */
    const float* bias;              /* device, packed order (rc_conv_pack_bias), or NULL          */
    /* epilogue on v = acc + bias, in this order:
     *   film_scale!=NULL: v = v*scale[b][c] + shift[b][c] + v        (Res_GFM, LiteISP.py:556)
     *   act                                                          (none / relu / leaky)
     *   mul_plus1!=NULL : v = v * (mul_plus1[b][y][x][c] + 1)        (LiteISP.py:2014)
     *   out_scale!=NULL : v = v * out_scale[b][c]                    (networks.py:270, last field)
     *   residual!=NULL  : v = v + residual[b][y][x][c]                                         */
    const float* film_scale;        /* (B, cout) fp32                                             */
    const float* film_shift;        /* (B, cout) fp32                                             */
    int32_t act;                    /* rc_act                                                     */
    float act_slope;
    const void* mul_plus1;          /* NHWC (B,H,W,cout), activation dtype                        */
    const void* residual;           /* NHWC (B,H,W,cout), activation dtype                        */
    void* out;
    int32_t out_mode;               /* rc_out_mode                                                */
    int32_t out_dtype;              /* rc_dtype of `out` (RC_OUT_NCHW may emit fp32 from a bf16 / fp16 net;
                                       other modes require out_dtype == dtype)                    */
    int32_t out_h, out_w;           /* RC_OUT_NCHW crop size (<= height,width), RC_OUT_PIXEL_SHUFFLE2_NCHW crop size (<= 2 height, 2 width); else ignored */
    /* optional per-channel partial sums of v (the value stored), for CALayer's global mean
     * (networks.py:268): fp32 (B, rc_conv_sum_tiles(), cout), reduced in fixed order by rc_ca_gate */
    float* chan_sums;
    /* ksize 2 only, 0 = unused: in0 is the stride-2 convolution's OWN input (B, src_h, src_w, cin / 4) and the kernel gathers the
     * space-to-depth channels while staging (channel p*(cin/4) + k of map pixel (y, x) = channel k of source pixel (2y + (p >> 1),
     * 2x + (p & 1)), zero beyond the source edge -- rc_space_to_depth2's order), so no space-to-depth pass is launched.  Needs
     * height = ceil(src_h / 2), width = ceil(src_w / 2), cin / 4 a multiple of 64, no gated input.
     * With src_h set the layer IS a stride-2 3x3 convolution: the 7 of 16 (tap, phase) weight blocks such a convolution never touches (tap row -1 with
     * phase row 0, tap column -1 with phase column 0) are taken as zero and their multiplications are not issued, whatever the weight tensor holds there. */
    int32_t src_h, src_w;
    /* optional (B, cout) fp32: v = v * out_scale[b][c], applied after act / mul_plus1 and BEFORE the residual add -- the CALayer gate of this
     * conv's own output when it is known ahead of the launch (rc_ca_gate_ahead): RCABlock's x + CA(conv(...)) (networks.py:311, 270) leaves
     * the second conv as ONE map, x_new = conv2(t) * gate + x, instead of r = conv2(t) followed by r * gate + x in the next layer's staging. */
    const float* out_scale;
    /* ABI 10: partial-sum slots per image the caller allocated for chan_sums: rc_conv_sum_slots(desc) (what this launch fills -- the carried-sums
     * kernels write one slot per (residue class of their tile walk, wave): 2 048 per image at 4K instead of 32 640) or 0 / rc_conv_sum_tiles() = the
     * per-tile layout every kernel can write.  Any other value is an error. */
    int32_t chan_sums_slots;
    /* ABI 11 (the slot was reserved0): cout tile width in channels, 0 = automatic (64 / 48 / 80 / 16 by shape).  A multiple of 16 <= 80: narrower tiles give the
     * general kernel more blocks on maps too small to fill the chip (fp32 128 -> 128 at 135 x 240, B = 1: 272 blocks of 64 couts for 256 CUs; 16-wide tiles: 1 088).
     * The packed order depends on it: pack weights and bias with rc_conv_pack_weights_ct / rc_conv_pack_bias_ct and the SAME value.  Plain NHWC / NCHW stores, ksize 1 / 3. */
    int32_t cout_tile;
    /* ABI 12: 0 = the implicit GEMM (every shape above).  1 = Winograd F(2x2, 3x3) (csrc/wino.hip): the same stride-1 3x3 convolution with 2.25x fewer
     * multiplications -- 16 products M_xi = U_xi V_xi per 2x2 output tile, U = G g G^T packed by rc_wino_pack_weights (NOT rc_conv_pack_weights), V = B^T d B and
     * Y = A^T M A formed in registers.  fp32, ksize 3, cin % 8 == 0, cout % 16 == 0, RC_OUT_NHWC; bias / film vectors in NATURAL channel order (no rc_conv_pack_bias);
     * epilogue: bias, film, act (none / relu / leaky / relu_post), out_scale, residual, chan_sums (rc_conv_sum_slots(desc) slots); no gated input, mul_plus1, GELU,
     * cout_tile or src_h.  Anything else returns RC_ERR_UNSUPPORTED.  Results differ from algo 0 by fp32 rounding only (exact on small-integer data). */
    int32_t algo;
} rc_conv_desc;

/* Size in bytes of the packed weight buffer for (cin,cout,ksize,dtype,out_mode); 0 on error. */
size_t rc_conv_packed_bytes(int cin, int cout, int ksize, int dtype, int out_mode);
/* Host-side repack.  w_oihw: host fp32 (cout,cin,k,k) as in the state_dict; dst: host buffer of
 * rc_conv_packed_bytes() bytes (then copied to the device by the caller). */
int rc_conv_pack_weights(const float* w_oihw_host, int cin, int cout, int ksize, int dtype,
                         int out_mode, void* dst_host);
/* Packed-order length of bias / film vectors (cout rounded up to the kernel's cout tile) and the
 * host-side permutation: dst[j] = bias[perm(j)] or 0 for padding lanes. */
int rc_conv_packed_cout(int cin, int cout, int ksize, int dtype, int out_mode);
int rc_conv_pack_bias(const float* bias_host, int cin, int cout, int ksize, int dtype, int out_mode,
                      float* dst_host);
/* The same three with a caller-chosen cout tile width (rc_conv_desc.cout_tile; 0 = the functions above). */
size_t rc_conv_packed_bytes_ct(int cin, int cout, int ksize, int dtype, int out_mode, int cout_tile);
int rc_conv_packed_cout_ct(int cin, int cout, int ksize, int dtype, int out_mode, int cout_tile);
int rc_conv_pack_weights_ct(const float* w_oihw_host, int cin, int cout, int ksize, int dtype, int out_mode, int cout_tile, void* dst_host);
int rc_conv_pack_bias_ct(const float* bias_host, int cin, int cout, int ksize, int dtype, int out_mode, int cout_tile, float* dst_host);
/* Winograd form (rc_conv_desc.algo == 1): bytes of the packed U = G g G^T buffer (16 * cin * cout elements; 0 on an unsupported shape) and the host-side packer
 * (w_oihw: host fp32 (cout, cin, 3, 3); products accumulated in double, rounded once). */
size_t rc_wino_packed_bytes(int cin, int cout, int dtype);
int rc_wino_pack_weights(const float* w_oihw_host, int cin, int cout, int dtype, void* dst_host);
/* Number of partial-sum slots per image the conv kernel writes to chan_sums (4 waves per 8x32 tile; depends only on H,W). */
int rc_conv_sum_tiles(int height, int width);
/* Slots per image the launch described by `d` fills in chan_sums (pointers are only tested for NULL; d->chan_sums_slots is ignored): the answer comes from
 * the launcher itself, so an allocation sized by it cannot drift from the dispatch.  Either rc_conv_sum_tiles() (per (8x32 tile, wave)) or, for the
 * carried-sums kernels, grid x waves.  Consumers (rc_ca_gate, rc_ca_gate_ahead) fold whatever count they are given, in fixed order.  -1 on a bad desc. */
int rc_conv_sum_slots(const rc_conv_desc* d);
int rc_conv2d(const rc_conv_desc* desc, void* stream);
/* sizeof(rc_conv_desc) as compiled into the library: lets an FFI binding verify its struct mirror. */
size_t rc_conv_desc_size(void);

/* ---- a11 folded: the tail as ONE convolution ------------------------------------------------------
 * Replaces: self.tail = seq(conv(C, 4C, 'C'), nn.PixelShuffle(2), conv(C, 3, 'C')) (models/LiteISP.py:1996-2000, 2379-2383; applied at
 * :2033, :2410).  There is no activation between the two convolutions, so conv2(PixelShuffle(conv1(x))) is one linear map: a 5x5 convolution
 * C -> 4*O whose channel 4o + 2i + j is output channel o at sub-pixel (i, j) (each sub-pixel uses a 4x4 subset of the 5x5 taps; 36 % of the
 * folded weights are structurally zero).  It does 19 200 instead of 88 128 MACs per packed pixel and the 2H x 2W x C intermediate map (6.4 GB
 * written + 7.7 GB read per 8 frames of 4K) never exists.
 *   rc_tail_fold_weights (host): w1 (4C,C,3,3), b1 (4C) or NULL, w2 (O,C,3,3), b2 (O) or NULL -> wc (4O,C,5,5), bc (4O); accumulated in
 *     double.  Run the result as rc_conv2d ksize 5 (4O <= 16; bf16 / fp16 C = 48 k / 32 k, fp32 C = 16 k) with RC_OUT_PIXEL_SHUFFLE2_NCHW.
 * The fold is exact everywhere except the outermost ring of output pixels (the second convolution zero-pads the shuffled map; the fold sees
 * conv1 evaluated beyond the edge there).  The ring is recomputed with the two original convolutions on four thin strips:
 *   rc_tail_ring_gather : x NHWC (B,H,W,C) -> rows (2B,2,W,C) = [x[:,0:2], x[:,H-2:H]], cols (2B,2,H,C) = [x[:,:,0:2], x[:,:,W-2:W]] TRANSPOSED
 *     (cols pixel (r, y) = x[b][y][r]: the side strips run as 2 x H images -- a 2-pixel-wide image would waste 15/16 of every conv tile)
 *   (caller: conv1 with RC_OUT_PIXEL_SHUFFLE2 + conv2 with RC_OUT_NCHW on both strip batches, the transposed batch with ky <-> kx swapped weights and
 *    conv1's sub-pixel order 4c+2i+j <-> 4c+2j+i -> rows_out (2B,O,4,2W), cols_out (2B,O,4,2H))
 *   rc_tail_ring_scatter: output row 0 / row 2H-1 from rows_out rows 0 / 3, column 0 / 2W-1 from cols_out ROWS 0 / 3 -> out (B,O,out_h,out_w),
 *     skipping what the crop (out_h < 2H, out_w < 2W) removes.  dtype = element type of the strips and of out. */
int rc_tail_fold_weights(const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host, int c, int o,
                         float* wc_host, float* bc_host);
int rc_tail_ring_gather(const void* d_x, void* d_rows, void* d_cols, int dtype, int batch, int H, int W, int c, void* stream);
int rc_tail_ring_scatter(const void* d_rows_out, const void* d_cols_out, void* d_out, int dtype, int batch, int c_out, int H, int W,
                         int out_h, int out_w, void* stream);

/* ---- a5+a6 fused: two 3x3 convolutions with the intermediate kept on chip ------------------------
 * Replaces, for 48-channel bf16 feature maps (the flagship width):
 *   RCABlock.res      conv -> ReLU -> conv                 (models/networks.py:296-311; + CALayer sums)
 *   Res_GFM           conv0 -> x*scale+shift+x -> LeakyReLU -> conv1 -> + x     (models/LiteISP.py:553-558)
 * i.e. exactly two rc_conv2d calls whose intermediate NHWC map never goes to HBM (the 48->48 layers run at
 * the HBM copy rate, so this halves their traffic).  Same operands as rc_conv_desc where they apply:
 * in1/in_gate/in_store feed conv1's input staging (x = in0*gate + in1), act1 is RC_ACT_RELU, or
 * RC_ACT_LEAKY together with film_scale/film_shift; residual is added to conv2's result (FiLM form only);
 * chan_sums receives rc_conv_pair_sum_slots() partials per image (ReLU form only) for rc_ca_gate.
 * w1/w2: rc_conv_pack_weights(48,48,3,RC_BF16,RC_OUT_NHWC); b1/b2: rc_conv_pack_bias or NULL.
 * Other widths / fp32 return RC_ERR_UNSUPPORTED-style errors: callers issue two rc_conv2d calls instead. */
typedef struct rc_conv_pair_desc {
    int32_t batch, height, width, channels;
    int32_t dtype;                  /* RC_BF16                                                    */
    const void* in0;                /* NHWC (B,H,W,48)                                            */
    const void* in1;                /* optional skip tensor (with in_gate)                        */
    const float* in_gate;           /* optional (B,48) fp32 CALayer gate                          */
    void* in_store;                 /* optional: materialised in0*gate + in1                      */
    const void* w1; const float* b1;
    const float* film_scale;        /* (B,48) fp32, FiLM form                                     */
    const float* film_shift;
    int32_t act1;                   /* RC_ACT_RELU | RC_ACT_LEAKY                                 */
    float act1_slope;
    const void* w2; const float* b2;
    const void* residual;           /* optional NHWC (B,H,W,48), added to conv2's result          */
    void* out;                      /* NHWC (B,H,W,48)                                            */
    float* chan_sums;               /* optional fp32 (B, rc_conv_pair_sum_slots(), 48)            */
} rc_conv_pair_desc;
int rc_conv_pair(const rc_conv_pair_desc* desc, void* stream);
int rc_conv_pair_sum_slots(int height, int width);
size_t rc_conv_pair_desc_size(void);

/* ---- a5 fused: the lens-shading MLP as one launch ------------------------------------------------
 * Replaces: Lens_Shading_Correction.model = Conv1x1(cin0,48) -> LeakyReLU -> [Conv1x1(48,48) -> LeakyReLU] x (n_mid-1)
 * -> Conv1x1(48,48) (models/LiteISP.py:363-378) when the width is 48 and the tensors are bf16: a 1x1 conv has no
 * halo, so each wave carries its 64 pixels through all layers in LDS and HBM sees only the coordinates in and the
 * final map out (layer by layer, every intermediate 48-channel map is written and re-read).
 * d_x NHWC (pixels, cin0 <= 8) bf16; d_w0packed = rc_conv_pack_weights(cin0,48,1,RC_BF16,RC_OUT_NHWC) (one zero-padded MFMA
 * step), d_b0 its packed bias (or NULL); d_wpacked[m] = rc_conv_pack_weights(48,48,1,RC_BF16,RC_OUT_NHWC) device buffers,
 * d_bias[m] packed fp32 (or NULL), 1 <= n_mid <= 4
 * (host arrays of device pointers); slope in [0,1]; d_out NHWC (pixels, 48) bf16.  fp32 / other widths: error,
 * callers run the layers through rc_conv2d. */
int rc_pointwise_chain48(const void* d_x, int cin0, const void* d_w0packed, const float* d_b0, const void* const* d_wpacked,
                         const float* const* d_bias, int n_mid, float slope, void* d_out, int dtype, long long pixels,
                         void* stream);

/* The chain with register-resident activations, optionally with the consuming convolution folded in (models/LiteISP.py:363-378 and
 * :2012-2014 `h = head(raw); h = h * (lsc(coord) + 1)`; ISPUNet :1352-1355; models/raw2bit.py:1775-1781 at width 128):
 *   d_out = chain(d_x)                                         when d_raw == NULL
 *   d_out = (conv3x3(d_raw) + bias) * (chain(d_x) + 1)         otherwise -- one launch, the lens-shading map never reaches HBM.
 * A wave carries 64 pixels through every layer in MFMA fragments (no LDS round trip between layers); the map is rounded to bf16 where the
 * two-launch path stores it.  bf16 only, c = 32, 48, 64 or 128, cin0 <= 4, raw_c <= 4, 1 <= n_mid <= 4 (layers after the first).
 * d_blob: rc_lsc_pack's output (rc_lsc_packed_bytes bytes) on the device: w0 (c,cin0), wmid[l] (c,c), whead (c,raw_c,3,3) fp32 as in the
 * state_dict (+ biases, or NULL) re-ordered into pair-packed MFMA fragments.  d_x NHWC (batch,H,W,cin0), d_raw NHWC (batch,H,W,raw_c). */
size_t rc_lsc_packed_bytes(int c, int n_mid, int has_head);
int rc_lsc_pack(const float* w0, const float* b0, int cin0, const float* const* wmid, const float* const* bmid, int n_mid,
                const float* whead, const float* bhead, int raw_c, int c, void* dst);
int rc_lsc_chain(const void* d_x, int cin0, const void* d_blob, int c, int n_mid, float slope, const void* d_raw, int raw_c,
                 void* d_out, int batch, int H, int W, void* stream);

/* ---- a8: CALayer gate -------------------------------------------------------------------------
 * Replaces: AdaptiveAvgPool2d(1) -> Conv1x1(C,C/r) -> ReLU -> Conv1x1(C/r,C) -> Sigmoid
 * (models/networks.py:259-269).  d_sums: (B, n_tiles, C) partials from rc_conv2d; w0 (Cr,C), b0 (Cr),
 * w1 (C,Cr), b1 (C) fp32 device; gate: (B,C) fp32.  Fixed-order reduction => run-to-run bitwise stable.
 * d_sums is scratch after the call (large images are folded in place in a first stage). */
int rc_ca_gate(float* d_sums, int batch, int n_tiles, int c, int cr, float inv_hw,
               const float* d_w0, const float* d_b0, const float* d_w1, const float* d_b1,
               float* d_gate, void* stream);

/* The same gate, computed AHEAD of the convolution whose output CALayer pools: RCABlock is x + CA(conv2(t)), t = relu(conv1(x))
 * (models/networks.py:296-311), and mean_HW(conv2(t)) is linear in t: b2 + 1/HW * sum_{c,tap} W2[o][c][tap] * S_tap[c], S_tap = the sum of t[c] over
 * the pixels tap (dy,dx) reaches inside the image (total - cut-off border row / column + corner).  d_sums: conv1's channel-sum partials of t
 * (B, n_tiles, C) (scratch after the call, as in rc_ca_gate); d_t: the NHWC map t itself (B,H,W,C), read for its four border lines only;
 * d_w2t (C_in,3,3,C_out) fp32 = conv2's OIHW weight permuted (1,2,3,0) / d_b2 (C) or NULL: conv2's parameters; d_scratch: rc_ca_gate_ahead_scratch_floats(B, C) floats.  The gate then goes
 * into conv2's launch as rc_conv_desc.out_scale (+ residual = x): one map written per RCAB body instead of r and r*gate + x. */
size_t rc_ca_gate_ahead_scratch_floats(int batch, int c);
int rc_ca_gate_ahead(float* d_sums, int batch, int n_tiles, int c, int cr, const void* d_t, int dtype, int H, int W,
                     const float* d_w2t, const float* d_b2, const float* d_w0, const float* d_b0, const float* d_w1, const float* d_b1,
                     float* d_scratch, float* d_gate, void* stream);

/* Per-channel partial sums of an NHWC map (B, n_pix, C): the AdaptiveAvgPool2d(1) of a standalone CALayer
 * (models/networks.py:259,268) when no producing conv emitted them.  d_sums: fp32 (B, rc_channel_sums_slots(n_pix), C),
 * fixed-order partials in the layout rc_ca_gate folds. */
int rc_channel_sums_slots(int n_pix);
int rc_channel_sums(const void* d_x, int dtype, int batch, int n_pix, int c, float* d_sums, void* stream);

/* y = r*gate[b][c] + x  (CALayer scale + RCAB skip, networks.py:270,311) for call sites where the
 * gated tensor is not consumed by a conv; d_x == NULL: y = r*gate (CALayer alone, networks.py:270).
 * NHWC, n_pix = H*W per image. */
int rc_gate_residual(const void* d_r, const float* d_gate, const void* d_x, void* d_y, int dtype,
                     int batch, int n_pix, int c, void* stream);

/* GFMLayer applied to a feature map (models/LiteISP.py:308-321; Res_GFM_LFM :601-620): y = x*scale[b][c] + shift[b][c] + x with the
 * two (B,C) fp32 vectors of rc_gfm_vector.  NHWC, n_pix = H*W per image. */
int rc_film_apply(const void* d_x, const float* d_scale, const float* d_shift, void* d_y, int dtype, int batch, int n_pix, int c, void* stream);

/* ---- a19 (SWAtten, models/tcm.py:284-289): y = a * sigmoid(b) + identity, element-wise on NHWC maps of n_elems
 * elements (a multiple of 16 bytes); y may alias a. */
int rc_sigmoid_gate_add(const void* d_a, const void* d_b, const void* d_identity, void* d_y, int dtype, long long n_elems,
                        void* stream);

/* ---- a20 (CompressAI layers under models/tcm.py:336-357, restated; parity unpinned) -----------------------------------
 * Stride-2 sampling of an NHWC map: dst (B, ceil(H/2), ceil(W/2), C)[y][x] = src (B,H,W,C)[2y][2x].  A 3x3 stride-2 padding-1
 * convolution (conv3x3(stride=2) in ResidualBlockWithStride / g_a / h_a) is rc_conv2d followed by this; a 1x1 stride-2
 * convolution (the block's skip) is this followed by rc_conv2d. */
int rc_subsample2(const void* d_src, void* d_dst, int dtype, int batch, int H, int W, int c, void* stream);
/* ---- a18 (models/raw2bit.py): nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) of HyCondModDecBlock (:790-793) on NHWC maps:
 * dst (B,2H,2W,c); source coordinate = dst * (H-1)/(2H-1) per axis. */
int rc_upsample_bilinear2(const void* d_src, void* d_dst, int dtype, int batch, int H, int W, int c, void* stream);
/* SpatialFeatureTransform (:877-885) + the block's identity (:313): y = x*scale + shift + x (+ identity if d_identity != NULL). */
int rc_sft_apply(const void* d_x, const void* d_scale, const void* d_shift, const void* d_identity, void* d_y, int dtype,
                 long long n_elems, void* stream);
/* Space-to-depth by 2 on NHWC maps of any width: dst (B, ceil(H/2), ceil(W/2), 4c)[y][x][(2i+j)*c + k] = src (B,H,W,c)[2y+i][2x+j][k], zero
 * beyond the bottom / right edge.  A 3x3 stride-2 padding-1 convolution is then a 3x3 stride-1 convolution over the 4c-channel map
 * with the taps re-indexed (row offset -1 <- phase 1 of the previous row pair, 0 <- phases 0 and 1), which rc_conv2d runs at the
 * OUTPUT resolution. */
int rc_space_to_depth2(const void* d_src, void* d_dst, int dtype, int batch, int H, int W, int c, void* stream);
/* nn.PixelShuffle(2) on NHWC maps of any width: dst (B,2H,2W,c)[2y+i][2x+j][k] = src (B,H,W,4c)[y][x][4k + 2i + j].  (rc_conv2d's
 * RC_OUT_PIXEL_SHUFFLE2 store covers c % 16 == 0; this is for the narrow tails, e.g. subpel_conv3x3(2N, 3, 2) of g_s.) */
int rc_pixel_shuffle2(const void* d_src, void* d_dst, int dtype, int batch, int H, int W, int c_out, void* stream);
/* The same shuffle written straight into NCHW: d_src (batch,H,W,4*c_out) NHWC -> d_dst (batch,c_out,2H,2W) -- the codecs' x_hat at the
 * module boundary (subpel_conv3x3(2N, 3, 2) closing g_s, models/tcm.py:364) without a separate layout pass. */
int rc_pixel_shuffle2_nchw(const void* d_src, void* d_dst, int dtype, int batch, int H, int W, int c_out, void* stream);
/* GDN / inverse GDN around a 1x1 rc_conv2d:  rc_square gives x^2 (the conv input, weights gamma, bias beta);
 * rc_gdn_apply gives y = x * rsqrt(norm) (inverse=0) or x * sqrt(norm) (inverse=1), + identity if d_identity != NULL
 * (the residual add that follows the GDN in both residual blocks). */
int rc_square(const void* d_x, void* d_y, int dtype, long long n_elems, void* stream);
int rc_gdn_apply(const void* d_x, const void* d_norm, const void* d_identity, void* d_y, int dtype, int inverse, long long n_elems,
                 void* stream);

/* ---- a19: the likelihood path TCM.forward asks of CompressAI's entropy models (models/tcm.py:441-446, 467-469, 475-477),
 * restated from their published definitions (parity unpinned); element-wise on NHWC maps, likelihoods always fp32.
 * rc_entropy_bottleneck: EntropyBottleneck.forward in eval mode + the z_hat of :443-446.
 *   d_params: (C, 58) fp32 per channel, the 1-3-3-3-3-1 cumulative-logit network with the parameter non-linearities already
 *   applied on the host: [softplus(_matrix0) 3 | _bias0 3 | tanh(_factor0) 3] then for layers 1..3
 *   [softplus(_matrix_l) 3x3 row-major (out, in) | _bias_l 3 | tanh(_factor_l) 3], then [softplus(_matrix4) 3 | _bias4 1];
 *   d_medians: (C) fp32 = quantiles[:, 0, 1].
 *   likelihood = max(|sigmoid(s*upper) - sigmoid(s*lower)|, bound), s = -sign(lower + upper), evaluated at round(z - med) + med -+ 0.5;
 *   z_hat = (round(t) - t + t) + med, t = z - med  (ste_round). */
int rc_entropy_bottleneck(const void* d_z, const float* d_params, const float* d_medians, void* d_z_hat, float* d_likelihood,
                          int dtype, long long n_pix, int channels, float likelihood_bound, void* stream);
/* GaussianConditional.forward(y, scales, means) in eval mode + the y_hat of :470:
 *   likelihood = max(Phi((0.5 - |q|)/s) - Phi((-0.5 - |q|)/s), bound), q = round(y - mu), s = max(scale, scale_bound (0.11)),
 *   Phi(x) = 0.5 erfc(-x / sqrt 2);  y_hat = ste_round(y - mu) + mu. */
int rc_gaussian_conditional(const void* d_y, const void* d_scale, const void* d_mu, void* d_y_hat, float* d_likelihood, int dtype,
                            long long n_elems, float scale_bound, float likelihood_bound, void* stream);
/* y_hat_slice += 0.5 * tanh(lrp)  (:478-479) */
int rc_tanh_half_add(const void* d_a, const void* d_lrp, void* d_out, int dtype, long long n_elems, void* stream);

/* ---- a10: Haar DWT / IDWT as the reference's frozen grouped conv -----------------------------
 * Replaces: DWTForward (models/networks.py:224-235) / DWTInverse (:238-249).  taps: device fp32
 * (4C,1,2,2) exactly as stored in the state_dict ("down1.3.weight", "up1.0.weight").
 * forward: (B,H,W,C) -> (B,H/2,W/2,4C), channel 4c+k.  inverse: (B,h,w,4C) -> (B,2h,2w,C).
 * taps_uniform != 0: the caller guarantees every channel carries the taps of channel 0 (true for the
 * reference's Haar init, networks.py:228-233); the kernel then keeps the 16 taps in scalar registers. */
int rc_dwt_forward(const void* d_x, void* d_y, const float* d_taps, int taps_uniform, int dtype,
                   int batch, int H, int W, int c, void* stream);
int rc_dwt_inverse(const void* d_x, void* d_y, const float* d_taps, int taps_uniform, int dtype,
                   int batch, int h, int w, int c4, void* stream);

/* ---- a6: Color_Condition_GFM (global colour prior) --------------------------------------------
 * Replaces: color_block (models/LiteISP.py:23-30) = Conv1x1 -> AvgPool2d(3,2,1,count_include_pad)
 * -> LeakyReLU(0.2) [-> InstanceNorm2d(affine)], and the closing Conv1x1 + AdaptiveAvgPool2d(1)
 * (models/LiteISP.py:345-361).  All fp32, NCHW (the cond image is small).
 *   rc_color_block:  y = lrelu_0.2(avgpool3s2p1(conv1x1(x)))   x:(B,cin,h,w) -> y:(B,cout,ho,wo)
 *                    with ho=(h-1)/2+1; if d_in_mean!=NULL the previous block's InstanceNorm
 *                    (x-mean)*rstd*gamma+beta is applied to x on load.
 *   rc_instance_stats: per (b,c) mean and 1/sqrt(var+eps) (biased var, eps 1e-5).
 *   rc_color_head:   v[b][o] = mean_hw(conv1x1(x))  -> (B,cout)   (the 5th block has no norm)      */
int rc_color_block(const void* d_x, int x_dtype, float* d_y, int batch, int cin, int cout, int h, int w,
                   const float* d_w, const float* d_b,
                   const float* d_in_mean, const float* d_in_rstd, const float* d_in_gamma,
                   const float* d_in_beta, void* stream);
int rc_instance_stats(const float* d_x, float* d_mean, float* d_rstd, int batch, int c, int hw,
                      float eps, void* stream);
/* InstanceNorm2d(affine) of a standalone CB block (models/LiteISP.py:215-230) with the statistics of rc_instance_stats:
 * y = (x - mean[b][c]) * rstd[b][c] * gamma[c] + beta[c], fp32 NCHW (inside the colour branch the norm is folded into the next
 * block's load instead). */
int rc_instance_norm(const float* d_x, float* d_y, const float* d_mean, const float* d_rstd, const float* d_gamma, const float* d_beta,
                     int batch, int c, int hw, void* stream);
int rc_color_head(const float* d_x, float* d_vec, int batch, int cin, int cout, int hw,
                  const float* d_w, const float* d_b, void* stream);

/* ---- a7: GFM vector MLPs ----------------------------------------------------------------------
 * Replaces: GFM_{scale,shift}_conv1(leaky_relu(GFM_{scale,shift}_conv0(vec), 0.1))
 * (models/LiteISP.py:554-555).  vec (B,cond_c); w0 (nf,cond_c) b0 (nf) w1 (c,nf) b1 (c); out (B,c). */
int rc_gfm_vector(const float* d_vec, int batch, int cond_c, int nf, int c,
                  const float* d_w0, const float* d_b0, const float* d_w1, const float* d_b1,
                  float* d_out, void* stream);

/* ---- a14-a16: GroupMix attention (GMA_Block) ---------------------------------------------------
 * Replaces the non-GEMM parts of models/groupmix.py:159-299 (identical copy models/raw2bit.py:98-142); the
 * four nn.Linear layers run through rc_conv2d as 1x1 convolutions (tokens (B,N,C) == NHWC pixels).
 *
 * rc_dwconv2d: depth-wise KxK (3/5/7), stride 1, 'same' zero padding, on channel sub-ranges of NHWC tensors:
 *   y[b,p, y_c0 + r*y_rep_stride + c] = bias[r*w_rep_stride + c] + sum_t wT[t][r*w_rep_stride + c] *
 *                                       x[b,p+t, x_c0 + r*x_rep_stride + c]  (+ x[b,p,..] if add_identity)
 *   for r < n_rep, c < n_ch.  wT: device fp32, TAP-MAJOR (K*K, n_w).  Replaces ConvPosEnc.proj
 *   (groupmix.py:206,215), SeparableConv2d.conv1 (:244) and ConvRelPosEnc.conv_list (:127-133).
 * rc_layernorm: nn.LayerNorm over C of (tokens, C) (groupmix.py:280,285).
 * rc_gma_pointwise: Aggregator tail (groupmix.py:92-100) with BatchNorm(eval) folded to scale/shift:
 *   qkv (B,N,3C), dw = depth-wise outputs of groups 1..3 (token t, rep r, group g at dw + t*dw_tok_stride +
 *   r*dw_rep_stride + (g-1)*seg), dwl = local depth-wise output (dwl + t*dwl_tok_stride + r*dwl_rep_stride); both may
 *   live in one (B,N,3,4seg) tensor written by a single rc_dwconv2d launch (strides 12seg / 4seg, dwl = dw + 3seg)
 *   -> qkvp (B,N,3,4seg) [q|k|v, channel = head*Ch + i], loc (B,N,seg).
 * rc_gma_kv: softmax over the N tokens fused with k^T v (groupmix.py:187-188): per-channel max pass, exp-sum +
 *   k^T v pass, fixed-order merge: ktv (B,heads,Ch,Ch) fp32 = scale * softmax_N(k)^T v.  d_scratch: rc_gma_kv_scratch_bytes().
 * rc_gma_apply: out (B,N,C) = [ q.ktv + q*convv | loc ]  (groupmix.py:189-194). */
/* ---- a15/a16 fused per-token stages of GMA_Block for dim 80 (5 x 16, 8 heads), bf16 (csrc/gma_fused.hip) --------------------
 * Chain weights: an nn.Linear / 1x1 conv weight (cout, cin) fp32 host -> bf16 MFMA fragments whose output rows are ordered so
 * that a layer's accumulator fragments are the next layer's B fragments (rc_chain_packed_bytes bytes); biases fp32 in the same
 * row order, zero padded (rc_chain_packed_rows(cout) floats; b NULL: zeros).  Host functions.
 * rc_gma_ln_qkv: qkv = Linear_qkv(LayerNorm1(x (tokens, 80))), written PLANAR BY 16-CHANNEL SEGMENT: d_qkv[15][tokens][16], segment
 *                s = channel / 16 = 5 * {q,k,v} + group -- the layout rc_gma_aggregate reads            (groupmix.py:178 after :293)
 * rc_gma_tail:   (d_qkvp, d_convv: the segment-planar tensors of rc_gma_aggregate / rc_gma_crpe; d_loc (tokens,16); d_x (tokens,80))
 *                y = [ q.ktv + q*convv | loc ] (groupmix.py:189-194); x2 = proj(y) + x (:197, :294); x3 = x2 + fc2(GELU(fc1(LN2(x2))))
 *                (:296-298); cout == 0: out (tokens, 80) = x3; cout == 192: out (tokens, 192) = Conv1x1(x3) + res (the cfg3 net's
 *                gma_out + d1, realcamnet_amd/LiteISP.py).  d_ktv (B,8,8,8) fp32 from rc_gma_kv; d_ktv_frags: B * 8 KiB scratch.
 * Rounding points are those of the layer-by-layer path (bf16 wherever that path stored a tensor), accumulation fp32; GELU's erf is
 * evaluated to 1.5e-7 absolute (far below the bf16 rounding of its result). */
size_t rc_chain_packed_bytes(int cin, int cout);
int rc_chain_packed_rows(int cout);
int rc_chain_pack_weights(const float* w, int cin, int cout, void* dst);
int rc_chain_pack_bias(const float* b, int cout, float* dst);
int rc_gma_ln_qkv(const void* d_x, void* d_qkv, long long tokens, const void* d_wpacked, const float* d_bias_packed,
                  const float* d_ln_gamma, const float* d_ln_beta, float eps, void* stream);
int rc_gma_tail(const void* d_qkvp, const void* d_convv, const void* d_loc, const void* d_x, const float* d_ktv, void* d_ktv_frags,
                int batch, int n_tok, const void* d_w_proj, const float* d_b_proj, const float* d_ln_gamma, const float* d_ln_beta,
                float eps, const void* d_w_fc1, const float* d_b_fc1, const void* d_w_fc2, const float* d_b_fc2, const void* d_res,
                const void* d_w_out, const float* d_b_out, int cout, void* d_out, void* stream);

/* rc_gma_aggregate: the whole Aggregator (groupmix.py:56-105) for dim 80, bf16, one launch: qkv in rc_gma_ln_qkv's segment-planar
 * layout [15][B,H,W][16] -> qkvp, segment-planar too: [12 = 4 * {q,k,v} + group][B,H,W][16]
 * [q|k|v][group 0: BN+Hardswish | groups 1..3: dw 3/5/7 -> pw 16x16 -> BN -> Hardswish] and loc (B,H,W,16) = Hardswish(LN(pw(dw3x3(
 * [q4|k4|v4])))).  dw3/5/7: tap-major (K*K,16) fp32; dwl (3,9,16); pw (3,16,16) [out][in]; pwl (16,48); bn_scale/shift (4,16)
 * (BatchNorm(eval) folded); ln (16).  Same values as rc_dwconv2d + rc_gma_pointwise up to the point-wise product's summation order. */
int rc_gma_aggregate(const void* d_qkv, void* d_qkvp, void* d_loc, int batch, int H, int W, const float* d_dw3, const float* d_dw5,
                     const float* d_dw7, const float* d_dwl, const float* d_pw, const float* d_pwl, const float* d_bn_scale,
                     const float* d_bn_shift, const float* d_ln_g, const float* d_ln_b, float* d_kmax, void* stream);

/* rc_gma_qkv_aggregate (ABI 13): rc_gma_ln_qkv + rc_gma_aggregate as ONE launch (groupmix.py:178 after :293, then :56-105) -- the 240-channel
 * qkv map is never written: a block LayerNorms x (B,H,W,80) for a 16 x 32 tile + halo once, keeps the normalised tokens in registers as MFMA B
 * fragments and produces qkv one 16-channel segment at a time into an LDS tile; the depth-wise K x K windows run ON THE MATRIX CORES as banded
 * Toeplitz products (one MFMA per channel, kernel row and 16-pixel group), then point-wise / BatchNorm / Hardswish as rc_gma_aggregate.
 * d_wq_natural: the (240, 80) qkv weight as rc_chain_pack_weights_natural fragments (output rows in natural channel order: 16-row tile m =
 * segment m); d_bq (240) fp32 or NULL; d_toeplitz: rc_gma_toeplitz_bytes() bytes from rc_gma_toeplitz_pack (host) over the same tap tensors
 * rc_gma_aggregate takes (dw3 / dw5 / dw7 tap-major (K*K,16), dwl (3,9,16)); the other arguments as rc_gma_ln_qkv / rc_gma_aggregate.
 * Same rounding points as the two-launch path; the depth-wise sums are formed in the matrix pipe's order (exact bf16 products, fp32 sums), so
 * results agree with it to the last fp32 bits before the bf16 rounding (tests hold: >= 99.9 % of the values bit-equal, the rest 1 bf16 ulp). */
int rc_chain_pack_weights_natural(const float* w, int cin, int cout, void* dst);   /* host; rc_chain_packed_bytes(cin, cout) bytes; 16 | cin, 16 | cout */
size_t rc_gma_toeplitz_bytes(void);
int rc_gma_toeplitz_pack(const float* dw3, const float* dw5, const float* dw7, const float* dwl, void* dst);   /* host */
/* rc_gma_in_cpe (ABI 14): the cfg3 net's `gma_in` (Conv1x1 192 -> 80, realcamnet_amd/LiteISP.py) followed by the block's ConvPosEnc (depth-wise 3x3 + identity,
 * groupmix.py:203-217, :293) as ONE launch: d_x (B,H,W,80) = a + dw3x3(a) + b_cpe, a = W_in d_d1 + b_in rounded to bf16 (zero outside the image: the depth-wise
 * convolution's padding); the 80-channel map a never reaches HBM.  bf16.  d_w_in_natural: rc_chain_pack_weights_natural(192 -> 80) fragments; d_b_in / d_b_cpe (80)
 * fp32 or NULL; d_toeplitz3: 3 * 80 KiB from rc_dw_toeplitz_pack(taps, 3, 80, .) (host; taps tap-major (9, 80) fp32).  The depth-wise sums are formed in the
 * matrix pipe's order and the 1x1 sums add the bias last: equal to rc_conv2d + rc_dwconv2d on > 99.8 % of the values, the rest within a few bf16 ulps of the
 * intermediate (tested); bitwise stable from run to run (tested). */
int rc_dw_toeplitz_pack(const float* taps, int K, int n_ch, void* dst);        /* host; K * n_ch KiB; K = 3, 5 or 7 */
int rc_gma_in_cpe(const void* d_d1, const void* d_w_in_natural, const float* d_b_in, const void* d_toeplitz3, const float* d_b_cpe, void* d_x,
                  int batch, int H, int W, void* stream);
int rc_gma_qkv_aggregate(const void* d_x, const void* d_wq_natural, const float* d_bq, const float* d_ln1_gamma, const float* d_ln1_beta, float eps,
                         void* d_qkvp, void* d_loc, int batch, int H, int W, const void* d_toeplitz, const float* d_pw, const float* d_pwl,
                         const float* d_bn_scale, const float* d_bn_shift, const float* d_ln_g, const float* d_ln_b, float* d_kmax, void* stream);

/* d_kmax (optional, may be NULL): (batch, 64) fp32, on return the per-channel maximum over the image of the aggregated k (the stored bf16
 * values) -- the shift of softmax_N(k) (models/groupmix.py:190) -- accumulated by the aggregator itself with integer atomics (a maximum is
 * order-independent, so this stays bitwise reproducible).  With it the two-pass rc_gma_kv_planar is replaced by ONE pass on the matrix cores:
 *   rc_gma_kv_mfma: ktv[b][h][i][j] = scale * sum_t softmax_t(k)[t][h,i] v[t][h,j] for 8 heads x 8 channels, segment-planar bf16 qkv'
 * (d_scratch: rc_gma_kv_mfma_scratch_bytes bytes).  exp(k - max) is rounded to bf16 for the MFMA (numerator and denominator use the same
 * rounded values); accumulation fp32, block partials merged in fixed order. */
/* Transformer-block MLP of the codecs (models/tcm.py:234-235: x + mlp(ln2(x)), mlp = Linear(C,4C) -> GELU -> Linear(4C,C)) as ONE launch with
 * register-resident activations: d_out = d_x + fc2(GELU(fc1(LayerNorm(d_x)))).  bf16, token width c = 32 or 64, d_x / d_out (tokens, c);
 * weights packed by rc_chain_pack_weights(c -> 4c) and (4c -> c), biases by rc_chain_pack_bias (or NULL).  Rounding points are those of
 * rc_layernorm + two rc_conv2d launches (LayerNorm output and GELU output to bf16). */
int rc_ln_mlp(const void* d_x, void* d_out, long long tokens, int c, const void* d_w_fc1, const float* d_b_fc1, const void* d_w_fc2,
              const float* d_b_fc2, const float* d_ln_gamma, const float* d_ln_beta, float eps, void* stream);

/* LayerNorm + Linear in one launch (the W-MSA embedding layer behind ln1, models/tcm.py:179-181, 232): d_out (tokens, cout) =
 * Linear(LayerNorm(d_x (tokens, c))), bf16, c = 32 or 64, cout a multiple of 32 (<= 512); weights by rc_chain_pack_weights(c -> cout). */
int rc_ln_linear(const void* d_x, void* d_out, long long tokens, int c, int cout, const void* d_w, const float* d_b, const float* d_ln_gamma,
                 const float* d_ln_beta, float eps, void* stream);
/* (ABI 14) the same launch with d_out SEGMENT-PLANAR: [cout / 8 segments][tokens][8 channels] -- the q / k / v layout rc_window_attention_planar8 reads. */
int rc_ln_linear_planar8(const void* d_x, void* d_out, long long tokens, int c, int cout, const void* d_w, const float* d_b, const float* d_ln_gamma,
                         const float* d_ln_beta, float eps, void* stream);

/* GDN / inverse GDN (compressai.layers.GDN inside ResidualBlockWithStride / ResidualBlockUpsample; call sites models/tcm.py:336-364) as one
 * per-token launch: d_out = d_x * rsqrt(beta + gamma . d_x^2)  (inverse != 0: * sqrt(..))  [+ d_identity], bf16, c = 64 or 128 channels,
 * tensors (tokens, c).  d_gamma_packed = rc_chain_pack_weights of the EFFECTIVE (re-parametrised) gamma (c, c), d_beta_packed =
 * rc_chain_pack_bias of the effective beta.  Same rounding points as rc_square -> rc_conv2d -> rc_gdn_apply. */
int rc_gdn_chain(const void* d_x, const void* d_identity, void* d_out, long long tokens, int c, const void* d_gamma_packed,
                 const float* d_beta_packed, int inverse, void* stream);

/* Linear over the channel concatenation of two token maps + residual, without the concatenated map (the closing
 * `conv1_2(torch.cat((conv_x, trans_x), dim=1)) + x` of ConvTransBlock, models/tcm.py:265-267; raw2bit.py:324-327):
 * d_out (tokens, c) = d_residual + W . [d_a (tokens, c/2) ; d_b (tokens, c/2)] + bias.  bf16, c = 64 or 128; d_w = rc_chain_pack_weights(c -> c),
 * d_bias = rc_chain_pack_bias (or NULL), d_residual may be NULL; d_a_add (or NULL): the first half is d_a + d_a_add, rounded to bf16
 * (ConvTransBlock's `conv_block(conv_x) + conv_x`, models/tcm.py:262, without its own launch). */
int rc_cat_linear(const void* d_a, const void* d_a_add, const void* d_b, const void* d_residual, void* d_out, long long tokens, int c,
                  const void* d_w, const float* d_bias, void* stream);

int rc_gma_kv_mfma_blocks(int n_tok);
size_t rc_gma_kv_mfma_scratch_bytes(int batch, int n_tok);
int rc_gma_kv_mfma(const void* d_qkvp, int batch, int n_tok, float scale, const float* d_kmax, float* d_scratch, float* d_ktv, void* stream);

/* rc_gma_crpe: ConvRelPosEnc's depth-wise conv of v (groupmix.py:127-133,146-150) for dim 80 / 8 heads of 8, bf16: v = segments 8..11
 * of rc_gma_aggregate's segment-planar qkvp -> convv, segment-planar [4][B,H,W][16]; four 16-channel segments with windows 3, 5, 7, 7 (tap-major (K*K,16) fp32 each; segment 2 holds
 * heads of window 5 and 7, its window-5 taps zero-padded to 7x7), bias (64).  Same values as rc_dwconv2d. */
int rc_gma_crpe(const void* d_qkvp, void* d_convv, int batch, int H, int W, const float* d_taps0, const float* d_taps1,
                const float* d_taps2, const float* d_taps3, const float* d_bias, void* stream);

int rc_dwconv2d(const void* d_x, int x_stride_c, int x_c0, void* d_y, int y_stride_c, int y_c0, int dtype,
                int batch, int H, int W, int n_ch, int ksize, const float* d_wT, int n_w, const float* d_bias,
                int n_rep, int x_rep_stride, int y_rep_stride, int w_rep_stride, int add_identity,
                const int* d_kvec /* optional: true window per 16-byte weight vector when taps are zero-padded to K */,
                void* stream);
int rc_layernorm(const void* d_x, void* d_y, int dtype, long long tokens, int c, const float* d_gamma,
                 const float* d_beta, float eps, void* stream);
int rc_gma_pointwise(const void* d_qkv, const void* d_dw, const void* d_dwl, int dw_tok_stride, int dw_rep_stride,
                     int dwl_tok_stride, int dwl_rep_stride, void* d_qkvp, void* d_loc, int dtype, long long tokens, int c,
                     const float* d_pw, const float* d_bn_scale, const float* d_bn_shift, const float* d_pwl,
                     const float* d_ln_g, const float* d_ln_b, void* stream);
int rc_gma_kv_blocks(int n_tok);
size_t rc_gma_kv_scratch_bytes(int batch, int n_tok, int heads, int ch);
int rc_gma_kv(const void* d_qkvp, int dtype, int batch, int n_tok, int heads, int ch, float scale, float* d_scratch,
              float* d_ktv, void* stream);
/* rc_gma_kv on rc_gma_aggregate's segment-planar qkvp ([12][B * n_tok][16], bf16). */
int rc_gma_kv_planar(const void* d_qkvp, int batch, int n_tok, int heads, int ch, float scale, float* d_scratch, float* d_ktv, void* stream);
int rc_gma_apply(const void* d_qkvp, const void* d_convv, const void* d_loc, const float* d_ktv, void* d_out, int dtype,
                 int batch, int n_tok, int heads, int ch, int seg, void* stream);

/* ---- a18 plumbing: channel split / concat of NHWC tensors -----------------------------------------
 * Replaces torch.split / torch.cat along the channel dim in ConvTransBlock.forward (models/tcm.py:261-266):
 * dst[p, dst_c0 + c] = src[p, src_c0 + c] for c < n_ch, all offsets / counts whole 16-byte vectors. */
int rc_channel_copy(const void* d_src, int src_stride_c, int src_c0, void* d_dst, int dst_stride_c, int dst_c0, int n_ch,
                    long long pixels, int dtype, void* stream);
/* torch.cat of 1..8 NHWC tensors along the channel dim in ONE launch (the slice loop's `torch.cat([latent_means] + support_slices, dim=1)`,
 * models/tcm.py:460-466, 609-617: 2..6 parts, 22 times per forward): d_parts[k] is (pixels, widths[k]) dense, dst (pixels, sum widths). */
int rc_channel_concat(const void* const* d_parts, const int* widths, int n_parts, void* d_dst, long long pixels, int dtype, void* stream);

/* ---- a17: TCM window attention -------------------------------------------------------------------
 * Replaces the core of WMSA.forward (models/tcm.py:179-206): per ws x ws window of the cyclically shifted NHWC map
 * and per head, softmax(q k^T / sqrt(hd) + relpos[h, dy, dx] (+ -inf across the wrap in the last window row/column
 * when shifted)) v.  d_qkv (B,H,W,3C) = embedding_layer output on the UN-shifted map ([q | k | v], head-major inside
 * each), d_relpos = relative_position_params (heads, 2ws-1, 2ws-1) fp32, d_out (B,H,W,C) attention output at the
 * un-shifted pixel positions (ready for `linear`).  shift = 0 for type 'W', ws/2 for 'SW'.  The Linear layers,
 * LayerNorms and the MLP of tcm.Block (:214-236) are rc_conv2d (1x1) / rc_layernorm. */
int rc_window_attention(const void* d_qkv, const float* d_relpos, void* d_out, int dtype, int batch, int H, int W, int C,
                        int head_dim, int window, int shift, void* stream);
/* (ABI 14) the same attention over a SEGMENT-PLANAR d_qkv: [3C / 8 segments][B H W pixels][8 channels], segment = channel / 8 of the (B,H,W,3C) form above
 * (rc_ln_linear_planar8 writes it).  With head_dim 8 a lane of the interleaved form reads 16 of a pixel record's 384 bytes -- one 64-byte sector per lane; in its
 * segment's plane the 8 pixels of a window row are 128 contiguous bytes.  Exists for the matrix-core form only (bf16, 8 x 8 windows, B H W 3C < 2^31:
 * rc_window_attention_planar8_ok() != 0); RC_ERR_UNSUPPORTED otherwise.  Same arithmetic, same bits as rc_window_attention on the interleaved tensor. */
int rc_window_attention_planar8(const void* d_qkv, const float* d_relpos, void* d_out, int dtype, int batch, int H, int W, int C,
                                int head_dim, int window, int shift, void* stream);
int rc_window_attention_planar8_ok(int dtype, int batch, int H, int W, int C, int window);

/* ---- measurement helpers (bench.py): HIP-event timing of every rc_conv2d launch on its stream -
 * rc_prof_enable(1) brackets each subsequent rc_conv2d with hipEventRecord on the launch stream;
 * rc_prof_collect() synchronises the events and returns launches / total ms / total algorithmic
 * FLOPs (2*MAC at the padded size) since the last rc_prof_enable(1). */
/* A/B switches for tests and benches.  "persist": 0 = general kernel only, 1 (default) = automatic choice between the
 * persistent weights-resident kernel and its producer/consumer (wave-specialised) form, 2 = producer/consumer
 * wherever eligible, 3 = persistent only.  Results must be identical in all modes.
 * Others (all bit-identical alternatives of one operation, defaults in brackets): "conv32" [0] which layers take the
 * 32x32x16 MFMA forms (0 none, 4 = where measured faster, 1 / 2 / 3 = everywhere eligible in one of three forms; set BEFORE
 * packing: the packed weight order depends on it -- and on no other knob: such a layer runs its own kernel in every "persist" mode); "pair_impl" [0] which of the two rc_conv_pair kernels; "pss" [0] the
 * 48 -> 192 + PixelShuffle layer with its output staged through LDS; "dw3_seg16" [1] rc_dwconv2d's bf16 3x3 single-rep
 * case on 16-channel segments; "wmsa_mfma" [1] rc_window_attention's bf16 8 x 8-window calls on the matrix cores (0: the one-lane-per-query kernel, which such a
 * call otherwise reaches only past 2^31 elements per image; rc_window_attention_planar8_ok then answers 0 and rc_window_attention_planar8 is refused: the planar layout exists for the matrix-core form only); "conv_flags" knock-outs for timing experiments (1 no stores, 8 stores into one 4 MB
 * window: results are then meaningless; 64 one persistent block per CU instead of two: results unchanged, an occupancy experiment);
 * "persist_auto" [1] the wave-autonomous kernels 6 / 7 (0 off, 1 all but the residual forms of kernel 6, 2 every eligible form); "sums_compact" [1] the compact
 * channel-sum slot layout (rc_conv_sum_slots); "thin" [2] kernel 4b (one barrier per stage) in place of the multi-chunk kernel 4: 1 = only where the stages are thin (weights and tiles by LDS-DMA, tiles two stages
 * ahead), 2 = also the 3x3 layers with <= 36 KB of weights per chunk (tile through registers, one stage ahead), 0 = kernel 4; "lds_poison" [0] test aid: every rc_conv2d launch is preceded by rc_debug_poison_lds (NaNs in all LDS). "wino_nnt" [0] the Winograd kernel's item size: 0 automatic (4 x 16-pixel items where one image's 4 x 32 regions quantise badly over the chip, 4 x 32 otherwise), 1 / 2 forced.
 * "pw_grid_cap" [4194304 = 2^22] test aid: the most blocks any streaming kernel of pointwise.hip is launched with; past it a thread loops over its items with the grid's stride.
 * The default is never reached below 16 GiB of data, so a test sets a handful of blocks to run those loops at a small size; 0 (or anything outside 1 .. 2^22) restores the default. */
int rc_debug_set(const char* key, int value);
/* Current value of an integer knob ("persist", "conv32", "conv_flags", "pss"), -1 for an unknown key.  The host mirror keys its packed-weight cache
 * on "conv32" (the packed order of the 32x32x16 layers depends on it and on nothing else). */
int rc_debug_get(const char* key);
/* "conv_phase_timing": device buffer of >= 512 int64; the producer/consumer conv kernel then records s_memtime
 * cycle counts per tile phase for one compute wave and one loader wave (NULL switches it off). */
int rc_debug_set_ptr(const char* key, void* d_ptr);
/* Calibration: sustained rate of back-to-back v_mfma_f32_16x16x32_bf16 on every SIMD (1 or 2 waves per SIMD),
 * and s_memtime ticks per MFMA per SIMD: what this part's clocks allow, to read MFMA utilisation against. */
/* Experiment: a HIP stream confined to half of the chip's CUs (hipExtStreamCreateWithCUMask); kind 0/1 = lower / upper 128
 * mask bits, 2/3 = lower / upper 16 bits of every 32-bit word.  Never destroyed (debug only). */
int rc_debug_stream_create_masked(int kind, void** stream_out);
/* HBM streaming probe on the default stream: mode 0 copy / 1 read / 2 write of `bytes`; nt = non-temporal accesses;
 * contiguous = one range per block (else grid-stride); blocks = 0 -> one-shot grid (4 x 16 B per thread). */
int rc_debug_hbm_probe(const void* src, void* dst, size_t bytes, int mode, int nt, int contiguous, int blocks, int iters,
                       double* ms_per_iter);
/* waves_per_simd 11 / 12 (both calibrations): the same loop on RANDOM operands that change from MFMA to MFMA (4 A x 4 B register sets per wave):
 * on toggling data the part runs at its board power cap, not at its maximum clock (tools/power_probe.py); ticks are not reported (0). */
int rc_debug_mfma_peak(int waves_per_simd, int iters, double* tflops, double* memtime_ticks_per_mfma);
/* The same calibration on v_mfma_f32_32x32x16_bf16 (8 independent accumulators per wave). */
int rc_debug_mfma_peak32(int waves_per_simd, int iters, double* tflops, double* memtime_ticks_per_mfma);
/* Test aid: fill the whole LDS allocation of every CU with `pattern` (e.g. 0x7FC07FC0: bf16 / fp32 NaNs) on `stream`, so that a kernel reading LDS it has not
 * written, or before the write has landed, fails the parity tests whatever ran before it (LDS contents survive from one kernel to the next). */
int rc_debug_poison_lds(unsigned pattern, void* stream);
int rc_prof_enable(int on);
int rc_prof_collect(int64_t* n_launches, double* total_ms, double* total_flops);
/* The same records grouped by layer shape (cin, cout, ksize): launches, summed HIP-event ms, algorithmic FLOPs and algorithmic BYTES (every map
 * the launch has to touch once: input, output, residual / multiplier operand, the gated form's skip and materialised input) -- what bench.py's
 * roofline line names its dominant kernel from.  Does not clear the records (rc_prof_enable does). */
typedef struct rc_prof_row { int cin, cout, ksize, launches; double ms, flops, bytes; } rc_prof_row;
int rc_prof_collect_rows(rc_prof_row* rows, int max_rows, int* n_rows);

/* ---- f3: on-device entropy coding (csrc/rans.hip) ----------------------------------------------------------
 * Replaces the `.tolist()` symbol dumps + CompressAI `BufferedRansEncoder` / `RansDecoder` calls of compress() / decompress()
 * (models/tcm.py:511-570, 592-637; models/raw2bit.py:1876-1944, 1961-2027) and the table construction of `update()`
 * (models/tcm.py:430-435).  The coder is CompressAI's published rANS (64-bit state, 32-bit words, 16-bit probabilities, 4-bit bypass
 * escapes); CompressAI itself is absent from /root/reference: restated, parity unpinned.
 *
 * rc_pmf_to_quantized_cdf (host): `compressai._CXX.pmf_to_quantized_cdf`: n probabilities -> n + 1 cumulative frequencies.
 * rc_gc_symbols: GaussianConditional side of compress(): y, mu, scale NHWC (B, hw, C) -> symbols = round(y - mu) and CDF indexes
 *   (`build_indexes`: scale table search with the 0.11 lower bound) as int32 in the coder's (b, c, hw) order, y_hat = symbols + mu
 *   (NHWC).  d_y == NULL: indexes only (decompress()).   rc_gc_dequantize: y_hat = symbols + mu.
 * rc_eb_symbols: EntropyBottleneck side: symbols = round(z - median[c]), index = c, z_hat (encode = 1), or z_hat from symbols (0).
 * rc_rans_encode_chunks: two launches -- all symbols' (CDF row, escape, start, freq, reciprocal of freq) in parallel into d_scratch
 *   (rc_rans_encode_scratch_bytes, 8-byte aligned), then one lane per chunk of `chunk` consecutive symbols doing only the state updates
 *   (division-free, bit-identical to the dividing form: rc_debug_rans_rcp_selftest); every chunk a complete stream in BufferedRansEncoder's
 *   layout written at the END of its rc_rans_chunk_words(chunk)-word slot of d_words; d_nbytes[chunk] = its length (-1: bad index).
 *   rc_rans_compact gathers the streams at the given byte offsets.   rc_rans_decode_chunks: the inverse; every chunk's stream is bounded by the
 *   next chunk's offset (the last by stream_bytes): d_err = 1 bad CDF index, 2 truncated / corrupt stream (a read past a chunk's end, a chunk
 *   shorter than the flushed state or not word-sized, an escape longer than 8 nibbles) -- never an out-of-bounds read.
 * rc_rans_encode_host / rc_rans_decode_host: the same primitives on the host for ONE stream over all symbols = CompressAI's wire
 *   format; decode keeps the decoder state in state[2] (zero-initialised at the start of a stream) like RansDecoder.decode_stream. */
int rc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf);
int rc_gc_symbols(const void* d_y, const void* d_mu, const void* d_scale, int dtype, int batch, long long hw, int channels,
                  const float* d_scale_table, int n_levels, float scale_bound, int32_t* d_symbols, int32_t* d_indexes, void* d_y_hat,
                  void* stream);
int rc_gc_dequantize(const int32_t* d_symbols, const void* d_mu, int dtype, int batch, long long hw, int channels, void* d_y_hat, void* stream);
int rc_eb_symbols(const void* d_z, const float* d_medians, int dtype, int batch, long long hw, int channels, int encode, int32_t* d_symbols,
                  int32_t* d_indexes, void* d_z_hat, void* stream);
int rc_rans_chunk_words(int chunk);
size_t rc_rans_encode_scratch_bytes(long long n, int chunk);
int rc_rans_encode_chunks(const int32_t* d_symbols, const int32_t* d_indexes, long long n, int chunk, const int32_t* d_cdf, int cdf_stride,
                          int n_cdfs, const int32_t* d_cdf_sizes, const int32_t* d_offsets, uint32_t* d_words, int32_t* d_nbytes, void* d_scratch,
                          void* stream);
long long rc_debug_rans_rcp_selftest(long long trials, unsigned long long seed);
int rc_rans_compact(const uint32_t* d_words, int chunk, const int32_t* d_nbytes, const long long* d_offsets, long long n_chunks, void* d_out,
                    void* stream);
int rc_rans_decode_chunks(const void* d_stream, long long stream_bytes, const long long* d_offsets, const int32_t* d_indexes, long long n, int chunk,
                          const int32_t* d_cdf, int cdf_stride, int n_cdfs, const int32_t* d_cdf_sizes, const int32_t* d_cdf_offsets, int32_t* d_symbols,
                          int32_t* d_err, void* stream);
long long rc_rans_encode_host(const int32_t* symbols, const int32_t* indexes, long long n, const int32_t* cdf, int cdf_stride, int n_cdfs,
                              const int32_t* cdf_sizes, const int32_t* offsets, void* out, long long out_cap);
int rc_rans_decode_host(const void* stream_bytes, long long n_bytes, unsigned long long* state, const int32_t* indexes, long long n, const int32_t* cdf,
                        int cdf_stride, int n_cdfs, const int32_t* cdf_sizes, const int32_t* offsets, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* REALCAM_HIP_H */
