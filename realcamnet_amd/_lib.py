"""ctypes binding of librealcam_hip.so (include/realcam_hip.h).

There is no CPU fallback: if the library is missing or does not export a declared symbol the import
fails loudly, and every op refuses non-CUDA tensors.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["RC_HIP_LIB"]) if os.environ.get("RC_HIP_LIB") else PKG / "librealcam_hip.so"   # override: kernel experiments only
HEADER = PKG.parent / "include" / "realcam_hip.h"

RC_F32, RC_BF16, RC_U16, RC_F16 = 0, 1, 2, 3
RC_ACT_NONE, RC_ACT_RELU, RC_ACT_LEAKY, RC_ACT_GELU, RC_ACT_RELU_POST = 0, 1, 2, 3, 4
RC_OUT_NHWC, RC_OUT_PIXEL_SHUFFLE2, RC_OUT_NCHW, RC_OUT_PIXEL_SHUFFLE2_NCHW, RC_OUT_NHWC_DWT = 0, 1, 2, 3, 4
ABI_VERSION = 15
RC_RAW_F32, RC_RAW_BF16, RC_RAW_U16, RC_RAW_F16, RC_RAW_U8, RC_RAW_MIPI10, RC_RAW_MIPI12 = 0, 1, 2, 3, 4, 5, 6
RC_CFA_RGGB, RC_CFA_BGGR, RC_CFA_GRBG, RC_CFA_GBRG = 0, 1, 2, 3
RC_YUV_NV12, RC_YUV_P010, RC_YUV_I420 = 0, 1, 2
(RC_YUV_NV16, RC_YUV_P210, RC_YUV_I422, RC_YUV_I210, RC_YUV_I010, RC_YUV_I444, RC_YUV_I410, RC_YUV_YUY2, RC_YUV_UYVY, RC_YUV_Y210,
 RC_YUV_V210) = range(16, 27)            # 3..15 are not layouts
RC_MATRIX_BT601, RC_MATRIX_BT709, RC_MATRIX_BT2020 = 0, 1, 2
RC_RANGE_LIMITED, RC_RANGE_FULL = 0, 1
RC_SITING_LEFT, RC_SITING_CENTER = 0, 1
RC_JPEG_420, RC_JPEG_444 = 0, 1
RC_FILTER_AREA, RC_FILTER_BILINEAR = 0, 1
RC_RESIZE_MAX_TAPS, RC_RESIZE_MAX_RATIO = 20, 8
RC_LUT3D_MIN_SIZE, RC_LUT3D_MAX_SIZE = 2, 65
RC_WARP_BILINEAR, RC_WARP_BICUBIC = 0, 1
RC_WARP_CLAMP, RC_WARP_CONSTANT = 0, 1
RC_WARP_MIN_CELL_LOG2, RC_WARP_MAX_CELL_LOG2, RC_WARP_MAX_DIM = 3, 6, 1 << 23
RC_STATS_MAX_GRID, RC_STATS_SLOTS = 64, 8
RC_MOTION_MAX_LEVELS, RC_MOTION_MAX_RANGE = 4, 8
RC_TONE_MAX_GRID, RC_TONE_BINS = 16, 256
RC_DEFECT_HOT, RC_DEFECT_COLD = 1, 2
RC_CALIB_GAINS, RC_CALIB_CLIP, RC_CALIB_MAX_KNOTS = 1, 2, 16
RC_HDR_MOTION = 1
RC_TNR_RESET, RC_TNR_GAIN = 1, 2
RC_QUAD_REMOSAIC, RC_QUAD_BIN = 0, 1
RC_RAW_STATS_SLOTS, RC_RAW_STATS_MAX_GRID, RC_RAW_STATS_MAX_HIST_BITS = 8, 64, 10
RC_RAW_NOISE_EBINS, RC_RAW_NOISE_MAX_LEVEL_BITS = 320, 6
RC_CA_MAX_REACH = 8


class ConvDesc(C.Structure):
    """Mirror of `struct rc_conv_desc` -- field order and types must match the header exactly."""
    _fields_ = [
        ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("cin", C.c_int32), ("cout", C.c_int32), ("ksize", C.c_int32),
        ("dtype", C.c_int32),
        ("in0", C.c_void_p), ("in1", C.c_void_p), ("in_gate", C.c_void_p), ("in_store", C.c_void_p),
        ("wpacked", C.c_void_p), ("bias", C.c_void_p),
        ("film_scale", C.c_void_p), ("film_shift", C.c_void_p),
        ("act", C.c_int32), ("act_slope", C.c_float),
        ("mul_plus1", C.c_void_p), ("residual", C.c_void_p),
        ("out", C.c_void_p), ("out_mode", C.c_int32), ("out_dtype", C.c_int32),
        ("out_h", C.c_int32), ("out_w", C.c_int32),
        ("chan_sums", C.c_void_p),
        ("src_h", C.c_int32), ("src_w", C.c_int32),
        ("out_scale", C.c_void_p),
        ("chan_sums_slots", C.c_int32), ("cout_tile", C.c_int32),
        ("algo", C.c_int32),
    ]


class ConvPairDesc(C.Structure):
    """Mirror of `struct rc_conv_pair_desc`."""
    _fields_ = [
        ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
        ("dtype", C.c_int32),
        ("in0", C.c_void_p), ("in1", C.c_void_p), ("in_gate", C.c_void_p), ("in_store", C.c_void_p),
        ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("film_scale", C.c_void_p), ("film_shift", C.c_void_p),
        ("act1", C.c_int32), ("act1_slope", C.c_float),
        ("w2", C.c_void_p), ("b2", C.c_void_p),
        ("residual", C.c_void_p), ("out", C.c_void_p), ("chan_sums", C.c_void_p),
    ]


class RawFormatDesc(C.Structure):
    """Mirror of `struct rc_raw_format`."""
    _fields_ = [
        ("storage", C.c_int32), ("cfa", C.c_int32), ("line_bytes", C.c_int32), ("width", C.c_int32),
        ("black", C.c_float * 4), ("white", C.c_float), ("reserved", C.c_int32 * 4),
    ]


class OutFormatDesc(C.Structure):
    """Mirror of `struct rc_out_format`."""
    _fields_ = [
        ("layout", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32), ("siting", C.c_int32),
        ("pitch", C.c_int32), ("rows", C.c_int32), ("chroma_offset", C.c_int32 * 2), ("reserved", C.c_int32 * 4),
    ]


class JpegDesc(C.Structure):
    """Mirror of `struct rc_jpeg_desc`."""
    _fields_ = [("quality", C.c_int32), ("subsampling", C.c_int32), ("restart", C.c_int32), ("reserved", C.c_int32 * 5)]


class JpegPlanInfo(C.Structure):
    """Mirror of `struct rc_jpeg_plan_info`."""
    _fields_ = [("header_bytes", C.c_longlong), ("mcu_cols", C.c_longlong), ("mcu_rows", C.c_longlong), ("intervals", C.c_longlong),
                ("capacity", C.c_longlong), ("scratch_bytes", C.c_longlong)]


class DngDesc(C.Structure):
    """Mirror of `struct rc_dng_desc`."""
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("components", C.c_int32), ("reserved", C.c_int32 * 5)]


class DngPlanInfo(C.Structure):
    """Mirror of `struct rc_dng_plan_info`."""
    _fields_ = [("tile_header_bytes", C.c_longlong), ("tiles_x", C.c_longlong), ("tiles_y", C.c_longlong), ("capacity", C.c_longlong),
                ("scratch_bytes", C.c_longlong)]


class StatsDesc(C.Structure):
    """Mirror of `struct rc_stats_desc`."""
    _fields_ = [
        ("roi", C.c_int32 * 4), ("grid", C.c_int32 * 2), ("bits", C.c_int32), ("matrix", C.c_int32), ("dark", C.c_int32), ("clip", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class MotionDesc(C.Structure):
    """Mirror of `struct rc_motion_desc`."""
    _fields_ = [("block", C.c_int32), ("range", C.c_int32), ("pred_shift", C.c_int32), ("reserved", C.c_int32 * 5)]


class DefectDesc(C.Structure):
    """Mirror of `struct rc_defect_desc`."""
    _fields_ = [
        ("flags", C.c_int32), ("hot_abs", C.c_float), ("hot_rel", C.c_float), ("cold_abs", C.c_float), ("cold_rel", C.c_float),
        ("reserved", C.c_int32 * 3),
    ]


class CalibDesc(C.Structure):
    """Mirror of `struct rc_calib_desc`."""
    _fields_ = [
        ("flags", C.c_int32), ("knots", C.c_int32), ("cell", C.c_int32), ("curve_x", C.c_float * 16), ("curve_y", C.c_float * 16),
        ("gains", C.c_float * 4), ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("reserved", C.c_int32 * 3),
    ]


class HdrDesc(C.Structure):
    """Mirror of `struct rc_hdr_desc`."""
    _fields_ = [
        ("exposures", C.c_int32), ("flags", C.c_int32), ("times", C.c_float * 4), ("knee_lo", C.c_float), ("knee_hi", C.c_float),
        ("motion_abs", C.c_float), ("motion_rel", C.c_float), ("exposure_stride_bytes", C.c_longlong), ("frame_stride_bytes", C.c_longlong),
        ("reserved", C.c_int32 * 4),
    ]


class SharpenDesc(C.Structure):
    """Mirror of `struct rc_sharpen_desc`."""
    _fields_ = [("radius", C.c_int32), ("matrix", C.c_int32), ("amount", C.c_float), ("core", C.c_float), ("overshoot", C.c_float)]


class ToneDesc(C.Structure):
    """Mirror of `struct rc_tone_desc`."""
    _fields_ = [("grid", C.c_int32 * 2), ("matrix", C.c_int32), ("clip_q8", C.c_int32), ("strength", C.c_float), ("max_gain", C.c_float),
                ("reserved", C.c_int32 * 4)]


class TemporalDesc(C.Structure):
    """Mirror of `struct rc_temporal_desc`."""
    _fields_ = [
        ("flags", C.c_int32), ("noise_abs", C.c_float), ("noise_rel", C.c_float), ("alpha", C.c_float), ("ramp", C.c_float), ("gain", C.c_float),
        ("reserved", C.c_int32 * 4),
    ]


class QuadDesc(C.Structure):
    """Mirror of `struct rc_quad_desc`."""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32 * 3)]


class RawStatsDesc(C.Structure):
    """Mirror of `struct rc_raw_stats_desc`."""
    _fields_ = [
        ("roi", C.c_int32 * 4), ("grid", C.c_int32 * 2), ("bits", C.c_int32), ("hist_bits", C.c_int32), ("top", C.c_float), ("sat", C.c_int32),
        ("dark", C.c_int32), ("reserved", C.c_int32 * 4),
    ]


class RawNoiseDesc(C.Structure):
    """Mirror of `struct rc_raw_noise_desc`."""
    _fields_ = [
        ("roi", C.c_int32 * 4), ("tile", C.c_int32), ("bits", C.c_int32), ("level_bits", C.c_int32), ("top", C.c_float), ("sat", C.c_int32),
        ("floor", C.c_int32), ("reserved", C.c_int32 * 4),
    ]


class CaDesc(C.Structure):
    """Mirror of `struct rc_ca_desc`."""
    _fields_ = [("interp", C.c_int32), ("cell", C.c_int32), ("reach", C.c_int32), ("reserved", C.c_int32 * 5)]


def declared_symbols() -> list[str]:
    """Every function the public header declares (used by the CPU-side ABI test)."""
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", text)))


_P, _I, _F, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_SIGS = {
    "rc_abi_version": (C.c_int, []),
    "rc_last_error": (C.c_char_p, []),
    "rc_build_info": (C.c_char_p, []),
    "rc_device_arch": (C.c_int, [C.c_char_p, _SZ]),
    "rc_bayer_unshuffle": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_raw_ingest": (C.c_int, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P]),
    "rc_raw_format_size": (_SZ, []),
    "rc_raw_ingest_fmt": (C.c_int, [_P, C.POINTER(RawFormatDesc), _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_rgb_encode": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_out_format_size": (_SZ, []),
    "rc_yuv_frame_bytes": (_SZ, [C.POINTER(OutFormatDesc), _I, _I]),
    "rc_yuv_encode": (C.c_int, [_P, _I, C.POINTER(OutFormatDesc), _P, _I, _I, _I, _I, _I, _P]),
    "rc_jpeg_desc_size": (_SZ, []),
    "rc_jpeg_tables": (C.c_int, [_I, _P, _P]),
    "rc_jpeg_plan": (C.c_int, [C.POINTER(JpegDesc), _I, _I, C.POINTER(JpegPlanInfo)]),
    "rc_jpeg_header": (C.c_int, [C.POINTER(JpegDesc), _I, _I, _P, _SZ, C.POINTER(_SZ)]),
    "rc_jpeg_encode": (C.c_int, [_P, _I, C.POINTER(JpegDesc), _P, _P, _P, _P, _I, _I, _I, _I, _I, C.c_longlong, _P]),
    "rc_debug_jpeg_passes": (C.c_int, [_I]),
    "rc_resize_taps": (C.c_int, [_I, _I, _I, _I, _P, _P, C.POINTER(C.c_int)]),
    "rc_resize": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "rc_lut3d": (C.c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_sharpen_desc_size": (_SZ, []),
    "rc_sharpen": (C.c_int, [_P, _I, _P, _I, C.POINTER(SharpenDesc), _I, _I, _I, _I, _I, _P]),
    "rc_tone_desc_size": (_SZ, []),
    "rc_tone_axis": (C.c_int, [_I, _I, _P, _P]),
    "rc_tone_hist": (C.c_int, [_P, _I, C.POINTER(ToneDesc), _P, _I, _I, _I, _I, _I, _P]),
    "rc_tone_gains": (C.c_int, [_P, C.POINTER(ToneDesc), _P, _I, _P]),
    "rc_tone_apply": (C.c_int, [_P, _I, _P, _I, C.POINTER(ToneDesc), _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_warp": (C.c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _F, _F, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_stats_desc_size": (_SZ, []),
    "rc_frame_stats": (C.c_int, [_P, _I, C.POINTER(StatsDesc), _P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_motion_desc_size": (_SZ, []),
    "rc_motion_pyramid": (C.c_int, [_P, _I, _I, _I, C.POINTER(_P), _I, _I, _I, _I, _I, _P]),
    "rc_motion_search": (C.c_int, [_P, _P, C.POINTER(MotionDesc), _P, _I, _I, _P, _I, _I, _I, _P]),
    "rc_defect_desc_size": (_SZ, []),
    "rc_raw_defects": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(DefectDesc), _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    "rc_calib_desc_size": (_SZ, []),
    "rc_raw_calibrate": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(CalibDesc), _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "rc_hdr_desc_size": (_SZ, []),
    "rc_raw_hdr_merge": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(HdrDesc), _P, _I, _P, _I, _I, _I, _I, _P]),
    "rc_temporal_desc_size": (_SZ, []),
    "rc_raw_temporal": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(TemporalDesc), _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    "rc_raw_motion_pyramid": (C.c_int, [_P, C.POINTER(RawFormatDesc), _F, _P, _I, _I, C.POINTER(_P), _I, _I, _I, _P]),
    "rc_raw_temporal_mc": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(TemporalDesc), _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "rc_quad_desc_size": (_SZ, []),
    "rc_raw_quad": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(QuadDesc), _P, _I, _I, _I, _I, _P]),
    "rc_raw_stats_desc_size": (_SZ, []),
    "rc_raw_stats": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(RawStatsDesc), _P, _P, _I, _I, _I, _P]),
    "rc_raw_noise_desc_size": (_SZ, []),
    "rc_raw_noise": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(RawNoiseDesc), _P, _P, _I, _I, _I, _P]),
    "rc_ca_desc_size": (_SZ, []),
    "rc_raw_aberration": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(CaDesc), _P, _P, _I, _I, _I, _I, _P]),
    "rc_dng_desc_size": (_SZ, []),
    "rc_dng_plan": (C.c_int, [C.POINTER(DngDesc), C.POINTER(RawFormatDesc), _I, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(DngPlanInfo)]),
    "rc_dng_tile_header": (C.c_int, [C.POINTER(DngDesc), C.POINTER(RawFormatDesc), _P, _SZ, C.POINTER(_SZ)]),
    "rc_dng_encode": (C.c_int, [_P, C.POINTER(RawFormatDesc), C.POINTER(DngDesc), _P, C.c_longlong, C.c_longlong, C.c_longlong, _P, _P, _P, _I, _I, _I,
                                C.c_longlong, _P]),
    "rc_debug_dng_passes": (C.c_int, [_I]),
    "rc_nchw_to_nhwc": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_nhwc_to_nchw": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_conv_packed_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "rc_conv_pack_weights": (C.c_int, [_P, _I, _I, _I, _I, _I, _P]),
    "rc_conv_packed_cout": (C.c_int, [_I, _I, _I, _I, _I]),
    "rc_conv_pack_bias": (C.c_int, [_P, _I, _I, _I, _I, _I, _P]),
    "rc_conv_packed_bytes_ct": (_SZ, [_I, _I, _I, _I, _I, _I]),
    "rc_wino_packed_bytes": (_SZ, [_I, _I, _I]),
    "rc_wino_pack_weights": (C.c_int, [_P, _I, _I, _I, _P]),
    "rc_conv_packed_cout_ct": (C.c_int, [_I, _I, _I, _I, _I, _I]),
    "rc_conv_pack_weights_ct": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_conv_pack_bias_ct": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_conv_sum_tiles": (C.c_int, [_I, _I]),
    "rc_conv_sum_slots": (C.c_int, [_P]),
    "rc_conv2d": (C.c_int, [C.POINTER(ConvDesc), _P]),
    "rc_conv_desc_size": (_SZ, []),
    "rc_tail_fold_weights": (C.c_int, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "rc_tail_ring_gather": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_tail_ring_scatter": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_debug_stream_create_masked": (C.c_int, [_I, C.POINTER(C.c_void_p)]),
    "rc_debug_hbm_probe": (C.c_int, [_P, _P, C.c_size_t, _I, _I, _I, _I, _I, C.POINTER(C.c_double)]),
    "rc_debug_mfma_peak": (C.c_int, [_I, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rc_debug_mfma_peak32": (C.c_int, [_I, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rc_debug_poison_lds": (C.c_int, [C.c_uint, _P]),
    "rc_pointwise_chain48": (C.c_int, [_P, _I, _P, _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I, _F, _P, _I, C.c_longlong, _P]),
    "rc_lsc_packed_bytes": (C.c_size_t, [_I, _I, _I]),
    "rc_lsc_pack": (C.c_int, [_P, _P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I, _P, _P, _I, _I, _P]),
    "rc_lsc_chain": (C.c_int, [_P, _I, _P, _I, _I, _F, _P, _I, _P, _I, _I, _I, _P]),
    "rc_film_apply": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "rc_sigmoid_gate_add": (C.c_int, [_P, _P, _P, _P, _I, C.c_longlong, _P]),
    "rc_subsample2": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_entropy_bottleneck": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_longlong, _I, C.c_float, _P]),
    "rc_gaussian_conditional": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_longlong, C.c_float, C.c_float, _P]),
    "rc_tanh_half_add": (C.c_int, [_P, _P, _P, _I, C.c_longlong, _P]),
    "rc_upsample_bilinear2": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_sft_apply": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_longlong, _P]),
    "rc_space_to_depth2": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_pixel_shuffle2": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_pixel_shuffle2_nchw": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "rc_square": (C.c_int, [_P, _P, _I, C.c_longlong, _P]),
    "rc_gdn_apply": (C.c_int, [_P, _P, _P, _P, _I, _I, C.c_longlong, _P]),
    "rc_channel_copy": (C.c_int, [_P, _I, _I, _P, _I, _I, _I, C.c_longlong, _I, _P]),
    "rc_channel_concat": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), _I, _P, C.c_longlong, _I, _P]),
    "rc_window_attention": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_window_attention_planar8": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "rc_window_attention_planar8_ok": (C.c_int, [_I, _I, _I, _I, _I, _I]),
    "rc_conv_pair": (C.c_int, [C.POINTER(ConvPairDesc), _P]),
    "rc_conv_pair_sum_slots": (C.c_int, [_I, _I]),
    "rc_conv_pair_desc_size": (_SZ, []),
    "rc_ca_gate": (C.c_int, [_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "rc_ca_gate_ahead_scratch_floats": (_SZ, [_I, _I]),
    "rc_ca_gate_ahead": (C.c_int, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rc_gate_residual": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "rc_channel_sums_slots": (C.c_int, [_I]),
    "rc_channel_sums": (C.c_int, [_P, _I, _I, _I, _I, _P, _P]),
    "rc_dwt_forward": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_dwt_inverse": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_color_block": (C.c_int, [_P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "rc_instance_stats": (C.c_int, [_P, _P, _P, _I, _I, _I, _F, _P]),
    "rc_instance_norm": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rc_color_head": (C.c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "rc_gfm_vector": (C.c_int, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "rc_dwconv2d": (C.c_int, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "rc_layernorm": (C.c_int, [_P, _P, _I, C.c_longlong, _I, _P, _P, _F, _P]),
    "rc_gma_pointwise": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, C.c_longlong, _I, _P, _P, _P, _P, _P, _P, _P]),
    "rc_chain_packed_bytes": (_SZ, [_I, _I]),
    "rc_chain_packed_rows": (C.c_int, [_I]),
    "rc_chain_pack_weights": (C.c_int, [_P, _I, _I, _P]),
    "rc_chain_pack_bias": (C.c_int, [_P, _I, _P]),
    "rc_gma_ln_qkv": (C.c_int, [_P, _P, C.c_longlong, _P, _P, _P, _P, _F, _P]),
    "rc_gma_tail": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "rc_gma_aggregate": (C.c_int, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rc_chain_pack_weights_natural": (C.c_int, [_P, _I, _I, _P]),
    "rc_gma_toeplitz_bytes": (_SZ, []),
    "rc_gma_toeplitz_pack": (C.c_int, [_P, _P, _P, _P, _P]),
    "rc_dw_toeplitz_pack": (C.c_int, [_P, _I, _I, _P]),
    "rc_gma_in_cpe": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "rc_gma_qkv_aggregate": (C.c_int, [_P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rc_cat_linear": (C.c_int, [_P, _P, _P, _P, _P, C.c_longlong, _I, _P, _P, _P]),
    "rc_gdn_chain": (C.c_int, [_P, _P, _P, C.c_longlong, _I, _P, _P, _I, _P]),
    "rc_ln_linear": (C.c_int, [_P, _P, C.c_longlong, _I, _I, _P, _P, _P, _P, _F, _P]),
    "rc_ln_linear_planar8": (C.c_int, [_P, _P, C.c_longlong, _I, _I, _P, _P, _P, _P, _F, _P]),
    "rc_ln_mlp": (C.c_int, [_P, _P, C.c_longlong, _I, _P, _P, _P, _P, _P, _P, _F, _P]),
    "rc_gma_kv_mfma_blocks": (C.c_int, [_I]),
    "rc_gma_kv_mfma_scratch_bytes": (C.c_size_t, [_I, _I]),
    "rc_gma_kv_mfma": (C.c_int, [_P, _I, _I, _F, _P, _P, _P, _P]),
    "rc_gma_crpe": (C.c_int, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "rc_gma_kv_blocks": (C.c_int, [_I]),
    "rc_gma_kv_scratch_bytes": (_SZ, [_I, _I, _I, _I]),
    "rc_gma_kv": (C.c_int, [_P, _I, _I, _I, _I, _I, _F, _P, _P, _P]),
    "rc_gma_kv_planar": (C.c_int, [_P, _I, _I, _I, _I, _F, _P, _P, _P]),
    "rc_gma_apply": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "rc_pmf_to_quantized_cdf": (C.c_int, [_P, _I, _I, _P]),
    "rc_gc_symbols": (C.c_int, [_P, _P, _P, _I, _I, C.c_longlong, _I, _P, _I, _F, _P, _P, _P, _P]),
    "rc_gc_dequantize": (C.c_int, [_P, _P, _I, _I, C.c_longlong, _I, _P, _P]),
    "rc_eb_symbols": (C.c_int, [_P, _P, _I, _I, C.c_longlong, _I, _I, _P, _P, _P, _P]),
    "rc_rans_chunk_words": (C.c_int, [_I]),
    "rc_rans_encode_scratch_bytes": (_SZ, [C.c_longlong, _I]),
    "rc_rans_encode_chunks": (C.c_int, [_P, _P, C.c_longlong, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "rc_debug_rans_rcp_selftest": (C.c_longlong, [C.c_longlong, C.c_ulonglong]),
    "rc_rans_compact": (C.c_int, [_P, _I, _P, _P, C.c_longlong, _P, _P]),
    "rc_rans_decode_chunks": (C.c_int, [_P, C.c_longlong, _P, _P, C.c_longlong, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "rc_rans_encode_host": (C.c_longlong, [_P, _P, C.c_longlong, _P, _I, _I, _P, _P, _P, C.c_longlong]),
    "rc_rans_decode_host": (C.c_int, [_P, C.c_longlong, _P, _P, C.c_longlong, _P, _I, _I, _P, _P, _P]),
    "rc_debug_set": (C.c_int, [C.c_char_p, _I]),
    "rc_debug_get": (C.c_int, [C.c_char_p]),
    "rc_debug_set_ptr": (C.c_int, [C.c_char_p, _P]),
    "rc_prof_enable": (C.c_int, [_I]),
    "rc_prof_collect": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rc_prof_collect_rows": (C.c_int, [_P, _I, C.POINTER(C.c_int)]),
}

_lib = None
_knobs = {}


def knob(key: bytes) -> int:
    """rc_debug_get(key), cached until the knob is set again (rc_debug_set through this binding drops the cached value)."""
    v = _knobs.get(key)
    if v is None:
        v = _knobs[key] = load().rc_debug_get(key)
    return v


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m realcamnet_amd.build` (hipcc, gfx950). "
            "There is no CPU / PyTorch fallback for the HIP path.")
    lib = C.CDLL(os.fspath(LIB_PATH))
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{LIB_PATH.name} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.rc_abi_version() != ABI_VERSION:
        raise RuntimeError(f"ABI mismatch: library {lib.rc_abi_version()} vs binding {ABI_VERSION}")
    # rc_debug_get is asked on every conv (pack-cache key): mirror the knobs here and invalidate the mirror whenever one is set through this binding
    raw_set = lib.rc_debug_set

    def _set(key, value):
        _knobs.pop(bytes(key), None)
        return raw_set(key, value)
    lib.rc_debug_set = _set
    _lib = lib
    # kernel experiments only: RC_DEBUG="key=value,key=value" applies rc_debug_set knobs at load (A/B runs of bench.py without code edits)
    for kv in filter(None, os.environ.get("RC_DEBUG", "").split(",")):
        k, _, v = kv.partition("=")
        if lib.rc_debug_set(k.strip().encode(), int(v or "1")) != 0:
            raise RuntimeError(f"RC_DEBUG: unknown knob {k!r}")
    return lib


class HipError(RuntimeError):
    pass


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = load().rc_last_error().decode(errors="replace")
        raise HipError(f"{what or 'librealcam_hip'} failed ({code}): {msg}")
