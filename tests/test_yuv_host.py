"""CPU: the video-encoder output of forward_mosaic (include/realcam_hip.h rc_out_format / rc_yuv_frame_bytes / rc_yuv_encode).
OutFormat and its plane layout, the ctypes mirror, the argument checks made before any launch, the kernels' resources, fake-tensor
traces, and the elementwise torch restatement of the fixed arithmetic that the GPU tests use as their yardstick (checked here
against the colour-bar codes of the standards)."""
import ctypes as C

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F32

# ---- the yardstick: the header's arithmetic as plain elementwise torch ops, one rounding per op, in the order written -------------------
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def restated_codes(y, fmt, crop_hw=None, dtype=torch.float32):
    """Planar (B,3,H,W) -> integer codes (int32, before the P010 shift): Y (B,h,w), Cb, Cr (B,h/2,w/2).  dtype float32 restates the
    kernel; float64 is the same chain without fp32 rounding (constants included)."""
    h, w = crop_hw if crop_hw is not None else y.shape[2:]
    x = y[:, :, :h, :w].cpu().to(dtype)
    x = torch.where(torch.isnan(x), torch.zeros((), dtype=dtype), x).clamp(0.0, 1.0)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    kr, kb = KR_KB[fmt.matrix]
    t = lambda v: torch.tensor(v, dtype=dtype)                       # a double rounded to `dtype` once
    yy = ((t(kr) * r) + (t(1.0 - kr - kb) * g)) + (t(kb) * b)
    cb = (b - yy) * t(0.5 / (1.0 - kb))
    cr = (r - yy) * t(0.5 / (1.0 - kr))

    def sub(c):
        if fmt.chroma_siting == "center":
            return ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * t(0.25)
        left = torch.cat([c[..., :1], c[..., :-1]], -1)               # c[x - 1], clamped to column 0
        tt = ((left[..., 0::2] + c[..., 1::2]) + (c[..., 0::2] + c[..., 0::2])) * t(0.25)
        return (tt[:, 0::2] + tt[:, 1::2]) * t(0.5)

    n = fmt.bits
    k = float(1 << (n - 8))
    top = float((1 << n) - 1)
    if fmt.range == "limited":
        qy, qc = (219 * k, 16 * k, 16 * k, 235 * k), (224 * k, 128 * k, 16 * k, 240 * k)
    else:
        qy, qc = (top, 0.0, 0.0, top), (top, float(1 << (n - 1)), 0.0, top)
    q = lambda v, p: ((v * t(p[0])) + t(p[1])).round().clamp(p[2], p[3]).to(torch.int32)
    return q(yy, qy), q(sub(cb), qc), q(sub(cr), qc)


def restated_frames(y, fmt, crop_hw=None):
    """The whole (B, frame_elems) buffer ops.yuv_encode returns, padding included (zero), from restated_codes and plane_layout."""
    h, w = crop_hw if crop_hw is not None else y.shape[2:]
    pl = fmt.plane_layout(h, w)
    sh = 6 if fmt.layout == "p010" else 0
    yc, cb, cr = (c << sh for c in restated_codes(y, fmt, (h, w)))
    parts = {"y": yc, "cb": cb, "cr": cr, "cbcr": torch.stack([cb, cr], -1).flatten(2)}
    es = pl.elem_bytes
    buf = torch.zeros(y.shape[0], pl.frame_bytes // es, dtype=torch.int32)
    for p in pl.planes:
        v = buf[:, p.offset // es:(p.offset + p.pitch * p.alloc_rows) // es].unflatten(1, (p.alloc_rows, p.pitch // es))
        v[:, :p.rows, :p.valid_bytes // es] = parts[p.name]
    return buf.to(torch.uint8) if es == 1 else buf.to(torch.uint16)


# 100 % colour bars white, yellow, cyan, green, magenta, red, blue, black: limited-range (Y, Cb, Cr) codes at 8 and 10 bits
BARS_RGB = [(1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (1, 0, 1), (1, 0, 0), (0, 0, 1), (0, 0, 0)]
BARS = {
    ("bt601", 8): [(235, 128, 128), (210, 16, 146), (170, 166, 16), (145, 54, 34), (106, 202, 222), (81, 90, 240), (41, 240, 110), (16, 128, 128)],
    ("bt601", 10): [(940, 512, 512), (840, 64, 585), (678, 663, 64), (578, 215, 137), (426, 809, 887), (326, 361, 960), (164, 960, 439), (64, 512, 512)],
    ("bt709", 8): [(235, 128, 128), (219, 16, 138), (188, 154, 16), (173, 42, 26), (78, 214, 230), (63, 102, 240), (32, 240, 118), (16, 128, 128)],
    ("bt709", 10): [(940, 512, 512), (877, 64, 553), (754, 615, 64), (691, 167, 105), (313, 857, 919), (250, 409, 960), (127, 960, 471), (64, 512, 512)],
    ("bt2020", 8): [(235, 128, 128), (222, 16, 137), (177, 159, 16), (164, 47, 25), (87, 209, 231), (74, 97, 240), (29, 240, 119), (16, 128, 128)],
    ("bt2020", 10): [(940, 512, 512), (888, 64, 548), (710, 637, 64), (658, 189, 100), (346, 835, 924), (294, 387, 960), (116, 960, 476), (64, 512, 512)],
}


def bars_image(bar_w=16, bar_h=4, dtype=torch.float32):
    """(1,3,bar_h,8*bar_w): the eight bars side by side."""
    cols = torch.tensor(BARS_RGB, dtype=torch.float32).t()            # (3, 8)
    return cols[:, None, :, None].expand(3, bar_h, 8, bar_w).reshape(1, 3, bar_h, 8 * bar_w).to(dtype).contiguous()


@pytest.mark.parametrize("matrix", sorted(KR_KB))
@pytest.mark.parametrize("layout", ("nv12", "p010"))
def test_restatement_gives_the_standard_colour_bar_codes(matrix, layout):
    for siting in ("left", "center"):
        fmt = M.OutFormat(layout, matrix=matrix, chroma_siting=siting)
        for dtype in (torch.float32, torch.float64):
            yc, cb, cr = restated_codes(bars_image(), fmt, dtype=dtype)
            for i, want in enumerate(BARS[matrix, fmt.bits]):
                # inside a bar (for "left", its first chroma column sees the bar to the left)
                assert (int(yc[0, 1, 16 * i + 5]), int(cb[0, 1, 8 * i + 3]), int(cr[0, 1, 8 * i + 3])) == want, (matrix, layout, siting, i)


# ---- OutFormat ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(layout="nv21"), dict(layout="NV12"), dict(layout=0), dict(matrix="bt470"), dict(range="video"), dict(chroma_siting="top"),
    dict(pitch_align=0), dict(pitch_align=48), dict(pitch_align=-64), dict(pitch_align=64.0), dict(pitch_align=True),
    dict(height_align=0), dict(height_align=1.5),
])
def test_out_format_rejects(kw):
    with pytest.raises(ValueError):
        M.OutFormat(**kw)


def test_out_format_defaults_and_frozen():
    f = M.OutFormat()
    assert (f.layout, f.matrix, f.range, f.chroma_siting, f.pitch_align, f.height_align) == ("nv12", "bt709", "limited", "left", 1, 1)
    assert M.OutFormat("p010").bits == 10 and f.bits == 8
    with pytest.raises(Exception):
        f.layout = "i420"
    assert f == M.OutFormat("nv12") and hash(f) == hash(M.OutFormat("nv12"))
    for bad in ((7, 8), (8, 7), (0, 8), (8, 0), (8.0, 8)):
        with pytest.raises(ValueError):
            f.plane_layout(*bad)


def test_plane_layout_hand_computed():
    # 4K NV12, pitch to 256 bytes, height to 16 rows: 3840 = 15 x 256 and 2160 = 135 x 16 stay as they are
    pl = M.OutFormat("nv12", pitch_align=256, height_align=16).plane_layout(2160, 3840)
    assert pl.pitch == 3840 and pl.frame_bytes == 3840 * 2160 * 3 // 2 == 12441600 and pl.planes[1].offset == 3840 * 2160
    # ... and height to 64 rows (HEVC coding tree blocks): 2160 -> 2176
    pl = M.OutFormat("nv12", pitch_align=256, height_align=64).plane_layout(2160, 3840)
    assert pl.pitch == 3840 and pl.elem_bytes == 1 and pl.frame_bytes == 3840 * 2176 * 3 // 2 == 12533760
    y, c = pl.planes
    assert y == ("y", 0, 3840, 2160, 3840, 2176) and c == ("cbcr", 3840 * 2176, 3840, 1080, 3840, 1088)
    # 1080p NV12 the same way: 1920 -> 2048 bytes, 1080 -> 1088 rows
    pl = M.OutFormat("nv12", pitch_align=256, height_align=16).plane_layout(1080, 1920)
    assert pl.pitch == 2048 and pl.planes[1].offset == 2048 * 1088 and pl.frame_bytes == 2048 * (1088 + 544)
    # I420 with an odd half width: w = 154 -> 77 chroma bytes; tight: pitch 154, chroma pitch 77
    pl = M.OutFormat("i420").plane_layout(70, 154)
    assert pl.pitch == 154 and [tuple(p) for p in pl.planes] == [("y", 0, 154, 70, 154, 70), ("cb", 10780, 77, 35, 77, 35), ("cr", 10780 + 2695, 77, 35, 77, 35)]
    assert pl.frame_bytes == 10780 + 2 * 2695
    # ... and aligned to 64: the Y pitch goes to 2 x 64 so that the chroma pitch is a multiple of 64 too
    pl = M.OutFormat("i420", pitch_align=64, height_align=16).plane_layout(70, 154)
    assert pl.pitch == 256 and pl.planes[1].pitch == 128 and pl.planes[0].alloc_rows == 80 and pl.planes[1].alloc_rows == 40
    assert pl.planes[1].offset == 256 * 80 and pl.planes[2].offset == 256 * 80 + 128 * 40 and pl.frame_bytes == 256 * 80 + 2 * 128 * 40
    # P010: the pitch is in bytes, two per sample
    pl = M.OutFormat("p010").plane_layout(70, 154)
    assert pl.pitch == 308 and pl.elem_bytes == 2 and pl.planes[0].valid_bytes == 308 and pl.planes[1] == ("cbcr", 308 * 70, 308, 35, 308, 35)
    assert pl.frame_bytes == 308 * 105
    pl = M.OutFormat("p010", pitch_align=256).plane_layout(2160, 3840)
    assert pl.pitch == 7680 and pl.frame_bytes == 7680 * 3240
    # an odd height alignment: 70 -> 75 Y rows, ceil(75 / 2) chroma rows
    pl = M.OutFormat("nv12", height_align=25).plane_layout(70, 16)
    assert pl.planes[0].alloc_rows == 75 and pl.planes[1].alloc_rows == 38 and pl.frame_bytes == 16 * (75 + 38)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def _desc(layout=_lib.RC_YUV_NV12, matrix=_lib.RC_MATRIX_BT709, vrange=0, siting=0, pitch=0, rows=0, c0=0, c1=0):
    d = _lib.OutFormatDesc(layout=layout, matrix=matrix, range=vrange, siting=siting, pitch=pitch, rows=rows)
    d.chroma_offset[0], d.chroma_offset[1] = c0, c1
    return d


def test_out_format_struct_matches_header_and_symbols_exported():
    lib = _lib.load()
    assert lib.rc_out_format_size() == C.sizeof(_lib.OutFormatDesc) == 48
    for name in ("rc_out_format_size", "rc_yuv_frame_bytes", "rc_yuv_encode"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15


@pytest.mark.parametrize("fmt,h,w", [
    (M.OutFormat("nv12"), 70, 154), (M.OutFormat("nv12", pitch_align=256, height_align=64), 2160, 3840),
    (M.OutFormat("p010", pitch_align=64, height_align=8), 70, 154), (M.OutFormat("i420"), 70, 154),
    (M.OutFormat("i420", pitch_align=64, height_align=16), 70, 154), (M.OutFormat("nv12", height_align=25), 70, 16),
])
def test_library_plans_the_frame_plane_layout_states(fmt, h, w):
    from realcamnet_amd.out_format import LAYOUTS
    pl = fmt.plane_layout(h, w)
    d = _desc(layout=LAYOUTS[fmt.layout], pitch=pl.pitch, rows=pl.planes[0].alloc_rows)
    assert _lib.load().rc_yuv_frame_bytes(C.byref(d), h, w) == pl.frame_bytes
    tight = _desc(layout=LAYOUTS[fmt.layout])                        # pitch 0 / rows 0: the tight frame
    assert _lib.load().rc_yuv_frame_bytes(C.byref(tight), h, w) == M.OutFormat(fmt.layout).plane_layout(h, w).frame_bytes


FAKE = 1 << 20           # a non-null, 16-byte aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"),
    ("null format", dict(fmt=None), b"null"),
    ("null dst", dict(dst=None), b"null"),
    ("bad dtype", dict(dtype=_lib.RC_U16), b"dtype"),
    ("crop beyond the source", dict(h=18), b"bad shape"),
    ("odd h", dict(h=7), b"even"),
    ("odd w", dict(w=15), b"even"),
    ("unknown layout", dict(fmt=_desc(layout=3)), b"layout"),
    ("unknown matrix", dict(fmt=_desc(matrix=3)), b"matrix"),
    ("unknown range", dict(fmt=_desc(vrange=2)), b"range"),
    ("unknown siting", dict(fmt=_desc(siting=-1)), b"siting"),
    ("pitch below the row (nv12)", dict(fmt=_desc(pitch=15)), b"pitch shorter"),
    ("pitch below the row (p010: 2 bytes a sample)", dict(fmt=_desc(layout=_lib.RC_YUV_P010, pitch=30)), b"pitch shorter"),
    ("odd pitch (p010)", dict(fmt=_desc(layout=_lib.RC_YUV_P010, pitch=33)), b"multiple"),
    ("odd pitch (i420)", dict(fmt=_desc(layout=_lib.RC_YUV_I420, pitch=17)), b"multiple"),
    ("rows below h", dict(fmt=_desc(rows=14)), b"rows"),
    ("chroma inside Y", dict(fmt=_desc(c0=16 * 16 - 1)), b"overlap"),
    ("Cr inside Y (i420)", dict(fmt=_desc(layout=_lib.RC_YUV_I420, c0=256, c1=255)), b"overlap"),
    ("Cr inside Cb (i420)", dict(fmt=_desc(layout=_lib.RC_YUV_I420, c0=256, c1=256 + 63)), b"overlap"),
    ("Cb inside Cr (i420, planes swapped)", dict(fmt=_desc(layout=_lib.RC_YUV_I420, c0=256 + 63, c1=256)), b"overlap"),
    ("Cr offset for nv12", dict(fmt=_desc(c1=512)), b"chroma_offset"),
    ("odd chroma offset (p010)", dict(fmt=_desc(layout=_lib.RC_YUV_P010, c0=32 * 16 + 1)), b"multiple"),
    ("dst misaligned", dict(dst=FAKE + 8), b"16-byte"),
    ("src misaligned", dict(src=FAKE + 2), b"misaligned"),
])
def test_yuv_encode_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, dtype=RC_F32, fmt=_desc(), dst=FAKE, b=1, H=16, W=16, h=16, w=16)
    kw.update(kwargs)
    lib = _lib.load()
    fmt = None if kw["fmt"] is None else C.byref(kw["fmt"])
    assert lib.rc_yuv_encode(kw["src"], kw["dtype"], fmt, kw["dst"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None) == -1, case
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())
    if msg in (b"even", b"pitch shorter", b"multiple", b"rows", b"overlap", b"chroma_offset", b"layout"):     # the surface plan's own refusals
        assert lib.rc_yuv_frame_bytes(fmt, kw["h"], kw["w"]) == 0 and msg in lib.rc_last_error(), case


def test_reserved_fields_must_be_zero():
    d = _desc()
    d.reserved[2] = 1
    assert _lib.load().rc_yuv_encode(FAKE, RC_BF16, C.byref(d), FAKE, 1, 16, 16, 16, 16, None) == -1 and b"reserved" in _lib.load().rc_last_error()


# ---- kernels and traces ---------------------------------------------------------------------------------------------------------------
def test_yuv_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "yuv420_kernel" in k}
    assert len(mine) == 18, sorted(mine)                              # 3 source types x 3 layouts x 2 sitings
    assert all(v["tu"] == "yuv_encode.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0) or v.get("lds", 0)]
    assert not [k for k, v in res.items() if v["tu"] == "yuv_encode.hip" and k not in mine]


def test_python_and_ops_refuse_before_any_launch():
    from realcamnet_amd import ops
    with pytest.raises(TypeError):
        ops.yuv_encode(torch.zeros(1, 3, 8, 8), "nv12")
    with pytest.raises(Exception):
        ops.yuv_encode(torch.zeros(1, 3, 8, 8), M.OutFormat())      # a CPU tensor: there is no CPU path
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 16, 32)
            for bad in ((15, 32), (16, 31), (18, 32), (16, 34)):
                with pytest.raises(ValueError):
                    ops.yuv_encode(y, M.OutFormat(), crop_hw=bad)
            with pytest.raises(ValueError):
                ops.yuv_encode(torch.empty(2, 4, 16, 32), M.OutFormat())
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            with torch.no_grad():
                for bad in (8, ("nv12",), M.RawFormat()):
                    with pytest.raises(TypeError):
                        net.forward_mosaic(mosaic, None, coord, out_format=bad)
                for bad in ("nv12", "rgb10", "yuv"):                   # a layout name is not a format: OutFormat("nv12") is
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, out_format=bad)


def test_fake_trace_of_yuv_forwards():
    """forward_mosaic(out_format=OutFormat(...)) under FakeTensorMode: the buffer's and the plane views' shapes, dtypes and device for a DWT
    net, a strided net and the GroupMix net; the codec refuses."""
    import realcamnet_amd.raw2bit as RB
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC", "LiteISPNet_GFM_LSC_GMA"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        out = net.forward_mosaic(mosaic, None, coord, out_format=M.OutFormat("nv12"))
                        assert isinstance(out, M.YuvFrames) and out.buffer.shape == (2, 208 * 216) and out.buffer.dtype == torch.uint8, name
                        assert out.buffer.device.type == "cuda" and len(out.planes) == 2
                        assert out.planes[0].shape == (2, 144, 208) and out.planes[1].shape == (2, 72, 104, 2)
                        out = net.forward_mosaic(mosaic, None, coord, out_format=M.OutFormat("p010", pitch_align=256, height_align=16))
                        assert out.buffer.shape == (2, 256 * 216) and out.buffer.dtype == torch.uint16          # 416 -> 512 bytes = 256 samples
                        assert out.planes[0].shape == (2, 144, 208) and out.planes[0].stride() == (256 * 216, 256, 1)
                        assert out.planes[1].shape == (2, 72, 104, 2) and out.planes[1].dtype == torch.uint16
                        out = net.forward_mosaic(mosaic, None, coord, out_format=M.OutFormat("i420", matrix="bt601", range="full", chroma_siting="center"))
                        assert out.buffer.shape == (2, 208 * 216) and [tuple(p.shape) for p in out.planes] == [(2, 144, 208), (2, 72, 104), (2, 72, 104)]
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with torch.no_grad():
                    with pytest.raises(ValueError):
                        codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), out_format=M.OutFormat("nv12"))
                buf = torch.ops.realcam.yuv_encode(torch.empty(3, 3, 80, 160, dtype=torch.float16), _lib.RC_YUV_I420, 0, 1, 1, 256, 80, 70, 154)
                assert buf.shape == (3, 256 * 80 + 2 * 128 * 40) and buf.dtype == torch.uint8
    finally:
        torch.set_default_dtype(old)
