"""CPU: the professional video surfaces of rc_yuv_encode (the layouts from RC_YUV_NV16 on: 4:2:2, 4:4:4, planar 10 bit, packed, v210).
OutFormat and its plane layouts written out by hand, the library's plan against them, the argument checks made before any launch, the
NumPy restatement (yuv_surface_ref.py) against float64, its packers against their unpackers, the kernels' resources and fake-tensor
traces."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
import yuv_surface_ref as R
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_F32
from realcamnet_amd.out_format import LAYOUTS, frame_layout

NEW = ("nv16", "p210", "i422", "i210", "i010", "i444", "i410", "yuy2", "uyvy", "y210", "v210")
SUB = {"nv16": "422", "p210": "422", "i422": "422", "i210": "422", "i010": "420", "i444": "444", "i410": "444", "yuy2": "422", "uyvy": "422",
       "y210": "422", "v210": "422"}
BITS = {"nv16": 8, "p210": 10, "i422": 8, "i210": 10, "i010": 10, "i444": 8, "i410": 10, "yuy2": 8, "uyvy": 8, "y210": 10, "v210": 10}


# ---- OutFormat --------------------------------------------------------------------------------------------------------------------------
def test_out_format_accepts_the_new_names_and_numbers_them_from_16():
    assert tuple(R.NEW) == NEW
    for i, name in enumerate(NEW):
        f = M.OutFormat(name)
        assert LAYOUTS[name] == 16 + i and f.subsampling == SUB[name] and f.bits == BITS[name], name
        assert f.elem_bytes == (1 if name == "v210" else (BITS[name] + 7) // 8), name
    assert [LAYOUTS[n] for n in ("nv12", "p010", "i420")] == [0, 1, 2]
    assert [M.OutFormat(n).subsampling for n in ("nv12", "p010", "i420")] == ["420"] * 3
    assert (_lib.RC_YUV_NV16, _lib.RC_YUV_I010, _lib.RC_YUV_V210) == (16, 20, 26)


@pytest.mark.parametrize("name", ("nv21", "nv61", "YUY2", "V210", "I422", "y410", "ayuv", 16))
def test_out_format_rejects_other_names(name):
    with pytest.raises(ValueError):
        M.OutFormat(name)


@pytest.mark.parametrize("name", NEW)
def test_size_rule_per_layout(name):
    f = M.OutFormat(name)
    sub = SUB[name]
    f.plane_layout(6, 8)
    for hw, ok in (((5, 8), sub != "420"), ((6, 7), sub == "444"), ((5, 7), sub == "444"), ((1, 2), sub != "420"), ((1, 1), sub == "444")):
        if ok:
            f.plane_layout(*hw)
        else:
            with pytest.raises(ValueError) as e:
                f.plane_layout(*hw)
            assert ("4:2:0 needs an even height and width" if sub == "420" else "4:2:2") in str(e.value)
    for bad in ((0, 8), (8, 0), (8.0, 8), (True, 8)):
        with pytest.raises(ValueError):
            f.plane_layout(*bad)


def test_output_applies_each_layouts_own_rule():
    M.Output(M.OutFormat("uyvy"), M.Resize((35, 52)))                       # 4:2:2: an odd height is fine
    M.Output(M.OutFormat("i444"), M.Resize((35, 51)))                       # 4:4:4: any size
    with pytest.raises(ValueError, match="4:2:2 .uyvy. needs an even width"):
        M.Output(M.OutFormat("uyvy"), M.Resize((36, 51)))
    with pytest.raises(ValueError, match="4:2:0 .i010. needs an even height and width"):
        M.Output(M.OutFormat("i010"), M.Resize((35, 52)))
    with pytest.raises(ValueError, match="4:2:0 .nv12. needs an even height and width, Resize.size is"):
        M.Output(M.OutFormat("nv12"), M.Resize((35, 52)))
    assert M.Output(M.OutFormat("v210"), M.Resize((35, 52))).plan(144, 208) == (35, 52)
    with pytest.raises(ValueError):
        M.Output(M.OutFormat("v210")).plan(144, 207)


def test_plane_layout_hand_computed():
    t = lambda pl: [tuple(p) for p in pl.planes]
    # semi-planar 4:2:2: the CbCr plane has as many rows as Y
    pl = M.OutFormat("nv16").plane_layout(70, 154)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (154, 21560, 1) and t(pl) == [("y", 0, 154, 70, 154, 70), ("cbcr", 10780, 154, 70, 154, 70)]
    pl = M.OutFormat("p210", pitch_align=256, height_align=16).plane_layout(2160, 3840)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (7680, 33177600, 2) and t(pl) == [("y", 0, 7680, 2160, 7680, 2160), ("cbcr", 16588800, 7680, 2160, 7680, 2160)]
    pl = M.OutFormat("p210").plane_layout(70, 154)
    assert pl.pitch == 308 and pl.frame_bytes == 43120 and pl.planes[1] == ("cbcr", 21560, 308, 70, 308, 70)
    # planar 4:2:2: chroma pitch = pitch / 2, `rows` chroma rows
    pl = M.OutFormat("i422").plane_layout(70, 154)
    assert (pl.pitch, pl.frame_bytes) == (154, 21560) and t(pl) == [("y", 0, 154, 70, 154, 70), ("cb", 10780, 77, 70, 77, 70), ("cr", 16170, 77, 70, 77, 70)]
    pl = M.OutFormat("i422", pitch_align=64, height_align=16).plane_layout(70, 154)             # 154 -> 2 x 64 x 2 = 256, chroma 128; 70 -> 80 rows
    assert (pl.pitch, pl.frame_bytes) == (256, 40960) and t(pl) == [("y", 0, 256, 70, 154, 80), ("cb", 20480, 128, 70, 77, 80), ("cr", 30720, 128, 70, 77, 80)]
    pl = M.OutFormat("i210").plane_layout(70, 154)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (308, 43120, 2) and t(pl) == [("y", 0, 308, 70, 308, 70), ("cb", 21560, 154, 70, 154, 70), ("cr", 32340, 154, 70, 154, 70)]
    pl = M.OutFormat("i210", pitch_align=256).plane_layout(2160, 3840)
    assert (pl.pitch, pl.frame_bytes) == (7680, 33177600) and pl.planes[1] == ("cb", 16588800, 3840, 2160, 3840, 2160) and pl.planes[2].offset == 24883200
    # planar 10-bit 4:2:0: i420's numbers in 2-byte samples
    pl = M.OutFormat("i010").plane_layout(70, 154)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (308, 32340, 2) and t(pl) == [("y", 0, 308, 70, 308, 70), ("cb", 21560, 154, 35, 154, 35), ("cr", 26950, 154, 35, 154, 35)]
    pl = M.OutFormat("i010", pitch_align=256, height_align=64).plane_layout(2160, 3840)          # 2160 -> 2176 rows, 1088 chroma rows
    assert (pl.pitch, pl.frame_bytes) == (7680, 25067520) and pl.planes[1] == ("cb", 16711680, 3840, 1080, 3840, 1088) and pl.planes[2].offset == 20889600
    # 4:4:4: three planes at one pitch
    pl = M.OutFormat("i444").plane_layout(70, 154)
    assert (pl.pitch, pl.frame_bytes) == (154, 32340) and t(pl) == [("y", 0, 154, 70, 154, 70), ("cb", 10780, 154, 70, 154, 70), ("cr", 21560, 154, 70, 154, 70)]
    pl = M.OutFormat("i444").plane_layout(69, 153)
    assert (pl.pitch, pl.frame_bytes) == (153, 31671)
    pl = M.OutFormat("i410", pitch_align=256).plane_layout(2160, 3840)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (7680, 49766400, 2) and pl.planes[2] == ("cr", 33177600, 7680, 2160, 7680, 2160)
    # packed 4:2:2: one plane of 2 w samples
    for name in ("yuy2", "uyvy"):
        pl = M.OutFormat(name).plane_layout(70, 154)
        assert (pl.pitch, pl.frame_bytes, len(pl.planes)) == (308, 21560, 1) and pl.planes[0][1:] == (0, 308, 70, 308, 70)
        pl = M.OutFormat(name, pitch_align=256).plane_layout(2160, 3840)
        assert (pl.pitch, pl.frame_bytes) == (7680, 16588800)
    assert M.OutFormat("yuy2").plane_layout(70, 154).planes[0].name == "yuyv" and M.OutFormat("uyvy").plane_layout(70, 154).planes[0].name == "uyvy"
    pl = M.OutFormat("y210", pitch_align=64, height_align=4).plane_layout(70, 154)               # 616 -> 640 bytes, 70 -> 72 rows
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (640, 46080, 2) and t(pl) == [("yuyv", 0, 640, 70, 616, 72)]
    # v210: ceil(w / 48) x 128 bytes a row, ceil(w / 6) x 16 of them groups; the buffer is bytes
    pl = M.OutFormat("v210", pitch_align=256).plane_layout(2160, 3840)
    assert (pl.pitch, pl.frame_bytes, pl.elem_bytes) == (10240, 22118400, 1) and t(pl) == [("v210", 0, 10240, 2160, 10240, 2160)]
    pl = M.OutFormat("v210").plane_layout(720, 1280)                                              # 27 x 128 = 3456; 214 groups = 3424 bytes
    assert (pl.pitch, pl.frame_bytes) == (3456, 2488320) and t(pl) == [("v210", 0, 3456, 720, 3424, 720)]
    pl = M.OutFormat("v210").plane_layout(70, 154)                                                # 4 x 128; 26 groups (154 = 25 x 6 + 4)
    assert (pl.pitch, pl.frame_bytes) == (512, 35840) and t(pl) == [("v210", 0, 512, 70, 416, 70)]
    assert M.OutFormat("v210", pitch_align=1024).pitch(154) == 1024 and M.OutFormat("v210").pitch(1280) == 3456 and M.OutFormat("v210").pitch(3840) == 10240


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def _desc(layout, matrix=_lib.RC_MATRIX_BT709, vrange=0, siting=0, pitch=0, rows=0, c0=0, c1=0):
    d = _lib.OutFormatDesc(layout=layout, matrix=matrix, range=vrange, siting=siting, pitch=pitch, rows=rows)
    d.chroma_offset[0], d.chroma_offset[1] = c0, c1
    return d


def test_abi_version_and_struct_stay():
    lib = _lib.load()
    assert lib.rc_out_format_size() == C.sizeof(_lib.OutFormatDesc) == 48 and _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15


@pytest.mark.parametrize("name", NEW)
def test_library_plans_the_frame_plane_layout_states(name):
    lib = _lib.load()
    for h, w in ((70, 154), (2160, 3840)) + (() if SUB[name] == "420" else ((5, 22),)) + (((7, 5),) if SUB[name] == "444" else ()):
        for fmt in (M.OutFormat(name, pitch_align=64, height_align=16), M.OutFormat(name, pitch_align=256, height_align=25)):
            pl = fmt.plane_layout(h, w)
            d = _desc(LAYOUTS[name], pitch=pl.pitch, rows=pl.planes[0].alloc_rows)
            assert lib.rc_yuv_frame_bytes(C.byref(d), h, w) == pl.frame_bytes, (name, h, w, lib.rc_last_error())
        tight = lib.rc_yuv_frame_bytes(C.byref(_desc(LAYOUTS[name])), h, w)                        # pitch 0 / rows 0: the tight frame
        if name == "v210":                                                                        # the C entry's tight row is the groups' bytes
            assert tight == -(-w // 6) * 16 * h
            pl = frame_layout(LAYOUTS[name], -(-w // 6) * 16, h, h, w)
        else:
            pl = M.OutFormat(name).plane_layout(h, w)
        assert tight == pl.frame_bytes, (name, h, w)


FAKE = 1 << 20           # a non-null, 16-byte aligned address that is never dereferenced: every case below fails before a launch
L = _lib


@pytest.mark.parametrize("case,kwargs,msg", [
    ("unknown layout 3", dict(fmt=_desc(3)), b"layout"),
    ("unknown layout 15", dict(fmt=_desc(15)), b"layout"),
    ("unknown layout 27", dict(fmt=_desc(27)), b"layout"),
    ("unknown matrix", dict(fmt=_desc(L.RC_YUV_V210, matrix=3)), b"matrix"),
    ("unknown siting (4:4:4 too)", dict(fmt=_desc(L.RC_YUV_I444, siting=2)), b"siting"),
    ("odd w (nv16)", dict(fmt=_desc(L.RC_YUV_NV16), w=15), b"even width"),
    ("odd w (i210)", dict(fmt=_desc(L.RC_YUV_I210), w=15), b"even width"),
    ("odd w (yuy2)", dict(fmt=_desc(L.RC_YUV_YUY2), w=15), b"even width"),
    ("odd w (v210)", dict(fmt=_desc(L.RC_YUV_V210), w=15), b"even width"),
    ("odd h (i010)", dict(fmt=_desc(L.RC_YUV_I010), h=15), b"even height"),
    ("odd w (i010)", dict(fmt=_desc(L.RC_YUV_I010), w=15), b"even height"),
    ("short pitch (nv16)", dict(fmt=_desc(L.RC_YUV_NV16, pitch=15)), b"pitch shorter"),
    ("short pitch (i410: 2 bytes a sample)", dict(fmt=_desc(L.RC_YUV_I410, pitch=30)), b"pitch shorter"),
    ("short pitch (uyvy: 2 samples a pixel)", dict(fmt=_desc(L.RC_YUV_UYVY, pitch=30)), b"pitch shorter"),
    ("short pitch (y210)", dict(fmt=_desc(L.RC_YUV_Y210, pitch=62)), b"pitch shorter"),
    ("short pitch (v210: 3 groups)", dict(fmt=_desc(L.RC_YUV_V210, pitch=44)), b"pitch shorter"),
    ("pitch not a multiple of 4 (v210)", dict(fmt=_desc(L.RC_YUV_V210, pitch=50)), b"multiple"),
    ("odd pitch (p210)", dict(fmt=_desc(L.RC_YUV_P210, pitch=33)), b"multiple"),
    ("odd pitch (i422: the chroma pitch is pitch / 2)", dict(fmt=_desc(L.RC_YUV_I422, pitch=17)), b"multiple"),
    ("pitch / 2 odd (i210)", dict(fmt=_desc(L.RC_YUV_I210, pitch=34)), b"multiple"),
    ("rows below h", dict(fmt=_desc(L.RC_YUV_V210, rows=14)), b"rows"),
    ("chroma inside Y (nv16)", dict(fmt=_desc(L.RC_YUV_NV16, c0=255)), b"overlap"),
    ("Cr inside Y (i444)", dict(fmt=_desc(L.RC_YUV_I444, c0=256, c1=255)), b"overlap"),
    ("Cr inside Cb (i444)", dict(fmt=_desc(L.RC_YUV_I444, c0=256, c1=511)), b"overlap"),
    ("Cr inside Cb (i422: 16 rows of 8 bytes)", dict(fmt=_desc(L.RC_YUV_I422, c0=256, c1=256 + 127)), b"overlap"),
    ("Cb inside Cr (i010, planes swapped)", dict(fmt=_desc(L.RC_YUV_I010, c0=512 + 127, c1=512)), b"multiple"),
    ("Cb inside Cr (i010, planes swapped, aligned)", dict(fmt=_desc(L.RC_YUV_I010, c0=512 + 126, c1=512)), b"overlap"),
    ("Cr offset for p210", dict(fmt=_desc(L.RC_YUV_P210, c1=2048)), b"chroma_offset"),
    ("chroma offset for yuy2", dict(fmt=_desc(L.RC_YUV_YUY2, c0=512)), b"chroma_offset"),
    ("chroma offset for uyvy", dict(fmt=_desc(L.RC_YUV_UYVY, c1=512)), b"chroma_offset"),
    ("chroma offset for y210", dict(fmt=_desc(L.RC_YUV_Y210, c0=1024)), b"chroma_offset"),
    ("chroma offset for v210", dict(fmt=_desc(L.RC_YUV_V210, c0=1024)), b"chroma_offset"),
    ("odd chroma offset (i210)", dict(fmt=_desc(L.RC_YUV_I210, c0=32 * 16 + 1)), b"multiple"),
    ("dst misaligned", dict(fmt=_desc(L.RC_YUV_V210), dst=FAKE + 8), b"16-byte"),
])
def test_bad_arguments_are_reported_before_any_launch(case, kwargs, msg):
    kw = dict(src=FAKE, dtype=RC_F32, dst=FAKE, b=1, H=16, W=16, h=16, w=16)
    kw.update(kwargs)
    lib = _lib.load()
    fmt = C.byref(kw["fmt"])
    assert lib.rc_yuv_encode(kw["src"], kw["dtype"], fmt, kw["dst"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None) == -1, case
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())
    if msg != b"16-byte":                                             # the surface plan's own refusals
        assert lib.rc_yuv_frame_bytes(fmt, kw["h"], kw["w"]) == 0 and msg in lib.rc_last_error(), case


@pytest.mark.parametrize("name", NEW)
def test_reserved_fields_must_be_zero(name):
    d = _desc(LAYOUTS[name])
    d.reserved[3] = 1
    lib = _lib.load()
    assert lib.rc_yuv_encode(FAKE, RC_F32, C.byref(d), FAKE, 1, 16, 16, 16, 16, None) == -1 and b"reserved" in lib.rc_last_error()
    assert lib.rc_yuv_frame_bytes(C.byref(d), 16, 16) == 0 and b"reserved" in lib.rc_last_error()


def test_odd_heights_and_sizes_the_layouts_hold_are_planned():
    lib = _lib.load()
    for name in NEW:
        ok_odd_h, ok_odd_w = SUB[name] != "420", SUB[name] == "444"
        assert (lib.rc_yuv_frame_bytes(C.byref(_desc(LAYOUTS[name])), 15, 16) > 0) == ok_odd_h, name
        assert (lib.rc_yuv_frame_bytes(C.byref(_desc(LAYOUTS[name])), 16, 15) > 0) == ok_odd_w, name
    assert lib.rc_yuv_frame_bytes(C.byref(_desc(L.RC_YUV_V210, pitch=52)), 16, 16) == 52 * 16          # any multiple of 4 >= 3 groups


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _inputs():
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 64, 96, generator=g) * 1.2 - 0.1
    return {"fp32": x.numpy(), "bf16": x.to(torch.bfloat16).float().numpy()}


INPUTS = _inputs()


@pytest.mark.parametrize("matrix", sorted(R.KR_KB))
@pytest.mark.parametrize("sub,siting", [("422", "left"), ("422", "center"), ("444", "left")])
def test_ref_is_within_one_code_of_float64(matrix, sub, siting):
    """The cap: no code more than 1 off the float64 chain, and at most 0.2 % of a case's samples differ (measured: 0.011 % worst)."""
    for bits in (8, 10):
        for rng in ("limited", "full"):
            for kind, x in INPUTS.items():
                a = R.codes(x, sub, bits, matrix, rng, siting, np.float32)
                b = R.codes(x, sub, bits, matrix, rng, siting, np.float64)
                for p, q in zip(a, b):
                    d = np.abs(p - q)
                    assert d.max() <= 1 and (d != 0).mean() <= 0.002, (matrix, sub, siting, bits, rng, kind, d.max(), (d != 0).mean())


def test_ref_422_is_the_row_step_of_420():
    """The header's statement: 4:2:2 LEFT is the row step t of the 4:2:0 LEFT rule; grey has chroma 128 / 512 and the bars' luma codes."""
    x = np.zeros((1, 3, 2, 8), np.float32)
    x[:, :, :, 4:] = 1.0
    y, cb, cr = R.codes(x, "422", 8)
    assert y[0, 0].tolist() == [16] * 4 + [235] * 4 and cb.shape == (1, 2, 4) and (cb == 128).all() and (cr == 128).all()
    y, cb, cr = R.codes(x, "444", 10, vrange="full")
    assert y[0, 1].tolist() == [0] * 4 + [1023] * 4 and cb.shape == (1, 2, 8) and (cb == 512).all()
    x = np.zeros((1, 3, 2, 8), np.float32)
    x[0, 2, :, 3] = 1.0                                               # one blue column at x = 3: LEFT sees a quarter of it at x = 2 and x = 4
    _, cb_l, _ = R.codes(x, "422", 8, "bt601", "full", "left")
    _, cb_c, _ = R.codes(x, "422", 8, "bt601", "full", "center")
    assert cb_l[0, 0].tolist() == [128, 160, 160, 128] and cb_c[0, 0].tolist() == [128, 192, 128, 128]
    _, cb420, _ = R.codes(x, "420", 8, "bt601", "full", "left")
    assert cb420[0, 0].tolist() == cb_l[0, 0].tolist()                # both rows equal: the vertical half changes nothing


@pytest.mark.parametrize("w", (2, 22, 50, 96, 146))                  # w mod 6 = 2, 4, 2, 0, 2
@pytest.mark.parametrize("name", NEW)
def test_packers_round_trip(name, w):
    h = 6
    sub, bits = SUB[name], BITS[name]
    g = np.random.default_rng(w)
    cw, ch = (w if sub == "444" else w // 2), (h // 2 if sub == "420" else h)
    want = (g.integers(0, 1 << bits, (2, h, w), dtype=np.int32), g.integers(0, 1 << bits, (2, ch, cw), dtype=np.int32),
            g.integers(0, 1 << bits, (2, ch, cw), dtype=np.int32))
    for fmt in (M.OutFormat(name), M.OutFormat(name, pitch_align=64, height_align=4)):
        pl = fmt.plane_layout(h, w)
        buf = R.pack(name, *want, pl)
        assert buf.shape == (2, pl.frame_bytes)
        got = R.unpack(name, buf, pl, h, w)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, w)
        assert R.pack(name, *got, pl).tobytes() == buf.tobytes()
    if name == "v210":                                                # the words themselves, for one full and one partial group
        y, cb, cr = (np.arange(1, 9, dtype=np.int32)[None, None], np.arange(101, 105, dtype=np.int32)[None, None], np.arange(201, 205, dtype=np.int32)[None, None])
        wd = R.v210_words(y, cb, cr)[0, 0].tolist()
        assert wd[0] == [101 | 1 << 10 | 201 << 20, 2 | 102 << 10 | 3 << 20, 202 | 4 << 10 | 103 << 20, 5 | 203 << 10 | 6 << 20]
        assert wd[1] == [104 | 7 << 10 | 204 << 20, 8, 0, 0]


def test_packed_byte_orders():
    y, cb, cr = np.array([[[1, 2, 3, 4]]], np.int32), np.array([[[10, 11]]], np.int32), np.array([[[20, 21]]], np.int32)
    assert R.pack("yuy2", y, cb, cr, M.OutFormat("yuy2").plane_layout(1, 4))[0].tolist() == [1, 10, 2, 20, 3, 11, 4, 21]
    assert R.pack("uyvy", y, cb, cr, M.OutFormat("uyvy").plane_layout(1, 4))[0].tolist() == [10, 1, 20, 2, 11, 3, 21, 4]
    assert R.pack("y210", y, cb, cr, M.OutFormat("y210").plane_layout(1, 4))[0].tolist()[:8] == [64, 0, 128, 2, 128, 0, 0, 5]     # 1 << 6, 10 << 6, 2 << 6, 20 << 6
    assert R.pack("nv16", y, cb, cr, M.OutFormat("nv16").plane_layout(1, 4))[0].tolist() == [1, 2, 3, 4, 10, 20, 11, 21]
    assert R.pack("i210", y, cb, cr, M.OutFormat("i210").plane_layout(1, 4))[0].tolist() == [1, 0, 2, 0, 3, 0, 4, 0, 10, 0, 11, 0, 20, 0, 21, 0]


# ---- kernels and traces -----------------------------------------------------------------------------------------------------------------
def test_surface_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if v["tu"] == "yuv_surface.hip"}
    assert len(mine) == 60, sorted(mine)                              # 3 source types x (9 subsampled layouts x 2 sitings + 2 4:4:4 layouts)
    assert all("yuv_surface_kernel" in k and "yuv420_kernel" not in k for k in mine)
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0) or v.get("lds", 0)]


def test_fake_traces():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                net = M.LiteISPNet_GFM_LSC().eval()
                with torch.no_grad():
                    out = net.forward_mosaic(mosaic, None, coord, out_format=M.OutFormat("v210"))
                    assert isinstance(out, M.YuvFrames) and out.buffer.shape == (2, 640 * 144) and out.buffer.dtype == torch.uint8      # 208 -> 5 x 128 bytes
                    assert len(out.planes) == 1 and out.planes[0].shape == (2, 144, 35, 4) and out.planes[0].dtype == torch.int32
                    outs = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(M.OutFormat("i210", pitch_align=64), M.Resize((71, 104))),
                                                                            M.Output(M.OutFormat("uyvy"), M.Resize((35, 52)))])
                    a, b = outs
                    assert a.buffer.shape == (2, 128 * 71 * 2) and a.buffer.dtype == torch.uint16                     # 208 bytes -> 256 = 128 samples; Cb + Cr = one more Y plane
                    assert [tuple(p.shape) for p in a.planes] == [(2, 71, 104), (2, 71, 52), (2, 71, 52)] and a.planes[1].stride() == (128 * 142, 64, 1)
                    assert b.buffer.shape == (2, 104 * 35) and b.buffer.dtype == torch.uint8 and [tuple(p.shape) for p in b.planes] == [(2, 35, 26, 4)]
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(M.OutFormat("i010"), M.Resize((71, 104)))])
                from realcamnet_amd import ops
                y = torch.empty(2, 3, 16, 32)
                for name, shapes, dt in (("nv16", [(2, 15, 30), (2, 15, 15, 2)], torch.uint8), ("p210", [(2, 15, 30), (2, 15, 15, 2)], torch.uint16),
                                         ("i444", [(2, 15, 30)] * 3, torch.uint8), ("i410", [(2, 15, 30)] * 3, torch.uint16),
                                         ("i422", [(2, 15, 30), (2, 15, 15), (2, 15, 15)], torch.uint8), ("y210", [(2, 15, 15, 4)], torch.uint16)):
                    out = ops.yuv_encode(y, M.OutFormat(name), crop_hw=(15, 30))
                    assert [tuple(p.shape) for p in out.planes] == shapes and out.buffer.dtype == dt and all(p.dtype == dt for p in out.planes), name
                out = ops.yuv_encode(y, M.OutFormat("i010"), crop_hw=(14, 30))
                assert [tuple(p.shape) for p in out.planes] == [(2, 14, 30), (2, 7, 15), (2, 7, 15)] and out.buffer.dtype == torch.uint16
                for name, bad in (("uyvy", (16, 31)), ("i010", (15, 30)), ("i444", (17, 32))):
                    with pytest.raises(ValueError):
                        ops.yuv_encode(y, M.OutFormat(name), crop_hw=bad)
                buf = torch.ops.realcam.yuv_encode(torch.empty(3, 3, 80, 160, dtype=torch.float16), _lib.RC_YUV_V210, 0, 1, 1, 420, 80, 70, 154)
                assert buf.shape == (3, 420 * 80) and buf.dtype == torch.uint8
    finally:
        torch.set_default_dtype(old)
