"""GPU: the video-encoder output of forward_mosaic (rc_yuv_encode).  The yardstick is the elementwise fp32 torch restatement of the header's
arithmetic in test_yuv_host.py (never the kernel's own output): every plane and every padding byte is compared bit for bit; the
colour bars against the standards' codes; a float64 restatement bounds what fp32 costs."""
import ctypes as C

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.out_format import LAYOUTS, MATRICES, RANGES, SITINGS
from test_raw_formats_host import mipi_pack
from test_yuv_host import BARS, bars_image, restated_codes, restated_frames

DEV = "cuda"
DTS = (torch.float32, torch.bfloat16, torch.float16)
LAYOUT_NAMES = ("nv12", "p010", "i420")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def source(dt, b=2, H=80, W=160, h=70, w=154, seed=0):
    """(B,3,H,W) in [-0.2, 1.2] with NaN, +-inf and exact rounding ties planted; everything outside the (h,w) crop is NaN so that a read
    beyond the crop shows."""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(b, 3, H, W, generator=g) * 1.4 - 0.2
    # values that put v * S + O exactly on a half in exact arithmetic (round half to even decides): grey 1/2 (219 / 2, 255 / 2, 1023 / 2 and
    # their 10-bit forms), grey odd / 8 (876 * odd / 8), and pure blue / pure red odd / 32 on whole 2x2 blocks (Cb = b / 2, Cr = r / 2:
    # 224 * odd / 64).  The fp32 chain lands on some of them exactly and next to the others; the restatement says which.
    odd8 = ((2 * torch.arange(w) + 1) % 8).float() / 8.0
    odd32 = ((2 * (torch.arange(w) // 2) + 1) % 32).float() / 32.0
    y[:, :, 4, :w] = 0.5
    y[:, :, 5, :w] = odd8
    y[:, :, 6:10, :w] = 0.0
    y[:, 2, 6:8, :w] = odd32
    y[:, 0, 8:10, :w] = odd32
    y[0, 0, 0, :6] = torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0, 0.0, float("nan")])
    y[0, 1, 1, 150:154] = torch.tensor([float("inf"), float("nan"), float("-inf"), 0.5])
    y[1, 2, 69, 0:3] = torch.tensor([float("nan"), float("-inf"), float("inf")])
    y[1, :, 33, 16] = float("nan")
    y[:, :, h:, :] = float("nan")
    y[:, :, :, w:] = float("nan")
    return y.to(dt)


def check_frames(got, y, fmt, crop_hw):
    want = restated_frames(y, fmt, crop_hw)
    assert same(got.buffer, want), (fmt, (got.buffer.cpu().to(torch.int32) != want.to(torch.int32)).sum().item())
    yc, cb, cr = restated_codes(y, fmt, crop_hw)
    sh = 6 if fmt.layout == "p010" else 0
    p = [t.cpu().to(torch.int32) for t in got.planes]
    assert torch.equal(p[0], yc << sh)
    if fmt.layout == "i420":
        assert torch.equal(p[1], cb << sh) and torch.equal(p[2], cr << sh)
    else:
        assert torch.equal(p[1][..., 0], cb << sh) and torch.equal(p[1][..., 1], cr << sh)


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("siting", ("left", "center"))
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("dt", DTS)
def test_yuv_encode_equals_restatement(hip, dt, layout, siting):
    """3 source types x 3 layouts x 2 sitings x 2 ranges x 3 matrices on a ragged (70,154) crop of a padded (80,160) source, each with the
    tight pitch (the element store path) and with pitch / height alignment (the 16-byte store path, ragged right edge, zero padding)."""
    y = source(dt)
    yd = y.to(DEV)
    for matrix in ("bt601", "bt709", "bt2020"):
        for rng in ("limited", "full"):
            for pa, ha in ((1, 1), (256, 16)):
                fmt = M.OutFormat(layout, matrix=matrix, range=rng, chroma_siting=siting, pitch_align=pa, height_align=ha)
                check_frames(ops.yuv_encode(yd, fmt, crop_hw=(70, 154)), y, fmt, (70, 154))
    # an uncropped source whose rows are not 16-byte aligned (the element load path), and a one-strip frame
    for shape in ((1, 3, 6, 18), (2, 3, 2, 2), (1, 3, 4, 34)):
        ys = torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
        ys[0, 1, 1, 1] = float("nan")
        ys = ys.to(dt)
        for pa in (1, 16):
            fmt = M.OutFormat(layout, chroma_siting=siting, pitch_align=pa)
            check_frames(ops.yuv_encode(ys.to(DEV), fmt), ys, fmt, shape[2:])


# ---- 2. the standards' colour bars ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("matrix", ("bt601", "bt709", "bt2020"))
def test_colour_bars(hip, dt, matrix):
    img = bars_image(dtype=dt).to(DEV)
    for layout in LAYOUT_NAMES:
        for siting in ("left", "center"):
            fmt = M.OutFormat(layout, matrix=matrix, chroma_siting=siting)
            out = ops.yuv_encode(img, fmt)
            sh = 6 if layout == "p010" else 0
            p = [t.cpu().to(torch.int32) >> sh for t in out.planes]
            cb, cr = (p[1], p[2]) if layout == "i420" else (p[1][..., 0], p[1][..., 1])
            for i, want in enumerate(BARS[matrix, fmt.bits]):
                got = (int(p[0][0, 1, 16 * i + 5]), int(cb[0, 1, 8 * i + 3]), int(cr[0, 1, 8 * i + 3]))
                assert got == want, (matrix, layout, siting, i, got, want)
            assert int(p[0].min()) == 16 << (fmt.bits - 8) and int(p[0].max()) == 235 << (fmt.bits - 8)


# ---- 3. against float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("layout", ("nv12", "p010"))
def test_within_one_code_of_float64(hip, dt, layout):
    """>= 2 M seeded random samples per case: never more than one code from the float64 chain, and at most 0.2 % of the samples differ at
    all (twice the 0.098 % the fp32 chain shows on the CPU; a cap, so that "within one code" cannot hide a shifted plane)."""
    g = torch.Generator().manual_seed(2024)
    y = (torch.rand(2, 3, 1024, 1024, generator=g) * 1.2 - 0.1).to(dt)          # 2 M pixels: 2 M luma + 1 M chroma samples per frame pair
    for matrix, rng, siting in (("bt709", "limited", "left"), ("bt601", "full", "center"), ("bt2020", "limited", "center"), ("bt2020", "full", "left")):
        fmt = M.OutFormat(layout, matrix=matrix, range=rng, chroma_siting=siting)
        out = ops.yuv_encode(y.to(DEV), fmt)
        sh = 6 if layout == "p010" else 0
        p = [t.cpu().to(torch.int32) >> sh for t in out.planes]
        got = (p[0], p[1][..., 0], p[1][..., 1])
        want = restated_codes(y, fmt, dtype=torch.float64)
        n = sum(t.numel() for t in got)
        assert n >= 2_000_000
        diff = [(a - b).abs() for a, b in zip(got, want)]
        worst = max(int(d.max()) for d in diff)
        share = sum(int((d != 0).sum()) for d in diff) / n
        per_plane = ", ".join(f"{name} {100 * int((d != 0).sum()) / d.numel():.4f} %" for d, name in zip(diff, ("Y", "Cb", "Cr")))
        print(f"{dt} {layout} {matrix} {rng} {siting}: max |diff| {worst} code(s), {100 * share:.4f} % of {n} samples differ ({per_plane})")
        assert worst <= 1 and share <= 0.002, (matrix, rng, siting, worst, share)


# ---- 4. layout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_layout_padding_and_guard_band(hip, layout):
    """pitch_align 256 / height_align 16: planes at plane_layout's offsets, every padding byte zero, P010's low 6 bits clear, and -- through
    the C ABI into the middle of a sentinel-filled allocation -- not one byte written in front of or behind the frames."""
    dt = torch.bfloat16
    y = source(dt)
    fmt = M.OutFormat(layout, pitch_align=256, height_align=16)
    pl = fmt.plane_layout(70, 154)
    out = ops.yuv_encode(y.to(DEV), fmt, crop_hw=(70, 154))
    raw = out.buffer.cpu().view(torch.uint8).view(2, pl.frame_bytes).clone()
    assert out.buffer.shape == (2, pl.frame_bytes // pl.elem_bytes)
    valid = torch.zeros(pl.frame_bytes, dtype=torch.bool)
    for p, view in zip(pl.planes, out.planes):
        assert p.offset % 256 == 0 and p.pitch % (128 if p.name in ("cb", "cr") else 256) == 0
        for r in range(p.rows):
            valid[p.offset + r * p.pitch: p.offset + r * p.pitch + p.valid_bytes] = True
        assert view.data_ptr() == out.buffer.data_ptr() + p.offset and view.stride(0) * pl.elem_bytes == pl.frame_bytes
        assert view.stride(1) * pl.elem_bytes == p.pitch
    assert pl.planes[0].alloc_rows == 80 and pl.planes[1].alloc_rows == 40 and (~valid).sum() > 0
    assert int(raw[:, ~valid].to(torch.int32).abs().sum()) == 0                        # pitch and height padding
    if layout == "p010":
        assert int((out.buffer.cpu().to(torch.int32) & 63).sum()) == 0
    # guard bands through the C ABI
    guard = 4096
    big = torch.full((guard + 2 * pl.frame_bytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    d = _lib.OutFormatDesc(layout=LAYOUTS[layout], matrix=MATRICES[fmt.matrix], range=RANGES[fmt.range], siting=SITINGS[fmt.chroma_siting],
                           pitch=pl.pitch, rows=pl.planes[0].alloc_rows)
    yd = y.to(DEV)
    assert hip.rc_yuv_frame_bytes(C.byref(d), 70, 154) == pl.frame_bytes
    _lib.check(hip.rc_yuv_encode(yd.data_ptr(), _lib.RC_BF16, C.byref(d), big.data_ptr() + guard, 2, 80, 160, 70, 154,
                                 torch.cuda.current_stream().cuda_stream), "rc_yuv_encode")
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + 2 * pl.frame_bytes:] == 0xA5).all())
    assert torch.equal(big[guard:guard + 2 * pl.frame_bytes].view(2, pl.frame_bytes), raw)
    # the tight frame (element stores, odd pitches): the same guard-band check
    tight = M.OutFormat(layout)
    tl = tight.plane_layout(70, 154)
    nb = 2 * tl.frame_bytes
    big = torch.full((guard + nb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    d = _lib.OutFormatDesc(layout=LAYOUTS[layout], matrix=MATRICES[fmt.matrix], range=RANGES[fmt.range], siting=SITINGS[fmt.chroma_siting])
    _lib.check(hip.rc_yuv_encode(yd.data_ptr(), _lib.RC_BF16, C.byref(d), big.data_ptr() + guard, 2, 80, 160, 70, 154,
                                 torch.cuda.current_stream().cuda_stream), "rc_yuv_encode")
    torch.cuda.synchronize()
    big = big.cpu()
    assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + nb:] == 0xA5).all())
    assert torch.equal(big[guard:guard + nb], restated_frames(y, tight, (70, 154)).view(torch.uint8).flatten())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_siting_and_layout_relations(hip, dt):
    y = source(dt).to(DEV)
    kw = dict(matrix="bt601", range="full")
    nl = ops.yuv_encode(y, M.OutFormat("nv12", chroma_siting="left", **kw), crop_hw=(70, 154))
    nc = ops.yuv_encode(y, M.OutFormat("nv12", chroma_siting="center", **kw), crop_hw=(70, 154))
    il = ops.yuv_encode(y, M.OutFormat("i420", chroma_siting="left", pitch_align=64, **kw), crop_hw=(70, 154))
    pl = ops.yuv_encode(y, M.OutFormat("p010", chroma_siting="left", **kw), crop_hw=(70, 154))
    assert same(nl.planes[0], nc.planes[0]) and not torch.equal(nl.planes[1], nc.planes[1])         # siting: chroma only
    assert same(nl.planes[0].contiguous(), il.planes[0].contiguous())                               # nv12 and i420: one Y plane
    assert same(nl.planes[1][..., 0].contiguous(), il.planes[1].contiguous()) and same(nl.planes[1][..., 1].contiguous(), il.planes[2].contiguous())
    assert pl.planes[0].dtype == torch.uint16 and pl.planes[0].shape == nl.planes[0].shape


# ---- 5. whole nets ----------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dt", [("LiteISPNet_GFM_LSC", torch.bfloat16), ("LiteISPNet_GFM_LSC", torch.float16),
                                     ("ISPUNet_GFM_LSC", torch.bfloat16), ("ISPUNet_GFM_LSC", torch.float16),
                                     ("LiteISPNet_GFM_LSC_GMA", torch.bfloat16)])
def test_forward_mosaic_yuv_equals_restatement_of_float_result(hip, name, dt):
    g = torch.Generator().manual_seed(7)
    hh, ww = (128, 128) if name.endswith("GMA") else (36, 52)                         # packed size; the mosaic is twice that
    mosaic = (torch.rand(2, 1, 2 * hh, 2 * ww, generator=g) * 1.4 - 0.2).to(DEV, dt)
    coord = O.make_coord(2, hh, ww).to(DEV, dt)
    net = net_on_gpu(name, dt)
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord)
        for fmt in (M.OutFormat("nv12"), M.OutFormat("p010", matrix="bt2020", pitch_align=256, height_align=16),
                    M.OutFormat("i420", matrix="bt601", range="full", chroma_siting="center")):
            out = net.forward_mosaic(mosaic, None, coord, out_format=fmt)
            assert isinstance(out, M.YuvFrames)
            check_frames(out, y, fmt, (2 * hh, 2 * ww))


@pytest.mark.gpu
def test_forward_mosaic_nv12_at_4k_batch_8(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    g = torch.Generator().manual_seed(8)
    mosaic = torch.rand(8, 1, 2160, 3840, generator=g).to(DEV, torch.bfloat16)
    coord = ops.make_coord(8, 1080, 1920, DEV, torch.bfloat16)
    fmt = M.OutFormat("nv12", pitch_align=256, height_align=64)
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord).cpu()
        out = net.forward_mosaic(mosaic, None, coord, out_format=fmt)
    assert out.buffer.shape == (8, 3840 * 2176 * 3 // 2)
    check_frames(out, y, fmt, (2160, 3840))


@pytest.mark.gpu
def test_forward_mosaic_raw10_grbg_in_nv12_out(hip):
    g = torch.Generator().manual_seed(31)
    counts = torch.randint(0, 1024, (2, 80, 112), generator=g, dtype=torch.int32)
    lines = torch.from_numpy(mipi_pack(counts.numpy(), 10, 160)).unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    raw = M.RawFormat(cfa="GRBG", storage="mipi10", width=112, black_level=(64.0, 63.0, 65.0, 64.5), white_level=1023.0)
    fmt = M.OutFormat("nv12", pitch_align=64)
    with torch.no_grad():
        y = net.forward_mosaic(lines, None, coord, raw_format=raw)
        out = net.forward_mosaic(lines, None, coord, raw_format=raw, out_format=fmt)
    assert y.shape == (2, 3, 80, 112) and out.planes[0].shape == (2, 80, 112) and out.buffer.shape == (2, 128 * 120)
    check_frames(out, y, fmt, (80, 112))


@pytest.mark.gpu
def test_graphed_yuv_forward_equals_eager(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    fmt = M.OutFormat("nv12", pitch_align=256, height_align=16)
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, out_format=fmt))
    with torch.no_grad():
        e1 = net.forward_mosaic(m1, None, coord, out_format=fmt).buffer
        e2 = net.forward_mosaic(m2, None, coord, out_format=fmt).buffer
    g1 = call(m1, coord).buffer.clone()
    r2 = call(m2, coord)
    g2 = r2.buffer.clone()
    assert isinstance(r2, M.YuvFrames) and same(r2.planes[0].contiguous(), e2[:, :256 * 80].view(2, 80, 256)[:, :, :112].contiguous())
    assert g1.dtype == torch.uint8 and g1.shape == (2, 256 * 120)
    assert same(g1, e1) and same(g2, e2) and not torch.equal(g1, g2)


# ---- 6. the routes that were there stay ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"))
def test_default_and_rgb_routes_unchanged(hip, name):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(9)
    mosaic = (torch.rand(2, 1, 48, 80, generator=g) * 1.4 - 0.2).to(DEV, dt)
    coord = O.make_coord(2, 24, 40).to(DEV, dt)
    net = net_on_gpu(name, dt)
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord)
        y_none = net.forward_mosaic(mosaic, None, coord, out_format=None)
        q8 = net.forward_mosaic(mosaic, None, coord, out_format="rgb8")
        q16 = net.forward_mosaic(mosaic, None, coord, out_format="rgb16")
    assert y.dtype == dt and y.shape == (2, 3, 48, 80) and same(y, y_none)
    assert same(q8, ops.rgb_encode(y, 8)) and same(q16, ops.rgb_encode(y, 16))
    for bits, q in ((8, q8), (16, q16)):
        s = float((1 << bits) - 1)
        want = (y.float().cpu() * s).round().clamp(0, s).to(q.dtype).permute(0, 2, 3, 1).contiguous()
        assert same(q, want)
