"""GPU: the professional video surfaces of rc_yuv_encode (4:2:2, 4:4:4, planar 10 bit, packed, v210).  The yardstick is the NumPy
restatement in yuv_surface_ref.py (never the kernel's own output): every byte of every frame, pitch and height padding included, is
compared; the kernels that were there before (nv12, p010) cross-check the luma and the 4:2:0 chroma without the new restatement."""
import functools

import numpy as np
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
import yuv_surface_ref as R
from realcamnet_amd import _lib, ops
from realcamnet_amd.out_format import LAYOUTS, MATRICES, RANGES, SITINGS, frame_layout
from test_yuv_gpu import net_on_gpu

DEV = "cuda"
DTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NEW = R.NEW
CROPS = ((6, 2), (5, 22), (7, 50), (10, 96), (9, 146))              # one chroma sample; odd h, partial v210 group; a strip border; whole strips; ragged
CROPS_420 = ((6, 2), (10, 96), (8, 146))
MATRIX_NAMES, RANGE_NAMES = ("bt601", "bt709", "bt2020"), ("limited", "full")


@functools.lru_cache(maxsize=None)
def source(dt_name, W):
    """(2,3,12,W) in [-0.2, 1.2] with NaN, +-inf and exact rounding ties planted.  W = 150: no row is 16-byte aligned (element loads); W = 160:
    every row is (16-byte loads wherever a whole strip lies inside the source)."""
    g = torch.Generator().manual_seed(150)
    y = torch.rand(2, 3, 12, W, generator=g) * 1.4 - 0.2
    y[:, :, 3, :] = 0.5                                               # v S + O on a half in exact arithmetic: round half to even decides
    y[:, :, 4, :] = (((2 * torch.arange(W) + 1) % 8).float() / 8.0)
    y[0, 0, 0, :6] = torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0, 0.0, float("nan")])
    y[1, 2, 2, 93:99] = torch.tensor([float("nan"), float("-inf"), float("inf"), 0.25, float("nan"), 1.0])
    y[1, :, 1, 48] = float("nan")
    return y.to(DTS[dt_name])


@functools.lru_cache(maxsize=None)
def cropped(dt_name, W, hw):
    """The source with everything outside the (h, w) crop NaN, so that a read beyond the crop shows; as (torch on the device, fp32 numpy crop)."""
    h, w = hw
    y = source(dt_name, W).clone()
    y[:, :, h:, :] = float("nan")
    y[:, :, :, w:] = float("nan")
    return y.to(DEV), y[:, :, :h, :w].float().numpy()


@functools.lru_cache(maxsize=None)
def want_codes(dt_name, W, hw, sub, bits, matrix, rng, siting):
    return R.codes(cropped(dt_name, W, hw)[1], sub, bits, matrix, rng, "left" if sub == "444" else siting)


def frame_bytes(buf):
    return buf.contiguous().view(torch.uint8).cpu().numpy()


def first_diff(got, want):
    bad = np.argwhere(got != want)
    return (len(bad), bad[:4].tolist())


# ---- 1. every byte against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("siting", ("left", "center"))
@pytest.mark.parametrize("dt", sorted(DTS))
@pytest.mark.parametrize("layout", NEW)
def test_surface_equals_restatement(hip, layout, dt, siting):
    """Every layout x 3 source types x 2 sitings x 2 ranges x 3 matrices on five crops of a (2,3,12,150) source (element loads) and of a
    (2,3,12,160) one (16-byte loads), each with the tight pitch (element stores unless the row happens to be a multiple of 16) and with
    pitch_align=64, height_align=4 (16-byte stores, padded rows and columns).  Batch 2 checks the frame stride."""
    sub, bits, _, _ = R.LAYOUTS[layout]
    for W in (150, 160):
        for hw in (CROPS_420 if sub == "420" else CROPS):
            yd, _ = cropped(dt, W, hw)
            for matrix in MATRIX_NAMES:
                for rng in RANGE_NAMES:
                    want = want_codes(dt, W, hw, sub, bits, matrix, rng, siting)
                    for pa, ha in ((1, 1), (64, 4)):
                        fmt = M.OutFormat(layout, matrix=matrix, range=rng, chroma_siting=siting, pitch_align=pa, height_align=ha)
                        pl = fmt.plane_layout(*hw)
                        out = ops.yuv_encode(yd, fmt, crop_hw=hw)
                        got, ref = frame_bytes(out.buffer), R.pack(layout, *want, pl)
                        assert got.shape == ref.shape and np.array_equal(got, ref), (W, hw, matrix, rng, pa, first_diff(got, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTS))
def test_plane_views_are_the_codes(hip, dt):
    """YuvFrames.planes: views without padding, in the shapes the layouts state."""
    hw, W = (9, 146), 160
    yd, _ = cropped(dt, W, hw)
    for layout in NEW:
        sub, bits, cont, sh = R.LAYOUTS[layout]
        h, w = hw = (8, 146) if sub == "420" else (9, 146)
        yd, _ = cropped(dt, W, hw)
        yc, cb, cr = want_codes(dt, W, hw, sub, bits, "bt709", "limited", "left")
        out = ops.yuv_encode(yd, M.OutFormat(layout, pitch_align=64, height_align=4), crop_hw=hw)
        p = [t.cpu().to(torch.int64).numpy() for t in out.planes]
        if cont == "planar":
            assert len(p) == 3 and all(np.array_equal(a, b << sh) for a, b in zip(p, (yc, cb, cr))), layout
        elif cont == "semi":
            assert p[1].shape == (2, h, w // 2, 2) and np.array_equal(p[0], yc << sh) and np.array_equal(p[1][..., 0], cb << sh) and np.array_equal(p[1][..., 1], cr << sh), layout
        elif cont in ("yuyv", "uyvy"):
            o = 0 if cont == "yuyv" else 1
            assert p[0].shape == (2, h, w // 2, 4) and np.array_equal(p[0][..., o], yc[..., 0::2] << sh) and np.array_equal(p[0][..., 2 + o], yc[..., 1::2] << sh), layout
            assert np.array_equal(p[0][..., 1 - o], cb << sh) and np.array_equal(p[0][..., 3 - o], cr << sh), layout
        else:
            assert out.planes[0].dtype == torch.int32 and p[0].shape == (2, h, 25, 4) and np.array_equal(p[0], R.v210_words(yc, cb, cr).astype(np.int64)), layout


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTS))
def test_v210_pitches_the_c_entry_takes(hip, dt):
    """v210 with a pitch that is a multiple of 4 but not of 16 (dword stores) and with the groups' own bytes, through the op that takes the
    pitch as it is; one allocated row more than the frame has."""
    for hw in ((5, 22), (7, 50), (9, 146)):
        h, w = hw
        for W in (150, 160):
            yd, _ = cropped(dt, W, hw)
            want = want_codes(dt, W, hw, "422", 10, "bt601", "full", "left")
            for pitch in (-(-w // 6) * 16, -(-w // 6) * 16 + 4, -(-w // 6) * 16 + 72):
                buf = torch.ops.realcam.yuv_encode(yd, _lib.RC_YUV_V210, MATRICES["bt601"], RANGES["full"], SITINGS["left"], pitch, h + 1, h, w)
                pl = frame_layout(_lib.RC_YUV_V210, pitch, h + 1, h, w)
                got, ref = frame_bytes(buf), R.pack("v210", *want, pl)
                assert got.shape == ref.shape and np.array_equal(got, ref), (hw, W, pitch, first_diff(got, ref))


# ---- 2. against the kernels that were there before --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("siting", ("left", "center"))
@pytest.mark.parametrize("dt", sorted(DTS))
def test_cross_checks_against_nv12_and_p010(hip, dt, siting):
    for W, hw in ((150, (10, 96)), (160, (8, 146)), (160, (6, 2))):
        h, w = hw
        yd, _ = cropped(dt, W, hw)
        for matrix, rng in (("bt601", "full"), ("bt709", "limited"), ("bt2020", "limited")):
            kw = dict(matrix=matrix, range=rng, chroma_siting=siting)
            enc = lambda name: ops.yuv_encode(yd, M.OutFormat(name, pitch_align=64, **kw), crop_hw=hw)
            nv12, p010 = enc("nv12"), enc("p010")
            codes_of = lambda t: t.cpu().to(torch.int32).numpy()
            y8, y10, c10 = codes_of(nv12.planes[0]), codes_of(p010.planes[0]) >> 6, codes_of(p010.planes[1]) >> 6
            i010 = [codes_of(p) for p in enc("i010").planes]
            assert np.array_equal(i010[0], y10) and np.array_equal(i010[1], c10[..., 0]) and np.array_equal(i010[2], c10[..., 1]), (hw, kw)
            codes = {}
            for name in NEW:
                if name == "i010":
                    continue
                out = enc(name)
                pl = M.OutFormat(name, pitch_align=64, **kw).plane_layout(h, w)
                codes[name] = R.unpack(name, frame_bytes(out.buffer), pl, h, w)
                assert np.array_equal(codes[name][0], y8 if R.LAYOUTS[name][1] == 8 else y10), (name, hw, kw)
            for group in (("yuy2", "uyvy", "nv16", "i422"), ("y210", "p210", "i210", "v210")):
                for name in group[1:]:
                    assert all(np.array_equal(a, b) for a, b in zip(codes[name], codes[group[0]])), (name, hw, kw)


# ---- 3. forward_mosaic -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_mosaic_uyvy_and_a_v210_ladder(hip):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(7)
    mosaic = (torch.rand(2, 1, 72, 104, generator=g) * 1.4 - 0.2).to(DEV, dt)          # the smallest frame the net takes: 36 x 52 packed
    coord = O.make_coord(2, 36, 52).to(DEV, dt)
    net = net_on_gpu("LiteISPNet_GFM_LSC", dt)
    uyvy, v210, nv12 = M.OutFormat("uyvy", matrix="bt601"), M.OutFormat("v210", range="full", pitch_align=256), M.OutFormat("nv12", pitch_align=64)
    r1, r2 = M.Resize((35, 50)), M.Resize((36, 52), filter="bilinear")
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord)
        out = net.forward_mosaic(mosaic, None, coord, out_format=uyvy)
        outs = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(v210, r1), M.Output(nv12, r2), M.Output(None, r1), M.Output(None, r2)])
    assert isinstance(out, M.YuvFrames) and out.buffer.shape == (2, 72 * 208) and out.planes[0].shape == (2, 72, 52, 4)
    assert torch.equal(out.buffer, ops.yuv_encode(y, uyvy).buffer)
    want = R.pack("uyvy", *R.format_codes(y.float().cpu().numpy(), uyvy), uyvy.plane_layout(72, 104))
    assert np.array_equal(frame_bytes(out.buffer), want)
    a, b, fa, fb = outs
    assert fa.shape == (2, 3, 35, 50) and fb.shape == (2, 3, 36, 52) and a.buffer.shape == (2, 256 * 35) and a.planes[0].shape == (2, 35, 9, 4)
    assert torch.equal(a.buffer, ops.yuv_encode(fa, v210).buffer) and torch.equal(b.buffer, ops.yuv_encode(fb, nv12).buffer)
    want = R.pack("v210", *R.format_codes(fa.float().cpu().numpy(), v210), v210.plane_layout(35, 50))
    assert np.array_equal(frame_bytes(a.buffer), want)


# ---- 4. graph replay ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_v210_replays_on_a_rewritten_input(hip):
    fmt = M.OutFormat("v210", matrix="bt2020", pitch_align=128, height_align=2)
    hw = (9, 146)
    y1 = cropped("bf16", 160, hw)[0]
    y2 = (1.0 - y1.float()).to(torch.bfloat16)
    e1, e2 = ops.yuv_encode(y1, fmt, crop_hw=hw).buffer.clone(), ops.yuv_encode(y2, fmt, crop_hw=hw).buffer.clone()
    call = M.GraphedCall(lambda x: ops.yuv_encode(x, fmt, crop_hw=hw))
    g1 = call(y1).buffer.clone()
    r2 = call(y2)                                                     # the source the graph reads is overwritten
    assert isinstance(r2, M.YuvFrames) and r2.planes[0].shape == (2, 9, 25, 4)
    assert torch.equal(g1, e1) and torch.equal(r2.buffer, e2) and not torch.equal(e1, e2)
    want = R.pack("v210", *R.format_codes(y1[:, :, :9, :146].float().cpu().numpy(), fmt), fmt.plane_layout(*hw))
    assert np.array_equal(frame_bytes(g1), want)
