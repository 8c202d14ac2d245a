"""GPU: the rendition ladder of forward_mosaic (rc_resize).  The yardstick is the elementwise fp32 torch restatement of the header's
arithmetic in test_resize_host.py, built on tables restated in NumPy (never the kernel's own output or the library's tables): every
sample is compared bit for bit; a float64 resampling of the same source bounds what fp32 costs; whole nets with several outputs, RAW10
in, a graphed ladder, and the routes that were there before."""
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import ops
from test_raw_formats_host import mipi_pack
from test_resize_host import CASES, bound, restated_resize

DEV = "cuda"
DTS = (torch.float32, torch.bfloat16, torch.float16)
FILTERS = ("area", "bilinear")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


_SRC = {}


def source(shape, crop, dt):
    """(B,3,H,W) in [0, 1]; everything outside the crop is NaN so that a read beyond it that counts shows.  Made once per case."""
    key = (shape, crop, dt)
    if key not in _SRC:
        y = torch.rand(shape, generator=torch.Generator().manual_seed(17))
        if crop is not None:
            y[:, :, crop[0]:, :] = float("nan")
            y[:, :, :, crop[1]:] = float("nan")
        _SRC[key] = y.to(dt)
    return _SRC[key]


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dt", DTS)
def test_resize_equals_restatement(hip, dt, filt):
    """3 source types x 2 filters x 7 geometries: identity, 2:1, a ROI at 2.5 : 2.19, 7:1, a ROI at the tap limit (7.56 : 7.5), 1.67 : 1.23
    on an uncropped source, and a wide frame of 9 column tiles; fp32 out, and the source's type out (the restatement rounded once)."""
    for shape, crop, kw in CASES:
        y = source(shape, crop, dt)
        rs = M.Resize(filter=filt, **kw)
        want = restated_resize(y, rs, crop)
        got = ops.resize(y.to(DEV), rs, crop_hw=crop)
        assert not torch.isnan(want).any()
        assert same(got, want), (kw, int((got.cpu() != want).sum()), float((got.cpu() - want).abs().max()))
        if dt != torch.float32:
            assert same(ops.resize(y.to(DEV), rs, crop_hw=crop, out_dtype=dt), want.to(dt)), kw
    assert same(ops.resize(source((2, 3, 80, 160), (70, 154), dt).to(DEV), M.Resize((70, 154), filter=filt), crop_hw=(70, 154)),
                source((2, 3, 80, 160), (70, 154), dt)[:, :, :70, :154].float())                   # identity: the source itself


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dt", DTS)
def test_within_the_rounding_bound_of_float64(hip, dt, filt):
    for shape, crop, kw in CASES:
        y = source(shape, crop, dt)
        rs = M.Resize(filter=filt, **kw)
        h, w = crop if crop is not None else shape[2:]
        want = restated_resize(y, rs, crop, torch.float64)
        got = ops.resize(y.to(DEV), rs, crop_hw=crop).cpu()
        err = (got.double() - want).abs().max().item()
        print(f"{dt} {filt} {kw}: max |gpu - float64| = {err:.3e}, bound {bound(rs, h, w):.3e}")
        assert err <= bound(rs, h, w), (kw, err)


# ---- 3. whole nets --------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def check_rendition(got, y, out):
    """One element of the ladder against the existing encoders applied to the restated resize of the float result `y`."""
    t = y if out.resize is None else restated_resize(y, out.resize).to(DEV)
    if out.format is None:
        assert same(got, t)
    elif isinstance(out.format, str):
        assert same(got, ops.rgb_encode(t, 8 if out.format == "rgb8" else 16))
    else:
        want = ops.yuv_encode(t, out.format)
        assert isinstance(got, M.YuvFrames) and same(got.buffer, want.buffer) and len(got.planes) == len(want.planes)       # padding bytes included
        assert all(same(a.contiguous(), b.contiguous()) for a, b in zip(got.planes, want.planes))


@pytest.mark.gpu
def test_existing_routes_unchanged_then_forward_mosaic_with_several_outputs(hip):
    """In one process: the default, rgb8 and nv12 routes of two nets before any `outputs` call, the four-rung ladder of the issue, and the
    same routes again afterwards."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(7)
    mosaic = (torch.rand(2, 1, 144, 208, generator=g) * 1.4 - 0.2).to(DEV, dt)
    coord = O.make_coord(2, 72, 104).to(DEV, dt)
    nv12 = M.OutFormat("nv12")
    nets = [net_on_gpu(n, dt) for n in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC")]

    def routes(net):
        with torch.no_grad():
            return (net.forward_mosaic(mosaic, None, coord), net.forward_mosaic(mosaic, None, coord, out_format="rgb8"),
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12))
    before = [routes(n) for n in nets]
    ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.OutFormat("nv12"), M.Resize((72, 104))),
              M.Output("rgb8", M.Resize((36, 52), roi=(0, 0, 144, 208), filter="bilinear")), M.Output(None, M.Resize((72, 104)))]
    for net, (y, q8, f) in zip(nets, before):
        with torch.no_grad():
            outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
        assert isinstance(outs, list) and len(outs) == 4
        assert y.dtype == dt and y.shape == (2, 3, 144, 208)
        assert same(outs[0].buffer, f.buffer) and all(same(a.contiguous(), b.contiguous()) for a, b in zip(outs[0].planes, f.planes))
        assert outs[1].planes[0].shape == (2, 72, 104) and outs[2].shape == (2, 36, 52, 3) and outs[2].dtype == torch.uint8
        assert outs[3].shape == (2, 3, 72, 104) and outs[3].dtype == torch.float32
        for got, out in zip(outs, ladder):
            check_rendition(got, y, out)
    for net, (y, q8, f) in zip(nets, before):
        y2, q2, f2 = routes(net)
        assert same(y, y2) and same(q8, q2) and same(f.buffer, f2.buffer)
        assert same(q8, ops.rgb_encode(y, 8))


@pytest.mark.gpu
def test_forward_mosaic_raw10_grbg_in_nv12_ladder_out(hip):
    g = torch.Generator().manual_seed(31)
    counts = torch.randint(0, 1024, (2, 80, 112), generator=g, dtype=torch.int32)
    lines = torch.from_numpy(mipi_pack(counts.numpy(), 10, 160)).unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    raw = M.RawFormat(cfa="GRBG", storage="mipi10", width=112, black_level=(64.0, 63.0, 65.0, 64.5), white_level=1023.0)
    ladder = [M.Output(M.OutFormat("nv12", pitch_align=64)), M.Output(M.OutFormat("nv12", pitch_align=64), M.Resize((36, 64), roi=(4, 0, 72, 112)))]
    with torch.no_grad():
        y = net.forward_mosaic(lines, None, coord, raw_format=raw)
        outs = net.forward_mosaic(lines, None, coord, raw_format=raw, outputs=ladder)
    assert y.shape == (2, 3, 80, 112) and outs[0].planes[0].shape == (2, 80, 112) and outs[1].planes[0].shape == (2, 36, 64)
    for got, out in zip(outs, ladder):
        check_rendition(got, y, out)


@pytest.mark.gpu
def test_graphed_ladder_equals_eager(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    ladder = [M.Output(M.OutFormat("nv12", pitch_align=256, height_align=16)), M.Output(M.OutFormat("nv12"), M.Resize((40, 56))),
              M.Output(None, M.Resize((20, 28), filter="bilinear"))]
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    flat = lambda outs: [outs[0].buffer.clone(), outs[1].buffer.clone(), outs[2].clone()]
    with torch.no_grad():
        e1 = flat(net.forward_mosaic(m1, None, coord, outputs=ladder))                            # also the warm-up: the tables are on the device
        e2 = flat(net.forward_mosaic(m2, None, coord, outputs=ladder))
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, outputs=ladder))
    g1 = flat(call(m1, coord))
    g2 = flat(call(m2, coord))
    assert g1[0].shape == (2, 256 * 120) and g1[1].shape == (2, 56 * 60) and g1[2].shape == (2, 3, 20, 28)
    assert all(same(a, b) for a, b in zip(g1, e1)) and all(same(a, b) for a, b in zip(g2, e2))
    assert not any(torch.equal(a, b) for a, b in zip(g1, g2))
