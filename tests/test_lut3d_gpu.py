"""GPU: colour looks (rc_lut3d).  The yardstick is the elementwise fp32 torch restatement of the header's arithmetic in
test_lut3d_host.py (never the kernel's own output): every sample is compared bit for bit, on sources that carry every grid node, the
special values and every tie; a float64 evaluation of the same formula bounds what fp32 costs; whole nets with looked outputs, a
graphed ladder, and the routes that were there before."""
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import ops
from test_lut3d_host import SIZES, bound, lut_identity, lut_random, lut_source, restated_lut3d
from test_resize_host import restated_resize

DEV = "cuda"
DTS = (torch.float32, torch.bfloat16, torch.float16)
# (source, crop): an even crop of vector-aligned rows (the last strip of a row is partial), an odd crop, an uncropped frame several column
# tiles wide (the all-vector path), rows of odd length (element loads as well as element stores), and a frame three column tiles wide for
# the LDS form too (its tiles are 1024 pixels)
CASES = (((2, 3, 40, 72), (37, 70)), ((2, 3, 40, 72), (37, 71)), ((1, 3, 10, 600), None), ((1, 3, 9, 75), None), ((1, 3, 5, 2100), None))
GPU_SIZES = SIZES + (18,)        # 17 is the largest table of the LDS form, 18 the smallest of the gather form


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


_WANT = {}


def want32(shape, crop, n, dt, kind):
    """The fp32 restatement of one case, computed once."""
    key = (shape, crop, n, dt, kind)
    if key not in _WANT:
        _WANT[key] = restated_lut3d(lut_source(shape, crop, n, dt), (lut_random if kind == "random" else lut_identity)(n), crop)
    return _WANT[key]


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("random", "identity"))
@pytest.mark.parametrize("n", GPU_SIZES)
@pytest.mark.parametrize("dt", DTS)
def test_lut3d_equals_restatement(hip, dt, n, kind):
    lut = (lut_random if kind == "random" else lut_identity)(n)
    for shape, crop in CASES:
        y = lut_source(shape, crop, n, dt)
        want = want32(shape, crop, n, dt, kind)
        assert not torch.isnan(want).any()                                   # the NaN outside the crop and the planted NaN never reach the result
        got = ops.lut3d(y.to(DEV), lut, crop_hw=crop)
        assert same(got, want), (shape, crop, int((got.cpu() != want).sum()), float((got.cpu() - want).abs().max()))
        if dt != torch.float32:
            got = ops.lut3d(y.to(DEV), lut, crop_hw=crop, out_dtype=dt)
            assert same(got, want.to(dt)), (shape, crop, int((got.cpu() != want.to(dt)).sum()))


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_within_the_rounding_bound_of_float64(hip, n):
    for kind, lut in (("random", lut_random(n)), ("identity", lut_identity(n))):
        for dt in DTS:
            for shape, crop in CASES[:3]:
                y = lut_source(shape, crop, n, dt)
                ref = restated_lut3d(y, lut, crop, torch.float64)
                got = ops.lut3d(y.to(DEV), lut, crop_hw=crop).cpu()
                err = (got.double() - ref).abs().max().item()
                print(f"N = {n} {kind} {dt} {shape} {crop}: max |gpu - float64| = {err:.3e}, bound {bound(lut):.3e}")
                assert err <= bound(lut), (kind, dt, shape, err)


# ---- 3. whole nets --------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def check_rendition(got, y, out):
    """One element of the ladder against the existing encoders applied to the restated look of the restated resize of the float result `y`."""
    t = y if out.resize is None else restated_resize(y, out.resize)
    if out.look is not None:
        t = restated_lut3d(t, out.look)
    t = t.to(DEV)
    if out.format is None:
        assert same(got, t)
    elif isinstance(out.format, str):
        assert same(got, ops.rgb_encode(t, 8 if out.format == "rgb8" else 16))
    else:
        want = ops.yuv_encode(t, out.format)
        assert isinstance(got, M.YuvFrames) and same(got.buffer, want.buffer) and len(got.planes) == len(want.planes)       # padding bytes included
        assert all(same(a.contiguous(), b.contiguous()) for a, b in zip(got.planes, want.planes))


@pytest.mark.gpu
def test_existing_routes_unchanged_then_forward_mosaic_with_looked_outputs(hip):
    """In one process: the default, rgb8 and nv12 routes of two nets before any looked call, the four-rung ladder of the issue, and the
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
    ladder = [M.Output(nv12), M.Output(nv12, M.Resize((72, 104)), look=lut_random(33)),
              M.Output("rgb8", M.Resize((36, 52), filter="bilinear"), look=lut_random(17)), M.Output(None, look=lut_random(2))]
    for net, (y, q8, f) in zip(nets, before):
        with torch.no_grad():
            outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
        assert isinstance(outs, list) and len(outs) == 4
        assert y.dtype == dt and y.shape == (2, 3, 144, 208)
        assert same(outs[0].buffer, f.buffer) and all(same(a.contiguous(), b.contiguous()) for a, b in zip(outs[0].planes, f.planes))
        assert outs[1].planes[0].shape == (2, 72, 104) and outs[2].shape == (2, 36, 52, 3) and outs[2].dtype == torch.uint8
        assert outs[3].shape == (2, 3, 144, 208) and outs[3].dtype == torch.float32
        for got, out in zip(outs, ladder):
            check_rendition(got, y.cpu(), out)
        plain = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(nv12, M.Resize((72, 104)))])[0]
        assert not same(plain.buffer, outs[1].buffer)                        # the look did something
    for net, (y, q8, f) in zip(nets, before):
        y2, q2, f2 = routes(net)
        assert same(y, y2) and same(q8, q2) and same(f.buffer, f2.buffer)
        assert same(q8, ops.rgb_encode(y, 8))


@pytest.mark.gpu
def test_graphed_looked_ladder_equals_eager(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    ladder = [M.Output(M.OutFormat("nv12", pitch_align=256, height_align=16)), M.Output(M.OutFormat("nv12"), M.Resize((40, 56)), look=lut_random(33)),
              M.Output(None, M.Resize((20, 28), filter="bilinear"), look=lut_random(17))]
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    flat = lambda outs: [outs[0].buffer.clone(), outs[1].buffer.clone(), outs[2].clone()]
    with torch.no_grad():
        e1 = flat(net.forward_mosaic(m1, None, coord, outputs=ladder))                            # also the warm-up: the tables are on the device
        e2 = flat(net.forward_mosaic(m2, None, coord, outputs=ladder))
    kept = dict(ops._LUT3D_TABLES)
    assert sum(1 for k in kept if k[0] in (lut_random(33), lut_random(17))) == 2
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, outputs=ladder))
    g1 = flat(call(m1, coord))
    g2 = flat(call(m2, coord))
    assert all(ops._LUT3D_TABLES[k] is v for k, v in kept.items()) and len(ops._LUT3D_TABLES) == len(kept)       # nothing was built again
    assert g1[0].shape == (2, 256 * 120) and g1[1].shape == (2, 56 * 60) and g1[2].shape == (2, 3, 20, 28)
    assert all(same(a, b) for a, b in zip(g1, e1)) and all(same(a, b) for a, b in zip(g2, e2))
    assert not any(torch.equal(a, b) for a, b in zip(g1, g2))
