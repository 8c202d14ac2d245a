"""GPU: output sharpening (rc_sharpen).  The yardstick is the elementwise fp32 torch restatement of the header's arithmetic in
sharpen_ref.py, computed on the CPU (never the kernel's own output): every sample is compared bit for bit, on sources that carry NaN,
infinities, flat patches, impulses, a checkerboard and edges in every direction, on frames narrower than the halo, on crops with NaN
outside, on the element path, and across the seams of the kernel's strips and bands."""
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import ops
from realcamnet_amd import sharpen as SH
from sharpen_ref import bound, restated_sharpen, sharpen_source
from test_lut3d_host import lut_random, restated_lut3d
from test_resize_host import restated_resize
from test_stats_host import restated_stats
from test_warp_host import restated_warp

DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PARAMS = (dict(amount=1.5, core=1 / 64, overshoot=0.0), dict(amount=8.0, core=0.0, overshoot=1 / 32))
# (source, crop): frames narrower or shorter than the halo; two frames cropped on an even and an odd width with NaN outside (the replicated
# border at a crop edge); rows of odd length (element loads and stores); five strips wide (seams at columns 248 k) and five bands tall
GEOMETRIES = (((1, 3, 1, 1), None), ((1, 3, 1, 7), None), ((1, 3, 7, 1), None), ((1, 3, 2, 3), None), ((2, 3, 40, 72), (37, 70)), ((2, 3, 40, 72), (37, 71)),
              ((1, 3, 9, 75), None), ((1, 3, 5, 1100), None), ((1, 3, 150, 9), None))
assert 1100 >= 3 * SH.WAVE_OUT and 150 >= 3 * SH.BAND_ROWS                   # three strips and three bands at least


def same_bits(got, want):
    """Equal as bit patterns (a -0.0 for a 0.0 would show); both hold no NaN."""
    got, want = got.cpu(), want.cpu()
    view = torch.int32 if want.dtype == torch.float32 else torch.int16
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(view), want.contiguous().view(view))


def tsame(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def clamped(y, crop=None):
    h, w = crop if crop is not None else y.shape[2:]
    return torch.nan_to_num(y[:, :, :h, :w].float(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0, 1)


_WANT = {}


def want_for(shape, crop, dt, quantised, sp):
    """The restatement of one case, computed once and shared."""
    key = (shape, crop, dt, quantised, sp)
    if key not in _WANT:
        _WANT[key] = restated_sharpen(sharpen_source(shape, crop, dt, quantised), sp, crop)
    return _WANT[key]


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_sharpen_equals_restatement(hip, dt, radius):
    for k, (shape, crop) in enumerate(GEOMETRIES):
        for q, kw in enumerate(PARAMS):
            sp = M.Sharpen(radius=radius, matrix=("bt709", "bt601", "bt2020")[(k + q) % 3], **kw)
            for quantised in (False, True):
                y = sharpen_source(shape, crop, dt, quantised)
                want = want_for(shape, crop, dt, quantised, sp)
                yd = y.to(DEV)
                got = ops.sharpen(yd, sp, crop_hw=crop)
                assert same_bits(got, want), (shape, crop, kw, quantised, "fp32 out", (got.cpu() - want).abs().max().item())
                if dt != torch.float32:
                    got = ops.sharpen(yd, sp, crop_hw=crop, out_dtype=dt)
                    assert same_bits(got, want.to(dt)), (shape, crop, kw, quantised, "source-type out")


@pytest.mark.gpu
def test_misaligned_base_takes_the_element_path(hip):
    """A source that starts one element off a vector boundary: the same values through element loads."""
    sp = M.Sharpen(1.5, 2, 1 / 64, 1 / 32)
    for dt in (torch.bfloat16, torch.float32):
        y = sharpen_source((1, 3, 12, 264), None, dt)
        buf = torch.empty(y.numel() + 1, dtype=dt, device=DEV)
        view = buf[1:].view(y.shape)
        view.copy_(y)
        assert view.data_ptr() % (4 * y.element_size()) != 0 and view.is_contiguous()
        assert same_bits(ops.sharpen(view, sp), want_for((1, 3, 12, 264), None, dt, False, sp))


# ---- 2. the exact properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("radius", (1, 2))
def test_exact_properties_on_the_device(hip, radius):
    shape, crop = (2, 3, 40, 600), (37, 599)
    for dt in DTYPES:
        y = sharpen_source(shape, crop, dt)
        yd, want = y.to(DEV), clamped(y, crop).to(DEV)
        # amount = 0 and core = 1 return the clamped input, NaN -> 0
        for sp in (M.Sharpen(0.0, radius, 0.0, 0.5), M.Sharpen(0.0, radius, 1 / 64, 0.0), M.Sharpen(8.0, radius, 1.0, 1.0), M.Sharpen(1.5, radius, 1.0, 0.0, "bt2020")):
            assert torch.equal(ops.sharpen(yd, sp, crop_hw=crop), want), (dt, sp)
        # every output is finite and lies in [0, 1], whatever the input holds
        for kw in PARAMS:
            out = ops.sharpen(yd, M.Sharpen(radius=radius, **kw), crop_hw=crop)
            assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    # a frame whose three planes are each constant returns the clamped input, for any amount, radius and overshoot
    for vals in ((0.25, 0.5, 0.75), (1.3, -0.2, 0.1), (float("nan"), 0.6, float("inf")), (1e-3, 0.999, 0.3333)):
        flat = torch.tensor(vals).view(1, 3, 1, 1).expand(2, 3, 70, 523).contiguous()
        for dt in DTYPES:
            fd, want = flat.to(DEV, dt), clamped(flat.to(dt)).to(DEV)
            for amount in (0.5, 8.0):
                for over in (0.0, 1 / 32, 1.0):
                    assert torch.equal(ops.sharpen(fd, M.Sharpen(amount, radius, 0.0, over)), want), (vals, dt, amount, over)


@pytest.mark.gpu
def test_device_within_the_rounding_bound_of_float64(hip):
    shape = (1, 3, 150, 600)
    y = sharpen_source(shape)
    for radius in (1, 2):
        for amount in (0.5, 2.0, 8.0):
            sp = M.Sharpen(amount, radius, 1 / 64, 1 / 32)
            ref = restated_sharpen(y, sp, dtype=torch.float64)
            err = (ops.sharpen(y.to(DEV), sp).cpu().double() - ref).abs().max().item()
            print(f"radius {radius}, amount {amount}: max |device - fp64| = {err * 2 ** 24:.2f} x 2^-24, bound {bound(sp) * 2 ** 24:.2f} x 2^-24")
            assert err <= bound(sp)


# ---- 3. what the stage is for -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_focus_figure_rises_and_amount_zero_leaves_it(hip):
    """A textured frame, softened as a scaler softens it: the gradient-energy focus figure of ops.frame_stats, summed over the zones, is
    strictly larger after the stage and exactly the same after amount = 0."""
    g = torch.Generator().manual_seed(21)
    tex = torch.rand(2, 3, 130, 258, generator=g) * 0.6 + 0.2
    soft = restated_resize(tex, M.Resize((65, 129))).to(DEV)                 # 2 x 2 box averages, in (0.2, 0.8)
    spec = M.Stats(grid=(4, 4))
    focus = lambda t: ops.frame_stats(t, spec).zones[..., 7].sum().item()
    base = focus(soft)
    sharp, none = focus(ops.sharpen(soft, M.Sharpen(1.5, 2))), focus(ops.sharpen(soft, M.Sharpen(0.0, 2)))
    print(f"focus {base} -> {sharp} (amount 1.5, radius 2), {none} (amount 0)")
    assert sharp > base and none == base


# ---- 4. whole nets --------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def stats_same(got, want):
    return torch.equal(got.hist.cpu(), want[0]) and torch.equal(got.zones.cpu(), want[1])


@pytest.mark.gpu
def test_existing_routes_unchanged_then_forward_mosaic_with_sharpened_outputs(hip):
    """In one process: the default, rgb8 and nv12 routes of two nets before any sharpened call, a five-rung ladder whose rungs are the
    existing encoders (or ops.frame_stats) of the restated stages, and the same routes again afterwards."""
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
    look, src = lut_random(17), (144, 208)
    warp = M.Warp.rotate90(src, 1)
    s1, s2, s3 = M.Sharpen(1.5, 2, 1 / 64), M.Sharpen(8.0, 1, 0.0, 1 / 32, "bt601"), M.Sharpen(2.0, 2, 1 / 256, 1 / 64, "bt2020")
    ladder = [M.Output(nv12), M.Output(nv12, M.Resize((72, 104)), look, sharpen=s1), M.Output("rgb8", M.Resize((36, 52), filter="bilinear"), sharpen=s2),
              M.Output(None, warp=warp, sharpen=s3), M.Output(M.Stats(grid=(3, 5), bits=10), M.Resize((72, 104)), sharpen=s1)]
    twins = [M.Output(o.format, o.resize, o.look, o.warp) for o in ladder]
    for net, (y, q8, f) in zip(nets, before):
        with torch.no_grad():
            outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
            plain = net.forward_mosaic(mosaic, None, coord, outputs=twins)
        assert isinstance(outs, list) and len(outs) == 5 and y.dtype == dt and y.shape == (2, 3, 144, 208)
        assert tsame(outs[0].buffer, f.buffer) and all(tsame(a.contiguous(), b.contiguous()) for a, b in zip(outs[0].planes, f.planes))
        yc = y.cpu()
        r1 = restated_sharpen(restated_lut3d(restated_resize(yc, ladder[1].resize), look), s1)
        assert tsame(outs[1].buffer, ops.yuv_encode(r1.to(DEV), nv12).buffer)
        r2 = restated_sharpen(restated_resize(yc, ladder[2].resize), s2)
        assert tsame(outs[2], ops.rgb_encode(r2.to(DEV), 8))
        r3 = restated_sharpen(restated_warp(yc, warp.mesh, warp.size, warp.cell, warp.interp, warp.border, warp.fill), s3)
        assert outs[3].dtype == torch.float32 and outs[3].shape == (2, 3, 208, 144) and same_bits(outs[3], r3)
        r4 = restated_sharpen(restated_resize(yc, ladder[4].resize), s1)
        assert isinstance(outs[4], M.FrameStats) and stats_same(outs[4], restated_stats(r4, ladder[4].format))
        # a sharpened rung differs from its unsharpened twin
        assert not torch.equal(outs[1].buffer, plain[1].buffer) and not torch.equal(outs[2], plain[2]) and not torch.equal(outs[3], plain[3].float())
        assert not torch.equal(outs[4].zones, plain[4].zones) and tsame(outs[0].buffer, plain[0].buffer)
    for net, (y, q8, f) in zip(nets, before):
        y2, q2, f2 = routes(net)
        assert tsame(y, y2) and tsame(q8, q2) and tsame(f.buffer, f2.buffer)
        assert tsame(q8, ops.rgb_encode(y, 8))


# ---- 5. graph replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_sharpened_ladder_equals_eager(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    sp = M.Sharpen(1.5, 2, 1 / 64, 1 / 32)
    ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.OutFormat("nv12"), M.Resize((40, 56)), sharpen=sp), M.Output(None, M.Resize((20, 28), filter="bilinear"), sharpen=M.Sharpen(4.0, 1))]
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = (torch.rand(2, 1, 80, 112, generator=g) * 0.5).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    flat = lambda outs: [outs[0].buffer.clone(), outs[1].buffer.clone(), outs[2].clone()]
    with torch.no_grad():
        e1 = flat(net.forward_mosaic(m1, None, coord, outputs=ladder))
        e2 = flat(net.forward_mosaic(m2, None, coord, outputs=ladder))
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, outputs=ladder))
    g1 = flat(call(m1, coord))
    g2 = flat(call(m2, coord))
    assert all(tsame(a, b) for a, b in zip(g1, e1)) and all(tsame(a, b) for a, b in zip(g2, e2))
    assert not any(torch.equal(a, b) for a, b in zip(g1, g2))
