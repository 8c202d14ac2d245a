"""GPU: geometric correction (rc_warp).  The yardstick is the elementwise fp32 torch restatement of the header's arithmetic in
test_warp_host.py (never the kernel's own output): every sample is compared bit for bit, the sign of a zero included; a float64
evaluation of the same formula bounds what fp32 costs; the exact cases; whole nets with warped outputs against the hand composition, a
graphed ladder, and the routes that were there before."""
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import ops
from test_warp_host import BORDERS, FILL, GEOMETRIES, INTERPS, bits, bound, restated_warp, warp_mesh, warp_source

DEV = "cuda"
DTS = (torch.float32, torch.bfloat16, torch.float16)
# (source, frame = crop, output): a perturbed mesh over a cropped frame; an upscale; several column tiles of all-vector rows; odd rows
# (element stores, a partial last strip); a one-pixel source (every tap clamps); a single output pixel
CASES = (((2, 3, 40, 72), (37, 70), (37, 70)), ((1, 3, 33, 50), None, (48, 64)), ((1, 3, 9, 600), None, (9, 600)), ((1, 3, 9, 75), None, (11, 77)),
         ((1, 3, 1, 1), None, (5, 5)), ((1, 3, 9, 75), None, (1, 1)))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def frame_of(shape, crop):
    return crop if crop is not None else tuple(shape[2:])


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cell", (8, 64))
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("dt", DTS)
def test_warp_equals_restatement(hip, dt, interp, border, cell):
    for shape, crop, size in CASES:
        frame = frame_of(shape, crop)
        y = warp_source(shape, crop, dt)
        wp = M.Warp(warp_mesh(frame, size, cell)[0].numpy(), size, cell, interp, border, FILL)
        want = restated_warp(y, wp.mesh, size, cell, interp, border, FILL, crop)
        assert not torch.isnan(want).any()                                   # the NaN outside the frame never reaches the result
        got = ops.warp(y.to(DEV), wp, crop_hw=crop)
        assert same_bits(got, want), (shape, crop, size, int((bits(got.cpu()) != bits(want)).sum()), float((got.cpu() - want).abs().max()))
        if dt != torch.float32:
            got = ops.warp(y.to(DEV), wp, crop_hw=crop, out_dtype=dt)
            assert same_bits(got, want.to(dt)), (shape, crop, size, int((bits(got.cpu()) != bits(want.to(dt))).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_one_mesh_per_frame(hip, interp):
    shape, crop, size, cell = (2, 3, 40, 72), (37, 70), (37, 70), 8
    mesh = warp_mesh(crop, size, cell, batch=2, seed=1)
    assert not torch.equal(mesh[0], mesh[1])
    for dt in (torch.float32, torch.bfloat16):
        y = warp_source(shape, crop, dt)
        want = restated_warp(y, mesh, size, cell, interp, "constant", FILL, crop)
        got = ops.warp(y.to(DEV), mesh.to(DEV), size=size, cell=cell, interp=interp, border="constant", fill=FILL, crop_hw=crop)
        assert same_bits(got, want)
        first = ops.warp(y.to(DEV), mesh[0].to(DEV), size=size, cell=cell, interp=interp, border="constant", fill=FILL, crop_hw=crop)       # (Gh, Gw, 2): shared
        assert same_bits(first[0], want[0]) and not same_bits(first[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_device_mesh_with_non_finite_nodes_is_guarded(hip, interp, border):
    """Step 2: NaN, +inf, -inf and 1e30 at nodes of a device mesh.  The frame sits inside a larger NaN-filled source, so a read outside
    the frame that counted would show; the result equals the restatement and is finite."""
    shape, crop, size, cell = (2, 3, 40, 72), (37, 70), (37, 70), 8
    mesh = warp_mesh(crop, size, cell, batch=2, seed=2).clone()
    nan, inf = float("nan"), float("inf")
    for k, (j, i, c, v) in enumerate(((0, 0, 0, nan), (1, 2, 1, nan), (2, 4, 0, inf), (2, 5, 1, inf), (3, 7, 0, -inf), (4, 1, 1, -inf), (5, 9, 0, 1e30), (5, 0, 1, -1e30),
                                      (3, 3, 0, inf), (3, 3, 1, -inf), (1, 8, 0, 3e38), (0, 6, 1, nan))):
        mesh[k % 2, j, i, c] = v
    for dt in DTS:
        y = warp_source(shape, crop, dt)
        want = restated_warp(y, mesh, size, cell, interp, border, FILL, crop)
        assert torch.isfinite(want).all()
        got = ops.warp(y.to(DEV), mesh.to(DEV), size=size, cell=cell, interp=interp, border=border, fill=FILL, crop_hw=crop)
        assert same_bits(got, want), int((bits(got.cpu()) != bits(want)).sum())


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_within_the_rounding_bound_of_float64(hip, interp, border):
    for shape, crop, size, cell in GEOMETRIES:
        frame = frame_of(shape, crop)
        mesh = warp_mesh(frame, size, cell)
        for dt in DTS:
            y = warp_source(shape, crop, dt)
            ref = restated_warp(y, mesh, size, cell, interp, border, FILL, crop, torch.float64)
            got = ops.warp(y.to(DEV), mesh.to(DEV), size=size, cell=cell, interp=interp, border=border, fill=FILL, crop_hw=crop).cpu()
            err, lim = (got.double() - ref).abs().max().item(), bound(y, mesh, frame, interp, border, FILL)
            print(f"{interp} {border} {dt} {frame} -> {size}: max |gpu - float64| = {err:.3e}, bound {lim:.3e}")
            assert err <= lim, (dt, frame, err)


# ---- 3. exact cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_identity_turns_and_flips_on_the_gpu(hip, interp):
    for dt in DTS:
        y = warp_source((2, 3, 37, 70), None, dt).to(DEV)
        for cell in (8, 32):
            assert same(ops.warp(y, M.Warp.identity((37, 70), cell, interp=interp), out_dtype=dt), y)
        for k in range(4):
            assert same(ops.warp(y, M.Warp.rotate90((37, 70), k, cell=8, interp=interp), out_dtype=dt), torch.rot90(y, k, dims=(-2, -1)).contiguous())
        assert same(ops.warp(y, M.Warp.flip((37, 70), interp=interp), out_dtype=dt), torch.flip(y, dims=(-1,)))
        assert same(ops.warp(y, M.Warp.flip((37, 70), horizontal=False, interp=interp, border="constant"), out_dtype=dt), torch.flip(y, dims=(-2,)))


# ---- 4. whole nets --------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def lut_random(n):
    g = torch.Generator().manual_seed(2000 + n)
    return M.Lut3D((torch.rand(n, n, n, 3, generator=g) * 2 - 0.5).numpy())


def by_hand(y, out):
    """ops.warp -> ops.resize -> ops.lut3d -> the encoder, on the float result `y`."""
    t = y if out.warp is None else ops.warp(y, out.warp)
    t = t if out.resize is None else ops.resize(t, out.resize)
    t = t if out.look is None else ops.lut3d(t, out.look)
    if out.format is None:
        return t
    return ops.rgb_encode(t, 8 if out.format == "rgb8" else 16) if isinstance(out.format, str) else ops.yuv_encode(t, out.format)


def same_output(got, want):
    if isinstance(want, M.YuvFrames):
        return isinstance(got, M.YuvFrames) and same(got.buffer, want.buffer) and all(same(a.contiguous(), b.contiguous()) for a, b in zip(got.planes, want.planes))
    return same(got, want)


def lens(size, source, **kw):
    h, w = source
    return M.Warp.lens(size, source, fx=0.8 * w, fy=0.8 * w, cx=(w - 1) / 2, cy=(h - 1) / 2, k1=-0.12, k2=0.02, p1=1e-3, p2=-5e-4,
                       out_fx=0.8 * w * size[1] / w, out_fy=0.8 * w * size[0] / h, out_cx=(size[1] - 1) / 2, out_cy=(size[0] - 1) / 2, **kw)


@pytest.mark.gpu
def test_existing_routes_unchanged_then_forward_mosaic_with_warped_outputs(hip):
    """In one process: the default, rgb8 and nv12 routes and an unwarped ladder of two nets before any warped call, the warped ladder against
    the hand composition, and the same routes again afterwards."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(7)
    mosaic = (torch.rand(2, 1, 144, 208, generator=g) * 1.4 - 0.2).to(DEV, dt)
    coord = O.make_coord(2, 72, 104).to(DEV, dt)
    nv12 = M.OutFormat("nv12")
    nets = [net_on_gpu(n, dt) for n in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC")]
    plain = [M.Output(nv12), M.Output(nv12, M.Resize((72, 104)), look=lut_random(33)), M.Output(None, M.Resize((36, 52), filter="bilinear"))]

    def routes(net):
        with torch.no_grad():
            return (net.forward_mosaic(mosaic, None, coord), net.forward_mosaic(mosaic, None, coord, out_format="rgb8"),
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12), net.forward_mosaic(mosaic, None, coord, outputs=plain))
    before = [routes(n) for n in nets]
    src = (144, 208)
    ladder = [M.Output(nv12, warp=lens(src, src, interp="bicubic")),
              M.Output(nv12, M.Resize((104, 72)), lut_random(33), M.Warp.rotate90(src, 1)),
              M.Output("rgb8", None, lut_random(17), lens((201, 301), src, cell=32, border="constant", fill=FILL)),
              M.Output(None, M.Resize((36, 52), roi=(10, 20, 120, 160), filter="bilinear"), warp=lens(src, src, cell=8, interp="bicubic", border="constant"))]
    for net, (y, q8, f, pl) in zip(nets, before):
        assert y.dtype == dt and y.shape == (2, 3, 144, 208)
        assert same(q8, ops.rgb_encode(y, 8)) and same_output(f, ops.yuv_encode(y, nv12)) and all(same_output(a, by_hand(y, o)) for a, o in zip(pl, plain))
        with torch.no_grad():
            outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
        assert isinstance(outs, list) and len(outs) == 4
        assert outs[0].planes[0].shape == (2, 144, 208) and outs[1].planes[0].shape == (2, 104, 72) and outs[2].shape == (2, 201, 301, 3)
        assert outs[3].shape == (2, 3, 36, 52) and outs[3].dtype == torch.float32
        for got, out in zip(outs, ladder):
            assert same_output(got, by_hand(y, out))
        assert not same(outs[0].buffer, f.buffer)                            # the warp did something
        w = ladder[0].warp                                                   # and the stage inside the net is the restated one
        assert same_bits(ops.warp(y, w), restated_warp(y.cpu(), w.mesh, w.size, w.cell, w.interp, w.border, w.fill))
    for net, (y, q8, f, pl) in zip(nets, before):
        y2, q2, f2, pl2 = routes(net)
        assert same(y, y2) and same(q8, q2) and same(f.buffer, f2.buffer) and all(same_output(a, b) for a, b in zip(pl, pl2))


@pytest.mark.gpu
def test_graphed_warped_ladder_equals_eager(hip):
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    src = (80, 112)
    ladder = [M.Output(M.OutFormat("nv12", pitch_align=256, height_align=16), warp=lens(src, src)),
              M.Output(M.OutFormat("nv12"), M.Resize((56, 40)), lut_random(33), M.Warp.rotate90(src, 3, interp="bicubic")),
              M.Output(None, M.Resize((20, 28), filter="bilinear"), warp=lens(src, src, cell=8, interp="bicubic", border="constant", fill=FILL))]
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    flat = lambda outs: [outs[0].buffer.clone(), outs[1].buffer.clone(), outs[2].clone()]
    with torch.no_grad():
        e1 = flat(net.forward_mosaic(m1, None, coord, outputs=ladder))                            # also the warm-up: the meshes are on the device
        kept = dict(ops._WARP_MESHES)
        assert sum(1 for k in kept if k[0] in [o.warp for o in ladder]) == 3
        e2 = flat(net.forward_mosaic(m2, None, coord, outputs=ladder))
    assert all(ops._WARP_MESHES[k] is v for k, v in kept.items()) and len(ops._WARP_MESHES) == len(kept)         # a second call adds no entry
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, outputs=ladder))
    g1 = flat(call(m1, coord))
    g2 = flat(call(m2, coord))
    assert all(ops._WARP_MESHES[k] is v for k, v in kept.items()) and len(ops._WARP_MESHES) == len(kept)         # nothing was built again
    assert g1[0].shape == (2, 256 * 120) and g1[1].shape == (2, 40 * 84) and g1[2].shape == (2, 3, 20, 28)
    assert all(same(a, b) for a, b in zip(g1, e1)) and all(same(a, b) for a, b in zip(g2, e2))
    assert not any(torch.equal(a, b) for a, b in zip(g1, g2))
