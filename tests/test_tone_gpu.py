"""GPU: local tone mapping (rc_tone_hist / rc_tone_gains / rc_tone_apply).  The yardstick is the elementwise torch restatement of the
header's arithmetic in tone_ref.py, computed on the CPU (never the kernel's own output): every histogram count and every gain and
output sample is compared bit for bit, on sources that carry NaN, infinities, flat patches and gradients, on crops with NaN outside, on
the element path, on tiles of one pixel, and across the seams of the kernels' strips, bands and slabs."""
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import ops
from realcamnet_amd import tone as TN
from sharpen_ref import restated_sharpen
from test_resize_host import restated_resize
from test_stats_host import restated_stats
from tone_ref import clamped, restated_apply, restated_gains, restated_hist, restated_tone_map, tone_source

DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# (source, crop, grid): one pixel; one pixel per tile; tile widths of 4 and 5 on rows of odd length; two frames cropped with NaN outside;
# four strips wide; several bands tall
GEOMETRIES = (((1, 3, 1, 1), None, (1, 1)), ((1, 3, 5, 5), None, (5, 5)), ((1, 3, 9, 75), None, (4, 16)), ((2, 3, 40, 72), (37, 71), (3, 4)),
              ((1, 3, 5, 1100), None, (2, 16)), ((1, 3, 150, 9), None, (16, 2)))
assert 1100 > 4 * TN.WAVE_SPAN and 150 > 2 * TN.BAND_ROWS and 150 > 4 * TN.HIST_ROWS
PARAMS = (dict(), dict(clip=1.25, strength=0.75, max_gain=3.0), dict(clip=256.0, max_gain=64.0))


def same_bits(got, want):
    """Equal as bit patterns (a -0.0 for a 0.0 would show); both hold no NaN."""
    got, want = got.cpu(), want.cpu()
    view = torch.int32 if want.dtype == torch.float32 else torch.int16
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(view), want.contiguous().view(view))


def tsame(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


_WANT = {}


def want_for(shape, crop, dt, tm):
    """(hist, gains, out) of the restatement of one case, computed once and shared."""
    key = (shape, crop, dt, tm)
    if key not in _WANT:
        y = tone_source(shape, crop, dt)
        hist = restated_hist(y, tm, crop)
        gains = restated_gains(hist, tm)
        _WANT[key] = (hist, gains, restated_apply(y, gains, tm, crop))
    return _WANT[key]


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_the_three_ops_and_tone_map_equal_the_restatement(hip, dt):
    for k, (shape, crop, grid) in enumerate(GEOMETRIES):
        for q, kw in enumerate(PARAMS):
            tm = M.ToneMap(grid=grid, matrix=("bt709", "bt601", "bt2020")[(k + q) % 3], **kw)
            hist, gains, out = want_for(shape, crop, dt, tm)
            yd = tone_source(shape, crop, dt).to(DEV)
            got_h = ops.tone_hist(yd, tm, crop_hw=crop)
            assert tsame(got_h, hist), (shape, crop, kw, "hist")
            got_g = ops.tone_gains(got_h, tm)
            assert same_bits(got_g, gains), (shape, crop, kw, "gains", (got_g.cpu() - gains).abs().max().item())
            got = ops.tone_apply(yd, got_g, tm, crop_hw=crop)
            assert same_bits(got, out), (shape, crop, kw, "apply", (got.cpu() - out).abs().max().item())
            assert same_bits(ops.tone_map(yd, tm, crop_hw=crop), out), (shape, crop, kw, "tone_map")
            if dt != torch.float32:
                assert same_bits(ops.tone_map(yd, tm, crop_hw=crop, out_dtype=dt), out.to(dt)), (shape, crop, kw, "source-type out")


@pytest.mark.gpu
def test_a_flat_frame_counts_past_16_bits(hip):
    """67 600 pixels in one bin of one tile: a counter narrower than 32 bits would show."""
    tm = M.ToneMap(grid=(1, 1))
    for dt in DTYPES:
        y = torch.full((1, 3, 260, 260), 0.25).to(dt)
        hist = restated_hist(y, tm)
        assert hist.max().item() == 260 * 260 and (hist != 0).sum().item() == 1
        got = ops.tone_hist(y.to(DEV), tm)
        assert tsame(got, hist)
        assert same_bits(ops.tone_map(y.to(DEV), tm), restated_apply(y, restated_gains(hist, tm), tm))


@pytest.mark.gpu
def test_misaligned_base_takes_the_element_path(hip):
    """A source that starts one element off a vector boundary: the same values through element loads."""
    tm = M.ToneMap(grid=(2, 3), clip=1.5)
    shape = (1, 3, 12, 264)
    for dt in (torch.bfloat16, torch.float32):
        y = tone_source(shape, None, dt)
        buf = torch.empty(y.numel() + 1, dtype=dt, device=DEV)
        view = buf[1:].view(y.shape)
        view.copy_(y)
        assert view.data_ptr() % (4 * y.element_size()) != 0 and view.is_contiguous()
        hist, gains, out = want_for(shape, None, dt, tm)
        assert tsame(ops.tone_hist(view, tm), hist) and same_bits(ops.tone_map(view, tm), out)


# ---- 2. the exact properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_properties_on_the_device(hip):
    # strength = 0 returns the clamped input, NaN -> 0, whatever the grid and the clip
    for shape, crop, grid in (((2, 3, 40, 600), (37, 599), (3, 7)), ((1, 3, 150, 9), None, (16, 2)), ((1, 3, 5, 5), None, (5, 5))):
        for dt in DTYPES:
            y = tone_source(shape, crop, dt, dark=False)
            yd, want = y.to(DEV), clamped(y, crop).contiguous()
            for clip in (1.0, 2.0, 256.0):
                assert same_bits(ops.tone_map(yd, M.ToneMap(grid=grid, clip=clip, strength=0.0), crop_hw=crop), want), (shape, dt, clip)
    # a frame that repeats one 9 x 13 tile 3 x 4 times with grid (3, 4) equals the tile mapped with grid (1, 1), repeated
    g = torch.Generator().manual_seed(2)
    for kw in (dict(), dict(clip=1.25, strength=0.5, matrix="bt601"), dict(clip=256.0, max_gain=64.0)):
        tile = (torch.rand(2, 3, 9, 13, generator=g) * 0.3).to(DEV)
        one = ops.tone_map(tile, M.ToneMap(grid=(1, 1), **kw))
        assert same_bits(one, restated_tone_map(tile.cpu(), M.ToneMap(grid=(1, 1), **kw)))
        assert torch.equal(ops.tone_map(tile.repeat(1, 1, 3, 4), M.ToneMap(grid=(3, 4), **kw)), one.repeat(1, 1, 3, 4))
    # every output is finite and lies in [0, 1], whatever the input holds
    y = tone_source((2, 3, 40, 600), (37, 599), torch.float32, dark=False).to(DEV)
    out = ops.tone_map(y, M.ToneMap(grid=(3, 7), clip=256.0, max_gain=64.0), crop_hw=(37, 599))
    assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1


# ---- 3. the gains between the launches ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shared_gains_and_gains_written_in_place(hip):
    shape, crop, tm = (2, 3, 40, 72), (37, 71), M.ToneMap(grid=(3, 4))
    y = tone_source(shape, crop, torch.bfloat16)
    yd = y.to(DEV)
    gains = restated_gains(restated_hist(y, tm, crop), tm)
    # one set of tables for both frames
    shared = gains[1:2].contiguous()
    assert same_bits(ops.tone_apply(yd, shared.to(DEV), tm, crop_hw=crop), restated_apply(y, shared, tm, crop))
    # the tables are read when the kernel runs: a temporal smoothing written in place between two calls is what the second call uses
    state = gains.to(DEV)
    first = ops.tone_apply(yd, state, tm, crop_hw=crop)
    target = torch.ones_like(gains)
    state.lerp_(target.to(DEV), 0.25)
    second = ops.tone_apply(yd, state, tm, crop_hw=crop)
    assert same_bits(first, restated_apply(y, gains, tm, crop)) and same_bits(second, restated_apply(y, state.cpu(), tm, crop)) and not torch.equal(first, second)


@pytest.mark.gpu
def test_two_runs_of_tone_hist_on_noise_are_equal(hip):
    g = torch.Generator().manual_seed(9)
    y = torch.rand(2, 3, 300, 520, generator=g).to(DEV, torch.bfloat16)
    tm = M.ToneMap(grid=(8, 8))
    a, b = ops.tone_hist(y, tm), ops.tone_hist(y, tm)
    assert torch.equal(a, b) and a.sum().item() == 2 * 300 * 520 and tsame(a, restated_hist(y.cpu(), tm))


# ---- 4. graph replay and whole nets -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_tone_map_replays_on_a_rewritten_input(hip):
    tm = M.ToneMap(grid=(3, 4), clip=1.5)
    shape, crop = (2, 3, 40, 72), (37, 71)
    y1, y2 = tone_source(shape, crop, torch.bfloat16), tone_source(shape, crop, torch.bfloat16, seed=1, dark=False)
    w1, w2 = restated_tone_map(y1, tm, crop), restated_tone_map(y2, tm, crop)
    call = M.GraphedCall(lambda x: ops.tone_map(x, tm, crop_hw=crop))
    assert same_bits(call(y1.to(DEV)).clone(), w1) and same_bits(call(y2.to(DEV)).clone(), w2) and not torch.equal(w1, w2)
    # the same under a bare torch.cuda.graph: the memset of tone_hist and the three launches are captured
    x = y1.to(DEV)
    ops.tone_map(x, tm, crop_hw=crop)                                        # warm: the axis tables are on the device
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.tone_map(x, tm, crop_hw=crop)
    x.copy_(y2.to(DEV))
    graph.replay()
    assert same_bits(out, w2)
    x.copy_(y1.to(DEV))
    graph.replay()
    assert same_bits(out, w1)


@pytest.mark.gpu
def test_forward_mosaic_with_tone_mapped_outputs(hip):
    """The smallest net at 32 x 32: the rungs equal the existing encoders (or ops.frame_stats) of the restated stages, and an Output
    without the field returns what it returned before."""
    dt = torch.bfloat16
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=dt).eval()
    g = torch.Generator().manual_seed(7)
    mosaic = (torch.rand(2, 1, 32, 32, generator=g) * 0.4).to(DEV, dt)
    coord = O.make_coord(2, 16, 16).to(DEV, dt)
    t1, t2, sp = M.ToneMap(grid=(2, 2)), M.ToneMap(grid=(4, 3), clip=3.0, strength=0.5, matrix="bt601"), M.Sharpen(1.5, 1, 1 / 64)
    ladder = [M.Output("rgb8", M.Resize((16, 16)), tone=t1, sharpen=sp), M.Output(M.Stats(grid=(2, 2)), tone=t2), M.Output("rgb8", M.Resize((16, 16)), sharpen=sp), M.Output(None)]
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord)
        q8 = net.forward_mosaic(mosaic, None, coord, out_format="rgb8")
        before = net.forward_mosaic(mosaic, None, coord, outputs=[ladder[2], ladder[3]])
        outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
        after = net.forward_mosaic(mosaic, None, coord, outputs=[ladder[2], ladder[3]])
    assert y.shape == (2, 3, 32, 32) and y.dtype == dt
    yc = y.cpu()
    r0 = restated_sharpen(restated_tone_map(restated_resize(yc, ladder[0].resize), t1), sp)
    assert tsame(outs[0], ops.rgb_encode(r0.to(DEV), 8))
    want_h, want_z = restated_stats(restated_tone_map(yc, t2), ladder[1].format)
    assert isinstance(outs[1], M.FrameStats) and torch.equal(outs[1].hist.cpu(), want_h) and torch.equal(outs[1].zones.cpu(), want_z)
    r2 = restated_sharpen(restated_resize(yc, ladder[2].resize), sp)
    assert tsame(outs[2], ops.rgb_encode(r2.to(DEV), 8)) and not torch.equal(outs[0], outs[2])         # the tone-mapped rung differs from its twin
    for pair in (before, after):
        assert tsame(pair[0], outs[2]) and tsame(pair[1], y) and tsame(outs[3], y)
    assert tsame(q8, ops.rgb_encode(y, 8))
