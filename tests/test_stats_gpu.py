"""GPU: frame statistics (rc_frame_stats).  The yardstick is the elementwise torch restatement of the header's arithmetic in
test_stats_host.py, computed on the CPU (never the kernel's own output); the existing encoders are a second one.  Every comparison is
torch.equal on int64: the sums are integer, so there is no tolerance anywhere."""
import ctypes as C

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from test_lut3d_host import lut_random, restated_lut3d
from test_resize_host import restated_resize
from test_stats_host import DTYPES, restated_stats, stats_source

DEV = "cuda"
MATRICES = ("bt601", "bt709", "bt2020")
# (source, crop, roi, grids): a cropped frame with an inner ROI whose origin and width are odd (element loads, partial last strip, zones
# that cut a lane's four pixels); a frame three tiles wide (the all-vector path, lane 63's neighbour in the next tile) with one zone and
# with one-row zones of 9.4 columns; rows of odd length with zones of 1.2 columns; a frame nine tiles wide; a single pixel
CASES = (((2, 3, 40, 72), (37, 71), (1, 2, 35, 67), ((5, 7),)), ((1, 3, 10, 600), None, None, ((1, 1), (10, 64))), ((1, 3, 9, 75), None, None, ((9, 64),)),
         ((1, 3, 5, 2100), None, None, ((3, 64),)), ((1, 3, 1, 1), None, None, ((1, 1),)))


def same(got, want):
    hist, zones = want
    return (got.hist.dtype == got.zones.dtype == torch.int64 and got.hist.shape == hist.shape and got.zones.shape == zones.shape
            and torch.equal(got.hist.cpu(), hist) and torch.equal(got.zones.cpu(), zones))


def diff(got, want):
    return int((got.hist.cpu() != want[0]).sum()), int((got.zones.cpu() != want[1]).sum()), (got.zones.cpu() - want[1]).flatten(0, 2).abs().amax(0).tolist()


def thresholds_on_codes(hist, bits):
    """A (dark, clip) pair that sits exactly on codes present in the frame: the largest luma code of the lowest tenth, the smallest red code
    of the highest tenth (any present code where a tenth is empty)."""
    S = (1 << bits) - 1
    ycodes, rcodes = hist[:, 3].sum(0).nonzero().flatten(), hist[:, 0].sum(0).nonzero().flatten()
    low, high = ycodes[ycodes <= S // 10], rcodes[(rcodes >= S - S // 10) & (rcodes >= 1)]
    dark = int(low.max()) if len(low) else int(ycodes.min())
    clip = int(high.min()) if len(high) else max(1, int(rcodes.max()))
    return dark, clip


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("bits", (8, 10))
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_frame_stats_equals_restatement(hip, dt, bits, matrix):
    for shape, crop, roi, grids in CASES:
        y = stats_source(shape, crop, roi, dt)
        yd = y.to(DEV)
        for grid in grids:
            plain = M.Stats(grid=grid, bits=bits, matrix=matrix, roi=roi)
            want = restated_stats(y, plain, crop)
            got = ops.frame_stats(yd, plain, crop_hw=crop)
            assert same(got, want), (shape, grid, "no thresholds", diff(got, want))
            assert got.roi == plain.check(*(crop or shape[2:])) and got.spec is plain
            dark, clip = thresholds_on_codes(want[0], bits)
            spec = M.Stats(grid=grid, bits=bits, matrix=matrix, roi=roi, dark=dark, clip=clip)
            want = restated_stats(y, spec, crop)
            if shape[2] * shape[3] > 1:
                assert want[1][..., 5].sum() > 0 and want[1][..., 6].sum() > 0                   # both classes occur
            got = ops.frame_stats(yd, spec, crop_hw=crop)
            assert same(got, want), (shape, grid, (dark, clip), diff(got, want))
            assert torch.equal(got.zone_pixels, want[1][0][..., [0, 5, 6]].sum(-1))


# ---- 2. overflow ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_focus_sum_above_32_bits(hip):
    """A 10-bit checkerboard of 0 and 1: every difference is +-1023, so the one zone's focus sum is about 64 x 256 x 2 x 1023^2 = 3.4e10."""
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(256), indexing="ij")
    y = ((yy + xx) % 2).float().expand(1, 3, 64, 256).contiguous()
    spec = M.Stats(grid=(1, 1), bits=10)
    want = restated_stats(y, spec)
    assert want[1][0, 0, 0, 7] == (63 * 256 + 64 * 255) * 1023 ** 2 > 1 << 32
    for dt in DTYPES:
        got = ops.frame_stats(y.to(DEV, dt), spec)
        assert same(got, want), (dt, diff(got, want))


@pytest.mark.gpu
def test_sums_of_a_whole_1080p_zone_and_uneven_tiles(hip):
    """An all-ones 1080p frame at 10 bits, one zone: the luma sum and each colour sum is 1080 x 1920 x 1023 = 2.12e9, 99 % of 2^31: what a
    32-bit partial of the whole frame could just hold, and no partial in the kernel has to.
    The kernel's tiles are 256 columns x 64 rows: ceil(1920 / 256) x ceil(1080 / 64) = 8 x 17 = 136 per frame, walked by
    min(4 x CUs, 136 // 3) = 45 blocks on any device of 12 CUs or more: 136 = 3 x 45 + 1, so every block walks at least three tiles, one
    walks four, and the tile count is no multiple of the block count."""
    y = torch.ones(1, 3, 1080, 1920, dtype=torch.bfloat16)
    spec = M.Stats(grid=(1, 1), bits=10)
    want = restated_stats(y, spec)
    n = 1080 * 1920
    assert want[1].flatten().tolist() == [n, n * 1023, n * 1023, n * 1023, n * 1023, 0, 0, 0] and n * 1023 > 2.1e9
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 12
    got = ops.frame_stats(y.to(DEV), spec)
    assert same(got, want), diff(got, want)
    grid = M.Stats(grid=(64, 64), bits=10, dark=1023, clip=1024)                                 # every pixel dark, 64 x 64 zones of 16.9 x 30 pixels
    got, want = ops.frame_stats(y.to(DEV), grid), restated_stats(y, grid)
    assert same(got, want), diff(got, want)
    assert torch.equal(got.zones[0, :, :, 6].cpu(), got.zone_pixels)


# ---- 3. contention --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bits", (8, 10))
def test_flat_frame(hip, bits):
    """Every pixel one value: every lane of every wave counts into the same four bins."""
    y = torch.full((1, 3, 64, 512), 0.3)
    y[:, 1], y[:, 2] = 0.6, 0.9
    for dt in DTYPES:
        spec = M.Stats(grid=(4, 4), bits=bits)
        want = restated_stats(y.to(dt), spec)
        assert (want[0] != 0).sum() == 4 and want[0].max() == 64 * 512 and want[1][..., 7].sum() == 0   # one bin per channel holds every count
        got = ops.frame_stats(y.to(DEV, dt), spec)
        assert same(got, want), (dt, diff(got, want))


# ---- 4. the existing encoders as a second yardstick -------------------------------------------------------------------------------------------
def bincounts(codes, n):
    """(B, ...) integer codes -> (B, n) int64 counts."""
    return torch.stack([torch.bincount(c.flatten().long(), minlength=n) for c in codes.cpu()])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_histograms_are_the_encoders_codes(hip, dt):
    shape, crop = (2, 3, 40, 72), (36, 70)
    y = stats_source(shape, crop, None, dt).to(DEV)
    rgb = ops.rgb_encode(y, 8, crop_hw=crop)                                                     # (B, h, w, 3) uint8
    for m in MATRICES:
        got = ops.frame_stats(y, M.Stats(grid=(1, 1), bits=8, matrix=m), crop_hw=crop)
        for c in range(3):
            assert torch.equal(got.hist[:, c].cpu(), bincounts(rgb[..., c], 256)), (m, c)
        nv12 = ops.yuv_encode(y, M.OutFormat("nv12", matrix=m, range="full"), crop_hw=crop)
        assert torch.equal(got.hist[:, 3].cpu(), bincounts(nv12.planes[0], 256)), m
        got10 = ops.frame_stats(y, M.Stats(grid=(1, 1), bits=10, matrix=m), crop_hw=crop)
        p010 = ops.yuv_encode(y, M.OutFormat("p010", matrix=m, range="full"), crop_hw=crop)
        assert torch.equal(got10.hist[:, 3].cpu(), bincounts(p010.planes[0].cpu().to(torch.int32) >> 6, 1024)), m


# ---- 5. whole nets --------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def tsame(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


@pytest.mark.gpu
def test_existing_routes_unchanged_then_forward_mosaic_with_statistics(hip):
    """In one process: the default, rgb8 and nv12 routes of two nets before any statistics call, a four-rung ladder with two Stats rungs, and the
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
    look = lut_random(17)
    ladder = [M.Output(nv12), M.Output(M.Stats(grid=(4, 4))),
              M.Output(M.Stats(bits=10, grid=(3, 5), roi=(2, 4, 60, 90), dark=100, clip=900), M.Resize((72, 104)), look=look), M.Output("rgb8", M.Resize((36, 52)))]
    for net, (y, q8, f) in zip(nets, before):
        with torch.no_grad():
            outs = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
            alone = net.forward_mosaic(mosaic, None, coord, out_format=ladder[1].format)
        assert isinstance(outs, list) and len(outs) == 4 and y.dtype == dt and y.shape == (2, 3, 144, 208)
        assert tsame(outs[0].buffer, f.buffer) and all(tsame(a.contiguous(), b.contiguous()) for a, b in zip(outs[0].planes, f.planes))
        yc = y.cpu()
        assert isinstance(outs[1], M.FrameStats) and same(outs[1], restated_stats(yc, ladder[1].format))
        assert isinstance(alone, M.FrameStats) and same(alone, restated_stats(yc, ladder[1].format))           # out_format=Stats(...) on its own
        small = restated_lut3d(restated_resize(yc, ladder[2].resize), look)
        assert isinstance(outs[2], M.FrameStats) and outs[2].roi == (2, 4, 60, 90) and same(outs[2], restated_stats(small, ladder[2].format))
        assert tsame(outs[3], ops.rgb_encode(restated_resize(yc, ladder[3].resize).to(DEV), 8))
        luma = restated_stats(yc, ladder[1].format)[1][..., 4].sum((1, 2)).double() / (144 * 208 * 255)
        assert torch.equal(outs[1].mean_luma().cpu(), luma) and outs[1].awb_gains().shape == (2, 3) and outs[1].awb_gains().is_cuda
    for net, (y, q8, f) in zip(nets, before):
        y2, q2, f2 = routes(net)
        assert tsame(y, y2) and tsame(q8, q2) and tsame(f.buffer, f2.buffer)
        assert tsame(q8, ops.rgb_encode(y, 8))


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_ladder_with_statistics_equals_eager(hip):
    """The entry point zeroes its outputs on the stream itself, so the memsets are part of the graph: the second replay starts from zero."""
    net = net_on_gpu("LiteISPNet_GFM_LSC", torch.bfloat16)
    ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.Stats(grid=(5, 7), dark=20, clip=240)), M.Output(M.Stats(bits=10, grid=(2, 2)), M.Resize((40, 56)))]
    g = torch.Generator().manual_seed(5)
    m1 = torch.rand(2, 1, 80, 112, generator=g).to(DEV, torch.bfloat16)
    m2 = (torch.rand(2, 1, 80, 112, generator=g) * 0.5).to(DEV, torch.bfloat16)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    flat = lambda outs: [outs[0].buffer.clone(), outs[1].hist.clone(), outs[1].zones.clone(), outs[2].hist.clone(), outs[2].zones.clone()]
    with torch.no_grad():
        e1 = flat(net.forward_mosaic(m1, None, coord, outputs=ladder))
        e2 = flat(net.forward_mosaic(m2, None, coord, outputs=ladder))
    call = M.GraphedCall(lambda x, co: net.forward_mosaic(x, None, co, outputs=ladder))
    g1 = flat(call(m1, coord))
    g2 = flat(call(m2, coord))
    g3 = flat(call(m2, coord))
    assert all(tsame(a, b) for a, b in zip(g1, e1)) and all(tsame(a, b) for a, b in zip(g2, e2)) and all(tsame(a, b) for a, b in zip(g3, e2))
    assert not any(torch.equal(a, b) for a, b in zip(g1, g2))
    assert g2[1].sum(-1).eq(80 * 112).all() and g2[3].sum(-1).eq(40 * 56).all()                  # nothing of the first replay is left in the counts


# ---- 7. reproducibility ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_same_call_twice_and_prefilled_outputs(hip):
    shape, crop, roi = (2, 3, 40, 600), (37, 599), (1, 2, 35, 590)
    y = stats_source(shape, crop, roi, torch.bfloat16)
    yd = y.to(DEV)
    spec = M.Stats(grid=(5, 64), bits=10, roi=roi, dark=100, clip=900)
    want = restated_stats(y, spec, crop)
    a, b = ops.frame_stats(yd, spec, crop_hw=crop), ops.frame_stats(yd, spec, crop_hw=crop)
    assert same(a, want) and same(b, want)
    hist = torch.empty(2, 4, 1024, dtype=torch.int64, device=DEV)
    zones = torch.empty(2, 5, 64, 8, dtype=torch.int64, device=DEV)
    for t in (hist, zones):
        t.view(torch.uint8).fill_(0x7f)                                                          # the caller does not zero
    d = _lib.StatsDesc(roi=(C.c_int32 * 4)(*roi), grid=(C.c_int32 * 2)(5, 64), bits=10, matrix=_lib.RC_MATRIX_BT709, dark=100, clip=900)
    rc = hip.rc_frame_stats(yd.data_ptr(), _lib.RC_BF16, C.byref(d), hist.data_ptr(), zones.data_ptr(), 2, 40, 600, 37, 599, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.rc_last_error()
    assert torch.equal(hist.cpu(), want[0]) and torch.equal(zones.cpu(), want[1])               # every element written, none added to
