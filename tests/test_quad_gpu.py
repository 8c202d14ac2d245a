"""Quad-Bayer sensors on an MI355X: rc_raw_quad equals the elementwise restatement (tests/test_quad_host.py) bit for bit -- every storage and
both modes, the shapes at which the lane map can go wrong, strides, a bright sample on every seam, the tie arm, whole nets, a graph replay."""
import ctypes as C
import dataclasses

import pytest
import torch

import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.defects import Defects
from realcamnet_amd.exposures import Exposures
from realcamnet_amd.quad import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, WAVE_ROWS, WAVE_SPAN, QuadBayer
from realcamnet_amd.temporal import Temporal, TemporalState
from test_quad_host import CFA_NAMES, HAND, hand_counts, restated_quad
from test_raw_formats_host import mipi_pack

DEV = "cuda"
BITS = {"u16": 14, "u8": 8, "mipi10": 10, "mipi12": 12}
FLOATS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("u16", "u8", "mipi10", "mipi12", "fp32", "bf16", "fp16")
MODES = ("remosaic", "bin")


def same(a, b):
    a, b = a.cpu(), b.cpu()
    if a.dtype == torch.uint16:
        a, b = a.to(torch.int32), b.to(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def frame(kind, b, h, w, seed):
    """The host frame for the restatement: uniform-random counts of the storage's depth, or floats of its dtype in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind in BITS:
        return torch.randint(0, 1 << BITS[kind], (b, h, w), generator=g, dtype=torch.int32)
    return torch.rand(b, h, w, generator=g).to(FLOATS[kind])


def device_frame(kind, host, line_bytes=0):
    """The frame as the sensor delivers it, on the device, and the RawFormat fields that describe it."""
    if kind == "u16":
        return host.to(torch.uint16).to(DEV), dict(storage="u16", white_level=float(1 << BITS[kind]))
    if kind == "u8":
        return host.to(torch.uint8).to(DEV), dict(storage="u8", white_level=255.0)
    if kind in ("mipi10", "mipi12"):
        return torch.from_numpy(mipi_pack(host.numpy(), BITS[kind], line_bytes)).to(DEV), dict(storage=kind, width=host.shape[-1], white_level=float(1 << BITS[kind]))
    return host.to(DEV), dict(storage="float")


def out_dtype(kind, mode):
    return torch.float32 if mode == "bin" else torch.uint16 if kind in BITS else FLOATS[kind]


def check_host(kind, host, mode, cfa="RGGB", line_bytes=0):
    b, h, w = host.shape
    dev, fields = device_frame(kind, host, line_bytes)
    want = restated_quad(host, cfa, mode, out_dtype(kind, mode))
    got = ops.raw_quad(dev, M.RawFormat(cfa=cfa, **fields), QuadBayer(mode))
    assert got.is_contiguous() and got.shape == ((b, h // 2, w // 2) if mode == "bin" else (b, h, w)) and got.dtype == out_dtype(kind, mode)
    assert same(got, want), (kind, mode, cfa, h, w, (got.cpu().to(torch.float64) != want.to(torch.float64)).nonzero()[:8].tolist())
    return want


def check(kind, b, h, w, seed, mode, cfa="RGGB", line_bytes=0):
    return check_host(kind, frame(kind, b, h, w, seed), mode, cfa, line_bytes)


# ---- 1. storages, dtypes, phases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_storage_equals_the_restatement(hip, kind, mode):
    check(kind, 2, 40, 56, 11, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_every_phase_equals_the_restatement(hip, mode):
    outs = [check("u16", 1, 40, 56, 12, mode, cfa=cfa) for cfa in CFA_NAMES]
    if mode == "remosaic":                                                       # R and B swap roles, not recipes; the two G layouts differ
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and not torch.equal(outs[0], outs[2])
    check("mipi12", 1, 40, 56, 13, mode, cfa="GBRG")
    check("bf16", 1, 40, 56, 14, mode, cfa="GRBG")


@pytest.mark.gpu
@pytest.mark.parametrize("cfa", ("RGGB", "GRBG"))
def test_the_frames_computed_by_hand(hip, cfa):
    for name, src, outs, _ in HAND:
        host = torch.tensor(src, dtype=torch.int32).unsqueeze(0)
        for kind in ("u16", "mipi12"):
            dev, fields = device_frame(kind, host)
            got = ops.raw_quad(dev, M.RawFormat(cfa=cfa, **fields), QuadBayer())
            assert got.dtype == torch.uint16 and got.cpu().to(torch.int64)[0].tolist() == hand_counts(outs[cfa]), (name, kind)
        got = ops.raw_quad(host.to(torch.float32).to(DEV), M.RawFormat(cfa=cfa), QuadBayer())
        assert got.cpu()[0].tolist() == outs[cfa], name


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_shapes_at_which_the_lane_map_can_go_wrong(hip, mode):
    for kind in ("u16", "fp32", "mipi10", "mipi12"):
        check(kind, 2, 4, 4, 20, mode)                                           # every neighbour is a reflection
        check(kind, 2, 4, 8, 21, mode, cfa="GRBG")
        check(kind, 2, 8, 4, 22, mode)
    check("u16", 1, 8, WAVE_SPAN, 23, mode)                                      # a wave's span exactly: its last lane reflects
    check("u8", 1, 8, WAVE_SPAN + LANE_PX, 24, mode)                             # just past it: the second strip holds one lane's columns
    check("mipi10", 1, 8, BLOCK_SPAN, 25, mode)
    check("bf16", 1, 8, BLOCK_SPAN + LANE_PX, 26, mode, cfa="GBRG")              # just past a block's two strips
    check("u16", 1, WAVE_ROWS, 8, 27, mode)
    check("u16", 1, WAVE_ROWS + 4, 8, 28, mode)                                  # just past a wave's rows
    check("mipi12", 1, BLOCK_ROWS, 8, 29, mode)
    check("fp16", 1, BLOCK_ROWS + 4, 8, 30, mode, cfa="GRBG")                    # just past a block's rows
    check("u16", 2, BLOCK_ROWS + 8, BLOCK_SPAN + 2 * LANE_PX, 31, mode)          # four blocks; seams in both directions
    check("u16", 2, 12, 44, 32, mode)                                            # 88-byte rows: 8-byte loads, no 16-byte ones
    check("fp32", 2, 12, 52, 33, mode)


# ---- 3. strides ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_line_strides(hip, mode):
    for lb in (0, 61, 64):
        check("mipi10", 2, 36, 44, 40 + lb, mode, line_bytes=lb)                 # 55 bytes of samples; an odd stride moves every row's alignment
    for lb in (0, 69, 71, 72):
        check("mipi12", 2, 36, 44, 41 + lb, mode, line_bytes=lb)                 # a width that is 4 mod 8: 66 bytes
    host = frame("u16", 1, 12, 40, 42)                                           # a base that is 2 mod 8: the element path
    big = torch.cat([torch.zeros(1, dtype=torch.int32), host.flatten()]).to(torch.uint16).to(DEV)
    got = ops.raw_quad(big[1:].view(1, 12, 40), M.RawFormat(storage="u16", white_level=16383.0), QuadBayer(mode))
    assert same(got, restated_quad(host, "RGGB", mode, out_dtype("u16", mode)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_padded_destination_through_the_c_entry(hip, mode):
    for kind, pad in (("u16", 3), ("fp32", 5), ("mipi10", 8)):
        host = frame(kind, 2, 16, 24, 50)
        dev, fields = device_frame(kind, host)
        want = restated_quad(host, "GRBG", mode, out_dtype(kind, mode))
        oh, ow = want.shape[1:]
        if want.dtype == torch.uint16:
            dst = torch.full((2, oh, ow + pad), 7, dtype=torch.int16, device=DEV).view(torch.uint16)
        else:
            dst = torch.full((2, oh, ow + pad), 7.0, dtype=want.dtype, device=DEV)
        storage = {"u16": _lib.RC_RAW_U16, "fp32": _lib.RC_RAW_F32, "mipi10": _lib.RC_RAW_MIPI10}[kind]
        f = _lib.RawFormatDesc(storage=storage, cfa=_lib.RC_CFA_GRBG, line_bytes=dev.shape[2] * dev.element_size(), width=24, white=1.0)
        d = _lib.QuadDesc(mode=QuadBayer(mode).code)
        _lib.check(hip.rc_raw_quad(dev.data_ptr(), C.byref(f), C.byref(d), dst.data_ptr(), (ow + pad) * dst.element_size(), 2, 16, 24,
                                   torch.cuda.current_stream().cuda_stream), "rc_raw_quad")
        torch.cuda.synchronize()
        assert same(dst[:, :, :ow].contiguous(), want), kind
        fill = dst[:, :, ow:].contiguous().cpu()
        assert ((fill.to(torch.int32) if fill.dtype == torch.uint16 else fill) == 7).all(), kind         # the padding is not written


# ---- 4. direction and tie arms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfa", ("RGGB", "GRBG"))
def test_a_bright_sample_on_every_seam(hip, cfa):
    """One bright sample at a time next to a seam of the lane map -- lanes, waves, strips, row bands, the frame's corners: a lane exchange or
    a row of the window taken from the wrong side moves it to the wrong sites."""
    h, w = BLOCK_ROWS + 8, BLOCK_SPAN + 2 * LANE_PX
    xs = [0, 1, 3, 4, WAVE_SPAN - 1, WAVE_SPAN, WAVE_SPAN + 1, BLOCK_SPAN - 2, BLOCK_SPAN - 1, BLOCK_SPAN, BLOCK_SPAN + 3, w - 4, w - 2, w - 1]
    ys = [0, 1, 2, 3, 4, 5, WAVE_ROWS - 2, WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 2, h - 3, h - 2, h - 1]
    spots = [(ys[i % len(ys)], xs[i % len(xs)]) for i in range(len(xs) * len(ys)) if i % 5 == 0]       # 14 and 16 are coprime to 5: every row and column occurs
    assert {s[0] for s in spots} == set(ys) and {s[1] for s in spots} == set(xs)
    spots += [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    batch, seen = 8, 0
    for k in range(0, len(spots), batch):
        part = spots[k:k + batch]
        host = torch.full((len(part), h, w), 100, dtype=torch.int32)
        for i, (y, x) in enumerate(part):
            host[i, y, x] = 4000
        want = check_host("mipi12" if k % 16 else "u16", host, "remosaic", cfa)
        seen += sum(int((want[i].to(torch.int32) != 100).sum()) >= 1 for i in range(len(part)))
    assert seen >= len(spots) // 2, seen                                         # (a few photosites of a tile are read by no site: their frames stay flat)


@pytest.mark.gpu
def test_all_three_arms_of_the_g_rule_are_taken(hip):
    h, w = 24, WAVE_SPAN + 8
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    host = (1000 + 9 * ((y // 2 + x // 2) % 7) + 18 * ((y * x) % 3 == 0) * (x % 5 == 0)).to(torch.int32).unsqueeze(0)      # integer steps, symmetric in y and x on whole blocks
    for cfa in ("RGGB", "GRBG"):
        _, names = restated_quad(host[0], cfa, "remosaic", recipes=True)
        taken = {n: int((names == n).sum()) for n in ("G:H", "G:V", "G:tie")}
        assert min(taken.values()) >= 20, taken                                 # the tie arm among them, at many sites
        check_host("u16", host, "remosaic", cfa)
        check_host("fp32", host.to(torch.float32), "remosaic", cfa)


# ---- 5. through the nets ------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_of(name):
    if name not in _NETS:
        torch.manual_seed(0)
        _NETS[name] = getattr(M, name)().to(device=DEV, dtype=torch.bfloat16).eval()
    return _NETS[name]


def sensor_frame(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return (600 + 3 * ((y + 2 * x) % 300) + torch.randint(0, 40, (b, h, w), generator=g)).to(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("LiteISPNet", "ISPUNet_GFM_LSC"))
def test_forward_mosaic_with_quad_equals_the_stage_then_the_net(hip, name, mode):
    net = net_of(name)
    size = 64 if mode == "bin" else 32                                            # the network sees 32 x 32 either way
    host = sensor_frame(2, size, size, 60)
    lines = torch.from_numpy(mipi_pack(host.numpy(), 12, size * 3 // 2 + 4)).unsqueeze(1).to(DEV)
    fmt = M.RawFormat(storage="mipi12", cfa="GRBG", width=size, black_level=(64.0, 66.0, 62.0, 64.0), white_level=4095.0, quad=QuadBayer(mode))
    coord = torch.rand(2, 2, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16) if name != "LiteISPNet" else None
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        bayer = ops.raw_quad(lines, fmt)
        assert same(bayer, restated_quad(host, "GRBG", mode, out_dtype("mipi12", mode)))
        plain = dataclasses.replace(fmt, quad=None, storage="float" if mode == "bin" else "u16", width=None)
        ref = net.forward_mosaic(bayer, None, coord, raw_format=plain)
        asis = net.forward_mosaic(lines, None, coord, raw_format=dataclasses.replace(fmt, quad=None)) if mode == "remosaic" else None
    assert got.shape == (2, 3, 32, 32) and same(got, ref)                        # bin: half the sensor's size
    if mode == "remosaic":
        assert not torch.equal(got, asis)                                        # read as Bayer it is another picture


@pytest.mark.gpu
def test_quad_with_exposures_and_the_hot_test(hip):
    net = net_of("LiteISPNet")
    host = sensor_frame(4, 32, 32, 61).view(2, 2, 32, 32).clone()
    host[:, 1] = host[:, 1] * 2
    host[:, :, 8, 12] = 4095                                                     # a hot photosite at a site the remosaic keeps, in every exposure
    ex = Exposures(times=(1.0, 2.0), knee=(3000.0, 3600.0))
    hot = Defects(hot=(200.0, 0.25), counts=True)
    fmt = M.RawFormat(storage="u16", black_level=64.0, white_level=4095.0, exposures=ex, defects=hot, quad=QuadBayer())
    dev = host.to(torch.uint16).to(DEV)
    with torch.no_grad():
        got = net.forward_mosaic(dev, raw_format=fmt)
        counts = net.defect_counts.clone()
        bayer = ops.raw_quad(dev.view(4, 32, 32), M.RawFormat(storage="u16", white_level=4095.0, quad=QuadBayer())).view(2, 2, 32, 32)
        assert same(bayer, restated_quad(host.view(4, 32, 32), "RGGB", "remosaic", torch.uint16).view(2, 2, 32, 32))
        ref = net.forward_mosaic(bayer, raw_format=dataclasses.replace(fmt, quad=None))
        ref_counts = net.defect_counts.clone()
    assert same(got, ref) and same(counts, ref_counts) and counts.shape == (2, 2, 3) and int(counts[:, 0, 1].sum()) >= 2


@pytest.mark.gpu
def test_quad_with_temporal_over_two_calls(hip):
    net = net_of("LiteISPNet")
    frames = [sensor_frame(1, 64, 64, 62 + i) for i in range(2)]
    t = dict(noise=(6.0, 0.015625), alpha=0.25, ramp=3.0)
    base = dict(storage="u16", black_level=64.0, white_level=4095.0)
    fmt = M.RawFormat(quad=QuadBayer("bin"), temporal=Temporal(state=TemporalState(), **t), **base)
    ref = M.RawFormat(storage="float", black_level=64.0, white_level=4095.0, temporal=Temporal(state=TemporalState(), **t))
    with torch.no_grad():
        for i, f in enumerate(frames):
            dev = f.to(torch.uint16).to(DEV)
            got = net.forward_mosaic(dev, raw_format=fmt)
            want = net.forward_mosaic(ops.raw_quad(dev, M.RawFormat(**base), QuadBayer("bin")), raw_format=ref)
            assert got.shape == (1, 3, 32, 32) and same(got, want), i
    assert same(fmt.temporal.state.frame, ref.temporal.state.frame) and fmt.temporal.state.frame.shape == (1, 32, 32)


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_graph_of_raw_quad_replayed_on_rewritten_input(hip, mode):
    hosts = [frame("mipi10", 2, 40, 56, 70 + i) for i in range(3)]
    lines = [device_frame("mipi10", hst, 72) for hst in hosts]
    fmt = M.RawFormat(cfa="GBRG", quad=QuadBayer(mode), **lines[0][1])
    x = torch.empty_like(lines[0][0])
    x.copy_(lines[0][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                # a warm-up outside the capture
        ops.raw_quad(x, fmt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.raw_quad(x, fmt)
    for i in (1, 2):
        x.copy_(lines[i][0])                                                     # in place: the capture holds addresses, not values
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.raw_quad(lines[i][0], fmt)
        assert same(out, eager) and same(out, restated_quad(hosts[i], "GBRG", mode, out_dtype("mipi10", mode))), i
