"""Defective-pixel correction on an MI355X: rc_raw_defects equals the elementwise restatement (tests/test_defects_host.py) bit for bit --
every storage and dtype, the shapes at which the lane map can go wrong, defects on every seam, identity, counts, whole nets, a graph
replay."""
import ctypes as C
import dataclasses

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.defects import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, WAVE_SPAN, DefectMap, Defects
from test_defects_host import HAND_BLACKS, HAND_COUNTS, HAND_IN, HAND_MAP, HAND_OUT, restated_defects
from test_raw_formats_host import mipi_pack

DEV = "cuda"
BITS = {"u16": 14, "u8": 8, "mipi10": 10, "mipi12": 12}
FLOATS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BLACKS = (0.0625, 0.0703125, 0.05859375, 0.06640625)          # fractions of full scale, exact in bf16; scaled to the storage's units


def same(a, b):
    a, b = a.cpu(), b.cpu()
    if a.dtype == torch.uint16:
        a, b = a.to(torch.int32), b.to(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def frame(kind, b, h, w, seed, smooth=False):
    """(host frame for the restatement, full scale): uniform-random counts of the storage's depth, or floats of its dtype in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind in BITS:
        top = 1 << BITS[kind]
        c = torch.randint(0, top, (b, h, w), generator=g, dtype=torch.int32)
        if smooth:
            c = (top // 2 + 3 * (torch.arange(h)[:, None] + torch.arange(w)[None, :]) % (top // 4) + c % 5).to(torch.int32).expand(b, h, w).contiguous()
        return c, float(top)
    f = torch.rand(b, h, w, generator=g)
    if smooth:
        f = 0.5 + 0.001 * (torch.arange(h)[:, None] + torch.arange(w)[None, :]) % 0.25 + f * 0.004
    return f.to(FLOATS[kind]), 1.0


def device_frame(kind, host, line_bytes=0):
    """The frame as the sensor delivers it, on the device, and the RawFormat fields that describe it."""
    if kind == "u16":
        return host.to(torch.uint16).to(DEV), dict(storage="u16")
    if kind == "u8":
        return host.to(torch.uint8).to(DEV), dict(storage="u8")
    if kind in ("mipi10", "mipi12"):
        return torch.from_numpy(mipi_pack(host.numpy(), BITS[kind], line_bytes)).to(DEV), dict(storage=kind, width=host.shape[-1])
    return host.to(DEV), dict(storage="float")


def random_map(h, w, seed, density=0.04, coords=()):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(h, w, generator=g) < density
    for y, x in coords:
        if 0 <= y < h and 0 <= x < w:
            mask[y, x] = True
    return DefectMap.from_mask(mask)


def check(kind, b, h, w, seed, line_bytes=0, use_map=True, hot=True, cold=True, coords=(), cfa="RGGB", smooth=False):
    host, scale = frame(kind, b, h, w, seed, smooth)
    dev, fields = device_frame(kind, host, line_bytes)
    blacks = tuple(v * scale for v in BLACKS)
    dmap = random_map(h, w, seed + 1, coords=coords) if use_map else None
    thr_hot = (0.02 * scale, 0.0625) if hot else None
    thr_cold = (0.03 * scale, 0.125) if cold else None
    want, want_counts = restated_defects(host, blacks, None if dmap is None else dmap.mask(), thr_hot, thr_cold)
    fmt = M.RawFormat(cfa=cfa, black_level=blacks, white_level=scale, **fields)
    got, counts = ops.raw_defects(dev, fmt, Defects(map=dmap, hot=thr_hot, cold=thr_cold, counts=True))
    assert got.is_contiguous() and got.shape == (b, h, w)
    assert same(got, want), (kind, h, w, (got.cpu().to(torch.float64) != want.to(torch.float64)).nonzero()[:8].tolist())
    assert same(counts, want_counts), (counts.tolist(), want_counts.tolist())
    return want_counts


# ---- 1. storages and dtypes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "u8", "mipi10", "mipi12", "fp32", "bf16", "fp16"))
def test_every_storage_equals_the_restatement(hip, kind):
    n = check(kind, 2, 40, 56, 11)                                                # B = 2 sharing one map; per-position blacks; all three together
    assert (n > 0).all(), n.tolist()                                              # every path was taken in both frames
    only_map = check(kind, 2, 40, 56, 12, hot=False, cold=False)
    assert (only_map[:, 0] > 0).all() and (only_map[:, 1:] == 0).all()
    only_hot = check(kind, 2, 40, 56, 13, use_map=False, cold=False)
    assert (only_hot[:, 1] > 0).all() and only_hot[:, 0].sum() == 0 and only_hot[:, 2].sum() == 0
    only_cold = check(kind, 2, 40, 56, 14, use_map=False, hot=False)
    assert (only_cold[:, 2] > 0).all() and only_cold[:, :2].sum() == 0
    check(kind, 1, 40, 56, 15, cfa="GBRG", smooth=True)                           # the phase changes nothing: blacks are in position order


@pytest.mark.gpu
def test_the_frame_computed_by_hand(hip):
    src = torch.tensor(HAND_IN, dtype=torch.int32).unsqueeze(0)
    spec = Defects(map=DefectMap.from_coords((8, 8), HAND_MAP), hot=(64.0, 0.5), cold=(64.0, 0.5), counts=True)
    for kind in ("u16", "mipi12"):
        dev, fields = device_frame(kind, src)
        got, counts = ops.raw_defects(dev, M.RawFormat(black_level=HAND_BLACKS, white_level=4095.0, **fields), spec)
        assert got.dtype == torch.uint16 and got.cpu().to(torch.int32)[0].tolist() == HAND_OUT and counts.tolist() == [HAND_COUNTS]


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shapes_at_which_the_lane_map_can_go_wrong(hip):
    for kind in ("u16", "fp32", "mipi12"):
        host, scale = frame(kind, 2, 2, 2, 21)                                    # 2 x 2: no ring neighbour anywhere, the output is the input
        dev, fields = device_frame(kind, host)
        got = ops.raw_defects(dev, M.RawFormat(white_level=scale, **fields), Defects(map=DefectMap.from_coords((2, 2), [(0, 0), (1, 1)]), hot=(0.0, 0.0), cold=(0.0, 0.0)))
        assert same(got, host.to(torch.uint16) if kind in BITS else host)
        check(kind, 2, 2, 4, 20)                                                  # 2 x 4: one neighbour each, E or W (columns x and x +- 2)
        check(kind, 2, 4, 4, 22)
    for lb in (0, 61, 64):
        check("mipi10", 2, 38, 44, 23 + lb, line_bytes=lb)                        # 55 bytes of samples; an odd stride moves every row's alignment
    for lb in (0, 69, 71, 72):
        check("mipi12", 2, 38, 46, 24 + lb, line_bytes=lb)                        # an odd packed width: the last 3-byte group stands alone
    check("u16", 1, 8, WAVE_SPAN + LANE_PX, 25)                                   # just past a wave's span: the second strip holds one lane's columns
    check("u8", 1, 8, WAVE_SPAN + 2, 26)                                          # ... and two columns, on the element path
    check("mipi10", 1, 6, BLOCK_SPAN + LANE_PX, 27)                               # just past a block's two strips
    check("u16", 1, BLOCK_ROWS + 2, 12, 28)                                       # just past a block's rows
    check("bf16", 2, BLOCK_ROWS + 6, BLOCK_SPAN + 2 * LANE_PX, 29)                # four blocks; seams in both directions
    check("u16", 2, 10, 46, 30)                                                   # 92-byte rows: neither 8-byte loads nor 8-byte stores
    check("fp32", 2, 10, 50, 31)                                                  # 200-byte rows: no 16-byte access
    check("fp16", 1, 6, 18, 32)


@pytest.mark.gpu
def test_misaligned_views_take_the_element_path(hip):
    host, scale = frame("u16", 1, 12, 40, 33)
    big = torch.cat([torch.zeros(1, dtype=torch.int32), host.flatten()]).to(torch.uint16).to(DEV)
    view = big[1:].view(1, 12, 40)                                                # a base that is 2 mod 8
    dmap = random_map(12, 40, 34)
    want, _ = restated_defects(host, (0.0,) * 4, dmap.mask(), (100.0, 0.0), (100.0, 0.0))
    assert same(ops.raw_defects(view, M.RawFormat(storage="u16", white_level=scale), Defects(map=dmap, hot=(100.0, 0.0), cold=(100.0, 0.0))), want)


# ---- 3. placement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "mipi10"))
def test_defects_on_every_seam(hip, kind):
    h, w = BLOCK_ROWS + 8, BLOCK_SPAN + 16
    xs = (0, 1, 2, 3, LANE_PX, LANE_PX + 3, WAVE_SPAN - 4, WAVE_SPAN - 3, WAVE_SPAN - 2, WAVE_SPAN - 1, WAVE_SPAN, WAVE_SPAN + 1, WAVE_SPAN + 2, WAVE_SPAN + 3,
          BLOCK_SPAN - 2, BLOCK_SPAN - 1, BLOCK_SPAN, BLOCK_SPAN + 1, BLOCK_SPAN + 2, w - 4, w - 3, w - 2, w - 1)
    ys = (0, 1, 2, 3, BLOCK_ROWS - 3, BLOCK_ROWS - 2, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, BLOCK_ROWS + 2, h - 2, h - 1)
    coords = [(y, x) for y in ys for x in xs[::2]] + [(y, x) for y in ys[1::2] for x in xs[1::2]]           # corners, edges, lane / strip / band seams
    check(kind, 2, h, w, 41, coords=coords)
    # hot samples beside mapped ones that are stuck high: found only if the mapped neighbour is kept out of hi
    g = torch.Generator().manual_seed(42)
    host = 500 + torch.randint(0, 16, (1, h, w), generator=g, dtype=torch.int32)
    stuck = [(y, x) for y in ys for x in xs[::3]]
    hot_rows = (0, 3, BLOCK_ROWS - 3, BLOCK_ROWS, h - 2, h - 1)                     # no two rows 2 apart, no two columns 2 apart: no hot sample in another's ring
    hot = [(y, x + 2) for y, x in stuck if y in hot_rows and x + 2 < w]
    assert all(p not in stuck for p in hot)
    for y, x in stuck:
        host[0, y, x] = 1023
    for y, x in hot:
        host[0, y, x] = 900
    dmap = DefectMap.from_coords((h, w), stuck)
    want, n = restated_defects(host, (64.0,) * 4, dmap.mask(), (40.0, 0.25), None)
    assert len(hot) > 20 and n[0, 1] == len(hot) and all(int(want[0, y, x]) < 520 for y, x in hot)          # t = 40 + 0.25 (515 - 64) < 385
    dev, fields = device_frame(kind, host)
    got, counts = ops.raw_defects(dev, M.RawFormat(black_level=64.0, white_level=1023.0, **fields), Defects(map=dmap, hot=(40.0, 0.25), counts=True))
    assert same(got, want) and same(counts, n)


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "u8", "mipi10", "mipi12", "fp32", "bf16", "fp16"))
def test_nothing_to_correct_returns_the_decoded_frame(hip, kind):
    for h, w, lb in ((38, 44, 0), (38, 44, 67), (BLOCK_ROWS + 2, WAVE_SPAN + 6 if kind != "mipi10" else WAVE_SPAN + 8, 0)):
        host, scale = frame(kind, 2, h, w, 51)
        dev, fields = device_frame(kind, host, lb if kind in ("mipi10", "mipi12") else 0)
        spec = Defects(map=DefectMap.from_coords((h, w), []), hot=(2.0 * scale, 0.0), cold=(2.0 * scale, 0.0), counts=True)
        got, counts = ops.raw_defects(dev, M.RawFormat(white_level=scale, **fields), spec)
        assert same(got, host.to(torch.uint16) if kind in BITS else host)                                    # also the RAW10 / RAW12 unpack check
        assert counts.sum() == 0


# ---- 5. counts --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_counts_are_overwritten_and_runs_repeat(hip):
    host, scale = frame("u16", 2, 70, 300, 61)
    dmap = random_map(70, 300, 62)
    words = dmap.device_words(DEV)
    assert words is dmap.device_words(torch.device(DEV)) and words.dtype == torch.int32 and words.shape == (70, 10)     # uploaded once
    src = host.to(torch.uint16).to(DEV)
    want, n = restated_defects(host, (100.0,) * 4, dmap.mask(), (300.0, 0.0625), (300.0, 0.0625))
    f = _lib.RawFormatDesc(storage=_lib.RC_RAW_U16, cfa=0, line_bytes=0, width=0, white=scale)
    for k in range(4):
        f.black[k] = 100.0
    d = _lib.DefectDesc(flags=3, hot_abs=300.0, hot_rel=0.0625, cold_abs=300.0, cold_rel=0.0625)
    outs = []
    for fill in (777, -5):
        out = torch.full((2, 70, 300), 12345, dtype=torch.int32).to(torch.uint16).to(DEV)
        counts = torch.full((2, 3), fill, dtype=torch.int64, device=DEV)                                     # pre-filled: the entry point zeroes it
        _lib.check(hip.rc_raw_defects(src.data_ptr(), C.byref(f), C.byref(d), words.data_ptr(), 4 * words.shape[1], out.data_ptr(), 0, counts.data_ptr(), 2, 35, 150,
                                      torch.cuda.current_stream().cuda_stream), "rc_raw_defects")
        assert same(counts, n) and same(out, want)
        outs.append(out)
    assert same(outs[0], outs[1])
    no_counts = torch.empty_like(outs[0])
    _lib.check(hip.rc_raw_defects(src.data_ptr(), C.byref(f), C.byref(d), words.data_ptr(), 4 * words.shape[1], no_counts.data_ptr(), 0, None, 2, 35, 150,
                                  torch.cuda.current_stream().cuda_stream), "rc_raw_defects")
    assert same(no_counts, want)


# ---- 6. whole nets ----------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def isp_net():
    if "isp" not in _NETS:
        torch.manual_seed(0)
        _NETS["isp"] = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    return _NETS["isp"]


def planted_frame(b, h, w, seed):
    """10-bit counts with a smooth texture, stuck and hot / cold samples, the map, the spec and the restated corrected counts."""
    g = torch.Generator().manual_seed(seed)
    c = (300 + 2 * (torch.arange(h)[:, None] + torch.arange(w)[None, :]) % 400 + torch.randint(0, 6, (b, h, w), generator=g)).to(torch.int32)
    stuck = [(y, x) for y in range(3, h, 11) for x in range(1, w, 13)] + [(0, 0), (h - 1, w - 1)]
    for i, (y, x) in enumerate(stuck):
        c[:, y, x] = 1023 if i % 2 else 0
    for y in range(5, h, 9):
        for x in range(6, w, 17):
            if (y, x) not in stuck:
                c[:, y, x] = 1020 if (y + x) % 2 else 3
    dmap = DefectMap.from_coords((h, w), stuck)
    blacks = (64.0, 66.0, 62.0, 64.0)
    spec = Defects(map=dmap, hot=(48.0, 0.125), cold=(48.0, 0.125), counts=True)
    want, n = restated_defects(c, blacks, dmap.mask(), spec.hot, spec.cold)
    assert (n > 0).all()
    return c, blacks, spec, want, n


@pytest.mark.gpu
def test_forward_mosaic_with_defects_equals_the_corrected_mosaic(hip):
    net = isp_net()
    c, blacks, spec, want, n = planted_frame(2, 80, 112, 71)
    lines = torch.from_numpy(mipi_pack(c.numpy(), 10, 160)).unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=112, black_level=blacks, white_level=1023.0, defects=spec)
    plain = dataclasses.replace(fmt, defects=None)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        counts = net.defect_counts.clone()
        ref = net.forward_mosaic(want.to(DEV), None, coord, raw_format=M.RawFormat(storage="u16", cfa="GBRG", black_level=blacks, white_level=1023.0))
        raw = net.forward_mosaic(lines, None, coord, raw_format=plain)
        # defects=None is the route it was: the ingest of the frame as delivered, then the network
        a, cond = ops.raw_ingest(lines, dtype=torch.bfloat16, pad_to=16, cond_hw=(256, 256), raw_format=plain)
        h, vec = net._front(a, cond, ops.to_nhwc(coord, dtype=torch.bfloat16, pad_hw=(a.shape[1], a.shape[2])))
        route = net._trunk(h, vec, crop_hw=(80, 112))
    assert got.shape == (2, 3, 80, 112) and same(got, ref) and same(counts, n)
    assert same(raw, route) and not torch.equal(raw, got)


@pytest.mark.gpu
def test_codec_forward_mosaic_with_defects_equals_the_corrected_mosaic(hip):
    import realcamnet_amd.raw2bit as RB
    torch.manual_seed(0)
    net = RB.raw_compression_tcm_final(N=32).to(device=DEV, dtype=torch.bfloat16).eval()
    c, blacks, spec, want, n = planted_frame(1, 512, 512, 72)
    lines = torch.from_numpy(mipi_pack(c.numpy(), 10, 640)).to(DEV)
    coord = O.make_coord(1, 256, 256).to(DEV, torch.bfloat16)
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=512, black_level=blacks, white_level=1023.0, defects=spec)
    plain = dataclasses.replace(fmt, defects=None)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        counts = net.defect_counts.clone()
        ref = net.forward_mosaic(want.to(DEV), None, coord, raw_format=M.RawFormat(storage="u16", cfa="GBRG", black_level=blacks, white_level=1023.0))
        raw = net.forward_mosaic(lines, None, coord, raw_format=plain)
        a, cond = ops.raw_ingest(lines, dtype=torch.bfloat16, pad_to=128, cond_hw=(256, 256), raw_format=plain)
        route = net._forward_nhwc(a, cond, ops.to_nhwc(coord, dtype=torch.bfloat16, pad_hw=(a.shape[1], a.shape[2])))
    assert same(counts, n)
    for k in ("x_hat", "y"):
        assert same(got[k], ref[k]) and same(raw[k], route[k]), k
    assert not torch.equal(raw["x_hat"], got["x_hat"])


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_forward_with_defects_equals_eager(hip):
    net = isp_net()
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    frames = []
    for seed in (81, 82):
        c, blacks, spec, want, n = planted_frame(2, 80, 112, seed)
        frames.append((torch.from_numpy(mipi_pack(c.numpy(), 10, 160)).to(DEV), n))
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=112, black_level=blacks, white_level=1023.0, defects=spec)

    def fn(x, co):
        y = net.forward_mosaic(x, None, co, raw_format=fmt, out_format="rgb8")
        return y, net.defect_counts

    call = M.GraphedCall(fn)
    for lines, n in frames + frames[:1]:                        # the third call is the second replay of the capture
        with torch.no_grad():
            eager = net.forward_mosaic(lines, None, coord, raw_format=fmt, out_format="rgb8")
            eager_counts = net.defect_counts.clone()
        y, counts = call(lines, coord)
        assert same(y, eager) and same(counts, eager_counts) and same(counts, n)
