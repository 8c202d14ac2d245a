"""GPU: lateral chromatic aberration correction (rc_raw_aberration, ops.raw_aberration, RawFormat.aberration).  The yardstick is
restated_aberration of tests/test_aberration_host.py, the NumPy restatement of the header's arithmetic computed on the CPU (never the
kernel's own output), and every comparison is bit for bit (a zero may differ in sign: the header says so).

Most cases call the C entry on a byte buffer, so that every storage can have padded lines: the padding holds 0xFF bytes (NaN for the float
storages, full scale for the counts), and the destination is filled with a marker first, so a read beyond a line or a store beyond a row
shows.  The shapes are the smallest at which the kernel takes each of its paths: mosaics where every tap is clamped, exactly one tile of
64 x 64, one lane and one row past it, a width that is 2 mod 4, four tiles with shifts that cross every seam at the smallest and the
largest reach."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.aberration import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, Aberration
from realcamnet_amd.raw_format import CFAS
from raw_stats_ref import PACKERS, pad_lines
from test_aberration_host import HAND, RPOS, constant, random_mesh, restated_aberration, restated_mosaic

DEV = "cuda"
F32 = np.float32
NAN, INF = float("nan"), float("inf")
STORAGES = ("f32", "bf16", "f16", "u16", "u8", "mipi10", "mipi12")
INTERPS = ("bilinear", "bicubic")
CODE = {"f32": _lib.RC_RAW_F32, "bf16": _lib.RC_RAW_BF16, "f16": _lib.RC_RAW_F16, "u16": _lib.RC_RAW_U16, "u8": _lib.RC_RAW_U8, "mipi10": _lib.RC_RAW_MIPI10,
        "mipi12": _lib.RC_RAW_MIPI12}
FLOATS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FULL = {"u16": 65535, "u8": 255, "mipi10": 1023, "mipi12": 4095}
ESIZE = {"f32": 4, "bf16": 2, "f16": 2, "u16": 2, "u8": 1}
FORMAT = {"f32": "float", "bf16": "float", "f16": "float", "u16": "u16", "u8": "u8", "mipi10": "mipi10", "mipi12": "mipi12"}
MARK = -12345.0


def frame(storage, B, H, W, seed):
    """The decoded sample values (B, H, W) float32 -- what the restatement reads -- and the storage's bytes (B, H, row bytes)."""
    rng = np.random.default_rng(seed)
    if storage in FLOATS:
        t = torch.from_numpy(rng.uniform(0.0, 1.0, (B, H, W)).astype(F32)).to(FLOATS[storage])
        return t.float().numpy(), t.contiguous().view(torch.uint8).numpy().reshape(B, H, -1)
    v = rng.integers(0, FULL[storage] + 1, (B, H, W))
    return v.astype(F32), PACKERS[storage](v)


def row_bytes(storage, W):
    return W * 5 // 4 if storage == "mipi10" else W * 3 // 2 if storage == "mipi12" else W * ESIZE[storage]


def entry(hip, body, storage, cfa, shift, cell, interp, reach, H, W, line_bytes=None, dst_pad=0, expect=0):
    """rc_raw_aberration on the bytes `body` (B, H, row bytes) laid out with `line_bytes` and 0xFF filler, with the raw mesh `shift`
    (2, Gh, Gw, 2), into a destination whose rows are dst_pad floats longer than the mosaic's; returns the (B, H, W) result on the host after
    checking that the padding still holds the marker."""
    B = body.shape[0]
    src = torch.from_numpy(pad_lines(body, line_bytes, 0xFF)).to(DEV)
    lb = src.shape[2]
    mesh = torch.from_numpy(np.ascontiguousarray(shift, dtype=F32)).to(DEV)
    dst = torch.full((B, H, W + dst_pad), MARK, dtype=torch.float32, device=DEV)
    f = _lib.RawFormatDesc(storage=CODE[storage], cfa=CFAS[cfa], line_bytes=lb, width=W, black=(C.c_float * 4)(0, 0, 0, 0), white=1.0)
    d = _lib.CaDesc(interp=_lib.RC_WARP_BICUBIC if interp == "bicubic" else _lib.RC_WARP_BILINEAR, cell=cell, reach=reach)
    rc = hip.rc_raw_aberration(src.data_ptr(), C.byref(f), C.byref(d), mesh.data_ptr(), dst.data_ptr(), 4 * (W + dst_pad) if dst_pad else 0, B, H // 2, W // 2,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == expect, hip.rc_last_error()
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:, :, W:] == MARK).all()
    return out[:, :, :W]


def check(hip, storage, cfa, B, H, W, seed, ab, line_bytes=None, dst_pad=0):
    values, body = frame(storage, B, H, W, seed)
    want = restated_aberration(values, cfa, ab)
    got = entry(hip, body, storage, cfa, ab.shift.numpy(), ab.cell, ab.interp, ab.reach, H, W, line_bytes, dst_pad)
    bad = np.argwhere(got != want)
    assert got.dtype == F32 and not len(bad), (storage, cfa, (B, H, W), ab, len(bad), bad[:4].tolist(), [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]])
    return values, got


def tensor_of(storage, body):
    """The bytes as the tensor ops.raw_aberration takes for this storage."""
    t = torch.from_numpy(np.ascontiguousarray(body))
    if storage in FLOATS:
        return t.view(FLOATS[storage]).to(DEV)
    if storage == "u16":
        return t.view(torch.uint16).to(DEV)
    return t.to(DEV)


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("storage", STORAGES)
def test_every_storage_through_the_op(hip, storage, interp):
    """2 x 40 x 56 with a random mesh of reach 2, through ops.raw_aberration: the public path, the mesh uploaded once."""
    ab = random_mesh((40, 56), 8, 2.0, 11, interp)
    assert ab.reach == 2
    values, body = frame(storage, 2, 40, 56, 12)
    fmt = M.RawFormat(storage=FORMAT[storage], cfa="GRBG", width=56 if storage.startswith("mipi") else None, white_level=float(FULL.get(storage, 1)))
    got = ops.raw_aberration(tensor_of(storage, body), fmt, ab)
    assert got.shape == (2, 40, 56) and got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), restated_aberration(values, "GRBG", ab))
    assert ab.device_shift(got.device) is ab.device_shift(got.device)
    again = ops.raw_aberration(tensor_of(storage, body), dataclasses.replace(fmt, aberration=ab))        # the format's own field
    assert torch.equal(again, got)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_every_cfa(hip, interp):
    ab = random_mesh((40, 56), 16, 2.0, 13, interp)
    got = {cfa: check(hip, "u16", cfa, 2, 40, 56, 14, ab)[1] for cfa in sorted(CFAS)}
    # RGGB and BGGR differ only by which mesh moves which positions: with the planes of the mesh exchanged they are one picture
    swapped = Aberration(ab.blue.numpy(), ab.red.numpy(), 16, interp)
    assert np.array_equal(check(hip, "u16", "BGGR", 2, 40, 56, 14, swapped)[1], got["RGGB"]) and not np.array_equal(got["BGGR"], got["RGGB"])
    assert np.array_equal(check(hip, "u16", "GBRG", 2, 40, 56, 14, swapped)[1], got["GRBG"]) and not np.array_equal(got["GBRG"], got["GRBG"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_frames(hip, case):
    _, m, cfa, ab, want = case
    got = entry(hip, PACKERS["u16"](m.astype(np.int64)), "u16", cfa, ab.shift.numpy(), ab.cell, ab.interp, ab.reach, 8, 16)
    for (y, x), v in want.items():
        assert got[0, y, x] == F32(v), ((y, x), got[0, y, x], v)
    assert np.array_equal(got, restated_aberration(m, cfa, ab))


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("size", ((4, 4), (4, 8), (8, 4)))
def test_mosaics_where_every_tap_is_clamped(hip, size, interp):
    H, W = size
    for i, storage in enumerate(("u16", "mipi12", "f32", "mipi10" if W % 4 == 0 else "u8")):
        ab = random_mesh(size, 8, 3.0, 20 + i, interp)
        check(hip, storage, sorted(CFAS)[i], 3, H, W, 21 + i, ab)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("size", ((BLOCK_ROWS, BLOCK_SPAN), (BLOCK_ROWS, BLOCK_SPAN + LANE_PX), (BLOCK_ROWS + 2, BLOCK_SPAN), (BLOCK_ROWS + 2, BLOCK_SPAN + LANE_PX + 2)))
def test_one_tile_one_lane_past_it_one_row_past_it(hip, size, interp):
    """Exactly one tile; one lane past it; one row pair past it; both, with a width that is 2 mod 4 (the last lane holds two samples)."""
    H, W = size
    for i, storage in enumerate(("u16", "f32", "mipi12", "bf16")):
        ab = random_mesh(size, 8 << i, 2.5, 30 + i, interp)
        check(hip, storage, sorted(CFAS)[(i + 1) % 4], 1 + i % 2, H, W, 31 + i, ab)
    if W % 4 == 0:
        check(hip, "mipi10", "BGGR", 2, H, W, 35, random_mesh(size, 32, 2.5, 36, interp))


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("amount", (0.75, 7.5))
def test_shifts_across_the_tile_seams(hip, amount, interp):
    """Four tiles (128 x 128) and a constant shift of reach 1 / reach 8 pointing across a seam in each of the four directions -- red one
    way, blue the other -- so the taps of the samples next to a seam come from the halo the neighbouring tile's samples fill."""
    size = (2 * BLOCK_ROWS, 2 * BLOCK_SPAN)
    for i, (dx, dy) in enumerate(((amount, 0.0), (-amount, 0.0), (0.0, amount), (0.0, -amount))):
        ab = constant(size, (dx, dy), (-dx, -dy), cell=(8, 16, 64, 128)[i], interp=interp)
        assert ab.reach == (1 if amount < 1 else 8)
        check(hip, ("u16", "mipi10", "f32", "u8")[i], sorted(CFAS)[i], 1, size[0], size[1], 40 + i, ab)
    ab = random_mesh(size, 8, amount, 45, interp)                              # and every direction at once
    check(hip, "u16", "RGGB", 2, size[0], size[1], 46, ab)


@pytest.mark.gpu
def test_a_cell_larger_than_the_frame(hip):
    for interp in INTERPS:
        ab = random_mesh((40, 56), 128, 2.0, 50, interp)
        assert ab.shift.shape == (2, 2, 2, 2)
        check(hip, "u16", "GBRG", 2, 40, 56, 51, ab)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_padded_lines_unaligned_frames_and_a_dst_pitch(hip, interp):
    """42 x 56: MIPI lines with a stride that is no multiple of 4, so the second frame starts mid-dword and off a 16-byte boundary; element
    lines padded by whole vectors (the vector path) and by odd sample counts (the sample-by-sample path); destination rows padded by whole
    vectors and by one float."""
    ab = random_mesh((42, 56), 8, 2.0, 60, interp)
    for storage, lb in (("mipi10", 71), ("mipi10", 73), ("mipi12", 87), ("mipi12", 85)):
        assert (42 * lb) % 16 and lb >= row_bytes(storage, 56)
        check(hip, storage, "GRBG", 2, 42, 56, 61, ab, line_bytes=lb)
    for storage, pad in (("u16", 3), ("u16", 4), ("u8", 1), ("u8", 8), ("f32", 1), ("f32", 4), ("bf16", 2), ("f16", 5)):
        check(hip, storage, "BGGR", 2, 42, 56, 62, ab, line_bytes=(56 + pad) * ESIZE[storage])
    for pad in (4, 1, 7):
        check(hip, "u16", "RGGB", 2, 42, 56, 63, ab, dst_pad=pad)
        check(hip, "mipi12", "GBRG", 2, 42, 56, 64, ab, line_bytes=85, dst_pad=pad)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_a_wild_device_mesh_is_clamped(hip, interp):
    """Through the C entry, which does not look at the device mesh: NaN, +-inf and +-1e30 nodes.  The result is the restatement's guard
    (NaN -> 0, then the clamp to the reach) and the call returns RC_OK."""
    H, W = 72, 136                                                             # 36 x 68 cells: two tiles by three, ragged
    gh, gw = Aberration.nodes((H, W), 8)
    rng = np.random.default_rng(70)
    for reach in (1, 3, 8):
        shift = rng.uniform(-reach, reach, (2, gh, gw, 2)).astype(F32)
        wild = np.array([NAN, INF, -INF, 1e30, -1e30, 3e38, -40000.0], dtype=F32)
        idx = rng.integers(0, shift.size, 60)
        shift.reshape(-1)[idx] = wild[rng.integers(0, len(wild), 60)]
        values, body = frame("u16", 2, H, W, 71)
        want = restated_mosaic(values, "RGGB", shift, 8, interp, reach)
        assert np.isfinite(want).all()
        got = entry(hip, body, "u16", "RGGB", shift, 8, interp, reach, H, W)
        assert np.array_equal(got, want), (reach, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("interp", INTERPS)
def test_zero_mesh_and_whole_shift_on_the_device(hip, interp):
    size = (80, 120)
    values, body = frame("mipi12", 2, 80, 120, 80)
    zero = constant(size, (0.0, 0.0), (0.0, 0.0), interp=interp)
    assert np.array_equal(entry(hip, body, "mipi12", "GRBG", zero.shift.numpy(), 8, interp, 1, 80, 120, line_bytes=183), values)
    whole = constant(size, (3.0, -2.0), (-1.0, 4.0), interp=interp)
    got = entry(hip, body, "mipi12", "GRBG", whole.shift.numpy(), 8, interp, whole.reach, 80, 120)
    for pos, (dx, dy) in ((RPOS["GRBG"], (3, -2)), (3 - RPOS["GRBG"], (-1, 4))):
        p, g = values[:, pos >> 1::2, pos & 1::2], got[:, pos >> 1::2, pos & 1::2]
        h, w = p.shape[1:]
        assert np.array_equal(g[:, 6:h - 6, 6:w - 6], p[:, 6 + dy:h - 6 + dy, 6 + dx:w - 6 + dx])
    only_blue = Aberration(None, random_mesh(size, 8, 1.5, 81, interp).blue.numpy(), 8, interp)
    got = entry(hip, body, "mipi12", "GRBG", only_blue.shift.numpy(), 8, interp, only_blue.reach, 80, 120)
    r, b = RPOS["GRBG"], 3 - RPOS["GRBG"]
    assert np.array_equal(got[:, r >> 1::2, r & 1::2], values[:, r >> 1::2, r & 1::2]) and not np.array_equal(got[:, b >> 1::2, b & 1::2], values[:, b >> 1::2, b & 1::2])
    assert np.array_equal(got, restated_aberration(values, "GRBG", only_blue))


# ---- 2. graphs and forward_mosaic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eager_runs_and_graph_replays_are_equal(hip):
    ab = random_mesh((80, 120), 8, 2.0, 90)
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=120, white_level=1023.0, aberration=ab)
    frames = [frame("mipi10", 2, 80, 120, 91 + i) for i in range(2)]
    call = M.GraphedCall(lambda x: ops.raw_aberration(x, fmt))
    for values, body in frames + frames:
        x = torch.from_numpy(body).to(DEV)
        want = restated_aberration(values, "GBRG", ab)
        a, b = ops.raw_aberration(x, fmt), ops.raw_aberration(x, fmt)
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)
        assert np.array_equal(call(x).clone().cpu().numpy(), want) and np.array_equal(call(x).cpu().numpy(), want)


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
def test_forward_mosaic_equals_the_stages_by_hand(hip):
    net = net_of("LiteISPNet")
    dev = sensor_frame(2, 32, 32, 95).to(torch.uint16).to(DEV)
    ab = random_mesh((32, 32), 8, 2.0, 96)
    cal = M.Calibration(gains=(1.75, 1.0, 1.0, 1.5), clip=(0.0, 1.0))
    base = dict(storage="u16", cfa="GRBG", black_level=(64.0, 66.0, 62.0, 64.0), white_level=4095.0)
    with torch.no_grad():
        got = net.forward_mosaic(dev, raw_format=M.RawFormat(calibration=cal, aberration=ab, **base))
        by_hand = ops.raw_aberration(ops.raw_calibrate(dev, M.RawFormat(calibration=cal, **base)), M.RawFormat(cfa="GRBG"), ab)
        want = net.forward_mosaic(by_hand, raw_format=M.RawFormat(cfa="GRBG"))
        without = net.forward_mosaic(dev, raw_format=M.RawFormat(calibration=cal, **base))
        zero = net.forward_mosaic(dev, raw_format=M.RawFormat(calibration=cal, aberration=constant((32, 32), (0.0, 0.0), (0.0, 0.0)), **base))
        # without a calibration the stage reads the frame as delivered and the ingest keeps the levels
        bare = net.forward_mosaic(dev, raw_format=M.RawFormat(aberration=ab, **base))
        bare_want = net.forward_mosaic(ops.raw_aberration(dev, M.RawFormat(**base), ab), raw_format=M.RawFormat(**dict(base, storage="float")))
    assert got.shape == (2, 3, 32, 32) and torch.equal(got, want) and not torch.equal(got, without)
    assert torch.equal(zero, without) and torch.equal(bare, bare_want)


@pytest.mark.gpu
def test_forward_mosaic_with_every_stage_together(hip):
    from realcamnet_amd.defects import Defects
    from realcamnet_amd.temporal import Temporal, TemporalState
    net = net_of("LiteISPNet")
    host = sensor_frame(2, 32, 32, 97)
    host[:, 8, 12] = 4095                                                       # a hot photosite
    dev = host.to(torch.uint16).to(DEV)
    t = dict(noise=(6.0, 0.015625), alpha=0.25, ramp=3.0)
    cal = M.Calibration(gains=(1.75, 1.0, 1.0, 1.5), clip=(0.0, 1.0))
    base = dict(storage="u16", black_level=64.0, white_level=4095.0, defects=Defects(hot=(200.0, 0.25), counts=True), calibration=cal, stats=M.RawStats(grid=(2, 2), bits=12))
    ab = random_mesh((32, 32), 8, 2.0, 98)
    with torch.no_grad():
        plain = net.forward_mosaic(dev, raw_format=M.RawFormat(temporal=Temporal(state=TemporalState(), **t), **base))
        counts, hist, zones = net.defect_counts.clone(), net.raw_stats.hist.clone(), net.raw_stats.zones.clone()
        got = net.forward_mosaic(dev, raw_format=M.RawFormat(temporal=Temporal(state=TemporalState(), **t), aberration=ab, **base))
    assert got.shape == plain.shape == (2, 3, 32, 32) and not torch.equal(got, plain) and bool(torch.isfinite(got.float()).all())
    assert torch.equal(net.defect_counts, counts) and int(counts[:, 1].sum()) >= 2
    assert torch.equal(net.raw_stats.hist, hist) and torch.equal(net.raw_stats.zones, zones)
