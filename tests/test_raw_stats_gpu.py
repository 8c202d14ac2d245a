"""GPU: RAW-domain 3A statistics (rc_raw_stats, ops.raw_stats, RawFormat.stats).  The yardstick is tests/raw_stats_ref.py, the NumPy
restatement of the header's arithmetic computed on the CPU (never the kernel's own output).  Every comparison is torch.equal on int64: the
sums are integer, so there is no tolerance anywhere.

Most cases call the C entry directly on a byte buffer, so that every storage can have padded lines: the padding holds 0xFF bytes (NaN for
the float storages) and everything outside the ROI holds saturating values, so a read beyond a line or the ROI shows in the counts or in the
focus term.  The shapes are the smallest at which the kernel takes each of its paths: one cell; (6, 10), whose width of 2 mod 4 leaves a
lane with one cell (RAW12's two-sample tail); (34, 516), one lane beyond the 256-sample tile (lane 63's neighbour, a nearly empty tile); and
(130, 1028) x 2 frames, walked by several blocks and zone rows."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.raw_format import CFAS, SLOT_POS
from raw_stats_ref import PACKERS, pack_raw10, pack_raw12, pad_lines, restated_raw_stats

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
STORAGES = ("f32", "bf16", "f16", "u16", "u8", "mipi10", "mipi12")
CODE = {"f32": _lib.RC_RAW_F32, "bf16": _lib.RC_RAW_BF16, "f16": _lib.RC_RAW_F16, "u16": _lib.RC_RAW_U16, "u8": _lib.RC_RAW_U8, "mipi10": _lib.RC_RAW_MIPI10,
        "mipi12": _lib.RC_RAW_MIPI12}
FLOATS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FULL = {"u16": 65535, "u8": 255, "mipi10": 1023, "mipi12": 4095}                            # a count storage's largest sample
ESIZE = {"f32": 4, "bf16": 2, "f16": 2, "u16": 2, "u8": 1}


def levels(storage):
    """(black levels in position order, top) in the storage's own units."""
    if storage in FLOATS:
        return (0.0625, 0.05, 0.07, 0.06), 1.0
    full = FULL[storage]
    return tuple(float(round(full * f)) for f in (0.0625, 0.05, 0.07, 0.06)), float(full)


def frame(storage, B, H, W, seed, roi=None):
    """The decoded sample values (B, H, W) as float32 -- what the reference reads -- and the same as the storage's bytes (B, H, row bytes).
    Everything outside the ROI (cells) saturates.  Float frames hold NaN, +-inf, negative values and values above top inside the ROI."""
    rng = np.random.default_rng(seed)
    if storage in FLOATS:
        v = rng.uniform(-0.1, 1.15, (B, H, W)).astype(np.float32)
        cy0, cx0, rh, rw = roi if roi is not None else (0, 0, H // 2, W // 2)
        for i, x in enumerate((NAN, INF, -INF, -3.0, 7.5, 1.0, 0.0625)):
            p = (i * 7919 + 11) % (4 * rh * rw)
            v[i % B, 2 * cy0 + p // (2 * rw), 2 * cx0 + p % (2 * rw)] = x
        outside = np.float32(3.0e38)
        t = torch.from_numpy(v).to(FLOATS[storage])
    else:
        v = rng.integers(0, FULL[storage] + 1, (B, H, W)).astype(np.float32)
        outside = np.float32(FULL[storage])
        t = None
    if roi is not None:
        cy0, cx0, rh, rw = roi
        keep = np.zeros((H, W), dtype=bool)
        keep[2 * cy0:2 * (cy0 + rh), 2 * cx0:2 * (cx0 + rw)] = True
        v = np.where(keep[None], v, outside)
        if t is not None:
            t = torch.from_numpy(v).to(FLOATS[storage])
    if t is not None:
        values = t.float().numpy()                                                           # rounded to the storage type: exact from here on
        body = t.contiguous().view(torch.uint8).numpy().reshape(B, H, -1)
    else:
        values = v
        body = PACKERS[storage](v.astype(np.int64))
    return values, body


def line_bytes_of(storage, W, pad):
    """A line stride `pad` samples (element storages) or bytes (MIPI) longer than the row."""
    if storage == "mipi10":
        return W * 5 // 4 + pad
    if storage == "mipi12":
        return W * 3 // 2 + pad
    return (W + pad) * ESIZE[storage]


def launch(hip, body, storage, cfa, blacks, top, spec, h, w, line_bytes):
    """rc_raw_stats on the bytes `body` (B, 2h, row bytes) laid out with `line_bytes` and 0xFF filler, into outputs that hold garbage."""
    B = body.shape[0]
    src = torch.from_numpy(pad_lines(body, line_bytes, 0xFF)).to(DEV)
    assert src.data_ptr() % 4 == 0
    roi = spec.roi if spec.roi is not None else (0, 0, 0, 0)
    hist = torch.full((B, 4, spec.bins), -7, dtype=torch.int64, device=DEV)
    zones = torch.full((B,) + spec.grid + (8,), 1 << 40, dtype=torch.int64, device=DEV)
    f = _lib.RawFormatDesc(storage=CODE[storage], cfa=CFAS[cfa], line_bytes=line_bytes, width=2 * w, black=(C.c_float * 4)(*blacks), white=0.0)
    d = _lib.RawStatsDesc(roi=(C.c_int32 * 4)(*roi), grid=(C.c_int32 * 2)(*spec.grid), bits=spec.bits, hist_bits=spec.hist_bits, top=top, sat=spec.sat_code,
                          dark=spec.dark_code)
    _lib.check(hip.rc_raw_stats(src.data_ptr(), C.byref(f), C.byref(d), hist.data_ptr(), zones.data_ptr(), B, h, w, torch.cuda.current_stream().cuda_stream),
               "rc_raw_stats")
    torch.cuda.synchronize()
    return hist.cpu(), zones.cpu()


def diff(got, want):
    return int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()), (got[1] - want[1]).flatten(0, 2).abs().amax(0).tolist()


def check(hip, storage, cfa, B, H, W, seed, spec, pad, classes=False):
    blacks, top = levels(storage)
    values, body = frame(storage, B, H, W, seed, spec.roi)
    want = restated_raw_stats(values, cfa, blacks, top, spec)
    if classes:
        assert want[1][..., 0].sum() > 0 and want[1][..., 5].sum() > 0 and want[1][..., 6].sum() > 0          # all three classes occur
    got = launch(hip, body, storage, cfa, blacks, top, spec, H // 2, W // 2, line_bytes_of(storage, W, pad))
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (storage, cfa, (B, H, W), spec, pad, diff(got, want))


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
def test_one_cell(hip, storage):
    W = 4 if storage == "mipi10" else 2
    for cfa in sorted(CFAS):
        check(hip, storage, cfa, 1, 2, W, 3, M.RawStats(grid=(1, 1), bits=10, hist_bits=8), 0)
        check(hip, storage, cfa, 2, 2, W, 4, M.RawStats(grid=(1, 1), bits=8, hist_bits=6, sat=200, dark=20), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("cfa", sorted(CFAS))
@pytest.mark.parametrize("storage", STORAGES)
def test_the_matrix_equals_the_restatement(hip, storage, cfa):
    """All seven storages x four cfa over the partial-lane and the tile-edge shapes; bits 8 / 10 / 16, hist_bits 6 / 10, thresholds set and
    unset and the two kinds of line padding go round with the case, so that every value meets every storage and every cfa."""
    i = STORAGES.index(storage) + sorted(CFAS).index(cfa)
    W = 12 if storage == "mipi10" else 10
    for n in range(3):
        bits = (8, 10, 16)[(i + n) % 3]
        S = (1 << bits) - 1
        hb = 6 if (i + n) % 2 else min(10, bits)
        cut = dict(sat=S - S // 10, dark=S // 3)
        # the partial lane: the whole frame, and an inner ROI with odd offsets
        check(hip, storage, cfa, 2, 6, W, 10 + n, M.RawStats(grid=(3, W // 2), bits=bits, hist_bits=hb), (2, 1, 3)[n])
        check(hip, storage, cfa, 2, 6, W, 20 + n, M.RawStats(grid=(2, 3), bits=bits, hist_bits=hb, roi=(1, 1, 2, 3), **cut), (1, 3, 2)[n])
    bits = (10, 16, 8)[i % 3]
    S = (1 << bits) - 1
    # the tile edge: lane pairs straddle the ROI's odd left edge, boundaries that divide nothing; an aligned (vector loads) and an odd stride
    check(hip, storage, cfa, 1, 34, 516, 30, M.RawStats(grid=(5, 7), bits=bits, hist_bits=min(10, bits), roi=(1, 1, 15, 255), sat=S - S // 10, dark=S // 3),
          4 if i % 2 else 1, classes=True)
    check(hip, storage, cfa, 1, 34, 516, 31, M.RawStats(grid=(17, 64), bits=(8, 10, 16)[i % 3], hist_bits=6), 1 if i % 2 else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ("f32", "u16", "mipi10", "mipi12"))
def test_several_blocks_and_narrow_zones(hip, storage):
    """(130, 1028) x 2 frames: 65 x 514 cells, ten tiles walked by five blocks of two tiles each.  Zones of 1.02 x 8.03 cells; and an ROI 64 cells wide
    with 64 zone columns, where a lane's two cells always fall in different zones."""
    check(hip, storage, "GRBG", 2, 130, 1028, 40, M.RawStats(grid=(64, 64), bits=10, hist_bits=8, sat=1000, dark=200), 4, classes=True)
    check(hip, storage, "BGGR", 2, 130, 1028, 41, M.RawStats(grid=(7, 64), bits=12, hist_bits=10, roi=(0, 3, 65, 64), sat=4000, dark=1000), 3, classes=True)


@pytest.mark.gpu
def test_a_frame_that_does_not_start_on_a_dword(hip):
    """RAW12, two frames, an odd line stride: 6 lines of 17 bytes put frame 1 at byte 102."""
    spec = M.RawStats(grid=(3, 5), bits=12, hist_bits=10, sat=4000, dark=200)
    blacks, top = levels("mipi12")
    values, body = frame("mipi12", 2, 6, 10, 50)
    assert body.shape == (2, 6, 15) and (6 * 17) % 4 == 2
    want = restated_raw_stats(values, "GBRG", blacks, top, spec)
    got = launch(hip, body, "mipi12", "GBRG", blacks, top, spec, 3, 5, 17)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), diff(got, want)
    assert not torch.equal(want[1][0], want[1][1])                                          # the frames differ: frame 1 is not frame 0 read again


# ---- 2. the op: determinism, capture, helpers -------------------------------------------------------------------------------------------------
def same(a, b):
    return a.hist.dtype == b.hist.dtype == torch.int64 and torch.equal(a.hist, b.hist) and torch.equal(a.zones, b.zones)


@pytest.mark.gpu
def test_two_runs_and_two_replays_of_a_graph_are_equal(hip):
    rng = np.random.default_rng(60)
    hosts = [rng.integers(0, 1024, (2, 130, 1028)).astype(np.uint16) for _ in range(2)]
    frames = [torch.from_numpy(hst).to(DEV) for hst in hosts]
    fmt = M.RawFormat(storage="u16", cfa="GRBG", black_level=(64.0, 60.0, 66.0, 62.0), white_level=1023.0)
    spec = M.RawStats(grid=(9, 33), bits=10, hist_bits=8, sat=1000, dark=100)
    wants = [restated_raw_stats(hst, "GRBG", fmt.blacks(), 1023.0, spec) for hst in hosts]
    a, b = ops.raw_stats(frames[0], fmt, spec), ops.raw_stats(frames[0], fmt, spec)
    assert same(a, b) and torch.equal(a.hist.cpu(), wants[0][0]) and torch.equal(a.zones.cpu(), wants[0][1])
    x = frames[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                            # a warm-up outside the capture
        ops.raw_stats(x, fmt, spec)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.raw_stats(x, fmt, spec)
    for i in (0, 0, 1):                                                                      # the same input twice: the outputs are zeroed inside the graph
        x.copy_(frames[i])
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, ops.raw_stats(frames[i], fmt, spec)) and torch.equal(out.zones.cpu(), wants[i][1]) and torch.equal(out.hist.cpu(), wants[i][0]), i


@pytest.mark.gpu
def test_awb_gains_of_a_frame_with_known_ratios(hip):
    """R exactly half and B exactly twice the greens, GBRG, black 0, top 1023 at 10 bits (the codes are the samples): (2, 1, 1, 0.5)."""
    rng = np.random.default_rng(61)
    g = rng.integers(50, 200, (2, 16, 24)) * 2
    cells = (g // 2, g, g, g * 2)                                                            # R, G1, G2, B
    m = np.zeros((2, 32, 48), dtype=np.uint16)
    for c, pos in enumerate(SLOT_POS["GBRG"]):
        m[:, pos // 2::2, pos % 2::2] = cells[c]
    fs = ops.raw_stats(torch.from_numpy(m).to(DEV), M.RawFormat(storage="u16", cfa="GBRG", white_level=1023.0), M.RawStats(grid=(4, 4)))
    gains = fs.awb_gains()
    assert gains.dtype == torch.float32 and gains.is_cuda and gains.tolist() == [[2.0, 1.0, 1.0, 0.5]] * 2
    want = torch.from_numpy(np.stack([c.reshape(2, -1).sum(1) for c in cells], 1))
    assert torch.equal(fs.zones[..., 1:5].sum((1, 2)).cpu(), want) and fs.saturated_fraction().tolist() == [0.0, 0.0]
    assert torch.equal(fs.mean_level().cpu(), want.double() / (16 * 24 * 1023.0))
    cal = M.Calibration(gains=torch.ones(2, 4, device=DEV))
    cal.gains.lerp_(gains, 0.5)                                                              # the loop's step, on the device
    assert cal.gains.tolist() == [[1.5, 1.0, 1.0, 0.75]] * 2


# ---- 3. forward_mosaic ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_mosaic_measures_what_enters_the_calibration(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    rng = np.random.default_rng(62)
    c = (300 + (2 * (np.arange(32)[:, None] + np.arange(64)[None, :])) % 400 + rng.integers(0, 6, (2, 32, 64))).astype(np.int64)
    c[:, 5::9, 6::17] = 1020                                                                 # hot samples the repair replaces
    lines = torch.from_numpy(pack_raw10(c, 96)).unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 16, 32).to(DEV, torch.bfloat16)
    blacks = (64.0, 66.0, 62.0, 64.0)
    spec = M.RawStats()
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=64, black_level=blacks, white_level=1023.0, defects=M.Defects(hot=(48.0, 0.125)),
                      calibration=M.Calibration(gains=(1.9, 1.0, 1.0, 1.6), clip=(0.0, 1.0)), stats=spec)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        fs = net.raw_stats
        plain = net.forward_mosaic(lines, None, coord, raw_format=dataclasses.replace(fmt, stats=None))
        fixed = ops.raw_defects(lines, dataclasses.replace(fmt, calibration=None, stats=None))
    assert torch.equal(got, plain) and got.shape == (2, 3, 32, 64)                           # a measurement changes nothing
    assert fixed.dtype == torch.uint16 and not np.array_equal(fixed.cpu().numpy().astype(np.int64), c)      # the repair did something
    want = restated_raw_stats(fixed.cpu().numpy(), "GBRG", blacks, 1023.0, spec)
    assert isinstance(fs, M.RawFrameStats) and fs.roi == (0, 0, 16, 32) and fs.spec is spec
    assert torch.equal(fs.hist.cpu(), want[0]) and torch.equal(fs.zones.cpu(), want[1])
