"""GPU: RAW noise measurement (rc_raw_noise, ops.raw_noise, RawFormat.noise).  The yardstick is tests/raw_noise_ref.py, the NumPy restatement
of the header's arithmetic computed on the CPU (never the kernel's own output).  Every comparison of the tables is equality on integers: the
sums are integer, so there is no tolerance anywhere but in the last test, which compares a float64 fit.

Most cases call the C entry directly on a byte buffer, so that every storage can have padded lines: the padding holds 0xFF bytes (NaN for
the float storages) and everything outside the measured tiles holds saturating values, so a read beyond a line, the ROI or the last whole
tile spoils a tile or moves its energy.  The shapes are the smallest at which the kernel takes each of its paths: one tile; (40, 72) with
an ROI that starts on an odd row and leaves cells over on both sides; (144, 520) x 2 frames, three strips of 128 cells by three units of 32
cell rows, more than one block; and 2048 small frames, where a block has to walk several units."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.raw_format import CFAS
from raw_stats_ref import PACKERS, pack_raw10, pad_lines
import raw_noise_ref as R

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


def measured(spec, H, W):
    """(y0, y1, x0, x1) in samples: the whole tiles of the ROI."""
    cy0, cx0, rh, rw = spec.check(H // 2, W // 2)
    return 2 * cy0, 2 * (cy0 + rh // spec.tile * spec.tile), 2 * cx0, 2 * (cx0 + rw // spec.tile * spec.tile)


def frame(storage, B, H, W, seed, spec):
    """The decoded sample values (B, H, W) as float32 -- what the reference reads -- and the same as the storage's bytes (B, H, row bytes).
    Blocks of 16 x 16 samples at random levels from just below black to 85 % with a little noise, so that the tiles spread over the level
    bins and over low and high energy bins (a tile of 8 or 16 cells spans several blocks); a few samples at full scale, a few at 0 (far below
    black) and, for the float storages, NaN, +-inf and values beyond both clamps; everything outside the measured tiles saturates."""
    rng = np.random.default_rng(seed)
    y0, y1, x0, x1 = measured(spec, H, W)
    base = rng.uniform(0.06, 0.85, (B, -(-H // 16), -(-W // 16))).repeat(16, 1).repeat(16, 2)[:, :H, :W]
    v = base + rng.normal(0.0, 0.004, (B, H, W)) * rng.integers(0, 4, (B, 1, 1))
    n = (y1 - y0) * (x1 - x0)
    if storage in FLOATS:
        v = v.astype(np.float32)
        for i, x in enumerate((NAN, INF, -INF, -3.0, 7.5, 1.0, 0.0625, 0.0)):
            p = (i * 7919 + 11) % n
            v[i % B, y0 + p // (x1 - x0), x0 + p % (x1 - x0)] = x
        outside = np.float32(3.0e38)
    else:
        full = FULL[storage]
        v = np.rint(v * full).clip(0, full).astype(np.float32)
        for i, x in enumerate((full, 0, full, 0)):
            p = (i * 7919 + 11) % n
            v[i % B, y0 + p // (x1 - x0), x0 + p % (x1 - x0)] = x
        outside = np.float32(full)
    keep = np.zeros((H, W), dtype=bool)
    keep[y0:y1, x0:x1] = True
    v = np.where(keep[None], v, outside)
    if storage in FLOATS:
        t = torch.from_numpy(v).to(FLOATS[storage])
        return t.float().numpy(), t.contiguous().view(torch.uint8).numpy().reshape(B, H, -1)          # rounded to the storage type: exact from here on
    return v, PACKERS[storage](v.astype(np.int64))


def line_bytes_of(storage, W, pad):
    """A line stride `pad` samples (element storages) or bytes (MIPI) longer than the row."""
    if storage == "mipi10":
        return W * 5 // 4 + pad
    if storage == "mipi12":
        return W * 3 // 2 + pad
    return (W + pad) * ESIZE[storage]


def launch_on(hip, src, B, storage, cfa, blacks, top, spec, h, w, line_bytes):
    """rc_raw_noise on the device bytes `src`, into outputs that hold garbage; the outputs stay on the device."""
    roi = spec.roi if spec.roi is not None else (0, 0, 0, 0)
    hist = torch.full((B, 4, spec.levels, 320), -7, dtype=torch.int32, device=DEV)
    level = torch.full((B, 4, spec.levels), 1 << 40, dtype=torch.int64, device=DEV)
    f = _lib.RawFormatDesc(storage=CODE[storage], cfa=CFAS[cfa], line_bytes=line_bytes, width=2 * w, black=(C.c_float * 4)(*blacks), white=0.0)
    d = _lib.RawNoiseDesc(roi=(C.c_int32 * 4)(*roi), tile=spec.tile, bits=spec.bits, level_bits=spec.level_bits, top=top, sat=spec.sat_code, floor=spec.floor_code)
    _lib.check(hip.rc_raw_noise(src.data_ptr(), C.byref(f), C.byref(d), hist.data_ptr(), level.data_ptr(), B, h, w, torch.cuda.current_stream().cuda_stream),
               "rc_raw_noise")
    torch.cuda.synchronize()
    return hist, level


def launch(hip, body, storage, cfa, blacks, top, spec, h, w, line_bytes):
    """rc_raw_noise on the bytes `body` (B, 2h, row bytes) laid out with `line_bytes` and 0xFF filler."""
    src = torch.from_numpy(pad_lines(body, line_bytes, 0xFF)).to(DEV)
    assert src.data_ptr() % 4 == 0
    hist, level = launch_on(hip, src, body.shape[0], storage, cfa, blacks, top, spec, h, w, line_bytes)
    return hist.cpu().numpy(), level.cpu().numpy()


def diff(got, want):
    return int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()), int(got[0].sum()), int(want[0].sum())


def check(hip, storage, cfa, B, H, W, seed, spec, pad, spoiled=False):
    blacks, top = levels(storage)
    values, body = frame(storage, B, H, W, seed, spec)
    want = R.restated_raw_noise(values, cfa, blacks, top, spec)
    y0, y1, x0, x1 = measured(spec, H, W)
    tiles = B * 4 * ((y1 - y0) // (2 * spec.tile)) * ((x1 - x0) // (2 * spec.tile))
    assert 0 < want[0].sum() <= tiles and (not spoiled or want[0].sum() < tiles)             # tiles are measured; where asked, some are spoiled
    got = launch(hip, body, storage, cfa, blacks, top, spec, H // 2, W // 2, line_bytes_of(storage, W, pad))
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (storage, cfa, (B, H, W), spec, pad, diff(got, want))


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
def test_one_tile(hip, storage):
    for i, (tile, cfa) in enumerate(((4, "RGGB"), (8, "GRBG"), (16, "BGGR"), (4, "GBRG"))):
        bits = (10, 8, 16, 12)[i]                                                            # the last case: two tiles side by side
        check(hip, storage, cfa, 1 + i % 2, 2 * tile, 4 * tile if i == 3 else 2 * tile, 3 + i, M.RawNoise(tile=tile, bits=bits, level_bits=3 + i, sat=1 << bits), (0, 3, 4, 1)[i])


@pytest.mark.gpu
@pytest.mark.parametrize("cfa", sorted(CFAS))
@pytest.mark.parametrize("storage", STORAGES)
def test_the_matrix_equals_the_restatement(hip, storage, cfa):
    """All seven storages x four cfa x three tiles on a (40, 72) mosaic: the whole frame (left-over cells at tile 8 and 16) and an ROI with an
    odd cy0, an even cx0 and left-over cells on both axes; samples at full scale and at 0 against sat and floor set and unset, NaN / +-inf
    for the float storages; bits, level_bits and the two kinds of line padding go round with the case."""
    i = STORAGES.index(storage) + sorted(CFAS).index(cfa)
    for n, tile in enumerate((4, 8, 16)):
        bits = (8, 10, 16)[(i + n) % 3]
        S = (1 << bits) - 1
        lb = 3 + (i + n) % 4
        check(hip, storage, cfa, 2, 40, 72, 10 + n, M.RawNoise(tile=tile, bits=bits, level_bits=lb, sat=S + 1), (2, 1, 3)[n])
        check(hip, storage, cfa, 2, 40, 72, 20 + n, M.RawNoise(tile=tile, bits=bits, level_bits=lb, roi=(1, 2, 18, 33), sat=S - S // 10, floor=-(S // 50)), (1, 4, 2)[n],
              spoiled=True)


@pytest.mark.gpu
def test_sat_and_floor_are_met_exactly(hip):
    """u16 with top - black = S: the codes are the samples minus 64.  Four tiles of R at 500, one sample each at sat, sat - 1, floor, floor + 1."""
    v = np.full((1, 8, 32), 564, dtype=np.int64)
    for tx, x in enumerate((964, 963, 54, 55)):
        v[0, 2, 8 * tx + 4] = x
    spec = M.RawNoise(tile=4, bits=10, level_bits=3, sat=900, floor=-10)
    want = R.restated_raw_noise(v, "RGGB", (64.0,) * 4, 1087.0, spec)
    got = launch(hip, PACKERS["u16"](v), "u16", "RGGB", (64.0,) * 4, 1087.0, spec, 4, 16, 64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert R.tiles_of(got[0]).sum(-1).tolist() == [[2, 4, 4, 4]] and got[1][0, 0].sum() == 2 * 16 * 500 + (963 - 564) + (55 - 564)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ("f32", "u16", "mipi10", "mipi12"))
def test_several_strips_units_and_blocks(hip, storage):
    """(144, 520) x 2 frames: 72 x 260 cells -- three strips (the third holds 4 cells: one tile of 4, none of 8 or 16) by three units of 32
    cell rows (the third holds 8), nine units walked by three blocks per frame."""
    check(hip, storage, "GRBG", 2, 144, 520, 40, M.RawNoise(tile=4, bits=10, level_bits=5), 4, spoiled=True)
    check(hip, storage, "BGGR", 2, 144, 520, 41, M.RawNoise(tile=8, bits=12, level_bits=6, roi=(3, 2, 69, 258), sat=4096), 3)
    check(hip, storage, "RGGB", 2, 144, 520, 42, M.RawNoise(tile=16, bits=10, level_bits=4, roi=(1, 0, 70, 258)), 1, spoiled=True)


@pytest.mark.gpu
def test_a_block_walks_several_units(hip):
    """2048 frames share the blocks: each frame gets one block of four waves for the nine units of a (144, 520) frame.  The frames are copies
    of one frame, made on the device; the tables of every frame are that frame's."""
    spec = M.RawNoise(tile=8, bits=8, level_bits=3, sat=250, floor=-5)
    blacks, top = levels("u8")
    values, body = frame("u8", 1, 144, 520, 45, spec)
    want = R.restated_raw_noise(values, "GBRG", blacks, top, spec)
    src = torch.from_numpy(body).to(DEV).expand(2048, -1, -1).contiguous()
    hist, level = launch_on(hip, src, 2048, "u8", "GBRG", blacks, top, spec, 72, 260, 520)
    assert 0 < want[0].sum() < 4 * 9 * 32
    assert torch.equal(hist, torch.from_numpy(want[0]).to(DEV).expand(2048, -1, -1, -1)) and torch.equal(level, torch.from_numpy(want[1]).to(DEV).expand(2048, -1, -1))


@pytest.mark.gpu
def test_a_frame_that_does_not_start_on_a_dword(hip):
    """RAW12, two frames, an odd line stride: 10 lines of 13 bytes put frame 1 at byte 130.  One tile of 4 and a left-over cell row."""
    spec = M.RawNoise(tile=4, bits=12, level_bits=4, sat=4096)
    blacks, top = levels("mipi12")
    values, body = frame("mipi12", 2, 10, 8, 50, spec)
    assert body.shape == (2, 10, 12) and (10 * 13) % 4 == 2
    want = R.restated_raw_noise(values, "GBRG", blacks, top, spec)
    got = launch(hip, body, "mipi12", "GBRG", blacks, top, spec, 5, 4, 13)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), diff(got, want)
    assert want[0].sum() == 8 and not np.array_equal(want[1][0], want[1][1])                 # the frames differ: frame 1 is not frame 0 read again


@pytest.mark.gpu
def test_the_largest_energy_and_negative_sums(hip):
    """bits 16, tile 16, fp32 codes of +-S: position 0 alternates per cell column (e = 2 T^2 S^2, the largest there is: 64-bit, bin 311, s1 =
    0), position 1 is +S throughout (the top level bin), position 2 alternates the other way, position 3 is -S (a negative level sum)."""
    S, T = 65535, 16
    v = np.zeros((1, 32, 64), dtype=np.float32)
    sign = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)[None, None, :]
    v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2] = sign * 4.0, 1.0, -sign * INF, -2.0
    spec = M.RawNoise(tile=T, bits=16, level_bits=6, sat=S + 1)
    want = R.restated_raw_noise(v, "RGGB", (0.0,) * 4, 1.0, spec)
    got = launch(hip, v.view(np.uint8).reshape(1, 32, -1), "f32", "RGGB", (0.0,) * 4, 1.0, spec, 16, 32, 64 * 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), diff(got, want)
    assert got[0][0, 0, 0, 311] == got[0][0, 2, 0, 311] == 2 and got[0][0, 1, 63, 0] == 2 and got[0][0, 3, 0, 0] == 2 and got[0].sum() == 8
    assert got[1][0, :, [0, 63, 0, 0]].diagonal().tolist() == [0, 2 * T * T * S, 0, -2 * T * T * S]


# ---- 2. the op: determinism, capture ----------------------------------------------------------------------------------------------------------------
def same(a, b):
    return a.hist.dtype == b.hist.dtype == torch.int32 and a.level.dtype == torch.int64 and torch.equal(a.hist, b.hist) and torch.equal(a.level, b.level)


@pytest.mark.gpu
def test_two_runs_and_two_replays_of_a_graph_are_equal(hip):
    hosts = [R.patch_scene(60 + i, 0.5, 4.0, H=128, W=520, dark=0.2)[0].repeat(2, 0) for i in range(2)]
    frames = [torch.from_numpy(hst).to(DEV) for hst in hosts]
    fmt = M.RawFormat(storage="u16", cfa="GRBG", black_level=(64.0, 60.0, 66.0, 62.0), white_level=1087.0)
    spec = M.RawNoise(tile=4, level_bits=4)
    wants = [R.restated_raw_noise(hst, "GRBG", fmt.blacks(), 1087.0, spec) for hst in hosts]
    a, b = ops.raw_noise(frames[0], fmt, spec), ops.raw_noise(frames[0], fmt, spec)
    assert same(a, b) and np.array_equal(a.hist.cpu().numpy(), wants[0][0]) and np.array_equal(a.level.cpu().numpy(), wants[0][1])
    assert a.roi == (0, 0, 64, 260) and a.unit == tuple(R.unit_of("GRBG", fmt.blacks(), 1087.0, 10))
    x = frames[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                            # a warm-up outside the capture
        ops.raw_noise(x, fmt, spec)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.raw_noise(x, fmt, spec)
    for i in (0, 0, 1):                                                                      # the same input twice: the outputs are zeroed inside the graph
        x.copy_(frames[i])
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, ops.raw_noise(frames[i], fmt, spec)) and np.array_equal(out.hist.cpu().numpy(), wants[i][0]) and np.array_equal(out.level.cpu().numpy(), wants[i][1]), i


# ---- 3. forward_mosaic ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_mosaic_measures_the_repaired_unfiltered_frame(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    rng = np.random.default_rng(62)
    c = (300 + (2 * (np.arange(32)[:, None] + np.arange(64)[None, :])) % 400 + rng.integers(0, 6, (2, 32, 64))).astype(np.int64)
    c[:, 5::9, 6::17] = 1020                                                                 # hot samples the repair replaces
    lines = torch.from_numpy(pack_raw10(c, 96)).unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 16, 32).to(DEV, torch.bfloat16)
    blacks = (64.0, 66.0, 62.0, 64.0)
    spec = M.RawNoise(tile=4, level_bits=4)
    base = dict(storage="mipi10", cfa="GBRG", width=64, black_level=blacks, white_level=1023.0, defects=M.Defects(hot=(48.0, 0.125)),
                calibration=M.Calibration(gains=(1.9, 1.0, 1.0, 1.6), clip=(0.0, 1.0)))
    fmt = M.RawFormat(noise=spec, **base)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        ns = net.raw_noise
        plain = net.forward_mosaic(lines, None, coord, raw_format=M.RawFormat(**base))
        fixed = ops.raw_defects(lines, M.RawFormat(**dict(base, calibration=None)))
        again = ops.raw_noise(fixed, M.RawFormat(storage="u16", cfa="GBRG", black_level=blacks, white_level=1023.0), spec)
    assert torch.equal(got, plain) and got.shape == (2, 3, 32, 64)                           # a measurement changes nothing
    assert fixed.dtype == torch.uint16 and not np.array_equal(fixed.cpu().numpy().astype(np.int64), c)      # the repair did something
    want = R.restated_raw_noise(fixed.cpu().numpy(), "GBRG", blacks, 1023.0, spec)
    assert isinstance(ns, M.RawNoiseStats) and ns.roi == (0, 0, 16, 32) and ns.spec is spec and same(ns, again)
    assert np.array_equal(ns.hist.cpu().numpy(), want[0]) and np.array_equal(ns.level.cpu().numpy(), want[1]) and want[0].sum() > 0
    # with the filter set, the frame in front of it is measured: the second call's tables are the second frame's, not the filtered one's
    state = M.TemporalState()
    tf = M.RawFormat(noise=spec, temporal=M.Temporal((6.0, 0.02), state=state), **base)
    c2 = (c + rng.integers(-4, 5, c.shape)).clip(0, 1023)
    lines2 = torch.from_numpy(pack_raw10(c2, 96)).unsqueeze(1).to(DEV)
    with torch.no_grad():
        y1 = net.forward_mosaic(lines, None, coord, raw_format=tf)
        first = net.raw_noise
        y2 = net.forward_mosaic(lines2, None, coord, raw_format=tf)
        second = net.raw_noise
        fixed2 = ops.raw_defects(lines2, M.RawFormat(**dict(base, calibration=None)))
        state2 = M.TemporalState()
        plain_t = M.RawFormat(temporal=M.Temporal((6.0, 0.02), state=state2), **base)
        z1 = net.forward_mosaic(lines, None, coord, raw_format=plain_t)
        z2 = net.forward_mosaic(lines2, None, coord, raw_format=plain_t)
    want2 = R.restated_raw_noise(fixed2.cpu().numpy(), "GBRG", blacks, 1023.0, spec)
    assert same(first, ns) and np.array_equal(second.hist.cpu().numpy(), want2[0]) and np.array_equal(second.level.cpu().numpy(), want2[1])
    filtered = R.restated_raw_noise(state.frame.cpu().numpy(), "GBRG", blacks, 1023.0, spec)
    assert not np.array_equal(filtered[0], want2[0])                                         # the filter changed the energies: the tap is not behind it
    assert torch.equal(y1, z1) and torch.equal(y2, z2) and torch.equal(state.frame, state2.frame)       # bit for bit what it was, the state included


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_temporal_noise_of_a_noisy_frame_equals_the_restatement(hip):
    v, _ = R.patch_scene(70, 0.5, 4.0, H=256, W=384, lo=0.10, dark=0.25)
    spec = M.RawNoise(tile=8, level_bits=4)
    fmt = M.RawFormat(storage="u16", black_level=64.0, white_level=1087.0)
    ns = ops.raw_noise(torch.from_numpy(v).to(DEV), fmt, spec)
    hist, level = R.restated_raw_noise(v, "RGGB", fmt.blacks(), 1087.0, spec)
    assert np.array_equal(ns.hist.cpu().numpy(), hist) and np.array_equal(ns.level.cpu().numpy(), level)
    unit = R.unit_of("RGGB", fmt.blacks(), 1087.0, 10)
    tn = ns.temporal_noise()
    assert tn.is_cuda and tn.dtype == torch.float64 and tn.shape == (2,)
    want = R.temporal_noise_of(hist, level, spec, unit)
    print("temporal_noise", tn.tolist(), "restated", want.tolist())
    np.testing.assert_allclose(tn.cpu().numpy(), want, rtol=1e-5)                            # the tables are equal: only the fit's float order differs
    np.testing.assert_allclose(ns.profile().cpu().numpy(), R.profile_of(hist, level, spec, unit), rtol=1e-5)
    assert 1.0 < want[0] < 6.0 and 0.01 < want[1] < 0.04                                     # a chord of sigma = sqrt(4 + level / 2), 2 at black and 21 at 90 %: sanity, the figures are the host tests'
    M.Temporal(tuple(tn.tolist()), state=M.TemporalState())                                  # the calibration loop's last step
