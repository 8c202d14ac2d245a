"""Sensor calibration on an MI355X: rc_raw_calibrate equals the elementwise restatement (tests/test_calibrate_host.py) bit for bit -- every
storage, CFA and result dtype, the shapes at which the lane map can go wrong, unaligned bases and pitches, each step alone, per-frame device
gains, the ingest as a second yardstick, the chained pipeline and graph replays that see rewritten gains."""
import ctypes as C
import dataclasses

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.calibration import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, WAVE_SPAN, Calibration, GainMap, Pwl
from test_calibrate_host import HAND_BLACKS, HAND_CLIP, HAND_CURVE, HAND_GAINS, HAND_IN, HAND_MAP, HAND_OUT, HAND_WHITE, knee_with_a_visible_seam, restated_calibrate
from test_raw_formats_host import mipi_pack

DEV = "cuda"
BITS = {"u16": 16, "u8": 8, "mipi10": 10, "mipi12": 12}
FLOATS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("fp32", "bf16", "fp16", "u16", "u8", "mipi10", "mipi12")
STORAGE_ID = {"fp32": _lib.RC_RAW_F32, "bf16": _lib.RC_RAW_BF16, "fp16": _lib.RC_RAW_F16, "u16": _lib.RC_RAW_U16, "u8": _lib.RC_RAW_U8}
OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# in units of the storage's full scale: a knee curve that expands 4x, per-position blacks, a white level on the linear scale
KNEE_X, KNEE_Y = (0.0, 0.25, 0.5, 0.75, 0.9375), (0.0, 0.25, 0.6875, 1.75, 3.9375)
BLACKS, WHITE = (0.0625, 0.0703125, 0.05859375, 0.06640625), 3.75
GAINS, CLIP = (1.96875, 1.0, 1.015625, 1.5625), (0.0, 1.0)


def same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def frame(kind, b, h, w, seed):
    """(host frame, full scale): uniform-random counts of the storage's depth, or floats of its dtype in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind in BITS:
        return torch.randint(0, 1 << BITS[kind], (b, h, w), generator=g, dtype=torch.int32), float(1 << BITS[kind])
    return torch.rand(b, h, w, generator=g).to(FLOATS[kind]), 1.0


def delivered(kind, host, line_bytes=0):
    """The frame as the sensor delivers it, on the host (what the restatement reads), and the RawFormat fields that describe it."""
    if kind == "u16":
        return host.to(torch.uint16), dict(storage="u16")
    if kind == "u8":
        return host.to(torch.uint8), dict(storage="u8")
    if kind in ("mipi10", "mipi12"):
        return torch.from_numpy(mipi_pack(host.numpy(), BITS[kind], line_bytes)), dict(storage=kind, width=host.shape[-1])
    return host, dict(storage="float")


def random_map(h2, w2, cell, seed):
    g = torch.Generator().manual_seed(seed)
    gh, gw = GainMap.nodes((h2, w2), cell)
    return GainMap(0.75 + torch.rand(4, gh, gw, generator=g), cell)


def check(kind, b, h, w, seed, line_bytes=0, cell=8, curve=True, shading=True, gains=GAINS, clip=CLIP, cfa="RGGB", dtypes=(torch.float32,)):
    """One frame through ops.raw_calibrate against the restatement, for every dtype of `dtypes`."""
    host, scale = frame(kind, b, h, w, seed)
    src, fields = delivered(kind, host, line_bytes)
    pwl = Pwl(tuple(v * scale for v in KNEE_X), tuple(v * scale for v in KNEE_Y)) if curve else None
    gmap = random_map(h, w, cell, seed + 1) if shading else None
    blacks, white = tuple(v * scale for v in BLACKS), (WHITE if curve else 1.0) * scale
    if isinstance(gains, torch.Tensor):
        gains = gains.to(DEV)
    cal = Calibration(curve=pwl, shading=gmap, gains=gains, clip=clip)
    fmt = M.RawFormat(cfa=cfa, black_level=blacks, white_level=white, **fields)
    for dt in dtypes:
        want = restated_calibrate(src, fields["storage"] if kind not in FLOATS else "float", blacks, white, None if pwl is None else (pwl.x, pwl.y),
                                  None if gmap is None else gmap.gains, cell if shading else 0, cal.gains, cal.clip, dt, fields.get("width"))
        got = ops.raw_calibrate(src.to(DEV), fmt, cal, dtype=dt)
        assert got.is_contiguous() and got.shape == (b, h, w) and got.dtype == dt
        assert same(got, want), (kind, cfa, dt, h, w, (got.cpu().double() != want.double()).nonzero()[:8].tolist())
    return want


# ---- 1. storages, CFAs and result dtypes ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_every_storage_and_cfa_equals_the_restatement(hip, kind):
    for i, cfa in enumerate(("RGGB", "BGGR", "GRBG", "GBRG")):
        want = check(kind, 2, 18, 36, 11 + i, cfa=cfa, dtypes=OUT_DTYPES)         # 9 x 18 planes at cell 8: two node rows, three node columns
        assert 0.02 < (want == 0).float().mean() < 0.6 and 0.02 < (want == 1).float().mean() < 0.6 and ((want > 0) & (want < 1)).float().mean() > 0.2


@pytest.mark.gpu
def test_the_frame_computed_by_hand(hip):
    src = torch.tensor(HAND_IN, dtype=torch.int32).unsqueeze(0)
    cal = Calibration(curve=Pwl(*HAND_CURVE), shading=GainMap(torch.tensor(HAND_MAP), 8), gains=HAND_GAINS, clip=HAND_CLIP)
    for kind in ("u16", "u8", "mipi10", "mipi12", "fp32"):
        dev, fields = delivered(kind, src.to(torch.float32) if kind == "fp32" else src)
        got = ops.raw_calibrate(dev.to(DEV), M.RawFormat(black_level=HAND_BLACKS, white_level=HAND_WHITE, **fields), cal)
        assert got.dtype == torch.float32 and got.cpu()[0].tolist() == HAND_OUT, kind


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_smallest_frames_and_ragged_widths(hip):
    for kind in ("u16", "fp32", "mipi12", "u8", "bf16"):
        check(kind, 2, 2, 2, 21)                                                  # h = 1: Gh = 2 with fy = 0 everywhere
        check(kind, 2, 2, 4, 22)
        check(kind, 2, 6, 10, 23)                                                 # a width that is 2 mod 4: the last two columns go one by one
    check("mipi10", 2, 2, 4, 24)
    check("mipi10", 2, 6, 12, 25)
    for cell in (16, 32, 64, 128):                                                # every cell: 2^-k and the node strides
        check("u16", 1, 2 * cell + 6, 4 * cell + 6, 26 + cell, cell=cell)


@pytest.mark.gpu
def test_strip_and_band_seams(hip):
    assert (WAVE_SPAN, BLOCK_SPAN, BLOCK_ROWS, LANE_PX) == (256, 512, 16, 4)
    for i, w in enumerate((WAVE_SPAN - 2, WAVE_SPAN, WAVE_SPAN + 2, WAVE_SPAN + LANE_PX, BLOCK_SPAN + LANE_PX)):
        check("u16", 1, 6, w, 31 + i)                                             # just below, at and just above a strip; two strips + 4
        check("mipi12", 1, 4, w, 41 + i)
    for i, w in enumerate((WAVE_SPAN - LANE_PX, WAVE_SPAN, WAVE_SPAN + LANE_PX, BLOCK_SPAN + LANE_PX)):
        check("mipi10", 1, 4, w, 51 + i)
    check("fp32", 2, BLOCK_ROWS + 2, 12, 61)                                      # just past a block's rows
    check("bf16", 2, BLOCK_ROWS + 6, BLOCK_SPAN + 2 * LANE_PX, 62, dtypes=(torch.bfloat16,))      # four blocks; seams in both directions
    check("u8", 1, 2 * BLOCK_ROWS + 4, WAVE_SPAN + 6, 63, cell=16)                # three bands; the node row changes inside a band and at its edge


def call_c(hip, src, storage, width, blacks, white, cal, out, line_bytes=0, dst_pitch=0, batch=None, h2=None):
    """rc_raw_calibrate through ctypes, for what ops.raw_calibrate does not expose: line_bytes of an element storage, a padded dst pitch."""
    f = _lib.RawFormatDesc(storage=storage, cfa=0, line_bytes=line_bytes, width=0, black=(C.c_float * 4)(*blacks), white=white)
    d = _lib.CalibDesc(flags=(_lib.RC_CALIB_GAINS if isinstance(cal.gains, tuple) else 0) | (_lib.RC_CALIB_CLIP if cal.clip else 0),
                       knots=len(cal.curve.x) if cal.curve else 0, cell=cal.shading.cell if cal.shading else 0)
    if cal.curve:
        for k, (x, y) in enumerate(zip(cal.curve.x, cal.curve.y)):
            d.curve_x[k], d.curve_y[k] = x, y
    if isinstance(cal.gains, tuple):
        for k in range(4):
            d.gains[k] = cal.gains[k]
    if cal.clip:
        d.clip_lo, d.clip_hi = cal.clip
    gmap = cal.shading.device_gains(DEV) if cal.shading else None
    _lib.check(hip.rc_raw_calibrate(src.data_ptr(), C.byref(f), C.byref(d), None if gmap is None else gmap.data_ptr(), None, 0, out.data_ptr(),
                                    {torch.float32: _lib.RC_F32, torch.bfloat16: _lib.RC_BF16, torch.float16: _lib.RC_F16}[out.dtype], dst_pitch,
                                    batch or src.shape[0], (h2 or src.shape[1]) // 2, width // 2, torch.cuda.current_stream().cuda_stream), "rc_raw_calibrate")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_unaligned_bases_and_padded_pitches(hip):
    # a source view offset by one sample: the base is 2 mod 8 (u16), 4 mod 16 (fp32), 1 mod 4 (u8): sample by sample
    for kind in ("u16", "fp32", "u8"):
        host, scale = frame(kind, 1, 12, 40, 71)
        src, fields = delivered(kind, host)
        flat = host.flatten()
        big = torch.cat([flat[:1], flat]).to(src.dtype).to(DEV)
        view = big[1:].view(1, 12, 40)
        assert view.data_ptr() % (4 * src.element_size()) == src.element_size()
        pwl, gmap = Pwl(tuple(v * scale for v in KNEE_X), tuple(v * scale for v in KNEE_Y)), random_map(12, 40, 8, 72)
        cal = Calibration(curve=pwl, shading=gmap, gains=GAINS, clip=CLIP)
        blacks, white = tuple(v * scale for v in BLACKS), WHITE * scale
        want = restated_calibrate(src, fields["storage"], blacks, white, (pwl.x, pwl.y), gmap.gains, 8, GAINS, CLIP)
        assert same(ops.raw_calibrate(view, M.RawFormat(black_level=blacks, white_level=white, **fields), cal), want)
    # MIPI lines with padding bytes, odd strides included: every row's alignment moves
    for lb in (0, 61, 64):
        check("mipi10", 2, 10, 44, 73 + lb, line_bytes=lb)                        # 55 bytes of samples
    for lb in (0, 69, 71, 72):
        check("mipi12", 2, 10, 46, 74 + lb, line_bytes=lb)                        # an odd packed width: the last 3-byte group stands alone
    # element storages with line_bytes > the row, and a padded dst pitch, through the C entry
    for kind, out_dt, src_pad, dst_pad in (("u16", torch.float32, 3, 0), ("u16", torch.bfloat16, 4, 5), ("fp32", torch.float32, 1, 4), ("u8", torch.float16, 2, 3),
                                           ("bf16", torch.float32, 0, 1)):
        host, scale = frame(kind, 2, 10, 36, 75)
        src, fields = delivered(kind, host)
        wide = torch.zeros(2, 10, 36 + src_pad, dtype=src.dtype)
        wide[..., :36] = src
        out = torch.full((2, 10, 36 + dst_pad), -7.0, dtype=out_dt, device=DEV)
        pwl, gmap = Pwl(tuple(v * scale for v in KNEE_X), tuple(v * scale for v in KNEE_Y)), random_map(10, 36, 8, 76)
        cal = Calibration(curve=pwl, shading=gmap, gains=GAINS, clip=CLIP)
        blacks, white = tuple(v * scale for v in BLACKS), WHITE * scale
        call_c(hip, wide.to(DEV), STORAGE_ID[kind], 36, blacks, white, cal, out, line_bytes=wide.shape[-1] * src.element_size(), dst_pitch=out.shape[-1] * out.element_size())
        want = restated_calibrate(src, fields["storage"], blacks, white, (pwl.x, pwl.y), gmap.gains, 8, GAINS, CLIP, out_dt)
        assert same(out[..., :36], want), (kind, out_dt)
        assert (out[..., 36:] == -7.0).all()                                      # the padding of the destination is not written


# ---- 3. each step alone -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knots", (2, 16))
def test_curve_alone_on_every_knot_and_beyond_both_ends(hip, knots):
    x = tuple(float(100 + 37 * j + j * j) for j in range(knots))                   # uneven spacing; inexact slopes
    y = tuple(float(10 + 91 * j + 13 * j * j) / 7.0 for j in range(knots))
    pwl = Pwl(x, y)
    cal = Calibration(curve=pwl)
    planted = [0.0, 1.0, x[0] - 1.0, x[-1] + 1.0, x[-1] + 1000.0] + [v + d for v in x for d in (-1.0, 0.0, 1.0)]
    g = torch.Generator().manual_seed(81)
    counts = torch.randint(0, int(x[-1]) + 300, (2, 8, 40), generator=g, dtype=torch.int32)
    counts.view(-1)[:len(planted)] = torch.tensor(planted, dtype=torch.int32)
    counts[1].view(-1)[7:7 + len(planted)] = torch.tensor(planted, dtype=torch.int32)      # ... on other positions and lanes too
    white = y[-1] * 2.0
    for kind, src in (("u16", counts.to(torch.uint16)), ("float", counts.to(torch.float32) - 50.0), ("mipi12", torch.from_numpy(mipi_pack(counts.numpy(), 12)))):
        fields = dict(storage=kind, width=40) if kind == "mipi12" else dict(storage=kind)
        want = restated_calibrate(src, kind, (1.0, 2.0, 3.0, 4.0), white, (pwl.x, pwl.y), width=40)
        got = ops.raw_calibrate(src.to(DEV), M.RawFormat(black_level=(1.0, 2.0, 3.0, 4.0), white_level=white, **fields), cal)
        assert same(got, want), (kind, knots, (got.cpu() != want).nonzero()[:8].tolist())
    # a knot whose two segments disagree in fp32: the sample on it takes the segment that starts there
    kx, ky, from_below, starts_there = knee_with_a_visible_seam()
    got = ops.raw_calibrate(torch.full((1, 2, 4), kx[1], device=DEV), M.RawFormat(), Calibration(curve=Pwl(kx, ky)))
    assert (got == starts_there).all() and from_below != starts_there


@pytest.mark.gpu
def test_map_gains_and_clip_alone(hip):
    for kind in ("u16", "bf16", "mipi10"):
        check(kind, 2, 20, 44, 91, curve=False, gains=None, clip=None)            # a random map only
        check(kind, 2, 20, 44, 92, curve=False, shading=False, clip=None)         # gains only
        check(kind, 2, 20, 44, 93, curve=False, shading=False, gains=None, clip=(0.25, 0.5))       # clip only
    # a constant map multiplies by exactly that constant
    host, _ = frame("fp32", 1, 34, 38, 94)
    const = GainMap(torch.full((4, 4, 4), 1.2345678), 8)
    got = ops.raw_calibrate(host.to(DEV), M.RawFormat(), Calibration(shading=const))
    assert same(got, host * torch.tensor(1.2345678))


# ---- 4. per-frame gains from a device tensor ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_of_three_with_device_gains(hip):
    rows = torch.tensor([[1.5, 1.0, 1.0, 2.25], [0.0, 1.0, 0.5, 3.0], [2.0, 1.25, 1.25, 1.0]])
    for kind in ("u16", "mipi10", "fp16"):
        a = check(kind, 3, 18, 36, 101, gains=rows, clip=None)
        b = check(kind, 3, 18, 36, 101, gains=rows[1:2].clone(), clip=None)        # one row shared by every frame
        assert same(a[1], b[1]) and not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    with pytest.raises(ValueError, match="rows"):
        ops.raw_calibrate(torch.zeros(3, 4, 4, device=DEV), M.RawFormat(), Calibration(gains=torch.ones(2, 4, device=DEV)))
    with pytest.raises(RuntimeError, match="gains tensor"):
        ops.raw_calibrate(torch.zeros(3, 4, 4, device=DEV), M.RawFormat(), Calibration(gains=torch.ones(3, 4)))
    with pytest.raises(ValueError, match="contiguous"):
        ops.raw_calibrate(torch.zeros(3, 4, 4, device=DEV), M.RawFormat(), Calibration(gains=torch.ones(4, 3, device=DEV).t()))


# ---- 5. the ingest as a second yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_unit_gains_then_ingest_is_the_ingest_of_the_frame(hip, kind):
    """Step 2 is the ingest's own normalisation: calibrate with gains (1,1,1,1) only, ingest the fp32 result with levels 0 / 1, and the packed
    RAW and the cond image are those of the frame ingested with its own storage and levels."""
    host, scale = frame(kind, 2, 38, 44, 111)
    src, fields = delivered(kind, host, 61 if kind == "mipi10" else 0)
    blacks, white = tuple(v * scale for v in BLACKS), 0.96875 * scale
    for cfa in ("RGGB", "GBRG"):
        fmt = M.RawFormat(cfa=cfa, black_level=blacks, white_level=white, **fields)
        lin = ops.raw_calibrate(src.to(DEV), fmt, Calibration(gains=(1.0, 1.0, 1.0, 1.0)))
        for dt in (torch.bfloat16, torch.float32):
            a, cond = ops.raw_ingest(lin, dtype=dt, pad_to=16, cond_hw=(24, 40), raw_format=M.RawFormat(cfa=cfa, storage="float", black_level=0.0, white_level=1.0))
            ra, rcond = ops.raw_ingest(src.to(DEV), dtype=dt, pad_to=16, cond_hw=(24, 40), raw_format=fmt)
            assert same(a, ra) and same(cond, rcond), (kind, cfa, dt)


# ---- 6. whole nets ----------------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_of(name):
    if name not in _NETS:
        torch.manual_seed(0)
        _NETS[name] = getattr(M, name)().to(device=DEV, dtype=torch.bfloat16).eval()
    return _NETS[name]


def sensor(b, h, w, seed, gains):
    """RAW10 lines of a smooth 10-bit frame with a few stuck samples, and the format that repairs and calibrates them."""
    g = torch.Generator().manual_seed(seed)
    c = (200 + 3 * (torch.arange(h)[:, None] + torch.arange(w)[None, :]) % 700 + torch.randint(0, 6, (b, h, w), generator=g)).to(torch.int32)
    stuck = [(y, x) for y in range(3, h, 11) for x in range(1, w, 13)]
    for i, (y, x) in enumerate(stuck):
        c[:, y, x] = 1023 if i % 2 else 0
    lines = torch.from_numpy(mipi_pack(c.numpy(), 10, w * 10 // 8 + 20))
    cal = Calibration(curve=Pwl((0.0, 512.0, 768.0, 1023.0), (0.0, 512.0, 1536.0, 4096.0)), shading=GainMap.radial((h, w), 8, coeffs=((0.5,), (0.4,), (0.4,), (0.3,))),
                      gains=gains, clip=(0.0, 1.0))
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=w, black_level=(64.0, 66.0, 62.0, 64.0), white_level=4000.0,
                      defects=M.Defects(map=M.DefectMap.from_coords((h, w), stuck), hot=(48.0, 0.125)), calibration=cal)
    return lines, fmt


@pytest.mark.gpu
def test_forward_mosaic_runs_defects_then_calibrate_then_the_ingest(hip):
    net = net_of("LiteISPNet_GFM_LSC")
    wb = torch.tensor([[1.75, 1.0, 1.0, 1.5], [1.25, 1.0, 1.0, 2.0]], device=DEV)
    lines, fmt = sensor(2, 80, 112, 121, wb)
    lines = lines.unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        fixed = ops.raw_defects(lines, dataclasses.replace(fmt, calibration=None))                      # on the codes as delivered
        assert fixed.dtype == torch.uint16
        lin = ops.raw_calibrate(fixed, dataclasses.replace(fmt, storage="u16", width=None, defects=None))
        assert lin.dtype == torch.float32
        by_hand = net.forward_mosaic(lin, None, coord, raw_format=M.RawFormat(cfa="GBRG", storage="float"))
        plain = net.forward_mosaic(lines, None, coord, raw_format=dataclasses.replace(fmt, black_level=0.0, white_level=1023.0, defects=None, calibration=None))
    want = restated_calibrate(fixed, "u16", fmt.blacks(), fmt.white_level, (fmt.calibration.curve.x, fmt.calibration.curve.y), fmt.calibration.shading.gains, 8, wb,
                              fmt.calibration.clip)
    assert same(lin, want) and 0.0 < lin.mean() < 1.0
    assert got.shape == (2, 3, 80, 112) and same(got, by_hand) and not torch.equal(got, plain)


# ---- 7. graph capture: rewritten gains are seen on replay --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("LiteISPNet", "ISPUNet_GFM"))
def test_graph_replay_uses_the_gains_written_between_replays(hip, name):
    net = net_of(name)
    wb = torch.tensor([[1.75, 1.0, 1.0, 1.5], [1.25, 1.0, 1.0, 2.0]], device=DEV)
    lines, fmt = sensor(2, 80, 112, 131, wb)
    lines = lines.to(DEV)
    coord = O.make_coord(2, 40, 56).to(DEV, torch.bfloat16)
    stage_fmt = dataclasses.replace(fmt, defects=None)
    call = M.GraphedCall(lambda x, co: (net.forward_mosaic(x, None, co, raw_format=fmt, out_format="rgb8"), ops.raw_calibrate(x, stage_fmt)))
    seen = []
    for rows in ([[1.75, 1.0, 1.0, 1.5], [1.25, 1.0, 1.0, 2.0]], [[0.5, 0.75, 0.75, 0.25], [2.0, 1.0, 1.0, 1.0]], [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]):
        wb.copy_(torch.tensor(rows))                            # in place: the capture holds the tensor's address, not its values
        y, lin = call(lines, coord)                             # the first call captures, the others replay
        with torch.no_grad():
            eager = net.forward_mosaic(lines, None, coord, raw_format=fmt, out_format="rgb8")
        want = restated_calibrate(lines, "mipi10", fmt.blacks(), fmt.white_level, (fmt.calibration.curve.x, fmt.calibration.curve.y), fmt.calibration.shading.gains, 8,
                                  torch.tensor(rows), fmt.calibration.clip, width=112)
        assert same(y, eager) and same(lin, want), rows
        seen.append(y.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not lin[1].any()
