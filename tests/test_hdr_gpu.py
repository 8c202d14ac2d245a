"""Multi-exposure HDR merge on an MI355X: rc_raw_hdr_merge equals the elementwise restatement (tests/hdr_ref.py) bit for bit -- every storage,
CFA and exposure count, the shapes at which the lane map can go wrong, padded lines, unaligned bases and pitches, interleaved lines, every
branch of the knee and of the motion cut, the two exact identities, device times rewritten between calls and graph replays, and the chain
through forward_mosaic."""
import ctypes as C
import dataclasses

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from hdr_ref import F32, branch_shares, restated_merge
from realcamnet_amd import _lib, ops
from realcamnet_amd.calibration import Calibration, GainMap
from realcamnet_amd.exposures import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, WAVE_SPAN, Exposures
from test_hdr_host import (HAND_BLACKS, HAND_C, HAND_KNEE, HAND_MOTION, HAND_OUT, HAND_TIMES, consistent_exposures, saturated_exposures)
from test_raw_formats_host import mipi_pack

DEV = "cuda"
BITS = {"u16": 16, "u8": 8, "mipi10": 10, "mipi12": 12}
FLOATS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("fp32", "bf16", "fp16", "u16", "u8", "mipi10", "mipi12")
STORAGE_ID = {"fp32": _lib.RC_RAW_F32, "bf16": _lib.RC_RAW_BF16, "fp16": _lib.RC_RAW_F16, "u16": _lib.RC_RAW_U16, "u8": _lib.RC_RAW_U8,
              "mipi10": _lib.RC_RAW_MIPI10, "mipi12": _lib.RC_RAW_MIPI12}
CFAS = ("RGGB", "BGGR", "GRBG", "GBRG")
# the quotients t_0 / t_e are inexact for E = 3 and 4: the division in the kernel (device times) and on the host must round alike
TIMES = {2: (1.0, 8.0), 3: (1.0, 3.0, 10.0), 4: (1.0, 2.5, 6.0, 16.0)}
# in units of the storage's full scale S (2^bits codes, or 1.0 for the float storages)
BLACKS = ((0.0625, 0.0703125, 0.05859375, 0.06640625), (0.03125, 0.0625, 0.046875, 0.0390625), (0.0, 0.0078125, 0.015625, 0.0234375), (0.0625, 0.0625, 0.0625, 0.0625))
KNEE, MOTION = (0.5, 0.75), (0.0234375, 0.0625)


def same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def scale_of(kind):
    return float(1 << BITS[kind]) if kind in BITS else 1.0


def exposures_of(kind, b, e, h, w, seed, blacks=BLACKS[0]):
    """(B, E, H, W) samples of storage `kind` on the host (int32 counts, or floats of the storage's dtype): exposure 0 is half dim, half
    uniform; of every longer exposure 55 % of the samples follow exposure 0 at the ratio of the times (with a little noise, saturating at
    full scale) and the others are uniform over the upper three quarters of the scale -- so the knee's three branches and both outcomes of the motion cut are all well populated."""
    g = torch.Generator().manual_seed(seed)
    s, t = scale_of(kind), TIMES[e]
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    black = torch.tensor(blacks, dtype=torch.float64)[2 * (ys & 1) + (xs & 1)] * s
    dim = torch.rand(b, h, w, generator=g, dtype=torch.float64) * (s / t[-1])
    d0 = torch.where(torch.rand(b, h, w, generator=g) < 0.6, dim, torch.rand(b, h, w, generator=g, dtype=torch.float64) * (0.9 * s))
    planes = [black + d0]
    for k in range(1, e):
        follow = black + d0 * (t[k] / t[0]) + (torch.rand(b, h, w, generator=g, dtype=torch.float64) - 0.5) * (s / 256.0)
        free = (0.25 + 0.75 * torch.rand(b, h, w, generator=g, dtype=torch.float64)) * s
        planes.append(torch.where(torch.rand(b, h, w, generator=g) < 0.55, follow, free))
    c = torch.stack(planes, 1)
    if kind in BITS:
        return c.round().clamp(0, s - 1).to(torch.int32)
    return c.clamp(0.0, 1.0).to(FLOATS[kind])


def delivered(kind, host, line_bytes=0):
    """The exposures as the sensor delivers them, on the host (what the restatement reads), and the RawFormat fields that describe them."""
    if kind == "u16":
        return host.to(torch.uint16), dict(storage="u16")
    if kind == "u8":
        return host.to(torch.uint8), dict(storage="u8")
    if kind in ("mipi10", "mipi12"):
        return torch.from_numpy(mipi_pack(host.numpy(), BITS[kind], line_bytes)), dict(storage=kind, width=host.shape[-1])
    return host, dict(storage="float")


def request(kind, e, motion=True, times=None, layout="frames"):
    s = scale_of(kind)
    return Exposures(times=TIMES[e] if times is None else times, knee=(KNEE[0] * s, KNEE[1] * s), motion=(MOTION[0] * s, MOTION[1]) if motion else None, layout=layout)


def check(kind, b, e, h, w, seed, line_bytes=0, cfa="RGGB", blacks=BLACKS[0], motion=True, shares=False):
    """E exposures through ops.raw_hdr_merge against the restatement; with `shares`, first the condition on the input: every branch is live."""
    host = exposures_of(kind, b, e, h, w, seed, blacks)
    src, fields = delivered(kind, host, line_bytes)
    s = scale_of(kind)
    ex = request(kind, e, motion)
    levels = tuple(v * s for v in blacks)
    want, info = restated_merge(src, fields["storage"], levels, ex.times, ex.knee, ex.motion, fields.get("width"), details=True)
    if shares:
        got = branch_shares(info)
        assert bool(((got >= 0.1) & (got <= 0.6)).all()), (kind, e, got.tolist())
    got = ops.raw_hdr_merge(src.to(DEV), M.RawFormat(cfa=cfa, black_level=levels, white_level=s, **fields), ex)
    assert got.is_contiguous() and got.shape == (b, h, w) and got.dtype == F32
    assert same(got, want), (kind, cfa, e, h, w, (got.cpu() != want).nonzero()[:8].tolist())
    return want


# ---- 1. storages, CFAs and exposure counts ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("e", (2, 3, 4))
@pytest.mark.parametrize("kind", KINDS)
def test_every_storage_cfa_and_exposure_count_equals_the_restatement(hip, kind, e):
    w = 20 if kind == "mipi10" else 22                                            # 2 mod 4 where the storage allows: the ragged last lane; 18 rows: a band tail
    for i, cfa in enumerate(CFAS):
        want = check(kind, 2, e, 18, w, 11 + 4 * e + i, cfa=cfa, blacks=BLACKS[i])
        assert torch.isfinite(want).all()


@pytest.mark.gpu
def test_the_frame_computed_by_hand(hip):
    src = torch.tensor(HAND_C, dtype=torch.int32).unsqueeze(0)
    ex = Exposures(HAND_TIMES, HAND_KNEE, HAND_MOTION)
    for kind in ("u16", "mipi10", "mipi12", "fp32"):
        dev, fields = delivered(kind, src.to(torch.float32) if kind == "fp32" else src)
        got = ops.raw_hdr_merge(dev.to(DEV), M.RawFormat(black_level=HAND_BLACKS, white_level=1023.0, **fields), ex)
        assert got.dtype == F32 and got.cpu()[0].tolist() == HAND_OUT, kind


# ---- 2. shapes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_smallest_frames(hip):
    for e in (2, 3, 4):
        for kind in KINDS:
            if kind != "mipi10":
                check(kind, 2, e, 2, 2, 21 + e)
            check(kind, 2, e, 2, 4, 31 + e)


@pytest.mark.gpu
@pytest.mark.parametrize("h", (BLOCK_ROWS, BLOCK_ROWS + 2, 2 * BLOCK_ROWS + 2))
def test_strip_and_band_seams(hip, h):
    assert (WAVE_SPAN, BLOCK_SPAN, BLOCK_ROWS, LANE_PX) == (256, 512, 16, 4)
    for i, w in enumerate((WAVE_SPAN, WAVE_SPAN + LANE_PX, BLOCK_SPAN + LANE_PX, 2 * BLOCK_SPAN + LANE_PX)):    # a strip, one lane past it, past a block, past two
        check("u16", 1, 3, h, w, 41 + i)
        check("mipi12", 1, 4, h, w, 51 + i)
        check("mipi10", 1, 2, h, w, 61 + i)
    check("fp32", 2, 4, h, BLOCK_SPAN + 2, 71)                                    # the ragged lane in a block's second strip


# ---- 3. padded lines, unaligned bases and pitches -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_padded_mipi_lines(hip):
    for lb in (0, 28, 31, 32):                                                    # 25 bytes of samples; strides that are and are not a multiple of 4
        check("mipi10", 2, 3, 18, 20, 81 + lb, line_bytes=lb)
    for lb in (0, 34, 35, 36, 40):                                                # a width that is 2 mod 4: 33 bytes, the last 3-byte group stands alone
        check("mipi12", 2, 3, 18, 22, 82 + lb, line_bytes=lb)
        check("mipi12", 2, 4, 6, 22, 83 + lb, line_bytes=lb)


def call_c(hip, ptr, kind, e, h2, w2, blacks, ex, out, batch, line_bytes=0, exposure_stride=0, frame_stride=0, dst_pitch=0, times=None):
    """rc_raw_hdr_merge through ctypes, for what ops.raw_hdr_merge does not expose: a base inside an allocation, line_bytes and strides of an
    element storage, a padded dst pitch."""
    f = _lib.RawFormatDesc(storage=STORAGE_ID[kind], cfa=0, line_bytes=line_bytes, width=0, black=(C.c_float * 4)(*blacks), white=0.0)
    d = _lib.HdrDesc(exposures=e, flags=_lib.RC_HDR_MOTION if ex.motion else 0, knee_lo=ex.knee[0], knee_hi=ex.knee[1], exposure_stride_bytes=exposure_stride,
                     frame_stride_bytes=frame_stride)
    if times is None:
        for k, t in enumerate(ex.times):
            d.times[k] = t
    if ex.motion:
        d.motion_abs, d.motion_rel = ex.motion
    _lib.check(hip.rc_raw_hdr_merge(ptr, C.byref(f), C.byref(d), None if times is None else times.data_ptr(), 0 if times is None else times.shape[0], out.data_ptr(),
                                    dst_pitch, batch, h2 // 2, w2 // 2, torch.cuda.current_stream().cuda_stream), "rc_raw_hdr_merge")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_unaligned_bases_padded_strides_and_pitches(hip):
    b, e, h, w = 2, 3, 10, 38
    # a source that starts one sample into its allocation: the base is 2 mod 8 (u16), 4 mod 16 (fp32), 1 mod 4 (u8), 2 mod 8 (bf16): sample by sample
    for kind in ("u16", "fp32", "u8", "bf16"):
        host = exposures_of(kind, b, e, h, w, 91)
        src, fields = delivered(kind, host)
        s, ex = scale_of(kind), request(kind, e)
        levels = tuple(v * s for v in BLACKS[0])
        flat = host.flatten()
        big = torch.cat([flat[:1], flat]).to(src.dtype).to(DEV)                    # one sample of headroom in front
        ptr = big.data_ptr() + src.element_size()
        assert ptr % (4 * src.element_size()) == src.element_size()
        out = torch.full((b, h, w), -7.0, device=DEV)
        call_c(hip, ptr, kind, e, h, w, levels, ex, out, b)
        assert same(out, restated_merge(src, fields["storage"], levels, ex.times, ex.knee, ex.motion)), kind
    # padded lines, spare rows between the exposures and spare bytes between the frames, and a destination pitch that is no multiple of 16
    for kind, src_pad, rows_pad, dst_pad in (("u16", 3, 0, 1), ("u16", 4, 1, 0), ("fp32", 1, 1, 3), ("u8", 2, 0, 2), ("fp16", 0, 1, 1), ("u8", 4, 1, 4)):
        host = exposures_of(kind, b, e, h, w, 92)
        src, fields = delivered(kind, host)
        s, ex = scale_of(kind), request(kind, e)
        levels = tuple(v * s for v in BLACKS[1])
        wide = torch.zeros(b, e, h + rows_pad, w + src_pad, dtype=src.dtype)
        wide[:, :, :h, :w] = src
        out = torch.full((b, h, w + dst_pad), -7.0, device=DEV)
        lb = (w + src_pad) * src.element_size()
        call_c(hip, wide.to(DEV).data_ptr(), kind, e, h, w, levels, ex, out, b, line_bytes=lb, exposure_stride=(h + rows_pad) * lb, frame_stride=e * (h + rows_pad) * lb,
               dst_pitch=(w + dst_pad) * 4)
        assert same(out[..., :w], restated_merge(src, fields["storage"], levels, ex.times, ex.knee, ex.motion)), (kind, src_pad, rows_pad, dst_pad)
        assert (out[..., w:] == -7.0).all()                                       # the padding of the destination is not written


# ---- 4. interleaved lines -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "mipi12", "mipi10", "fp32", "u8"))
def test_interleaved_lines_equal_whole_frames(hip, kind):
    b, e, h, w = 2, 3, 18, 20
    for lb in ((0, 32, 35) if kind == "mipi12" else (0,)):
        host = exposures_of(kind, b, e, h, w, 101)
        src, fields = delivered(kind, host, lb)
        s = scale_of(kind)
        levels = tuple(v * s for v in BLACKS[2])
        fmt = M.RawFormat(cfa="GRBG", black_level=levels, white_level=s, **fields)
        lines = src.permute(0, 2, 1, 3).reshape(b, e * h, src.shape[-1]).contiguous()      # row r of exposure e at row r E + e
        whole = ops.raw_hdr_merge(src.to(DEV), fmt, request(kind, e))
        for view in (lines, lines.unsqueeze(1)):
            got = ops.raw_hdr_merge(view.to(DEV), fmt, request(kind, e, layout="lines"))
            assert same(got, whole), (kind, lb)
        ex = request(kind, e)
        assert same(whole, restated_merge(src, fields["storage"], levels, ex.times, ex.knee, ex.motion, fields.get("width")))


# ---- 5. every branch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_every_branch_of_the_knee_and_of_the_motion_cut_is_live(hip, kind):
    for e in (2, 3, 4):
        check(kind, 2, e, 34, 44, 111 + e, shares=True)
    check(kind, 2, 3, 34, 44, 115, motion=False)


@pytest.mark.gpu
def test_the_two_exact_identities(hip):
    blacks = (64.0, 60.0, 68.0, 66.0)
    ex = Exposures((1, 4, 16), (3000.0, 3500.0), (2.0, 0.0))
    c, _ = consistent_exposures(2, 34, 260, 121, tuple(int(v) for v in blacks))
    s = saturated_exposures(2, 34, 260, 122)
    for kind in ("u16", "mipi12"):
        for host in (c, s):
            src, fields = delivered(kind, host)
            got = ops.raw_hdr_merge(src.to(DEV), M.RawFormat(black_level=blacks, white_level=4095.0, **fields), ex)
            assert same(got, host[:, 0].to(F32)), kind


# ---- 6. device times --------------------------------------------------------------------------------------------------------------------------------
ROWS = ([[1.0, 3.0, 10.0], [1.0, 4.0, 16.0], [0.5, 1.75, 7.0]], [[2.0, 5.0, 11.0], [1.0, 2.0, 3.0], [0.001, 0.007, 0.05]], [[1.0, 8.0, 64.0], [3.0, 10.0, 33.0], [1.0, 1.5, 2.25]])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "mipi10"))
def test_device_times_are_read_when_the_kernel_runs(hip, kind):
    b, e, h, w = 3, 3, 18, 20
    host = exposures_of(kind, b, e, h, w, 131)
    src, fields = delivered(kind, host)
    s = scale_of(kind)
    levels = tuple(v * s for v in BLACKS[0])
    fmt = M.RawFormat(black_level=levels, white_level=s, **fields)
    dev = src.to(DEV)
    for nrows in (b, 1):
        times = torch.ones(nrows, e, device=DEV)
        ex = request(kind, e, times=times)
        seen = []
        for rows in ROWS:                                       # rewritten in place between two calls: no new Exposures, no host sync
            times.copy_(torch.tensor(rows[:nrows]))
            want = restated_merge(src, fields["storage"], levels, torch.tensor(rows[:nrows]), ex.knee, ex.motion, fields.get("width"))
            assert same(ops.raw_hdr_merge(dev, fmt, ex), want), (kind, nrows, rows)
            seen.append(want)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
        # host times give the bits of the same times on the device
        assert same(ops.raw_hdr_merge(dev, fmt, request(kind, e, times=tuple(ROWS[2][0]))), restated_merge(src, fields["storage"], levels, ROWS[2][0], ex.knee, ex.motion, fields.get("width")))
    with pytest.raises(ValueError, match="rows"):
        ops.raw_hdr_merge(dev, fmt, request(kind, e, times=torch.ones(2, e, device=DEV)))
    with pytest.raises(RuntimeError, match="times tensor"):
        ops.raw_hdr_merge(dev, fmt, request(kind, e, times=torch.ones(b, e)))
    with pytest.raises(ValueError, match="contiguous"):
        ops.raw_hdr_merge(dev, fmt, request(kind, e, times=torch.ones(e, b, device=DEV).t()))


@pytest.mark.gpu
@pytest.mark.parametrize("nrows", (1, 3))
def test_graph_replay_uses_the_times_written_between_replays(hip, nrows):
    b, e, h, w = 3, 3, 18, 22
    host = exposures_of("mipi12", b, e, h, w, 141)
    src, fields = delivered("mipi12", host, 36)
    levels = tuple(v * 4096.0 for v in BLACKS[3])
    fmt = M.RawFormat(cfa="GBRG", black_level=levels, white_level=4095.0, **fields)
    times = torch.ones(nrows, e, device=DEV)
    ex = request("mipi12", e, times=times)
    call = M.GraphedCall(lambda x: ops.raw_hdr_merge(x, fmt, ex))
    dev = src.to(DEV)
    seen = []
    for rows in ROWS:
        times.copy_(torch.tensor(rows[:nrows]))                 # in place: the capture holds the tensor's address, not its values
        got = call(dev)                                         # the first call captures, the others replay
        want = restated_merge(src, "mipi12", levels, torch.tensor(rows[:nrows]), ex.knee, ex.motion, w)
        assert same(got, want), rows
        seen.append(want)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 7. whole net -----------------------------------------------------------------------------------------------------------------------------------
def bracketed_sensor(b, e, h, w, seed):
    """RAW10 lines of E exposures of a smooth scene with a few stuck samples, and the format that repairs, merges and calibrates them."""
    g = torch.Generator().manual_seed(seed)
    t = TIMES[e]
    scene = (2 + (5 * torch.arange(h)[:, None] + 3 * torch.arange(w)[None, :]) % 300).to(torch.float64) / 3.0
    c = torch.stack([(64 + scene * t[k] + torch.randint(0, 4, (b, h, w), generator=g)).round().clamp(0, 1023) for k in range(e)], 1).to(torch.int32)
    stuck = [(y, x) for y in range(3, h, 11) for x in range(1, w, 13)]
    for i, (y, x) in enumerate(stuck):
        c[:, i % e, y, x] = 1023 if i % 2 else 0
    lines = torch.from_numpy(mipi_pack(c.numpy(), 10, w * 10 // 8 + 20))
    wb = torch.tensor([[1.75, 1.0, 1.0, 1.5], [1.25, 1.0, 1.0, 2.0]], device=DEV)
    cal = Calibration(shading=GainMap.radial((h, w), 8, coeffs=((0.5,), (0.4,), (0.4,), (0.3,))), gains=wb, clip=(0.0, 1.0))
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=w, black_level=(64.0, 66.0, 62.0, 64.0), white_level=1023.0,
                      exposures=Exposures(t, (700.0, 900.0), (6.0, 0.0625)), defects=M.Defects(map=M.DefectMap.from_coords((h, w), stuck), hot=(48.0, 0.125), counts=True),
                      calibration=cal)
    return lines, fmt


@pytest.mark.gpu
def test_forward_mosaic_runs_defects_per_exposure_then_merge_then_calibrate_then_the_ingest(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    b, e, h, w = 2, 3, 80, 112
    lines, fmt = bracketed_sensor(b, e, h, w, 151)
    lines = lines.to(DEV)
    coord = O.make_coord(b, h // 2, w // 2).to(DEV, torch.bfloat16)
    with torch.no_grad():
        got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
        counts_seen = net.defect_counts.clone()
        one = dataclasses.replace(fmt, exposures=None, calibration=None)
        fixed, counts = torch.empty(b, e, h, w, dtype=torch.uint16, device=DEV), []
        for k in range(e):                                                                         # 1. on each exposure, on the codes as delivered
            out_k, counts_k = ops.raw_defects(lines[:, k], one)
            assert out_k.dtype == torch.uint16
            fixed[:, k].copy_(out_k)
            counts.append(counts_k)
        merged = ops.raw_hdr_merge(fixed, dataclasses.replace(fmt, storage="u16", width=None, defects=None, calibration=None))     # 2.
        lin = ops.raw_calibrate(merged, dataclasses.replace(fmt, storage="float", width=None, exposures=None, defects=None))      # 3. the levels are kept
        by_hand = net.forward_mosaic(lin, None, coord, raw_format=M.RawFormat(cfa="GBRG", storage="float"))                        # 4. levels 0 / 1
        short = net.forward_mosaic(lines[:, 0].contiguous(), None, coord, raw_format=dataclasses.replace(fmt, exposures=None))
    ex = fmt.exposures
    assert same(merged, restated_merge(fixed, "u16", fmt.blacks(), ex.times, ex.knee, ex.motion))
    assert merged.dtype == F32 and lin.dtype == F32 and 0.0 < lin.mean() < 1.0
    assert counts_seen.shape == (b, e, 3) and same(counts_seen, torch.stack(counts, 1)) and int(counts_seen[..., 0].min()) > 0
    assert got.shape == (b, 3, h, w) and same(got, by_hand) and not torch.equal(got, short)
