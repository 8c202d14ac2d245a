"""Temporal noise reduction on an MI355X: rc_raw_temporal equals the elementwise restatement (tests/temporal_ref.py) bit for bit -- every
storage and CFA phase, the frames at which the tap fallbacks and the lane map's seams are live, padded lines and pitches, unaligned bases,
the gain given three ways and rewritten between calls, every branch of the weight, the three exact identities, a captured A -> B, B -> A
pair replayed on rewritten inputs, and the chain through forward_mosaic with its state."""
import ctypes as C
import dataclasses

import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from hdr_ref import decoded
from realcamnet_amd import _lib, ops
from realcamnet_amd.calibration import Calibration, GainMap
from realcamnet_amd.exposures import Exposures
from realcamnet_amd.temporal import BLOCK_ROWS, BLOCK_STRIPS, LANE_PX, WAVE_OUT, WAVE_SPAN, Temporal, TemporalState
from temporal_ref import F32, blacks_of, branch_shares, restated_temporal
from test_hdr_gpu import BLACKS, KINDS, STORAGE_ID, delivered, same
from test_raw_formats_host import mipi_pack
from test_temporal_host import (BRANCH_BLACKS, BRANCH_SEED, BRANCH_SHAPE, HAND_BLACKS, HAND_GAIN, HAND_PARAMS, codes, far_state, hand_frame, hand_out,
                                request_of, scale_of, stream_of)

DEV = "cuda"


def levels_of(kind, blacks):
    return tuple(v * scale_of(kind) for v in blacks)


def want_of(src, fields, state, levels, t, gain="own"):
    c = decoded(src, fields["storage"], fields.get("width"))
    return restated_temporal(c, state, blacks_of(levels, c.shape[-2], c.shape[-1]), t.params(), t.gain if gain == "own" else gain)


def check(kind, b, h, w, seed, line_bytes=0, cfa="RGGB", blacks=BLACKS[0], gain=None, reset=False):
    """One frame and its state through ops.raw_temporal against the restatement.  A gain stays within a percent or so of 1: an exposure step
    of a few noise levels, so that the gained state still meets every branch (a gain far from 1 reads as motion everywhere)."""
    host, state = stream_of(kind, b, h, w, seed, blacks)
    src, fields = delivered(kind, host, line_bytes)
    t, levels = request_of(kind, gain=gain), levels_of(kind, blacks)
    prev = None if reset else state
    want = want_of(src, fields, prev, levels, t)
    got = ops.raw_temporal(src.to(DEV), M.RawFormat(cfa=cfa, black_level=levels, white_level=scale_of(kind), temporal=t, **fields), prev=None if reset else state.to(DEV))
    assert got.is_contiguous() and got.shape == (b, h, w) and got.dtype == F32
    assert same(got, want), (kind, cfa, h, w, (got.cpu() != want).nonzero()[:8].tolist())
    return want


# ---- 1. storages and CFA phases -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_every_storage_and_two_cfa_phases_equal_the_restatement(hip, kind):
    w = 2 * WAVE_OUT + 20 if kind == "mipi10" else 2 * WAVE_OUT + 22              # 34 x 518 (516 for RAW10): a band and two rows, a third strip, a ragged last lane
    assert BLOCK_ROWS + 2 == 34 and w in (516, 518)
    for i, cfa in ((0, "RGGB"), (1, "GBRG")):                                     # four distinct blacks each: a wave's two positions differ by the row parity
        want = check(kind, 1, BLOCK_ROWS + 2, w, 11 + i, cfa=cfa, blacks=BLACKS[i])
        assert torch.isfinite(want).all()
    check(kind, 1, 6, 20, 13, reset=True)


@pytest.mark.gpu
def test_the_6x6_frame_of_the_scalar_loop(hip):
    c, s = hand_frame()
    for gain in (None, HAND_GAIN):
        t = Temporal(noise=HAND_PARAMS[:2], alpha=HAND_PARAMS[2], ramp=HAND_PARAMS[3], gain=gain)
        for kind in ("u16", "mipi12", "fp32"):
            dev, fields = delivered(kind, c if kind == "fp32" else c.to(torch.int32))
            got = ops.raw_temporal(dev.to(DEV), M.RawFormat(black_level=HAND_BLACKS, white_level=4095.0, temporal=t, **fields), prev=s.to(DEV))
            assert got.dtype == F32 and got.cpu()[0].tolist() == hand_out(gain)[0], (kind, gain)


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_smallest_frames(hip):
    for kind in KINDS:
        for i, (h, w) in enumerate(((2, 2), (2, 4), (4, 2), (4, 4), (6, 6))):     # the tap fallbacks: no neighbour at all, on one axis, on one side
            if kind == "mipi10" and w % 4:
                continue
            check(kind, 2, h, w, 21 + i)
            check(kind, 1, h, w, 26 + i, gain=1.0078125)


SEAM_WIDTHS = sorted({254, 256, 258, 260, 510, 512, 514, 1026,                                       # a 256-column strip, a pair of them, and past four
                      WAVE_OUT - 2, WAVE_OUT, WAVE_OUT + 2, WAVE_OUT + LANE_PX, WAVE_SPAN - LANE_PX - 2,    # the columns one strip produces, and where the next begins
                      WAVE_SPAN + 2 * LANE_PX, WAVE_SPAN + WAVE_OUT - 2, WAVE_SPAN + WAVE_OUT, WAVE_SPAN + WAVE_OUT + 2, WAVE_SPAN + WAVE_OUT + LANE_PX,    # two strips' worth: a block
                      BLOCK_STRIPS * WAVE_OUT + 2 * LANE_PX + 2})                                     # the first sample of a second block


@pytest.mark.gpu
def test_strip_seams(hip):
    assert (LANE_PX, WAVE_SPAN, WAVE_OUT, BLOCK_STRIPS, BLOCK_ROWS) == (4, 256, 248, 2, 32)
    for i, w in enumerate(SEAM_WIDTHS):
        check("u16", 1, 6, w, 41 + i)
        check("mipi12", 1, 4, w, 71 + i, gain=0.9921875)
        if w % 4 == 0:
            check("mipi10", 1, 6, w, 101 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("h", (BLOCK_ROWS - 2, BLOCK_ROWS, BLOCK_ROWS + 2, 2 * BLOCK_ROWS, 2 * BLOCK_ROWS + 2))
def test_band_seams(hip, h):
    check("u16", 2, h, 22, 131)                                                   # a width of 2 mod 4
    check("mipi12", 1, h, WAVE_SPAN + LANE_PX + 2, 132, gain=1.01171875)              # two strips, the second ragged
    check("fp32", 1, h, 12, 133)
    check("u8", 1, h, BLOCK_STRIPS * WAVE_OUT + 3 * LANE_PX, 134)                 # a second block in x


@pytest.mark.gpu
def test_random_width_sweep(hip):
    g = torch.Generator().manual_seed(141)
    sizes = [(2 * int(torch.randint(1, 24, (1,), generator=g)), 2 * int(torch.randint(1, 330, (1,), generator=g))) for _ in range(20)]
    for i, (h, w) in enumerate(sizes):
        kind = ("u16", "mipi12", "fp16", "u8", "bf16")[i % 5]
        check(kind, 1 + i % 2, h, w, 142 + i, gain=None if i % 3 else 0.98828125)


# ---- 3. padded lines and pitches, unaligned bases, batches ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_padded_mipi_lines(hip):
    for lb in (0, 28, 31, 32):                                                    # 25 bytes of samples; strides that are and are not a multiple of 4
        check("mipi10", 2, 18, 20, 151 + lb, line_bytes=lb)
    for lb in (0, 34, 35, 36, 40):                                                # a width that is 2 mod 4: 33 bytes, the last 3-byte group stands alone
        check("mipi12", 2, 18, 22, 152 + lb, line_bytes=lb)
    check("mipi12", 3, 34, WAVE_SPAN + 6, 153, line_bytes=3 * (WAVE_SPAN + 6) // 2 + 5)


def call_c(hip, ptr, kind, h2, w2, blacks, t, prev, out, batch, line_bytes=0, gain=None):
    """rc_raw_temporal through ctypes, for what ops.raw_temporal does not expose: a base inside an allocation and line_bytes of an element
    storage.  prev and out: (B, 2h, >= 2w) tensors whose rows may be padded."""
    f = _lib.RawFormatDesc(storage=STORAGE_ID[kind], cfa=0, line_bytes=line_bytes, width=0, black=(C.c_float * 4)(*blacks), white=0.0)
    d = _lib.TemporalDesc(flags=(_lib.RC_TNR_RESET if prev is None else 0) | (_lib.RC_TNR_GAIN if t.gain is not None else 0), noise_abs=t.noise[0], noise_rel=t.noise[1],
                          alpha=t.alpha, ramp=t.ramp, gain=0.0 if t.gain is None else t.gain)
    _lib.check(hip.rc_raw_temporal(ptr, C.byref(f), C.byref(d), None if prev is None else prev.data_ptr(), 0 if prev is None else 4 * prev.stride(1),
                                   None if gain is None else gain.data_ptr(), 0 if gain is None else gain.shape[0], out.data_ptr(), 4 * out.stride(1), batch, h2 // 2, w2 // 2,
                                   torch.cuda.current_stream().cuda_stream), "rc_raw_temporal")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_unaligned_bases_padded_lines_and_pitches(hip):
    b, h, w = 3, 10, 38
    # a source that starts one sample into its allocation: the base is 1 mod 4 (u8), 2 mod 8 (u16): sample by sample
    for kind in ("u8", "u16"):
        host, state = stream_of(kind, b, h, w, 161, BLACKS[0])
        src, fields = delivered(kind, host)
        t, levels = request_of(kind, gain=1.005859375), levels_of(kind, BLACKS[0])
        flat = host.flatten()
        big = torch.cat([flat[:1], flat]).to(src.dtype).to(DEV)                    # one sample of headroom in front
        ptr = big.data_ptr() + src.element_size()
        assert ptr % (4 * src.element_size()) == src.element_size()
        out = torch.full((b, h, w), -7.0, device=DEV)
        call_c(hip, ptr, kind, h, w, levels, t, state.to(DEV), out, b)
        assert same(out, want_of(src, fields, state, levels, t)), kind
    # padded source lines, and prev / out pitches that are and are not a multiple of 16 bytes
    for kind, src_pad, prev_pad, dst_pad in (("u16", 3, 1, 0), ("u16", 4, 4, 1), ("fp32", 1, 0, 3), ("u8", 2, 3, 4), ("fp16", 0, 2, 2), ("u8", 4, 4, 4)):
        host, state = stream_of(kind, b, h, w, 162, BLACKS[1])
        src, fields = delivered(kind, host)
        t, levels = request_of(kind), levels_of(kind, BLACKS[1])
        wide = torch.zeros(b, h, w + src_pad, dtype=src.dtype)
        wide[..., :w] = src
        prev = torch.full((b, h, w + prev_pad), -3.0, device=DEV)
        prev[..., :w] = state.to(DEV)
        out = torch.full((b, h, w + dst_pad), -7.0, device=DEV)
        call_c(hip, wide.to(DEV).data_ptr(), kind, h, w, levels, t, prev, out, b, line_bytes=(w + src_pad) * src.element_size())
        want = want_of(src, fields, state, levels, t)
        assert same(out[..., :w], want), (kind, src_pad, prev_pad, dst_pad)
        assert (out[..., w:] == -7.0).all()                                       # the padding of the destination is not written
        # the same through the op: views of padded buffers
        fmt = M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields)
        out.fill_(-7.0)
        assert ops.raw_temporal(src.to(DEV), fmt, prev=prev[..., :w], out=out[..., :w]).data_ptr() == out.data_ptr()
        assert same(out[..., :w], want) and (out[..., w:] == -7.0).all()
        with pytest.raises(ValueError, match="alias"):
            ops.raw_temporal(src.to(DEV), fmt, prev=prev[..., :w], out=prev[..., :w])


# ---- 4. the gain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "mipi10"))
def test_gain_as_a_host_number_and_as_a_device_tensor_read_when_the_kernel_runs(hip, kind):
    b, h, w = 3, 18, 20
    host, state = stream_of(kind, b, h, w, 171, BLACKS[0])
    src, fields = delivered(kind, host)
    levels = levels_of(kind, BLACKS[0])
    dev, prev = src.to(DEV), state.to(DEV)

    def fmt_of(t):
        return M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields)

    t = request_of(kind, gain=1.0078125)
    host_bits = ops.raw_temporal(dev, fmt_of(t), prev=prev)
    assert same(host_bits, want_of(src, fields, state, levels, t))
    assert not same(host_bits, want_of(src, fields, state, levels, t, gain=None))
    assert float((host_bits.cpu() != decoded(src, fields["storage"], fields.get("width"))).float().mean()) > 0.3     # the gained state is still filtered against
    for nrows in (1, b):
        gain = torch.ones(nrows, 1, device=DEV)
        t = request_of(kind, gain=gain)
        seen = []
        for rows in ([[1.0078125], [0.9921875], [1.015625]], [[0.984375], [1.01171875], [1.00390625]], [[1.0], [1.0], [1.0]]):
            gain.copy_(torch.tensor(rows[:nrows]))                                # rewritten in place between two calls: no new Temporal, no host sync
            want = want_of(src, fields, state, levels, t, gain=torch.tensor(rows[:nrows]))
            assert same(ops.raw_temporal(dev, fmt_of(t), prev=prev), want), (kind, nrows, rows)
            seen.append(want)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
        gain.fill_(1.0078125)                                                        # a host gain gives the bits of the same gain on the device
        assert same(ops.raw_temporal(dev, fmt_of(t), prev=prev), host_bits)
    with pytest.raises(ValueError, match="rows"):
        ops.raw_temporal(dev, fmt_of(request_of(kind, gain=torch.ones(2, 1, device=DEV))), prev=prev)
    with pytest.raises(RuntimeError, match="gain tensor"):
        ops.raw_temporal(dev, fmt_of(request_of(kind, gain=torch.ones(b, 1))), prev=prev)


# ---- 5. every branch, and the identities --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("u16", "mipi12", "fp32", "u8"))
def test_all_three_branches_of_the_weight_are_live(hip, kind):
    """The input whose shares tests/test_temporal_host.py pins in the restatement (each branch at least 10 %)."""
    b, h, w = BRANCH_SHAPE
    host, state = stream_of(kind, b, h, w, BRANCH_SEED, BRANCH_BLACKS)
    src, fields = delivered(kind, host)
    t, levels = request_of(kind), levels_of(kind, BRANCH_BLACKS)
    want, info = restated_temporal(decoded(src, fields["storage"], fields.get("width")), state, blacks_of(levels, h, w), t.params(), details=True)
    assert min(branch_shares(info)) >= 0.1
    got = ops.raw_temporal(src.to(DEV), M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields), prev=state.to(DEV))
    assert same(got, want), (kind, (got.cpu() != want).nonzero()[:8].tolist())


@pytest.mark.gpu
def test_the_three_exact_identities(hip):
    blacks, params = (64.0, 60.0, 68.0, 66.0), (6.0, 0.03125, 0.125, 3.0)
    t = Temporal(noise=params[:2], alpha=params[2], ramp=params[3])
    c = codes(2, 34, 260, 181)
    cf = c.to(F32)
    far = far_state(c, blacks, params, 182)
    for kind in ("u16", "mipi12"):
        src, fields = delivered(kind, c)
        fmt = M.RawFormat(black_level=blacks, white_level=4095.0, temporal=t, **fields)
        dev = src.to(DEV)
        assert same(ops.raw_temporal(dev, fmt), cf), kind                                              # a reset
        assert same(ops.raw_temporal(dev, fmt, prev=cf.to(DEV)), cf), kind                             # a frame equal to its state
        assert same(ops.raw_temporal(dev, fmt, prev=far.to(DEV)), cf), kind                            # motion everywhere
        assert not same(ops.raw_temporal(dev, fmt, prev=(cf + 1.5).to(DEV)), cf), kind


# ---- 6. capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_graph_of_two_calls_on_explicit_buffers_replayed_on_rewritten_inputs(hip):
    b, h, w = 2, 18, 22
    kind = "mipi12"
    levels = levels_of(kind, BLACKS[3])
    frames = [stream_of(kind, b, h, w, 191 + i, BLACKS[3])[0] for i in range(4)]
    lines = [delivered(kind, f, 36) for f in frames]
    fields = lines[0][1]
    start = stream_of(kind, b, h, w, 195, BLACKS[3])[1]
    gains = ([[1.0078125], [0.9921875]], [[0.98828125], [1.01171875]])
    gain = torch.ones(b, 1, device=DEV)
    t = request_of(kind, gain=gain)
    fmt = M.RawFormat(cfa="GBRG", black_level=levels, white_level=4095.0, temporal=t, **fields)
    x0, x1 = torch.empty_like(lines[0][0], device=DEV), torch.empty_like(lines[0][0], device=DEV)
    buf_a, buf_b = start.to(DEV), torch.zeros(b, h, w, device=DEV)
    x0.copy_(lines[0][0]); x1.copy_(lines[1][0]); gain.copy_(torch.tensor(gains[0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # a warm-up outside the capture, on scratch buffers
        ops.raw_temporal(x0, fmt, prev=buf_a.clone(), out=torch.empty_like(buf_b))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # a linear graph: A -> B, then B -> A
        ops.raw_temporal(x0, fmt, prev=buf_a, out=buf_b)
        ops.raw_temporal(x1, fmt, prev=buf_b, out=buf_a)
    want = start
    for rnd in range(2):
        x0.copy_(lines[2 * rnd][0]); x1.copy_(lines[2 * rnd + 1][0]); gain.copy_(torch.tensor(gains[rnd]))     # in place: the capture holds addresses, not values
        graph.replay()
        torch.cuda.synchronize()
        for i in (2 * rnd, 2 * rnd + 1):
            want = want_of(lines[i][0], fields, want, levels, t, gain=torch.tensor(gains[rnd]))
        assert same(buf_a, want), rnd
    assert not torch.equal(want, start)


# ---- 7. whole net -------------------------------------------------------------------------------------------------------------------------------
def video_sensor(b, h, w, seed, frames=3):
    """RAW10 lines of `frames` consecutive frames of a smooth scene with noise, a moving bar and a few stuck samples, and the format that
    repairs, filters and calibrates them."""
    g = torch.Generator().manual_seed(seed)
    scene = 64 + (2 + (5 * torch.arange(h)[:, None] + 3 * torch.arange(w)[None, :]) % 300).to(torch.float64) * 2.5
    stuck = [(y, x) for y in range(3, h, 11) for x in range(1, w, 13)]
    out = []
    for k in range(frames):
        c = (scene + torch.randn(b, h, w, generator=g, dtype=torch.float64) * 4.0).round()
        c[:, :, 20 + 12 * k:32 + 12 * k] += 300.0                                 # motion: the filter lets it through
        c = c.clamp(0, 1023).to(torch.int32)
        for i, (y, x) in enumerate(stuck):
            c[:, y, x] = 1023 if i % 2 else 0
        out.append(torch.from_numpy(mipi_pack(c.numpy(), 10, w * 10 // 8 + 20)))
    wb = torch.tensor([[1.75, 1.0, 1.0, 1.5], [1.25, 1.0, 1.0, 2.0]], device=DEV)
    cal = Calibration(shading=GainMap.radial((h, w), 8, coeffs=((0.5,), (0.4,), (0.4,), (0.3,))), gains=wb, clip=(0.0, 1.0))
    fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=w, black_level=(64.0, 66.0, 62.0, 64.0), white_level=1023.0,
                      temporal=Temporal((6.0, 0.015625), alpha=0.25, ramp=3.0, state=TemporalState()),
                      defects=M.Defects(map=M.DefectMap.from_coords((h, w), stuck), hot=(48.0, 0.125)), calibration=cal)
    return out, fmt


@pytest.mark.gpu
def test_forward_mosaic_runs_defects_then_temporal_then_calibrate_and_keeps_its_state(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    b, h, w = 2, 80, 112
    video, fmt = video_sensor(b, h, w, 201)
    video = [v.to(DEV) for v in video]
    state = fmt.temporal.state
    coord = O.make_coord(b, h // 2, w // 2).to(DEV, torch.bfloat16)
    plain = M.RawFormat(cfa="GBRG", storage="float", black_level=fmt.black_level, white_level=fmt.white_level, calibration=fmt.calibration)
    one = dataclasses.replace(fmt, temporal=None, calibration=None)
    step = dataclasses.replace(fmt, storage="u16", width=None, defects=None, calibration=None)
    prev, firsts = None, []
    with torch.no_grad():
        for k, lines in enumerate(video):
            got = net.forward_mosaic(lines, None, coord, raw_format=fmt)
            fixed = ops.raw_defects(lines, one)                                                        # 1. on the codes as delivered
            prev = ops.raw_temporal(fixed, step, prev=prev)                                            # 2. chained through an explicit prev
            assert same(state.frame, prev), k
            by_hand = net.forward_mosaic(prev, None, coord, raw_format=plain)                          # 3. + 4. the calibration and the ingest
            assert got.shape == (b, 3, h, w) and same(got, by_hand), k
            firsts.append(got)
        assert not same(prev, fixed.to(F32))                                                           # the third frame was filtered
        state.reset()                                                                                  # a scene cut: the next call equals a first call
        assert same(net.forward_mosaic(video[0], None, coord, raw_format=fmt), firsts[0])
        assert same(net.forward_mosaic(video[1], None, coord, raw_format=fmt), firsts[1])
        # a state of another shape starts over
        state.frame = torch.zeros(1, h, w, device=DEV)
        assert same(net.forward_mosaic(video[0], None, coord, raw_format=fmt), firsts[0]) and state.frame.shape == (b, h, w)


@pytest.mark.gpu
def test_forward_mosaic_with_exposures_in_front(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    b, e, h, w = 2, 2, 48, 64
    g = torch.Generator().manual_seed(211)
    scene = (2 + (5 * torch.arange(h)[:, None] + 3 * torch.arange(w)[None, :]) % 200).to(torch.float64)
    video = []
    for k in range(3):
        c = torch.stack([(64 + scene * tt + torch.randn(b, h, w, generator=g, dtype=torch.float64) * 3.0).round().clamp(0, 4095) for tt in (1.0, 8.0)], 1).to(torch.int32)
        video.append(c.to(torch.uint16).to(DEV))
    ex = Exposures((1.0, 8.0), (3000.0, 3500.0), (8.0, 0.0625))
    state = TemporalState()
    fmt = M.RawFormat(storage="u16", black_level=64.0, white_level=4095.0, exposures=ex, temporal=Temporal((5.0, 0.015625), alpha=0.25, state=state),
                      defects=M.Defects(hot=(200.0, 0.25)), calibration=Calibration(gains=(1.5, 1.0, 1.0, 1.75), clip=(0.0, 1.0)))
    coord = O.make_coord(b, h // 2, w // 2).to(DEV, torch.bfloat16)
    plain = M.RawFormat(storage="float", black_level=64.0, white_level=4095.0, calibration=fmt.calibration)
    one = dataclasses.replace(fmt, exposures=None, temporal=None, calibration=None)
    prev = None
    with torch.no_grad():
        for k, frames in enumerate(video):
            got = net.forward_mosaic(frames, None, coord, raw_format=fmt)
            fixed = torch.stack([ops.raw_defects(frames[:, i].contiguous(), one) for i in range(e)], 1)
            merged = ops.raw_hdr_merge(fixed, dataclasses.replace(fmt, defects=None, temporal=None, calibration=None))
            prev = ops.raw_temporal(merged, dataclasses.replace(fmt, storage="float", exposures=None, defects=None, calibration=None), prev=prev)
            assert same(state.frame, prev) and same(got, net.forward_mosaic(prev, None, coord, raw_format=plain)), k
    assert not same(prev, merged)


@pytest.mark.gpu
def test_forward_mosaic_with_temporal_refuses_a_capture_and_names_the_capturable_form(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    b, h, w = 1, 48, 64
    video, fmt = video_sensor(b, h, w, 221, frames=1)
    lines = video[0].to(DEV)
    coord = O.make_coord(b, h // 2, w // 2).to(DEV, torch.bfloat16)
    fmt = dataclasses.replace(fmt, calibration=None)
    state = fmt.temporal.state
    mark = torch.zeros(4, device=DEV)
    with torch.no_grad():
        first = net.forward_mosaic(lines, None, coord, raw_format=fmt)                                 # outside a capture it runs
        kept = state.frame.clone()
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match=r"cannot be captured.*ops\.raw_temporal\(mosaic, raw_format, prev=, out=\)"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                mark.add_(1.0)                                                                         # the graph is not empty when the capture ends
                net.forward_mosaic(lines, None, coord, raw_format=fmt)
        torch.cuda.synchronize()
    assert first.shape == (b, 3, h, w) and same(state.frame, kept)                                     # refused before the state was touched
