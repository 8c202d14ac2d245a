"""Motion-compensated temporal noise reduction on an MI355X: rc_raw_motion_pyramid and rc_raw_temporal_mc equal their restatement
(tests/temporal_mc_ref.py) bit for bit -- every storage, odd sizes at every level, padded lines and unaligned bases, the gain given both ways
and rewritten between replays; the band, strip and block seams of the filter, grids short of and beyond the frame, wild vectors, padded and
8-byte-unaligned states, every branch of the weight; the three identities; the chain of ops on a moving scene, captured and replayed; and
forward_mosaic with its state and field."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import liteisp_oracle as O
import motion_ref
import realcamnet_amd as M
import temporal_mc_ref as R
from hdr_ref import decoded
from realcamnet_amd import _lib, ops
from realcamnet_amd.calibration import Calibration
from realcamnet_amd.exposures import Exposures
from realcamnet_amd.temporal import BLOCK_ROWS, WAVE_OUT, WAVE_SPAN, Temporal, TemporalMotion, TemporalState
from temporal_ref import F32, blacks_of, branch_shares, restated_temporal
from test_hdr_gpu import BLACKS, KINDS, STORAGE_ID, delivered, same
from test_temporal_host import request_of, scale_of, stream_of

DEV = "cuda"
FIVE = ("u8", "u16", "mipi10", "mipi12", "fp32")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def levels_of(kind, blacks):
    return tuple(v * scale_of(kind) for v in blacks)


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------------------------
def raw_frame(kind, b, h2, w2, seed):
    """Samples over the storage's whole range, on the host; a quarter of the Bayer cells are dark (every sample in the lowest 5 % of the
    range) and a quarter bright (the highest 20 %): with a white level at 0.6 of full scale and black levels near 0.06, cells below black
    and above white are both common."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(b, h2, w2, generator=g)
    mode = torch.randint(0, 4, (b, (h2 + 1) // 2, (w2 + 1) // 2), generator=g).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h2, :w2]
    u = torch.where(mode == 0, u * 0.05, torch.where(mode == 1, 0.8 + u * 0.2, u))
    if kind == "fp32":
        return u * 1.25 - 0.125
    return (u * scale_of(kind)).floor().clamp(0, scale_of(kind) - 1).to(torch.int32)


def pyramid_case(kind, b, h, w, levels, seed, cfa="RGGB", blacks=BLACKS[0], gain=None, line_bytes=0, host=None):
    host = raw_frame(kind, b, 2 * h, 2 * w, seed) if host is None else host
    src, fields = delivered(kind, host, line_bytes)
    lv, white = levels_of(kind, blacks), 0.6 * scale_of(kind)
    want = R.pyramid(decoded(src, fields["storage"], fields.get("width")).numpy(), lv, white, levels,
                     gain.cpu().numpy() if isinstance(gain, torch.Tensor) else gain)
    fmt = M.RawFormat(cfa=cfa, black_level=lv, white_level=white, **fields)
    got = ops.raw_motion_pyramid(src.to(DEV), fmt, levels, gain=gain)
    assert len(got) == levels
    for k, (g_, w_) in enumerate(zip(got, want)):
        assert g_.dtype == torch.uint8 and g_.is_contiguous() and tuple(g_.shape) == (b, h >> k, w >> k) == w_.shape
        assert np.array_equal(g_.cpu().numpy(), w_), (kind, h, w, levels, k, np.argwhere(g_.cpu().numpy() != w_)[:6].tolist())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FIVE)
def test_pyramid_every_storage_size_and_level_count(hip, kind):
    seed = 300
    for h, w in ((1, 1), (3, 5), (17, 33), (40, 130)):                            # cells: odd sizes at every level; 130: a second wave and a ragged tile
        if kind == "mipi10" and (2 * w) % 4:
            w += 1                                                                # RAW10 rows hold whole groups of 4 samples: 1 x 2, 3 x 6, 17 x 34
        for levels in range(1, 5):
            if (h >> (levels - 1)) < 1 or (w >> (levels - 1)) < 1:
                continue
            seed += 1
            for i, cfa in ((0, "RGGB"), (1, "GBRG")):                             # two phases, four unequal blacks each
                want = pyramid_case(kind, 1 + (seed & 1), h, w, levels, seed, cfa=cfa, blacks=BLACKS[i])
        assert h * w < 100 or (want[0].min() == 0 and want[0].max() == 255)       # below black and above white


@pytest.mark.gpu
def test_pyramid_of_a_wide_frame_spans_blocks(hip):
    pyramid_case("u16", 2, 36, 530, 4, 331)                                       # three blocks of 256 cells, three of 16 rows
    pyramid_case("mipi12", 1, 19, 259, 4, 332)


@pytest.mark.gpu
def test_pyramid_nan_in_float_storage_is_code_zero(hip):
    host = raw_frame("fp32", 2, 34, 66, 341)
    host[:, ::3, ::5] = float("nan")
    host[:, 1::7, 2::3] = float("inf")
    host[0, 5, 5] = -float("inf")
    want = pyramid_case("fp32", 2, 17, 33, 4, 0, host=host)
    assert (want[0][:, 0, 0] == 0).all()                                          # the cell of sample (0, 0)


@pytest.mark.gpu
def test_pyramid_padded_mipi_lines(hip):
    for lb in (0, 28, 31, 32):                                                    # 25 bytes of samples; strides that are and are not a multiple of 4
        pyramid_case("mipi10", 2, 9, 10, 2, 351 + lb, line_bytes=lb)
    for lb in (0, 34, 35, 36, 40):                                                # a width that is 2 mod 4: the last 3-byte group stands alone
        pyramid_case("mipi12", 2, 9, 11, 2, 352 + lb, line_bytes=lb)


def pyramid_c(hip, ptr, kind, b, h, w, blacks, white, levels, line_bytes=0, gain=1.0):
    """rc_raw_motion_pyramid through ctypes, for what the op does not expose: a base inside an allocation, line_bytes of an element storage."""
    f = _lib.RawFormatDesc(storage=STORAGE_ID[kind], cfa=0, line_bytes=line_bytes, width=0, black=(C.c_float * 4)(*blacks), white=white)
    out = [torch.full((b, h >> k, w >> k), 77, dtype=torch.uint8, device=DEV) for k in range(levels)]
    ptrs = (C.c_void_p * levels)(*(t.data_ptr() for t in out))
    _lib.check(hip.rc_raw_motion_pyramid(ptr, C.byref(f), gain, None, 0, levels, ptrs, b, h, w, torch.cuda.current_stream().cuda_stream), "rc_raw_motion_pyramid")
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_pyramid_unaligned_bases_and_padded_element_lines(hip):
    b, h, w, levels = 2, 9, 21, 3
    for kind in ("u8", "u16", "fp32"):
        host = raw_frame(kind, b, 2 * h, 2 * w, 361)
        src, fields = delivered(kind, host)
        lv, white = levels_of(kind, BLACKS[1]), 0.6 * scale_of(kind)
        want = R.pyramid(decoded(src, fields["storage"]).numpy(), lv, white, levels)
        # one sample into its allocation: the base is no multiple of 4 samples (and not 16-byte aligned): sample by sample
        flat = host.flatten()
        big = torch.cat([flat[:1], flat]).to(src.dtype).to(DEV)                   # one sample of headroom in front
        ptr = big.data_ptr() + src.element_size()
        assert ptr % 16 != 0 and ptr % (4 * src.element_size()) != 0
        got = pyramid_c(hip, ptr, kind, b, h, w, lv, white, levels)
        assert all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(got, want)), kind
        for pad in (1, 4):                                                        # padded lines: a pitch that is not / is a multiple of 4 samples
            wide = torch.zeros(b, 2 * h, 2 * w + pad, dtype=src.dtype)
            wide[..., :2 * w] = src
            wide = wide.to(DEV)
            got = pyramid_c(hip, wide.data_ptr(), kind, b, h, w, lv, white, levels, line_bytes=(2 * w + pad) * src.element_size())
            assert all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(got, want)), (kind, pad)
    # a MIPI frame 4 bytes into its allocation: 4-byte aligned, not 16
    host = raw_frame("mipi12", b, 2 * h, 2 * w, 362)
    src, fields = delivered("mipi12", host, 68)
    big = torch.cat([torch.zeros(4, dtype=torch.uint8), src.flatten()]).to(DEV)
    lv, white = levels_of("mipi12", BLACKS[0]), 0.6 * 4096.0
    got = pyramid_c(hip, big.data_ptr() + 4, "mipi12", b, h, w, lv, white, levels, line_bytes=68)
    want = R.pyramid(decoded(src, "mipi12", 2 * w).numpy(), lv, white, levels)
    assert (big.data_ptr() + 4) % 16 == 4 and all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(got, want))


@pytest.mark.gpu
def test_pyramid_of_a_packed_frame_equals_that_of_its_decoded_copy(hip):
    b, h, w = 2, 17, 34
    for kind in ("mipi10", "mipi12", "u16", "u8"):
        host = raw_frame(kind, b, 2 * h, 2 * w, 371)
        src, fields = delivered(kind, host)
        lv, white = levels_of(kind, BLACKS[2]), 0.6 * scale_of(kind)
        packed = ops.raw_motion_pyramid(src.to(DEV), M.RawFormat(black_level=lv, white_level=white, **fields), 4)
        as_float = ops.raw_motion_pyramid(host.to(F32).to(DEV), M.RawFormat(storage="float", black_level=lv, white_level=white), 4)
        assert all(same(p, f) for p, f in zip(packed, as_float)), kind


@pytest.mark.gpu
def test_pyramid_gain_on_the_host_and_on_the_device_rewritten_between_replays_of_one_graph(hip):
    b, h, w, levels, kind = 3, 17, 33, 3, "u16"
    host = raw_frame(kind, b, 2 * h, 2 * w, 381)
    want_plain = pyramid_case(kind, b, h, w, levels, 0, host=host)
    want_host = pyramid_case(kind, b, h, w, levels, 0, host=host, gain=1.75)
    assert not np.array_equal(want_plain[0], want_host[0])
    pyramid_case(kind, b, h, w, levels, 0, host=host, gain=torch.tensor([[0.5]], device=DEV))
    pyramid_case(kind, b, h, w, levels, 0, host=host, gain=torch.tensor([[0.5], [1.0], [2.5]], device=DEV))
    src, fields = delivered(kind, host)
    lv, white = levels_of(kind, BLACKS[0]), 0.6 * scale_of(kind)
    fmt = M.RawFormat(black_level=lv, white_level=white, **fields)
    x, gain = src.to(DEV), torch.ones(b, 1, device=DEV)
    out = [torch.zeros(b, h >> k, w >> k, dtype=torch.uint8, device=DEV) for k in range(levels)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # a warm-up outside the capture
        ops.raw_motion_pyramid(x, fmt, levels, gain=gain)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.raw_motion_pyramid(x, fmt, levels, gain=gain, out=out)
    seen = []
    for rows in ([[1.75], [0.75], [1.0]], [[0.625], [3.0], [1.25]]):
        gain.copy_(torch.tensor(rows))                                            # in place: the capture holds the address, not the values
        graph.replay()
        torch.cuda.synchronize()
        want = R.pyramid(decoded(src, "u16").numpy(), lv, white, levels, np.array(rows, dtype=np.float32))
        assert all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(out, want)), rows
        seen.append(want[0])
    assert not np.array_equal(seen[0], seen[1])
    with pytest.raises(RuntimeError, match="gain tensor"):
        ops.raw_motion_pyramid(x, fmt, levels, gain=torch.ones(b, 1))


# ---- 2. the filter ----------------------------------------------------------------------------------------------------------------------------
def field_of(b, by, bx, seed, reach=6, wild=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-reach, reach + 1, (b, by, bx, 4), generator=g, dtype=torch.int32)
    v[..., 2:] = torch.randint(0, 1 << 18, (b, by, bx, 2), generator=g, dtype=torch.int32)      # cost and texture: not looked at
    if wild:
        w = torch.tensor([40000, -40000, INT_MIN, INT_MAX, 32768, -32769], dtype=torch.int64)
        pick = torch.randint(0, 6, (b, by, bx, 2), generator=g)
        hit = torch.rand(b, by, bx, 2, generator=g) < 0.4
        v[..., :2] = torch.where(hit, w[pick], v[..., :2].to(torch.int64)).to(torch.int32)
    return v


def moved_stream(kind, b, h2, w2, seed, blacks, vec, block, gain=None):
    """test_temporal_host.stream_of the other way round, so that it holds for any field: a fractional fp32 state of independent samples
    over 0.75 of the scale, and the frame of storage `kind` -- (B,H,W) int32 counts, or floats of the storage's dtype -- that the field
    displaces it onto: frame = the displaced (and gained) state plus uniform noise whose reach is fixed per 8 x 8 tile at 1, 4 or 16
    noise levels, the three taking turns along the rows and the columns of tiles (a frame of 30 x 6 has four tiles).  A gather has no collisions, so every sample of the frame -- at a seam, behind a clamped vector, past the grid -- sits at
    its intended distance from the one state sample step 0' names, and a sample fetched from anywhere else is an unrelated value: all
    three branches of the weight are live everywhere and the fetched sample decides the output bits."""
    g = torch.Generator().manual_seed(seed)
    s, t = scale_of(kind), request_of(kind)
    ys, xs = torch.arange(h2)[:, None], torch.arange(w2)[None, :]
    black = torch.tensor(blacks, dtype=torch.float64)[2 * (ys & 1) + (xs & 1)] * s
    state = (black + torch.rand(b, h2, w2, generator=g, dtype=torch.float64) * (0.75 * s)).to(F32)
    p = R.displaced(state, vec, block).to(torch.float64)
    if gain is not None:
        gg = gain.detach().cpu().to(torch.float64).reshape(-1, 1, 1) if isinstance(gain, torch.Tensor) else float(gain)
        p = black + (p - black) * gg
    level = t.noise[0] + t.noise[1] * (p - black).clamp_min(0.0)
    tiles = (torch.arange(b)[:, None, None] + torch.arange(-(-h2 // 8))[None, :, None] + torch.arange(-(-w2 // 8))[None, None, :] + seed) % 3
    reach = torch.tensor([1.0, 4.0, 16.0], dtype=torch.float64)[tiles].repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h2, :w2]
    c = p + (2.0 * torch.rand(b, h2, w2, generator=g, dtype=torch.float64) - 1.0) * reach * level
    if kind in ("u16", "u8", "mipi10", "mipi12"):
        return c.round().clamp(0, s - 1).to(torch.int32), state
    return c.clamp(0.0, 1.0).to({"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[kind]), state


def grid_of(h2, w2, block, mode):
    """(by, bx) of a field: "fit" covers the cells exactly (rounded up), "short" stops one node early on each axis, "beyond" has two more."""
    by, bx = -(-(h2 // 2) // block), -(-(w2 // 2) // block)
    return {"fit": (by, bx), "short": (max(by - 1, 1), max(bx - 1, 1)), "beyond": (by + 2, bx + 2)}[mode]


MIN_SHARE = 0.1          # of each branch of the weight, in every filter case: what test_temporal_host.py pins for stream_of's input


def filter_case(kind, b, h2, w2, seed, block=16, grid="fit", blacks=BLACKS[0], gain=None, wild=False, vec=None, prev_view=None, cfa="RGGB", reach=6):
    """One frame and a state it was moved off by a field, through ops.raw_temporal(vectors=) against the restatement; every branch of the
    weight holds MIN_SHARE of the samples or more (checked on the restatement), so the output's bits depend on the sample fetched."""
    t, levels = request_of(kind, gain=gain), levels_of(kind, blacks)
    if vec is None:
        vec = field_of(b, *grid_of(h2, w2, block, grid), seed + 1000, reach=reach, wild=wild)
    host, state = moved_stream(kind, b, h2, w2, seed, blacks, vec, block, t.gain)
    src, fields = delivered(kind, host)
    c = decoded(src, fields["storage"], fields.get("width"))
    want, info = R.restated_temporal_mc(c, state, blacks_of(levels, h2, w2), t.params(), vec, block,
                                        t.gain.cpu() if isinstance(t.gain, torch.Tensor) else t.gain, details=True)
    assert min(branch_shares(info)) >= MIN_SHARE, (kind, h2, w2, block, grid, branch_shares(info))
    prev = state.to(DEV) if prev_view is None else prev_view(state)
    fmt = M.RawFormat(cfa=cfa, black_level=levels, white_level=scale_of(kind), temporal=t, **fields)
    got = ops.raw_temporal(src.to(DEV), fmt, prev=prev, vectors=vec.to(DEV), block=block)
    assert got.is_contiguous() and got.shape == (b, h2, w2) and got.dtype == F32
    assert same(got, want), (kind, h2, w2, block, grid, (got.cpu() != want).nonzero()[:8].tolist())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("h2", (BLOCK_ROWS - 2, BLOCK_ROWS, BLOCK_ROWS + 2, 2 * BLOCK_ROWS, 2 * BLOCK_ROWS + 2))
def test_filter_band_strip_and_block_seams(hip, h2):
    """30 .. 66 rows by 6 .. 506 columns: temporal.py's band (32 rows) and strip (248 / 256 columns) seams; blocks of 8, 16 and 32 cells are
    half, one and two bands; the grid fits, is short of and is beyond the frame."""
    assert (BLOCK_ROWS, WAVE_OUT, WAVE_SPAN) == (32, 248, 256)
    i = 0
    for w2 in (6, WAVE_OUT + 2, WAVE_SPAN, WAVE_SPAN + 2, 2 * WAVE_OUT + 2, 2 * WAVE_OUT + 10):
        assert w2 in (6, 250, 256, 258, 498, 506)
        for block in (8, 16, 32):
            kind = "mipi10" if w2 % 4 == 0 and block == 16 else ("u16", "mipi12", "u8")[i % 3]
            filter_case(kind, 1 + i % 2, h2, w2, 400 + 10 * h2 + i, block=block, grid=("fit", "short", "beyond")[(i + i // 3) % 3])
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FIVE)
def test_filter_every_storage_with_every_branch_live(hip, kind):
    w2 = 2 * WAVE_OUT + 20 if kind == "mipi10" else 2 * WAVE_OUT + 22
    for i, cfa in ((0, "RGGB"), (1, "GBRG")):
        want = filter_case(kind, 2, BLOCK_ROWS + 2, w2, 500 + i, block=8, cfa=cfa, blacks=BLACKS[i])
        assert torch.isfinite(want).all()


@pytest.mark.gpu
def test_filter_wild_vectors_are_clamped(hip):
    for i, (kind, block) in enumerate((("u16", 8), ("mipi12", 16), ("fp32", 8), ("u8", 32))):
        filter_case(kind, 2, 66, 258, 520 + i, block=block, wild=True, grid=("fit", "beyond")[i % 2])
    b, h2, w2 = 1, 34, 22
    for dx, dy in ((INT_MAX, INT_MAX), (INT_MIN, INT_MIN), (40000, -40000), (-40000, 40000), (INT_MIN, 0), (0, INT_MAX)):
        vec = torch.tensor([dx, dy, 0, 0], dtype=torch.int64).to(torch.int32).expand(b, 2, 1, 4).contiguous()
        filter_case("u16", b, h2, w2, 530, block=8, vec=vec)


@pytest.mark.gpu
def test_filter_gain_on_the_host_and_on_the_device(hip):
    b, h2, w2 = 3, 34, 260
    base = filter_case("u16", b, h2, w2, 540, block=8)
    host = filter_case("u16", b, h2, w2, 540, block=8, gain=1.0078125)
    assert not torch.equal(base, host)
    one = filter_case("u16", b, h2, w2, 540, block=8, gain=torch.tensor([[1.0078125]], device=DEV))
    assert torch.equal(one, host)
    per = filter_case("mipi12", b, h2, w2, 541, block=16, gain=torch.tensor([[1.0078125], [0.9921875], [1.015625]], device=DEV))
    assert torch.isfinite(per).all()


@pytest.mark.gpu
def test_filter_states_with_padded_rows_and_bases_that_are_not_8_or_16_byte_aligned(hip):
    b, h2 = 2, 34
    for w2, pad, lead in ((256, 2, 0), (256, 3, 1), (258, 4, 2), (22, 1, 1), (260, 0, 0), (258, 2, 0)):
        def view(state, w2=w2, pad=pad, lead=lead):
            buf = torch.full((b, h2, w2 + pad + lead), -3.0, device=DEV)
            buf[..., lead:lead + w2] = state.to(DEV)
            return buf[..., lead:lead + w2]
        probe = view(torch.zeros(b, h2, w2))
        pitch, base = 4 * probe.stride(1), probe.data_ptr()
        filter_case("u16", b, h2, w2, 550 + pad + lead, block=8, prev_view=view)
        filter_case("fp32", b, h2, w2, 560 + pad + lead, block=16, prev_view=view, wild=True)
        assert (pitch % 8, base % 8) in ((0, 0), (4, 4), (0, 4), (4, 0)) and pitch >= 4 * w2
    # the three ways the state is read: 16-byte loads at 8 mod 16, 8-byte pairs (a pitch of 8 mod 16), single samples (4 mod 8)
    assert {(4 * (w + p + l)) % 16 for w, p, l in ((256, 2, 0), (256, 3, 1), (258, 4, 2), (22, 1, 1), (260, 0, 0), (258, 2, 0))} >= {0, 8}


def temporal_mc_c(hip, src, kind, h2, w2, blacks, t, prev, vec, out, batch, by, bx, block, reset=False):
    f = _lib.RawFormatDesc(storage=STORAGE_ID[kind], cfa=0, line_bytes=0, width=0, black=(C.c_float * 4)(*blacks), white=0.0)
    d = _lib.TemporalDesc(flags=_lib.RC_TNR_RESET if reset else 0, noise_abs=t.noise[0], noise_rel=t.noise[1], alpha=t.alpha, ramp=t.ramp, gain=0.0)
    _lib.check(hip.rc_raw_temporal_mc(src.data_ptr(), C.byref(f), C.byref(d), None if prev is None else prev.data_ptr(), 0, None, 0, out.data_ptr(), 0, batch, h2 // 2,
                                      w2 // 2, None if vec is None else vec.data_ptr(), by, bx, block, torch.cuda.current_stream().cuda_stream), "rc_raw_temporal_mc")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_a_reset_reads_neither_the_state_nor_the_field(hip):
    b, h2, w2 = 2, 34, 258
    for kind in ("u16", "fp32"):
        host, _ = stream_of(kind, b, h2, w2, 570, BLACKS[0])
        src, fields = delivered(kind, host)
        out = torch.full((b, h2, w2), -7.0, device=DEV)
        temporal_mc_c(hip, src.to(DEV), kind, h2, w2, levels_of(kind, BLACKS[0]), request_of(kind), None, None, out, b, 1, 1, 16, reset=True)
        assert same(out, decoded(src, fields["storage"])), kind


# ---- 3. the identities --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_zero_field_gives_the_bits_of_the_filter_without_vectors(hip):
    for i, (kind, h2, w2, block) in enumerate((("u16", 66, 506, 16), ("mipi12", 34, 258, 8), ("fp32", 64, 256, 32), ("u8", 30, 6, 8), ("mipi10", 32, 500, 16))):
        b = 2
        host, state = stream_of(kind, b, h2, w2, 600 + i, BLACKS[i % 4])
        src, fields = delivered(kind, host)
        t, levels = request_of(kind, gain=None if i % 2 else 1.0078125), levels_of(kind, BLACKS[i % 4])
        fmt = M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields)
        dev, prev = src.to(DEV), state.to(DEV)
        plain = ops.raw_temporal(dev, fmt, prev=prev)
        by, bx = grid_of(h2, w2, block, ("fit", "short", "beyond")[i % 3])
        vec = torch.zeros(b, by, bx, 4, dtype=torch.int32, device=DEV)
        vec[..., 2:] = 12345                                                       # cost and texture are not looked at
        assert same(ops.raw_temporal(dev, fmt, prev=prev, vectors=vec, block=block), plain), kind
        assert float((plain.cpu() != decoded(src, fields["storage"], fields.get("width"))).float().mean()) > 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_two_fetches_of_the_state_agree_for_every_storage_and_alignment_of_the_state(hip, kind):
    """The two kernels share one body (csrc/temporal_kernel.hpp) and differ in the fetch of the state alone: with a zero field they give the
    same bits wherever the state lies.  36 x 262 samples in a batch of 2: a band seam (32 rows), a strip seam (248 columns) and a last lane
    of two samples; RAW10 needs a width that is 0 mod 4 and takes 260.  The state, as (lead, pad) samples in front of and behind each row:
    dense; rows of 0 mod 16 bytes on a base of 0 mod 16 (16-byte loads in both kernels); the same 8 bytes on (the plain kernel goes sample by
    sample, the other loads 16 bytes at 8 mod 16 and 8-byte pairs); 4 bytes on with a pitch of 4 mod 8 (both sample by sample)."""
    b, h2, w2, block = 2, BLOCK_ROWS + 4, WAVE_OUT + (12 if kind == "mipi10" else 14), 16
    assert (h2, w2) == (36, 260 if kind == "mipi10" else 262)
    host, state = stream_of(kind, b, h2, w2, 640, BLACKS[1])
    src, fields = delivered(kind, host)
    t, levels = request_of(kind), levels_of(kind, BLACKS[1])
    fmt = M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields)
    want = restated_temporal(decoded(src, fields["storage"], fields.get("width")), state, blacks_of(levels, h2, w2), t.params())
    dev = src.to(DEV)
    vec = torch.zeros(b, *grid_of(h2, w2, block, "fit"), 4, dtype=torch.int32, device=DEV)
    seen = set()
    for lead, pad in ((0, 0), (0, -w2 % 4), (2, -(w2 + 2) % 4), (1, 0)):
        buf = torch.full((b, h2, lead + w2 + pad), -3.0, device=DEV)
        prev = buf[..., lead:lead + w2]
        prev.copy_(state)
        base, pitch = prev.data_ptr(), 4 * prev.stride(1)
        seen.add((base % 16, pitch % 16 if base % 8 == 0 else pitch % 8))
        plain = ops.raw_temporal(dev, fmt, prev=prev)
        assert torch.equal(ops.raw_temporal(dev, fmt, prev=prev, vectors=vec, block=block), plain), (kind, lead, pad)
        assert same(plain, want), (kind, lead, pad, (plain.cpu() != want).nonzero()[:8].tolist())
    assert seen >= {(0, 0), (8, 0), (4, 4)} and (kind == "mipi10" or (0, 8) in seen), seen


@pytest.mark.gpu
def test_any_field_gives_the_bits_of_the_filter_on_the_gathered_state(hip):
    for i, (kind, h2, w2, block) in enumerate((("u16", 66, 506, 16), ("mipi12", 34, 258, 8), ("fp32", 64, 256, 32), ("u8", 34, 22, 8))):
        b = 2
        t, levels = request_of(kind, gain=None if i % 2 else 0.9921875), levels_of(kind, BLACKS[i % 4])
        vec = field_of(b, *grid_of(h2, w2, block, ("fit", "short", "beyond")[i % 3]), 620 + i, wild=i == 3)
        host, state = moved_stream(kind, b, h2, w2, 610 + i, BLACKS[i % 4], vec, block, t.gain)
        src, fields = delivered(kind, host)
        fmt = M.RawFormat(black_level=levels, white_level=scale_of(kind), temporal=t, **fields)
        dev, prev = src.to(DEV), state.to(DEV)
        rows, cols = R.gather_index(h2, w2, vec.numpy(), block)                    # step 0' in torch ops on the device: an aligned copy of the state
        gathered = prev[torch.arange(b, device=DEV)[:, None, None], torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)].contiguous()
        two_passes = ops.raw_temporal(dev, fmt, prev=gathered)
        assert same(ops.raw_temporal(dev, fmt, prev=prev, vectors=vec.to(DEV), block=block), two_passes), kind
        assert not same(two_passes, ops.raw_temporal(dev, fmt, prev=prev))


@pytest.mark.gpu
def test_a_uniform_field_on_the_moved_frame_returns_the_frame(hip):
    b, h, w, block = 2, 33, 129, 16                                               # cells
    t = Temporal(noise=(6.0, 0.03125))
    g = torch.Generator().manual_seed(640)
    big = 1000 + torch.randint(-5, 6, (b, 2 * (h + 16), 2 * (w + 16)), generator=g, dtype=torch.int32)      # texture below the noise level: an uncompensated state is blended in
    for dx, dy in ((5, -3), (-7, 8), (0, 1)):
        frame = big[:, 16 + 2 * dy:16 + 2 * dy + 2 * h, 16 + 2 * dx:16 + 2 * dx + 2 * w].contiguous()      # frame cell (x, y) = state cell (x + dx, y + dy)
        state = big[:, 16:16 + 2 * h, 16:16 + 2 * w].to(F32).contiguous()
        for kind in ("u16", "mipi12"):
            src, fields = delivered(kind, frame)
            fmt = M.RawFormat(black_level=(64.0, 60.0, 68.0, 66.0), white_level=4095.0, temporal=t, **fields)
            vec = torch.tensor([dx, dy, 0, 0], dtype=torch.int32, device=DEV).expand(b, 3, 9, 4).contiguous()
            got = ops.raw_temporal(src.to(DEV), fmt, prev=state.to(DEV), vectors=vec, block=block).cpu()
            m = 2 * max(abs(dx), abs(dy)) + 2                                     # the clamped border and one tap
            assert torch.equal(got[:, m:-m, m:-m], frame.to(F32)[:, m:-m, m:-m]), (kind, dx, dy)
            assert not torch.equal(ops.raw_temporal(src.to(DEV), fmt, prev=state.to(DEV)).cpu()[:, m:-m, m:-m], frame.to(F32)[:, m:-m, m:-m])


# ---- 4. the chain on a moving scene -------------------------------------------------------------------------------------------------------------
SCENE_CELLS = (96, 160)
SCENE_BLACKS = (R.BLACK,) * 4


def scene_frames(shifts, sigma=4.0, cells=SCENE_CELLS, seed=7):
    h, w = cells
    sc = motion_ref.scene(h, w)
    return [torch.from_numpy(R.noisy_codes(R.clean_mosaic(sc, h, w, s), sigma, seed + i)) for i, s in enumerate(shifts)]


def reference_chain(codes, state, t, tm):
    """The chain of the four ops on the CPU: both pyramids, the estimate, the mask, the filter."""
    h2, w2 = codes.shape[-2:]
    g = t.gain.cpu() if isinstance(t.gain, torch.Tensor) else t.gain
    cur = R.pyramid(codes.numpy(), SCENE_BLACKS, R.WHITE, tm.levels)
    ref = R.pyramid(state.numpy(), SCENE_BLACKS, R.WHITE, tm.levels, None if g is None else (g.numpy() if isinstance(g, torch.Tensor) else g))
    field = motion_ref.estimate(cur, ref, tm.block, tm.search, tm.refine)[0]
    ok = field[..., 3] >= tm.min_texture
    if tm.max_sad is not None:
        ok &= field[..., 2] <= tm.max_sad
    field = field.copy()
    field[..., :2] *= ok[..., None]
    out = R.restated_temporal_mc(codes.to(F32), state, blacks_of(SCENE_BLACKS, h2, w2), t.params(), field, tm.block, g)
    return out, field


def ops_chain(x, fmt, prev, tm, out=None, pyramids=(None, None)):
    t = fmt.temporal
    cur = ops.raw_motion_pyramid(x, fmt, tm.levels, out=pyramids[0])
    ref = ops.raw_motion_pyramid(prev, dataclasses.replace(fmt, storage="float", width=None), tm.levels, gain=t.gain, out=pyramids[1])
    field = ops.motion_estimate(cur, ref, tm.spec())
    v = field.vectors
    if tm.min_texture > 0 or tm.max_sad is not None:
        v[..., :2] *= field.valid(tm.min_texture, tm.max_sad)[..., None]
    return ops.raw_temporal(x, fmt, prev=prev, out=out, vectors=v, block=tm.block), v


@pytest.mark.gpu
def test_the_chain_of_ops_equals_the_reference_chain_and_replays_as_one_graph(hip):
    h, w = SCENE_CELLS
    tm = TemporalMotion(levels=R.LEVELS, block=R.BLOCK, search=R.SEARCH, refine=R.REFINE)
    gain = torch.ones(1, 1, device=DEV)
    t = Temporal(noise=(4.0, 0.0), alpha=R.NOISE_ALPHA_RAMP[0], ramp=R.NOISE_ALPHA_RAMP[1], gain=gain)
    fmt = M.RawFormat(storage="u16", black_level=R.BLACK, white_level=R.WHITE, temporal=t)
    shifts = ((5, -3), (11, -7), (-6, 9))
    frames = scene_frames(shifts)
    states = [torch.from_numpy(R.clean_mosaic(motion_ref.scene(h, w), h, w, (k, -k))).to(F32) for k in range(3)]
    x, prev, out = torch.zeros(1, 2 * h, 2 * w, dtype=torch.uint16, device=DEV), torch.zeros(1, 2 * h, 2 * w, device=DEV), torch.zeros(1, 2 * h, 2 * w, device=DEV)
    pyramids = tuple([torch.zeros(s, dtype=torch.uint8, device=DEV) for s in tm.spec().level_shapes(1, h, w)] for _ in range(2))
    x.copy_(frames[0].to(torch.uint16)); prev.copy_(states[0])
    got, v = ops_chain(x, fmt, prev, tm)                                          # eager first: also the warm-up
    want, field = reference_chain(frames[0], states[0], t, tm)
    assert (field[..., 0] == 5).all() and (field[..., 1] == -3).all()
    assert np.array_equal(v.cpu().numpy(), field) and same(got, want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gv = ops_chain(x, fmt, prev, tm, out=out, pyramids=pyramids)
    for k, g in ((1, 1.0), (2, 1.0078125)):
        x.copy_(frames[k].to(torch.uint16)); prev.copy_(states[k]); gain.fill_(g)      # in place: the capture holds addresses, not values
        graph.replay()
        torch.cuda.synchronize()
        want, field = reference_chain(frames[k], states[k], t, tm)
        assert (field[..., 0] == shifts[k][0] - k).all() and (field[..., 1] == shifts[k][1] + k).all(), k
        assert np.array_equal(gv.cpu().numpy(), field) and same(out, want), k


# ---- 5. forward_mosaic ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_mosaic_estimates_compensates_and_keeps_its_state_and_field(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    cells = (64, 80)
    h2, w2 = 2 * cells[0], 2 * cells[1]
    shifts = ((0, 0), (3, -2), (7, -5))                                           # a pan of (3, -2) and then (4, -3) cells a frame
    video = [f.to(torch.uint16).to(DEV) for f in scene_frames(shifts, cells=cells)]
    state, tm = TemporalState(), TemporalMotion()
    t = Temporal(noise=(4.0, 0.0), state=state, motion=tm)
    fmt = M.RawFormat(storage="u16", black_level=R.BLACK, white_level=R.WHITE, temporal=t, calibration=Calibration(gains=(1.5, 1.0, 1.0, 1.75), clip=(0.0, 1.0)))
    step = dataclasses.replace(fmt, calibration=None)
    plain = M.RawFormat(storage="float", black_level=R.BLACK, white_level=R.WHITE, calibration=fmt.calibration)
    coord = O.make_coord(1, *cells).to(DEV, torch.bfloat16)
    prev, firsts, fields, states = None, [], [], []
    with torch.no_grad():
        for k, frame in enumerate(video):
            got = net.forward_mosaic(frame, None, coord, raw_format=fmt)
            if prev is None:
                prev, v = ops.raw_temporal(frame, step), None
                assert state.field is None
            else:
                prev, v = ops_chain(frame, step, prev, tm)
                assert same(state.field, v) and state.field.shape == (1, 4, 5, 4), k
                d = tuple(a - b for a, b in zip(shifts[k], shifts[k - 1]))          # the state shows the last frame: the vector is the pan's step
                assert (v[..., 0] == d[0]).all() and (v[..., 1] == d[1]).all(), (k, v[..., :2].reshape(-1, 2).tolist())
            assert same(state.frame, prev), k
            assert same(got, net.forward_mosaic(prev, None, coord, raw_format=plain)), k
            firsts.append(got)
            fields.append(v)
            states.append(prev)
        no_motion = dataclasses.replace(step, temporal=dataclasses.replace(t, motion=None))
        assert not same(ops.raw_temporal(video[2], no_motion, prev=states[1]), states[2])              # the field mattered
        state.reset()                                                             # a scene cut: the next calls equal the first ones
        assert state.field is None
        assert same(net.forward_mosaic(video[0], None, coord, raw_format=fmt), firsts[0]) and state.field is None
        assert same(net.forward_mosaic(video[1], None, coord, raw_format=fmt), firsts[1]) and same(state.field, fields[1])
        state.frame = torch.zeros(1, h2 + 2, w2, device=DEV)                      # a state of another shape starts over
        assert same(net.forward_mosaic(video[0], None, coord, raw_format=fmt), firsts[0]) and state.field is None and state.frame.shape == (1, h2, w2)
        # a texture threshold above every block's: every vector is zero, the bits are motion=None's
        top = max(int(f[..., 3].max()) for f in fields[1:]) + 1
        flat_state, none_state = TemporalState(), TemporalState()
        flat = dataclasses.replace(fmt, temporal=dataclasses.replace(t, state=flat_state, motion=TemporalMotion(min_texture=top)))
        none = dataclasses.replace(fmt, temporal=dataclasses.replace(t, state=none_state, motion=None))
        for k, frame in enumerate(video):
            assert same(net.forward_mosaic(frame, None, coord, raw_format=flat), net.forward_mosaic(frame, None, coord, raw_format=none)), k
            assert same(flat_state.frame, none_state.frame) and none_state.field is None
            if k > 0:
                assert int(flat_state.field[..., :2].abs().max()) == 0 and int(flat_state.field[..., 3].max()) < top
        assert not same(none_state.frame, prev)                                   # and without compensation the pan is not filtered the same way
        sad = TemporalState()
        capped = dataclasses.replace(fmt, temporal=dataclasses.replace(t, state=sad, motion=TemporalMotion(max_sad=0)))
        for frame in video[:2]:
            net.forward_mosaic(frame, None, coord, raw_format=capped)
        assert int(sad.field[..., :2].abs().max()) == 0 and int(sad.field[..., 2].min()) > 0


@pytest.mark.gpu
def test_forward_mosaic_with_exposures_in_front_of_the_compensated_filter(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    b, e, cells = 2, 2, (32, 48)
    h2, w2 = 2 * cells[0], 2 * cells[1]
    sc = motion_ref.scene(*cells)
    g = torch.Generator().manual_seed(711)
    video = []
    for k in range(3):
        base = torch.from_numpy(R.clean_mosaic(sc, *cells, (2 * k, -k))).expand(b, h2, w2) - R.BLACK       # the scene moves (2, -1) cells a frame
        c = torch.stack([(R.BLACK + base * tt * 0.45 + torch.randn(b, h2, w2, generator=g, dtype=torch.float64) * 3.0).round().clamp(0, 4095) for tt in (1.0, 8.0)], 1)
        video.append(c.to(torch.int32).to(torch.uint16).to(DEV))
    ex = Exposures((1.0, 8.0), (3000.0, 3500.0), (8.0, 0.0625))
    state, tm = TemporalState(), TemporalMotion(levels=2, block=8, search=3)
    fmt = M.RawFormat(storage="u16", black_level=R.BLACK, white_level=4095.0, exposures=ex, temporal=Temporal((5.0, 0.015625), alpha=0.25, state=state, motion=tm),
                      defects=M.Defects(hot=(200.0, 0.25)), calibration=Calibration(gains=(1.5, 1.0, 1.0, 1.75), clip=(0.0, 1.0)))
    coord = O.make_coord(b, *cells).to(DEV, torch.bfloat16)
    plain = M.RawFormat(storage="float", black_level=R.BLACK, white_level=4095.0, calibration=fmt.calibration)
    one = dataclasses.replace(fmt, exposures=None, temporal=None, calibration=None)
    step = dataclasses.replace(fmt, storage="float", exposures=None, defects=None, calibration=None)
    prev = None
    with torch.no_grad():
        for k, frames in enumerate(video):
            got = net.forward_mosaic(frames, None, coord, raw_format=fmt)
            fixed = torch.stack([ops.raw_defects(frames[:, i].contiguous(), one) for i in range(e)], 1)
            merged = ops.raw_hdr_merge(fixed, dataclasses.replace(fmt, defects=None, temporal=None, calibration=None))
            if prev is None:
                prev = ops.raw_temporal(merged, step)
                assert state.field is None
            else:
                prev, v = ops_chain(merged, step, prev, tm)
                assert same(state.field, v) and v.shape == (b, 4, 6, 4)
            assert same(state.frame, prev) and same(got, net.forward_mosaic(prev, None, coord, raw_format=plain)), k
    assert not same(prev, merged)


@pytest.mark.gpu
def test_forward_mosaic_with_motion_refuses_a_capture_with_the_same_message(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    cells = (64, 64)
    frame = scene_frames(((0, 0),), cells=cells)[0].to(torch.uint16).to(DEV)
    state = TemporalState()
    fmt = M.RawFormat(storage="u16", black_level=R.BLACK, white_level=R.WHITE, temporal=Temporal((4.0, 0.0), state=state, motion=TemporalMotion()))
    coord = O.make_coord(1, *cells).to(DEV, torch.bfloat16)
    mark = torch.zeros(4, device=DEV)
    with torch.no_grad():
        first = net.forward_mosaic(frame, None, coord, raw_format=fmt)
        kept = state.frame.clone()
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match=r"cannot be captured.*ops\.raw_temporal\(mosaic, raw_format, prev=, out=\)"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                mark.add_(1.0)                                                    # the graph is not empty when the capture ends
                net.forward_mosaic(frame, None, coord, raw_format=fmt)
        torch.cuda.synchronize()
    assert first.shape == (1, 3, 128, 128) and same(state.frame, kept) and state.field is None
