"""GPU: raw stills (rc_dng_encode, ops.raw_dng, RawFormat.dng).  The yardstick is tests/dng_ref.py, the NumPy restatement of the header's file
computed on the CPU (never the kernel's own output); every comparison is equality of bytes.  The reader half of dng_ref, which shares
nothing with the encoder half, decodes what the device wrote back to the samples.

Shapes are in samples, width x height: 32 x 16 with tile (32, 16), exactly one tile; 38 x 18 with tile (16, 16), 3 x 2 tiles padded on both
edges with a width of 2 mod 4 (RAW10, whose width is a multiple of 4, takes 40 x 18: the same grid, 8 padded columns); 528 x 20 with tile
(272, 16), two steps of the wave per line and a padded tile.  Every shape is coded as a batch of three frames -- flat, a ramp, uniform noise
over the storage's full range -- whose files have different lengths.

One test here needs no GPU and carries no `gpu` mark: test_the_cases_cover_... asserts, on the restatement's streams alone, that the cases above
contain what they are meant to; it runs with the CPU suite.
"""
import ctypes as C
import dataclasses
import functools
import numpy as np
import pytest
import torch

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.raw_format import CFAS
import dng_ref as R

DEV = "cuda"
FULL = {"u16": 65535, "u8": 255, "mipi10": 1023, "mipi12": 4095}
STORAGES = ("u16", "u8", "mipi10", "mipi12")
SHAPES = {"one_tile": ((32, 16), (32, 16)), "edges": ((38, 18), (16, 16)), "two_steps": ((528, 20), (272, 16))}
GUARD = 256


def size_of(shape, storage):
    (w, h), tile = SHAPES[shape]
    return ((40, h) if shape == "edges" and storage == "mipi10" else (w, h)), tile


@functools.lru_cache(maxsize=None)
def frames_of(shape, storage):
    """(3, H, W) int64: flat (every difference 0 but the first), a ramp, uniform noise over the storage's full range."""
    (w, h), _ = size_of(shape, storage)
    full = FULL[storage]
    rng = np.random.default_rng(sum(map(ord, shape + storage)))
    flat = np.full((h, w), full // 2 + 1, np.int64)              # 2^(P-1): the first difference is 0 too
    ramp = (3 * np.arange(w)[None, :] + 5 * np.arange(h)[:, None]) % (full + 1)
    return np.stack([flat, ramp, rng.integers(0, full + 1, (h, w))])


@functools.lru_cache(maxsize=None)
def want_of(shape, storage, nc):
    """[(file, tile streams)] of the three frames, by the restatement."""
    _, (tw, th) = size_of(shape, storage)
    return [R.encode(f, storage, tw, th, nc, white=FULL[storage]) for f in frames_of(shape, storage)]


def lines(frames, storage):
    return torch.from_numpy(np.stack([R.pack_lines(f, storage) for f in frames]))


def fmt_of(storage, w, **kw):
    return M.RawFormat(storage=storage, width=w if storage.startswith("mipi") else None, white_level=float(FULL[storage]), **kw)


def abi_encode(hip, body, storage, w, dng, capacity, pitch=None, shift=0, fmt=None):
    """rc_dng_encode through the C ABI on the lines `body` (B, H, row bytes) uint8 laid out with `pitch` bytes per line (0xFF filler), the
    frames' base `shift` bytes past a 256-byte boundary, and GUARD bytes of 0xA5 in front of and behind the B x capacity destination.
    Returns (the destination with its guards (uint8), lengths)."""
    b, h, row = body.shape
    pitch = row if pitch is None else pitch
    padded = np.full((b, h, pitch), 0xFF, np.uint8)
    padded[:, :, :row] = body
    src = torch.full((shift + padded.size + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[shift:shift + padded.size] = torch.from_numpy(padded.reshape(-1)).to(DEV)
    fmt = fmt_of(storage, w) if fmt is None else fmt
    plan = dataclasses.replace(dng, capacity=None).plan(h, w, fmt)
    header = torch.from_numpy(np.frombuffer(dng.header(h, w, fmt), np.uint8).copy()).to(DEV)
    f = _lib.RawFormatDesc(storage=R_CODE[storage], cfa=CFAS[fmt.cfa], line_bytes=pitch, width=w)
    d = dng.desc()
    dst = torch.full((2 * GUARD + b * capacity,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((b,), -1, dtype=torch.int64, device=DEV)
    scratch = torch.zeros((b * plan.scratch_bytes // 4,), dtype=torch.int32, device=DEV)
    _lib.check(hip.rc_dng_encode(src.data_ptr() + shift, C.byref(f), C.byref(d), header.data_ptr(), plan.header_bytes, plan.offsets_at, plan.counts_at,
                                 scratch.data_ptr(), dst.data_ptr() + GUARD, lengths.data_ptr(), b, h, w, capacity, torch.cuda.current_stream().cuda_stream),
               "rc_dng_encode")
    return dst.cpu().numpy(), lengths.cpu().tolist()


R_CODE = {"u16": _lib.RC_RAW_U16, "u8": _lib.RC_RAW_U8, "mipi10": _lib.RC_RAW_MIPI10, "mipi12": _lib.RC_RAW_MIPI12}


# ---- 0. what the cases cover (the restatement's streams; no GPU) ----------------------------------------------------------------------------------
def test_the_cases_cover_stuffing_every_padding_length_and_odd_tiles():
    stuffed, pads, odd = 0, set(), 0
    for shape in SHAPES:
        for storage in STORAGES:
            (w, h), (tw, th) = size_of(shape, storage)
            for nc in (1, 2):
                for f, (_, streams) in zip(frames_of(shape, storage), want_of(shape, storage, nc)):
                    odd += sum(len(s) & 1 for s in streams)
                    for ty in range(-(-h // th)):
                        for tx in range(-(-w // tw)):
                            data, pad = R.entropy_bytes(*R.entropy_bits(R.tile_samples(f, ty, tx, tw, th), R.PRECISION[storage], nc))
                            stuffed += data.count(b"\xff\x00")
                            pads.add(pad)
    assert stuffed > 0 and pads == set(range(8)) and odd > 0, (stuffed, pads, odd)


# ---- 1. the file, byte for byte --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_files_equal_the_restatement(hip, shape, storage):
    (w, h), tile = size_of(shape, storage)
    frames = frames_of(shape, storage)
    x = lines(frames, storage).to(DEV)
    for nc in (1, 2):
        want = want_of(shape, storage, nc)
        dng = M.Dng(tile=tile, components=nc)
        out = ops.raw_dng(x, fmt_of(storage, w), dng)
        assert out.fmt == dng and out.size == (h, w) and out.buffer.dtype == torch.uint8 and out.buffer.shape == (3, dng.plan(h, w, fmt_of(storage, w)).capacity)
        assert out.lengths.dtype == torch.int64 and out.lengths.cpu().tolist() == [len(f) for f, _ in want], (shape, storage, nc)
        files = out.files()
        assert len(set(map(len, files))) == 3                                                # frames of different compressed length
        for b, (f, _) in enumerate(want):
            assert files[b] == f and out.tobytes(b) == f, (shape, storage, nc, b)
        again = ops.raw_dng(x, fmt_of(storage, w), dng)                                      # two runs give identical bytes
        assert torch.equal(again.lengths, out.lengths) and again.files() == files
    img, ifd, _ = R.rd_file(files[2])                                                        # the independent reader: the noise frame comes back
    assert np.array_equal(img, frames[2]) and ifd[256][2] == (w,) and ifd[257][2] == (h,)


@pytest.mark.gpu
def test_planted_extreme_differences_u16(hip):
    """Differences of exactly +-32768 (SSSS 16, no extra bits), 32767 and -32767 (SSSS 15), in both component arrangements."""
    rng = np.random.default_rng(5)
    f = rng.integers(0, 65536, (16, 32))
    f[3, 4:14] = (0, 0, 32768, 32768, 1, 1, 32768, 32768, 0, 0)          # step 1 and step 2: +32768, -32767, +32767, -32768
    for nc in (1, 2):
        d = (f[3, nc:] - f[3, :-nc]) & 0xffff
        d = np.where(d >= 32768, d - 65536, d)
        assert {-32768, 32767, -32767} <= set(d.tolist())
        want, _ = R.encode(f, "u16", 32, 16, nc, white=65535)
        out = ops.raw_dng(lines(f[None], "u16").to(DEV), fmt_of("u16", 32), M.Dng(tile=(32, 16), components=nc))
        assert out.files() == [want]
        assert np.array_equal(R.rd_file(want)[0], f)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
def test_padded_pitch_and_a_base_off_the_vector_boundary(hip, storage):
    """64 x 32 through the C ABI: lines 12 bytes longer than their samples (0xFF filler) and the first frame 4 bytes past a 16-byte
    boundary, so no lane may use its vector load; and the same lines dense and aligned, which may."""
    rng = np.random.default_rng(17)
    frames = rng.integers(0, FULL[storage] + 1, (2, 32, 64))
    body = np.stack([R.pack_lines(f, storage).view(np.uint8).reshape(32, -1) for f in frames])
    dng = M.Dng(tile=(32, 16))
    want = [R.encode(f, storage, 32, 16, 2, white=FULL[storage])[0] for f in frames]
    cap = dng.plan(32, 64, fmt_of(storage, 64)).capacity
    for pitch, shift in ((body.shape[2] + 12, 4), (None, 0)):
        dst, lengths = abi_encode(hip, body, storage, 64, dng, cap, pitch=pitch, shift=shift)
        assert lengths == [len(f) for f in want]
        for b, f in enumerate(want):
            assert dst[GUARD + b * cap:GUARD + b * cap + len(f)].tobytes() == f, (storage, pitch, b)
        assert (dst[:GUARD] == 0xA5).all() and (dst[-GUARD:] == 0xA5).all()


# ---- 2. capacity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacity_one_byte_short(hip):
    """Frame 0 of 2 needs one byte more than the capacity: lengths[0] is still what it needs, frame 1 is intact, tobytes(0) names the capacity
    that would do -- and, through the C ABI with guard bytes around the frames, nothing outside a frame's capacity bytes is written."""
    frames = frames_of("edges", "u16")[[2, 0]]                                               # noise, then flat
    want = [R.encode(f, "u16", 16, 16, 2, white=65535)[0] for f in frames]
    cap = len(want[0]) - 1
    assert len(want[1]) < cap
    dng = M.Dng(tile=(16, 16), capacity=cap)
    out = ops.raw_dng(lines(frames, "u16").to(DEV), fmt_of("u16", 38), dng)
    assert out.buffer.shape == (2, cap) and out.lengths.cpu().tolist() == [len(f) for f in want]
    assert out.tobytes(1) == want[1]
    assert out.buffer[0].cpu().numpy().tobytes() == want[0][:cap]                            # clipped, not moved
    with pytest.raises(ValueError, match=f"capacity={len(want[0])}"):
        out.tobytes(0)
    with pytest.raises(ValueError, match=f"capacity={len(want[0])}"):
        out.files()
    body = lines(frames, "u16").numpy().view(np.uint8).reshape(2, 18, -1)
    for nframes, capacity in ((2, cap), (1, cap), (2, 1), (2, 101), (2, len(want[1]) - 1)):  # behind the buffer; behind frame 0 alone; both too large
        dst, lengths = abi_encode(hip, body[:nframes], "u16", 38, dng, capacity)
        assert lengths == [len(f) for f in want[:nframes]]
        assert (dst[:GUARD] == 0xA5).all() and (dst[GUARD + nframes * capacity:] == 0xA5).all(), (nframes, capacity)
        for b in range(nframes):
            n = min(capacity, len(want[b]))
            assert dst[GUARD + b * capacity:GUARD + b * capacity + n].tobytes() == want[b][:n], (nframes, capacity, b)


# ---- 3. graphs and forward_mosaic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_codes_the_new_input(hip):
    fmt, dng = fmt_of("mipi12", 38), M.Dng(tile=(16, 16))
    frames = frames_of("edges", "mipi12")
    a, b = lines(frames[[2, 1]], "mipi12").to(DEV), lines(frames[[1, 2]], "mipi12").to(DEV)
    want = [f for f, _ in want_of("edges", "mipi12", 2)]
    call = M.GraphedCall(lambda x: ops.raw_dng(x, fmt, dng))
    first = call(a).files()
    second = call(b)                                                                         # the source the graph reads is overwritten
    assert isinstance(second, M.DngFrames) and first == [want[2], want[1]] and second.files() == [want[1], want[2]]


@pytest.mark.gpu
def test_forward_mosaic_writes_the_frame_as_delivered(hip):
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=torch.bfloat16).eval()
    rng = np.random.default_rng(62)
    c = (300 + (2 * (np.arange(32)[:, None] + np.arange(64)[None, :])) % 400 + rng.integers(0, 6, (2, 32, 64))).astype(np.int64)
    c[:, 5::9, 6::17] = 1020                                                                 # hot samples the repair replaces: the file keeps them
    x = lines(c, "mipi10").unsqueeze(1).to(DEV)
    coord = O.make_coord(2, 16, 32).to(DEV, torch.bfloat16)
    blacks = (64.0, 66.0, 62.0, 64.0)
    base = dict(storage="mipi10", cfa="GBRG", width=64, black_level=blacks, white_level=1023.0, defects=M.Defects(hot=(48.0, 0.125)),
                calibration=M.Calibration(gains=(1.0, 1.6, 1.9, 1.0), clip=(0.0, 1.0)))             # G B R G
    dng = M.Dng(tile=(32, 16), make="acme", datetime="2024:05:06 07:08:09")
    tags = dict(cfa="GBRG", blacks=blacks, white=1023, make="acme", datetime="2024:05:06 07:08:09",
                neutral=(1.0 / float(np.float32(1.9)), 1.0, 1.0 / float(np.float32(1.6))))
    with torch.no_grad():
        got = net.forward_mosaic(x, None, coord, raw_format=M.RawFormat(dng=dng, **base))
        stills = net.raw_dng
        plain = net.forward_mosaic(x, None, coord, raw_format=M.RawFormat(**base))
        alone = ops.raw_dng(x, M.RawFormat(**base), dng)
    assert torch.equal(got, plain) and got.shape == (2, 3, 32, 64)                           # the still changes nothing
    assert isinstance(stills, M.DngFrames) and torch.equal(stills.lengths, alone.lengths) and stills.files() == alone.files()
    assert stills.files() == [R.encode(f, "mipi10", 32, 16, 2, **tags)[0] for f in c]
    assert np.array_equal(R.rd_file(stills.tobytes(1))[0], c[1])
    # a Quad-Bayer sensor: the file carries the 4x4 pattern, and the 2-component prediction is still lossless
    qbase = dict(storage="mipi10", cfa="GBRG", width=64, black_level=64.0, white_level=1023.0, quad=M.QuadBayer())
    with torch.no_grad():
        got = net.forward_mosaic(x, None, coord, raw_format=M.RawFormat(dng=dng, **qbase))
        stills = net.raw_dng
        plain = net.forward_mosaic(x, None, coord, raw_format=M.RawFormat(**qbase))
    assert torch.equal(got, plain)
    qtags = dict(tags, quad=True, blacks=(64.0,) * 4, neutral=(1.0, 1.0, 1.0))
    assert stills.files() == [R.encode(f, "mipi10", 32, 16, 2, **qtags)[0] for f in c]
    img, ifd, _ = R.rd_file(stills.tobytes(0))
    assert np.array_equal(img, c[0]) and ifd[33421][2] == (4, 4) and ifd[33422][2] == tuple(R.cfa_pattern("GBRG", True))
    # exposures: refused, and the message names the op on the (B E, ...) view
    ex = M.RawFormat(storage="u16", white_level=1023.0, exposures=M.Exposures(times=(1.0, 4.0), knee=(800.0, 1000.0)), dng=dng)
    with pytest.raises(ValueError, match=r"ops\.raw_dng on the \(B E, 2h, X\) view"):
        net.forward_mosaic(torch.from_numpy(np.zeros((2, 2, 32, 64), np.uint16)).to(DEV), None, coord, raw_format=ex)


@pytest.mark.gpu
def test_refusals(hip):
    x = torch.zeros(1, 16, 32, device=DEV)
    with pytest.raises(ValueError, match="a DNG holds sensor codes"):
        ops.raw_dng(x, M.RawFormat(), M.Dng())
    with pytest.raises(ValueError, match="even"):
        ops.raw_dng(torch.from_numpy(np.zeros((1, 16, 31), np.uint16)).to(DEV), M.RawFormat(storage="u16", white_level=1023.0), M.Dng())
    with pytest.raises(TypeError, match="dng must be a Dng"):
        ops.raw_dng(torch.from_numpy(np.zeros((1, 16, 32), np.uint16)).to(DEV), M.RawFormat(storage="u16", white_level=1023.0))


@pytest.mark.gpu
def test_a_graph_keeps_its_header_whatever_other_stills_are_written(hip):
    """The header a captured graph reads lives on its Dng: 80 other stills, each stamped with its own datetime= (a new header each), neither
    free it nor accumulate anywhere, and the replay still writes the restatement's file."""
    import gc
    import weakref
    fmt, dng = fmt_of("mipi12", 38), M.Dng(tile=(16, 16))
    frames = frames_of("edges", "mipi12")
    a, b = lines(frames[[2, 1]], "mipi12").to(DEV), lines(frames[[1, 2]], "mipi12").to(DEV)
    want = [f for f, _ in want_of("edges", "mipi12", 2)]
    call = M.GraphedCall(lambda x: ops.raw_dng(x, fmt, dng))
    assert call(a).files() == [want[2], want[1]]
    kept = ops.dng_header(dng, 18, 38, fmt, DEV)
    assert ops.dng_header(dng, 18, 38, fmt, DEV) is kept and not hasattr(ops, "_DNG_HEADERS")     # on the Dng, not in a module-level table
    other, x8 = fmt_of("u8", 32), lines(frames_of("one_tile", "u8")[:1], "u8").to(DEV)
    seen = []
    for k in range(80):
        stamped = M.Dng(tile=(32, 16), datetime=f"2024:05:06 07:{k // 60:02d}:{k % 60:02d}")
        ops.raw_dng(x8, other, stamped)
        seen.append(weakref.ref(ops.dng_header(stamped, 16, 32, other, DEV)))
        del stamped
    gc.collect()
    assert not any(r() is not None for r in seen)                                            # a header goes with its Dng
    junk = [torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV) for n in (kept.numel(),) * 64]      # would land in a freed header's block
    assert call(b).files() == [want[1], want[2]] and call(a).files() == [want[2], want[1]]
    assert ops.dng_header(dng, 18, 38, fmt, DEV) is kept and len(junk) == 64
