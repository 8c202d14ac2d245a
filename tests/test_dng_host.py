"""CPU: raw stills.  The restatement (tests/dng_ref.py) against its own independent reader and against Pillow; Dng's header against the
restatement's and against Pillow's TIFF parser, tag by tag; rc_dng_tile_header / rc_dng_plan (host functions of the library); validation."""
import ctypes as C
import io
import struct
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image, TiffImagePlugin

import realcamnet_amd as M
from realcamnet_amd import _lib, ops, torch_ops
from realcamnet_amd.dng import STORAGE_CODE, XYZ_TO_SRGB
import dng_ref as R

FULL = {"u16": 65535, "u8": 255, "mipi10": 1023, "mipi12": 4095}
STORAGES = ("u16", "u8", "mipi10", "mipi12")
# (width, height), tile: one tile; 3 x 2 tiles padded on both edges, width 2 mod 4; two wave steps per line and a padded tile
SIZES = (((32, 16), (32, 16)), ((38, 18), (16, 16)), ((528, 20), (272, 16)))


def fmt_of(storage, w=None, **kw):
    kw.setdefault("white_level", float(FULL[storage]))
    return M.RawFormat(storage=storage, width=w if storage.startswith("mipi") else None, **kw)


def noise(storage, w, h, seed):
    return np.random.default_rng(seed).integers(0, FULL[storage] + 1, (h, w))


# ---- 1. the restatement against readers that share nothing with it ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", (1, 2))
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
def test_reader_inverts_the_restatement(size, storage, nc):
    (w, h), (tw, th) = size
    f = noise(storage, w, h, w + nc)
    data, streams = R.encode(f, storage, tw, th, nc, white=FULL[storage])
    img, ifd, tiles = R.rd_file(data)
    assert np.array_equal(img, f)
    assert len(tiles) == -(-w // tw) * -(-h // th) == len(streams)
    for t, (samples, p, comps, _, _) in enumerate(tiles):
        assert p == R.PRECISION[storage] and comps == nc
        assert np.array_equal(samples, R.tile_samples(f, t // -(-w // tw), t % -(-w // tw), tw, th))      # the padding too
    # layout: even offsets, zero pad bytes, the length counts the last pad byte
    end = 0
    for off, cnt, s in zip(ifd[324][2], ifd[325][2], streams):
        assert off % 2 == 0 and data[off:off + cnt] == s and (cnt % 2 == 0 or data[off + cnt] == 0)
        end = off + cnt + (cnt & 1)
    assert end == len(data)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
def test_pillow_decodes_the_8_bit_one_component_tiles(size):
    """libjpeg-turbo opens a lossless (SOF3) stream of 8 bits and one component with this very table; it refuses 2 components and more than
    8 bits, so those rest on dng_ref's reader."""
    (w, h), (tw, th) = size
    f = noise("u8", w, h, 3)
    _, streams = R.encode(f, "u8", tw, th, 1, white=255)
    for t, s in enumerate(streams):
        im = Image.open(io.BytesIO(s))
        im.load()
        assert im.mode == "L" and im.size == (tw, th)
        assert np.array_equal(np.asarray(im), R.tile_samples(f, t // -(-w // tw), t % -(-w // tw), tw, th))


def test_flat_ramp_and_extreme_differences_round_trip():
    flat = np.full((16, 32), 512)
    assert len(R.tile_stream(flat, "mipi10", 2)) == 68 + 32 * 16 * 4 // 8 + 2                  # SSSS 0 is a 4-bit code
    f = np.random.default_rng(5).integers(0, 65536, (16, 32))
    f[3, 4:14] = (0, 0, 32768, 32768, 1, 1, 32768, 32768, 0, 0)
    for nc in (1, 2):
        words, lengths = R.entropy_bits(f, 16, nc)
        assert 13 in lengths and 12 + 15 in lengths and lengths.max() == 27                   # SSSS 16 has no extra bits; SSSS 15 is the longest
        assert np.array_equal(R.rd_file(R.encode(f, "u16", 32, 16, nc, white=65535)[0])[0], f)
    assert len(R.huff_table()) == 17 and max(n for _, n in R.huff_table().values()) == 13


# ---- 2. the header ----------------------------------------------------------------------------------------------------------------------------------
def pillow_ifd(data):
    ifd = TiffImagePlugin.ImageFileDirectory_v2(data[:8])
    fp = io.BytesIO(data)
    fp.seek(8)
    ifd.load(fp)
    return ifd


def test_every_tag_has_its_type_count_and_value():
    curve = M.Pwl((0.0, 512.0, 1023.0), (0.0, 512.0, 4600.0))
    fmt = fmt_of("mipi10", 76, cfa="GRBG", black_level=(64.0, 64.5, 63.25, 64.0), white_level=4600.0,
                 calibration=M.Calibration(curve=curve, gains=(1.0, 2.0, 1.5, 1.0)))
    dng = M.Dng(tile=(32, 16), make="acme", model="cam 1", noise_profile=((2e-4, 3e-6),), datetime="2024:05:06 07:08:09", software="sw 2")
    data = dng.header(36, 76, fmt)
    plan = dng.plan(36, 76, fmt)
    assert data[:4] == b"II*\0" and struct.unpack("<I", data[4:8]) == (8,) and len(data) % 2 == 0
    assert plan == M.dng.DngPlan(len(data), 68, 3, 3, len(data) + 9 * (68 + 2 + 4 * 32 * 16), 36, plan.offsets_at, plan.counts_at)
    mine = R.rd_ifd(data)                                                                    # the generic parser written from TIFF 6.0
    pil = pillow_ifd(data)
    table = tuple(int(v) for v in np.clip(np.rint(np.interp(np.arange(1024), curve.x, curve.y)), 0, 65535))
    q = lambda v: Fraction(int(np.rint(v * 2 ** 20)), 2 ** 20)
    want = {
        254: (4, 1, (0,)), 256: (4, 1, (76,)), 257: (4, 1, (36,)), 258: (3, 1, (16,)), 259: (3, 1, (7,)), 262: (3, 1, (32803,)),
        271: (2, 5, "acme\0"), 272: (2, 6, "cam 1\0"), 274: (3, 1, (1,)), 277: (3, 1, (1,)), 284: (3, 1, (1,)), 305: (2, 5, "sw 2\0"),
        306: (2, 20, "2024:05:06 07:08:09\0"), 322: (4, 1, (32,)), 323: (4, 1, (16,)), 324: (4, 9, (0,) * 9), 325: (4, 9, (0,) * 9),
        33421: (3, 2, (2, 2)), 33422: (1, 4, (1, 0, 2, 1)), 50706: (1, 4, (1, 4, 0, 0)), 50707: (1, 4, (1, 1, 0, 0)), 50708: (2, 11, "acme cam 1\0"),
        50710: (1, 3, (0, 1, 2)), 50711: (3, 1, (1,)), 50712: (3, 1024, table), 50713: (3, 2, (2, 2)),
        50714: (5, 4, (Fraction(64), Fraction(129, 2), Fraction(253, 4), Fraction(64))), 50717: (4, 1, (4600,)),
        50721: (10, 9, tuple(q(m) for m in XYZ_TO_SRGB)), 50728: (5, 3, (q(1.0 / 2.0), Fraction(1), q(1.0 / 1.5))), 50778: (3, 1, (21,)),
        51041: (12, 2, (2e-4, 3e-6)),
    }
    assert list(mine) == sorted(want)                                                        # exactly these tags, ascending
    for tag, (typ, count, value) in want.items():
        assert mine[tag] == (typ, count, value), tag
        assert pil.tagtype[tag] == typ, tag
        got = pil[tag]
        if typ == 2:
            assert got == value[:-1], tag
        else:
            got = got if isinstance(got, tuple) else (got,)
            if typ == 1:
                got = tuple(got[0]) if isinstance(got[0], bytes) else got
            assert len(got) == count and all(Fraction(g) == Fraction(v) for g, v in zip(got, value)), tag
    # BlackLevel: an integer may have the denominator 1
    at = plan.header_bytes - 0                                                               # (only that the rationals parse; their words:)
    assert struct.pack("<II", 64, 1) in data and struct.pack("<II", 129, 2) in data and at == len(data)
    # the two arrays stand where the plan says
    assert data[plan.offsets_at:plan.offsets_at + 36] == bytes(36) and data[plan.counts_at:plan.counts_at + 36] == bytes(36)
    # out-of-line values on even offsets
    n = struct.unpack_from("<H", data, 8)[0]
    for i in range(n):
        tag, typ, count, off = struct.unpack_from("<HHII", data, 10 + 12 * i)
        if count * R.RD_TYPES[typ][1] > 4:
            assert off % 2 == 0 and off >= 10 + 12 * n + 4, tag


def test_header_equals_the_restatement():
    for storage, (w, h), tile, kw, tags in (
            ("u16", (38, 18), (16, 16), dict(), dict()),
            ("u8", (32, 16), (32, 16), dict(cfa="BGGR", black_level=3.0), dict(cfa="BGGR", blacks=(3.0,) * 4)),            # one tile: the arrays are inline
            ("mipi12", (64, 32), (32, 16), dict(cfa="GBRG", quad=M.QuadBayer(), black_level=256.0), dict(cfa="GBRG", quad=True, blacks=(256.0,) * 4)),
    ):
        fmt = fmt_of(storage, w, **kw)
        for dkw, rkw in ((dict(), dict()), (dict(make="a", model="b", unique_model="c d", software="s", color_matrix=(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                                 as_shot_neutral=(0.5, 1.0, 0.75), noise_profile=(1e-4, 1e-6, 2e-4, 2e-6, 3e-4, 3e-6)),
                                            dict(make="a", model="b", unique_model="c d", software="s", color_matrix=(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                                 neutral=(0.5, 1.0, 0.75), noise_profile=(1e-4, 1e-6, 2e-4, 2e-6, 3e-4, 3e-6)))):
            dng = M.Dng(tile=tile, **dkw)
            want, offsets_at, counts_at = R.header(h, w, storage, *tile, white=FULL[storage], **tags, **rkw)
            plan = dng.plan(h, w, fmt)
            assert dng.header(h, w, fmt) == want and (plan.header_bytes, plan.offsets_at, plan.counts_at) == (len(want), offsets_at, counts_at)
    one = M.Dng(tile=(32, 16)).plan(16, 32, fmt_of("u8"))
    assert one.offsets_at < 8 + 2 + 12 * 40 and one.offsets_at % 12 == (8 + 2 + 8) % 12      # inside the IFD entry


def test_tile_header_and_plan_of_the_library():
    hip = _lib.load()
    for storage in STORAGES:
        for nc in (1, 2):
            dng = M.Dng(tile=(272, 16), components=nc)
            got = dng.tile_header(fmt_of(storage, 528))
            assert got == R.tile_header(storage, 272, 16, nc) and len(got) == 58 + 5 * nc
            fmt = fmt_of(storage, 528)
            plan = dng.plan(20, 528, fmt)
            p, d, f = _lib.DngPlanInfo(), dng.desc(), _lib.RawFormatDesc(storage=STORAGE_CODE[storage])
            _lib.check(hip.rc_dng_plan(C.byref(d), C.byref(f), 20, 528, plan.header_bytes, plan.offsets_at, plan.counts_at, C.byref(p)), "rc_dng_plan")
            assert (p.tile_header_bytes, p.tiles_x, p.tiles_y, p.capacity, p.scratch_bytes) == (plan.tile_header_bytes, 2, 2, plan.capacity, plan.scratch_bytes)
    d, f, p = M.Dng().desc(), _lib.RawFormatDesc(storage=_lib.RC_RAW_U16), _lib.DngPlanInfo()
    for args, why in (((20, 528, 501, 100, 200), "header_bytes must be even"), ((20, 527, 500, 100, 200), "even and at least 2"),
                      ((20, 528, 500, 101, 200), "offsets_at and counts_at must be even"), ((20, 528, 500, 100, 102), "overlap"),
                      ((20, 528, 500, 100, 494), "inside the header")):
        assert hip.rc_dng_plan(C.byref(d), C.byref(f), *args, C.byref(p)) != 0 and why in hip.rc_last_error().decode(), why
    f.storage = _lib.RC_RAW_F32
    assert hip.rc_dng_plan(C.byref(d), C.byref(f), 20, 528, 500, 100, 200, C.byref(p)) != 0 and "a DNG holds sensor codes" in hip.rc_last_error().decode()
    d.tile_w = 24
    f.storage = _lib.RC_RAW_U16
    assert hip.rc_dng_plan(C.byref(d), C.byref(f), 20, 528, 500, 100, 200, C.byref(p)) != 0 and "multiples of 16" in hip.rc_last_error().decode()


# ---- 3. the rules of the tags -----------------------------------------------------------------------------------------------------------------------
def test_linearization_table_rules():
    curve = M.Pwl((0.0, 128.0, 255.0), (0.0, 128.0, 4095.0))
    fmt = fmt_of("u8", white_level=4095.0, calibration=M.Calibration(curve=curve))
    table = M.Dng.linearization(fmt)
    s = curve.slopes()
    want = [curve.y[0] + c * s[0] if c < 128 else curve.y[1] + (c - 128.0) * s[1] for c in range(256)]
    assert len(table) == 256 and list(table) == [int(np.clip(np.rint(v), 0, 65535)) for v in want] and table[0] == 0 and table[255] == 4095
    assert M.Dng.linearization(fmt_of("u8")) is None and 50712 not in R.rd_ifd(M.Dng().header(16, 32, fmt_of("u8")))
    below = fmt_of("u8", white_level=300.0, calibration=M.Calibration(curve=M.Pwl((10.0, 255.0), (0.0, 300.0))))
    assert M.Dng.linearization(below)[:10] == (0,) * 10                                      # the extrapolated start is clamped at 0
    high = fmt_of("u8", white_level=60000.0, calibration=M.Calibration(curve=M.Pwl((0.0, 255.0), (0.0, 65536.0))))
    with pytest.raises(ValueError, match="LinearizationTable entry is a SHORT"):
        M.Dng().header(16, 32, high)


def test_as_shot_neutral_rules():
    import torch
    n = lambda dng, fmt: R.rd_ifd(dng.header(16, 32, fmt))[50728][2]
    q = lambda v: Fraction(int(np.rint(v * 2 ** 20)), 2 ** 20)
    assert n(M.Dng(), fmt_of("u16")) == (1, 1, 1)
    host = fmt_of("u16", cfa="RGGB", calibration=M.Calibration(gains=(2.0, 1.0, 1.5, 1.25)))
    assert n(M.Dng(), host) == (q(1.25 / 2.0), 1, q(1.25 / 1.25))
    assert n(M.Dng(as_shot_neutral=(0.4, 1.0, 0.7)), host) == (q(0.4), 1, q(0.7))            # given: it wins
    device = fmt_of("u16", calibration=M.Calibration(gains=torch.ones(1, 4)))                # a tensor is never read
    assert n(M.Dng(), device) == (1, 1, 1)
    with pytest.raises(ValueError, match="give as_shot_neutral"):
        M.Dng().header(16, 32, fmt_of("u16", calibration=M.Calibration(gains=(0.0, 1.0, 1.0, 1.0))))


def test_noise_profile_rules():
    assert 51041 not in R.rd_ifd(M.Dng().header(16, 32, fmt_of("u16")))
    assert R.rd_ifd(M.Dng(noise_profile=(1e-4, 2e-6)).header(16, 32, fmt_of("u16")))[51041] == (12, 2, (1e-4, 2e-6))
    three = ((1e-4, 1e-6), (2e-4, 2e-6), (3e-4, 3e-6))
    assert R.rd_ifd(M.Dng(noise_profile=three).header(16, 32, fmt_of("u16")))[51041] == (12, 6, (1e-4, 1e-6, 2e-4, 2e-6, 3e-4, 3e-6))
    for bad in ((1.0,), (1.0, 2.0, 3.0, 4.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="Dng.noise_profile must hold 2 or 6 finite numbers"):
            M.Dng(noise_profile=bad)


# ---- 4. validation ----------------------------------------------------------------------------------------------------------------------------------
def test_dng_validation_messages():
    for kw, err, why in ((dict(tile=(24, 16)), ValueError, "Dng.tile width must be a multiple of 16"), (dict(tile=(16, 0)), ValueError, "Dng.tile height must be 16 .. 65520"),
                         (dict(tile=(65536, 16)), ValueError, "Dng.tile width must be 16 .. 65520"), (dict(tile=16), TypeError, r"Dng.tile must be \(tw, th\)"),
                         (dict(tile=(16.0, 16)), TypeError, "Dng.tile width must be an int"), (dict(components=3), ValueError, "Dng.components must be 1 .. 2"),
                         (dict(capacity=0), ValueError, "Dng.capacity must be 1"), (dict(make=7), TypeError, "Dng.make must be a str"),
                         (dict(model="café"), ValueError, "Dng.model must be ASCII"), (dict(datetime="2024-05-06"), ValueError, "YYYY:MM:DD HH:MM:SS"),
                         (dict(color_matrix=(1.0,) * 8), ValueError, "Dng.color_matrix must hold 9"), (dict(as_shot_neutral=(1.0, 0.0, 1.0)), ValueError, "must be positive")):
        with pytest.raises(err, match=why):
            M.Dng(**kw)
    d = M.Dng()
    assert d.tile == (256, 64) and d.components == 2 and hash(d) == hash(M.Dng()) and d == M.Dng()
    with pytest.raises(Exception):
        d.components = 1                                                                     # frozen
    with pytest.raises(ValueError, match="a DNG holds sensor codes"):
        d.plan(16, 32, M.RawFormat())
    with pytest.raises(ValueError, match="must be even"):
        d.plan(16, 31, fmt_of("u16"))
    with pytest.raises(TypeError, match="raw_format must be a RawFormat"):
        d.plan(16, 32, None)
    with pytest.raises(ValueError, match="a file stays below 2\\^31"):
        d.plan(1 << 15, 1 << 15, fmt_of("u16"))
    with pytest.raises(ValueError, match="black levels must be finite and >= 0"):
        d.header(16, 32, fmt_of("u16", black_level=-1.0))
    with pytest.raises(ValueError, match="WhiteLevel must round to 1 .. 65535"):
        d.header(16, 32, fmt_of("u16", white_level=70000.0))
    with pytest.raises(ValueError, match="one black level for all positions"):
        d.header(16, 32, fmt_of("u16", quad=M.QuadBayer(), black_level=(1.0, 2.0, 1.0, 1.0)))
    assert d.plan(16, 32, fmt_of("u16")).capacity == d.plan(16, 32, fmt_of("u16")).header_bytes + 68 + 2 + 4 * 256 * 64
    assert M.Dng(capacity=1000).plan(16, 32, fmt_of("u16")).capacity == 1000


def test_raw_format_field_and_refusals():
    assert M.RawFormat().dng is None
    fmt = fmt_of("u16", dng=M.Dng())
    assert fmt.validate((2, 32, 64)) == (32, 64)
    with pytest.raises(TypeError, match="RawFormat.dng must be None or a Dng"):
        fmt_of("u16", dng=M.Jpeg()).validate((2, 32, 64))
    with pytest.raises(ValueError, match="a DNG holds sensor codes"):
        M.RawFormat(dng=M.Dng()).validate((2, 32, 64))
    with pytest.raises(ValueError, match=r"ops\.raw_dng on the \(B E, 2h, X\) view"):
        fmt_of("u16", dng=M.Dng(), exposures=M.Exposures(times=(1.0, 4.0), knee=(800.0, 1000.0))).validate((2, 2, 32, 64))
    import torch
    x = torch.zeros(1, 16, 32)
    with pytest.raises(ValueError, match="a DNG holds sensor codes"):
        ops.raw_dng(x, M.RawFormat(), M.Dng())
    with pytest.raises(ValueError, match=r"ops\.raw_dng on the \(B E, 2h, X\) view"):
        ops.raw_dng(x, fmt_of("u16", exposures=M.Exposures(times=(1.0, 4.0), knee=(800.0, 1000.0))), M.Dng())
    with pytest.raises(TypeError, match="dng must be a Dng"):
        ops.raw_dng(x, fmt_of("u16"))
    with pytest.raises(ValueError, match="even"):
        ops.raw_dng(torch.from_numpy(np.zeros((1, 16, 31), np.uint16)), fmt_of("u16"), M.Dng())


def test_frames_report_what_would_fit():
    import torch
    frames = M.DngFrames(torch.zeros(2, 10, dtype=torch.uint8), torch.tensor([8, 12]), M.Dng(), (16, 32))
    assert frames.tobytes(0) == bytes(8)
    with pytest.raises(ValueError, match="frame 1 needs 12 bytes, the buffer holds 10 per frame: encode it with Dng\\(capacity=12\\)"):
        frames.tobytes(1)
    with pytest.raises(ValueError, match="capacity=12"):
        frames.files()


# ---- 5. declared, bound, exported -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    hip = _lib.load()
    names = ("rc_dng_desc_size", "rc_dng_plan", "rc_dng_tile_header", "rc_dng_encode", "rc_debug_dng_passes")
    declared = _lib.declared_symbols()
    for name in names:
        assert name in declared and name in _lib._SIGS and hasattr(hip, name)
    assert hip.rc_abi_version() == 15 == _lib.ABI_VERSION
    assert hip.rc_dng_desc_size() == C.sizeof(_lib.DngDesc) == 32
    assert "Dng" in M.__all__ and "DngFrames" in M.__all__ and M.Dng is M.dng.Dng
    assert "raw_dng" in torch_ops.SCHEMAS
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():                                                                   # the fake implementation: shapes only, no library call
        src = torch.empty(2, 32, 64, dtype=torch.uint16, device="cuda")
        buf, lengths = torch.ops.realcam.raw_dng(src, torch.empty(500, dtype=torch.uint8, device="cuda"), _lib.RC_RAW_U16, 0, 64, 32, 16, 2, 100, 200, 4096)
        assert buf.shape == (2, 4096) and buf.dtype == torch.uint8 and lengths.shape == (2,) and lengths.dtype == torch.int64
        for bad_src, width, cap in ((torch.empty(32, 64, dtype=torch.uint16, device="cuda"), 64, 4096), (src, 63, 4096), (src, 64, 0)):
            with pytest.raises(ValueError, match="realcam::raw_dng"):
                torch.ops.realcam.raw_dng(bad_src, torch.empty(500, dtype=torch.uint8, device="cuda"), _lib.RC_RAW_U16, 0, width, 32, 16, 2, 100, 200, cap)
    for passes in (0, 7):
        assert hip.rc_debug_dng_passes(passes) == 0
