"""CPU: sensor RAW formats for forward_mosaic (include/realcam_hip.h rc_raw_format / rc_raw_ingest_fmt / rc_rgb_encode).
The ctypes mirror, the argument checks made before any launch, RawFormat.validate, the MIPI CSI-2 packing reference the GPU tests
use, the kernels' resources and fake-tensor traces of formatted forwards."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F32


# ---- MIPI CSI-2 RAW10 / RAW12 reference packer / unpacker (numpy): the GPU tests build their frames with it --------------------
def mipi_pack(counts: np.ndarray, bits: int, line_bytes: int = 0, pad_value: int = 0xA5) -> np.ndarray:
    """(..., rows, width) integer counts -> (..., rows, line_bytes) uint8 MIPI lines; the bytes past a line's samples are pad_value."""
    c = np.asarray(counts).astype(np.uint16)
    lead, width = c.shape[:-1], c.shape[-1]
    if bits == 10:
        assert width % 4 == 0
        g = c.reshape(lead + (width // 4, 4))
        body = np.concatenate([(g >> 2).astype(np.uint8), ((g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4
                                                           | (g[..., 3] & 3) << 6).astype(np.uint8)[..., None]], axis=-1)
    elif bits == 12:
        assert width % 2 == 0
        g = c.reshape(lead + (width // 2, 2))
        body = np.concatenate([(g >> 4).astype(np.uint8), ((g[..., 0] & 15) | (g[..., 1] & 15) << 4).astype(np.uint8)[..., None]], axis=-1)
    else:
        raise ValueError(bits)
    body = body.reshape(lead + (-1,))
    need = body.shape[-1]
    line_bytes = line_bytes or need
    assert line_bytes >= need
    out = np.full(lead + (line_bytes,), pad_value, np.uint8)
    out[..., :need] = body
    return out


def mipi_unpack(lines: np.ndarray, bits: int, width: int) -> np.ndarray:
    """The inverse of mipi_pack: (..., rows, line_bytes) uint8 -> (..., rows, width) uint16 counts."""
    b = np.asarray(lines).astype(np.uint16)
    if bits == 10:
        g = b[..., : width // 4 * 5].reshape(b.shape[:-1] + (width // 4, 5))
        px = [(g[..., k] << 2) | ((g[..., 4] >> (2 * k)) & 3) for k in range(4)]
    else:
        g = b[..., : width // 2 * 3].reshape(b.shape[:-1] + (width // 2, 3))
        px = [(g[..., 0] << 4) | (g[..., 2] & 15), (g[..., 1] << 4) | (g[..., 2] >> 4)]
    return np.stack(px, axis=-1).reshape(b.shape[:-1] + (width,)).astype(np.uint16)


@pytest.mark.parametrize("bits,width,line_bytes", [(10, 24, 0), (10, 40, 64), (10, 16, 23), (12, 6, 0), (12, 22, 64), (12, 10, 17)])
def test_mipi_reference_round_trips(bits, width, line_bytes):
    rng = np.random.default_rng(bits * 100 + width)
    counts = rng.integers(0, 1 << bits, size=(2, 6, width), dtype=np.uint16)
    lines = mipi_pack(counts, bits, line_bytes)
    assert lines.shape == (2, 6, line_bytes or width * bits // 8) and lines.dtype == np.uint8
    assert np.array_equal(mipi_unpack(lines, bits, width), counts)


def test_mipi_reference_byte_layout():
    """RAW10: bytes 0-3 = bits [9:2] of pixels 0-3, byte 4 bits 2k+1..2k = bits [1:0] of pixel k.  RAW12: byte 0 = p0[11:4], byte 1 =
    p1[11:4], byte 2 = p1[3:0] << 4 | p0[3:0]."""
    p = np.array([[0x3FF, 0x001, 0x2AA, 0x155]], np.uint16)
    assert mipi_pack(p, 10).tolist() == [[0xFF, 0x00, 0xAA, 0x55, 0b01_10_01_11]]
    q = np.array([[0xABC, 0x123]], np.uint16)
    assert mipi_pack(q, 12).tolist() == [[0xAB, 0x12, 0x3C]]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_raw_format_struct_matches_header_and_symbols_exported():
    lib = _lib.load()
    assert lib.rc_raw_format_size() == C.sizeof(_lib.RawFormatDesc)
    for name in ("rc_raw_format_size", "rc_raw_ingest_fmt", "rc_rgb_encode"):
        assert name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15


def _fmt(storage=_lib.RC_RAW_U16, cfa=_lib.RC_CFA_RGGB, line_bytes=0, width=0, black=(64.0,) * 4, white=1023.0):
    d = _lib.RawFormatDesc(storage=storage, cfa=cfa, line_bytes=line_bytes, width=width, white=white)
    for k in range(4):
        d.black[k] = black[k]
    return d


FAKE = 1 << 20           # a non-null, 16-byte aligned address that is never dereferenced: every case below fails before a launch


def _ingest(fmt, src=FAKE, packed=FAKE, cond=FAKE, out_dtype=RC_F32, b=1, h=8, w=8, hp=16, wp=16, ch=4, cw=4):
    return _lib.load().rc_raw_ingest_fmt(src, None if fmt is None else C.byref(fmt), packed, cond, out_dtype, b, h, w, hp, wp, ch, cw, None)


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"),
    ("null format", dict(fmt=None), b"null"),
    ("null packed", dict(packed=None), b"null"),
    ("null cond", dict(cond=None), b"null"),
    ("bad shape", dict(hp=4), b"bad shape"),
    ("bad out dtype", dict(out_dtype=_lib.RC_U16), b"dtype"),
    ("unknown storage", dict(fmt=_fmt(storage=7)), b"storage"),
    ("unknown cfa", dict(fmt=_fmt(cfa=4)), b"cfa"),
    ("black >= white", dict(fmt=_fmt(black=(64.0, 64.0, 1023.0, 64.0))), b"white"),
    ("short line (u16)", dict(fmt=_fmt(line_bytes=30)), b"line_bytes"),
    ("short line (RAW10)", dict(fmt=_fmt(storage=_lib.RC_RAW_MIPI10, line_bytes=19, width=16)), b"line_bytes"),
    ("short line (RAW12)", dict(fmt=_fmt(storage=_lib.RC_RAW_MIPI12, line_bytes=23, width=16)), b"line_bytes"),
    ("RAW10 2w % 4", dict(fmt=_fmt(storage=_lib.RC_RAW_MIPI10, width=14), w=7, wp=16), b"RAW10"),
    ("width mismatch", dict(fmt=_fmt(width=12)), b"width"),
    ("packed misaligned", dict(packed=FAKE + 8), b"16-byte"),
    ("MIPI source misaligned", dict(fmt=_fmt(storage=_lib.RC_RAW_MIPI12, width=16), src=FAKE + 2), b"misaligned"),
    ("line past 2 GiB", dict(fmt=_fmt(storage=_lib.RC_RAW_F32), w=1 << 28, wp=1 << 28), b"line_bytes"),       # 2w x 4 bytes = 2^31: no int
])
def test_raw_ingest_fmt_bad_arguments_are_reported(case, kwargs, msg):
    kwargs = dict(kwargs)
    fmt = kwargs.pop("fmt") if "fmt" in kwargs else _fmt()
    assert _ingest(fmt, **kwargs) < 0, case
    assert msg in _lib.load().rc_last_error(), (case, _lib.load().rc_last_error())


def test_rgb_encode_bad_arguments_are_reported():
    lib = _lib.load()
    assert lib.rc_rgb_encode(None, RC_F32, FAKE, 8, 1, 8, 8, 8, 8, None) < 0 and b"null" in lib.rc_last_error()
    assert lib.rc_rgb_encode(FAKE, RC_F32, None, 8, 1, 8, 8, 8, 8, None) < 0 and b"null" in lib.rc_last_error()
    assert lib.rc_rgb_encode(FAKE, _lib.RC_U16, FAKE, 8, 1, 8, 8, 8, 8, None) < 0 and b"dtype" in lib.rc_last_error()
    assert lib.rc_rgb_encode(FAKE, RC_BF16, FAKE, 12, 1, 8, 8, 8, 8, None) < 0 and b"out_bits" in lib.rc_last_error()
    assert lib.rc_rgb_encode(FAKE, RC_F32, FAKE, 8, 1, 8, 8, 9, 8, None) < 0 and b"bad shape" in lib.rc_last_error()
    assert lib.rc_rgb_encode(FAKE, RC_F32, FAKE + 4, 16, 1, 8, 8, 8, 8, None) < 0 and b"16-byte" in lib.rc_last_error()


# ---- RawFormat ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,shape", [
    (M.RawFormat(cfa="RGBG"), (1, 8, 8)),
    (M.RawFormat(storage="u12"), (1, 8, 8)),
    (M.RawFormat(black_level=(1.0, 2.0, 3.0)), (1, 8, 8)),
    (M.RawFormat(black_level="64"), (1, 8, 8)),
    (M.RawFormat(black_level=64.0, white_level=64.0), (1, 8, 8)),
    (M.RawFormat(black_level=(0.0, 0.0, 2.0, 0.0), white_level=1.0), (1, 8, 8)),
    (M.RawFormat(storage="mipi10"), (1, 8, 10)),                     # width missing
    (M.RawFormat(storage="mipi10", width=6), (1, 8, 10)),            # 2w % 4
    (M.RawFormat(storage="mipi10", width=8), (1, 8, 9)),             # line shorter than 10 bytes
    (M.RawFormat(storage="mipi12", width=8), (1, 8, 11)),            # line shorter than 12 bytes
    (M.RawFormat(storage="mipi12", width=7), (1, 8, 12)),            # odd width
    (M.RawFormat(storage="u16", width=10), (1, 8, 8)),               # width disagrees with the tensor
    (M.RawFormat(), (1, 7, 8)),                                      # odd height
    (M.RawFormat(), (1, 2, 8, 8)),                                   # two channels
    (M.RawFormat(), (8, 8)),
])
def test_raw_format_validate_rejects(fmt, shape):
    with pytest.raises(ValueError):
        fmt.validate(shape)


def test_raw_format_validate_accepts_and_sizes():
    assert M.RawFormat().validate((2, 1, 8, 12)) == (8, 12)
    assert M.RawFormat(cfa="GRBG", storage="mipi10", width=16, black_level=(64, 60, 66, 64), white_level=1023).validate((2, 8, 64)) == (8, 16)
    assert M.RawFormat(storage="mipi12", width=6, white_level=4095).validate((1, 1, 4, 9)) == (4, 6)
    f = M.RawFormat(black_level=3.0)
    assert f.blacks() == (3.0,) * 4
    with pytest.raises(Exception):
        f.cfa = "BGGR"                                               # frozen


def test_forward_mosaic_refuses_conflicting_levels_and_formats():
    with FakeTensorMode():
        with torch.device("cuda"):
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            with torch.no_grad():
                with pytest.raises(ValueError):
                    net.forward_mosaic(mosaic, None, coord, black_level=64.0, raw_format=M.RawFormat())
                with pytest.raises(ValueError):
                    net.forward_mosaic(mosaic, None, coord, out_format="rgb10")
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, raw_format=M.RawFormat(storage="u16"))      # a float tensor is not u16 storage


# ---- kernels and traces ---------------------------------------------------------------------------------------------------------
def test_new_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    res = build.kernel_resources()
    for pat, n in (("raw_ingest_fmt_kernel", 21), ("rgb_encode_kernel", 6)):
        mine = {k: v for k, v in res.items() if pat in k}
        assert len(mine) == n, (pat, sorted(mine))
        assert all(v["tu"] == "raw_format.hip" for v in mine.values())
        assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0)]
    assert sum(1 for v in res.values() if v.get("scratch", 0) or v.get("vgpr_spill", 0)) <= 25


def test_fake_trace_of_formatted_forwards():
    """forward_mosaic(raw_format=RAW10 GRBG, out_format="rgb8"): interleaved uint8 at the mosaic size from the MIPI line width, for a DWT
    net, a strided net and (input side only) the codec."""
    import realcamnet_amd.raw2bit as RB
    fmt = M.RawFormat(cfa="GRBG", storage="mipi10", width=184, black_level=(64, 64, 66, 60), white_level=1023)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                lines = torch.empty(2, 1, 100, 256, dtype=torch.uint8)          # 184 samples = 230 bytes, padded to 256
                coord = torch.empty(2, 2, 50, 92)
                for name, bits, dt in (("LiteISPNet_GFM_LSC", 8, torch.uint8), ("ISPUNet_GFM_LSC", 16, torch.uint16)):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        y = net.forward_mosaic(lines, None, coord, raw_format=fmt, out_format=f"rgb{bits}")
                    assert y.shape == (2, 100, 184, 3) and y.dtype == dt and y.device.type == "cuda", name
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with torch.no_grad():
                    out = codec.forward_mosaic(torch.empty(2, 512, 800, dtype=torch.uint8), None, torch.empty(2, 2, 256, 256),
                                               raw_format=M.RawFormat(cfa="GBRG", storage="mipi12", width=512, white_level=4095))
                    assert out["x_hat"].shape == (2, 3, 512, 512) and out["x_hat"].dtype == torch.bfloat16
                    with pytest.raises(ValueError):
                        codec.forward_mosaic(torch.empty(2, 512, 800, dtype=torch.uint8), None, torch.empty(2, 2, 256, 256),
                                             raw_format=M.RawFormat(storage="mipi12", width=512, white_level=4095), out_format="rgb8")
                packed, cnd = torch.ops.realcam.raw_ingest_fmt(torch.empty(3, 100, 75, dtype=torch.uint8), torch.float16, 16, _lib.RC_RAW_MIPI10,
                                                               _lib.RC_CFA_BGGR, 60, [0.0] * 4, 1023.0, 32, 48)
                assert packed.shape == (3, 64, 32, 4) and cnd.shape == (3, 4, 32, 48) and packed.dtype == torch.float16
                assert torch.ops.realcam.rgb_encode(torch.empty(2, 3, 20, 30), 16, 18, 30).shape == (2, 18, 30, 3)
    finally:
        torch.set_default_dtype(old)
