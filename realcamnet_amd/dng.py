"""The raw still forward_mosaic / ops.raw_dng write: the `RawFormat(dng=Dng(...))` field (include/realcam_hip.h, rc_dng_desc / rc_dng_encode).

A DNG file per frame: a little-endian TIFF whose one IFD holds the sensor mosaic AS DELIVERED in tiles, each a lossless JPEG stream coded on
the device.  The library knows nothing of TIFF: the header -- the TIFF header, IFD 0 and its out-of-line values -- is composed here, from the
RawFormat that describes the frame, and the device fills in the two tile arrays.

Pure Python: validation raises ValueError / TypeError and never touches the GPU.  Only `Dng.tile_header`, which restates nothing and asks
the library's host function, loads it.
"""
from __future__ import annotations

import ctypes as C
import math
import re
import struct
from dataclasses import dataclass
from fractions import Fraction
from typing import NamedTuple, Optional, Tuple

from . import _lib

PRECISION = {"u8": 8, "mipi10": 10, "mipi12": 12, "u16": 16}          # SOF3's P per storage
STORAGE_CODE = {"u8": _lib.RC_RAW_U8, "mipi10": _lib.RC_RAW_MIPI10, "mipi12": _lib.RC_RAW_MIPI12, "u16": _lib.RC_RAW_U16}
TILE_MIN, TILE_MAX = 16, 65520
MAX_FILE = (1 << 31) - 1
# XYZ (D65) -> linear sRGB (IEC 61966-2-1).  A PLACEHOLDER: the learned ISP has no camera matrix, so a raw developer that trusts ColorMatrix1
# renders the file as if the sensor's primaries were sRGB's.  Give color_matrix= for a characterised sensor.
XYZ_TO_SRGB = (3.2404542, -1.5371385, -0.4985314, -0.9692660, 1.8760108, 0.0415560, 0.0556434, -0.2040259, 1.0572252)
SOFTWARE = "realcamnet_amd"
_COLOR = {"R": 0, "G": 1, "B": 2}
_BYTE, _ASCII, _SHORT, _LONG, _RATIONAL, _SRATIONAL, _DOUBLE = 1, 2, 3, 4, 5, 10, 12


def _int(v, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not lo <= v <= hi:
        raise ValueError(f"{name} must be {lo} .. {hi}, got {v!r}")


def _ascii(v, name):
    if not isinstance(v, str):
        raise TypeError(f"{name} must be a str, got {type(v).__name__}")
    if not v.isascii() or "\0" in v:
        raise ValueError(f"{name} must be ASCII without NUL, got {v!r}")


def _numbers(v, name, counts):
    """`v` as a flat tuple of finite floats; one level of nesting (pairs, matrix rows) is flattened."""
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
        raise TypeError(f"{name} must be a sequence of numbers, got {v!r}")
    flat = []
    for e in v:
        flat.extend(e if hasattr(e, "__len__") and not isinstance(e, (str, bytes)) else (e,))
    if not all(isinstance(e, (int, float)) and not isinstance(e, bool) for e in flat):
        raise TypeError(f"{name} must hold numbers, got {v!r}")
    flat = tuple(float(e) for e in flat)
    if len(flat) not in counts or not all(math.isfinite(e) for e in flat):
        raise ValueError(f"{name} must hold {' or '.join(str(c) for c in counts)} finite numbers, got {v!r}")
    return flat


def _rational(v, what, signed=False):
    """rint(v 2^20) / 2^20 in lowest terms (an integer gets the denominator 1), as TIFF's two 32-bit words."""
    f = Fraction(int(round(float(v) * (1 << 20))), 1 << 20)          # round(): half to even, as rint
    lo, hi = (-(1 << 31), (1 << 31) - 1) if signed else (0, (1 << 32) - 1)
    if not lo <= f.numerator <= hi:
        raise ValueError(f"Dng: {what} {v!r} does not fit a TIFF {'SRATIONAL' if signed else 'RATIONAL'}")
    return struct.pack("<ii" if signed else "<II", f.numerator, f.denominator)


class DngPlan(NamedTuple):
    """What an (h2, w2) mosaic needs: the bytes of the TIFF header and of a tile's own header (SOI .. SOS), the tile grid, the bytes reserved
    per frame, the scratch bytes per frame, and where in the header the TileOffsets and TileByteCounts arrays stand."""
    header_bytes: int
    tile_header_bytes: int
    tiles_x: int
    tiles_y: int
    capacity: int
    scratch_bytes: int
    offsets_at: int
    counts_at: int


@dataclass(frozen=True)
class Dng:
    """A DNG raw still per frame, coded on the device: the mosaic as the sensor delivered it, losslessly, with the tags that describe it.

    tile             (tw, th) in mosaic samples, multiples of 16 in 16 .. 65520.  A tile is what one wave codes and what a reader decodes on
                     its own: a small one means more parallelism, and 60-odd header bytes more per tile.
    components       2 (default, the usual DNG arrangement): a tile is a JPEG frame of tw / 2 columns and 2 components, so every sample is
                     predicted from the sample two to its left, which has its own colour.  1: tw columns of one component; it compresses
                     worse, and an 8-bit stream of this kind is what general JPEG libraries open.
    capacity         bytes reserved per frame, or None: the header + per tile its header + 2 + 4 tw th.  A sample takes at most 27 bits, so
                     only a frame full of stuffed 0xFF bytes can exceed it (DngFrames.tobytes says so).
    make, model      tags Make and Model; unique_model: UniqueCameraModel, by default make + " " + model.
    color_matrix     ColorMatrix1, nine numbers row-major (XYZ -> camera).  The default is the XYZ (D65) -> linear sRGB matrix, a placeholder:
                     the learned ISP has no camera matrix.
    as_shot_neutral  AsShotNeutral, three numbers; by default derived from host-number Calibration.gains as (g / gR, 1, g / gB) with g the
                     mean of the two green gains, else (1, 1, 1).  Gains on the device are never read: no synchronisation.
    noise_profile    NoiseProfile: one (scale, offset) pair for all colours or three, R G B -- RawNoiseStats.profile()'s fit -- or None.
    software         tag Software (default "realcamnet_amd"); datetime: tag DateTime, "YYYY:MM:DD HH:MM:SS", or None (no tag).
    The black and white levels, the CFA phase (a 4x4 pattern for a Quad-Bayer sensor) and a Calibration.curve (as LinearizationTable) come
    from the RawFormat.  Any even h2, w2 is valid: tiles are padded by repeating the last sample of the same colour.
    """

    tile: Tuple[int, int] = (256, 64)
    components: int = 2
    capacity: Optional[int] = None
    make: str = ""
    model: str = "realcam"
    unique_model: Optional[str] = None
    color_matrix: Optional[Tuple[float, ...]] = None
    as_shot_neutral: Optional[Tuple[float, float, float]] = None
    noise_profile: Optional[Tuple[float, ...]] = None
    software: Optional[str] = None
    datetime: Optional[str] = None

    def __post_init__(self):
        t = self.tile
        if isinstance(t, (str, bytes)) or not hasattr(t, "__len__") or len(t) != 2:
            raise TypeError(f"Dng.tile must be (tw, th), got {t!r}")
        for v, name in zip(t, ("Dng.tile width", "Dng.tile height")):
            _int(v, name, TILE_MIN, TILE_MAX)
            if v % 16:
                raise ValueError(f"{name} must be a multiple of 16, got {v}")
        object.__setattr__(self, "tile", (t[0], t[1]))
        _int(self.components, "Dng.components", 1, 2)
        if self.capacity is not None:
            _int(self.capacity, "Dng.capacity", 1, (1 << 32) - 1)
        _ascii(self.make, "Dng.make")
        _ascii(self.model, "Dng.model")
        for name in ("unique_model", "software", "datetime"):
            if getattr(self, name) is not None:
                _ascii(getattr(self, name), f"Dng.{name}")
        if self.datetime is not None and not re.fullmatch(r"\d{4}:\d\d:\d\d \d\d:\d\d:\d\d", self.datetime):
            raise ValueError(f"Dng.datetime must be 'YYYY:MM:DD HH:MM:SS', got {self.datetime!r}")
        if self.color_matrix is not None:
            object.__setattr__(self, "color_matrix", _numbers(self.color_matrix, "Dng.color_matrix", (9,)))
        if self.as_shot_neutral is not None:
            n = _numbers(self.as_shot_neutral, "Dng.as_shot_neutral", (3,))
            if not all(v > 0.0 for v in n):
                raise ValueError(f"Dng.as_shot_neutral must be positive, got {n}")
            object.__setattr__(self, "as_shot_neutral", n)
        if self.noise_profile is not None:
            object.__setattr__(self, "noise_profile", _numbers(self.noise_profile, "Dng.noise_profile", (2, 6)))

    # ---- what the RawFormat says of the frame as delivered ----
    @staticmethod
    def _precision(raw_format) -> int:
        from .raw_format import RawFormat
        if not isinstance(raw_format, RawFormat):
            raise TypeError(f"Dng: raw_format must be a RawFormat, got {type(raw_format).__name__}")
        if raw_format.storage not in PRECISION:
            raise ValueError(f"Dng: a DNG holds sensor codes: storage must be one of {sorted(PRECISION)}, got {raw_format.storage!r} "
                             "(a float mosaic has left the sensor's code domain; write the frame as delivered)")
        return PRECISION[raw_format.storage]

    @staticmethod
    def _size(h2, w2):
        _int(h2, "Dng: the mosaic height", 2, 1 << 21)
        _int(w2, "Dng: the mosaic width", 2, 1 << 25)
        if h2 % 2 or w2 % 2:
            raise ValueError(f"Dng: the mosaic's height and width must be even (whole CFA cells), got ({h2}, {w2})")

    def desc(self) -> "_lib.DngDesc":
        return _lib.DngDesc(tile_w=self.tile[0], tile_h=self.tile[1], components=self.components)

    def neutral(self, raw_format) -> Tuple[float, float, float]:
        """AsShotNeutral: as_shot_neutral, else from host-number Calibration.gains, else (1, 1, 1)."""
        if self.as_shot_neutral is not None:
            return self.as_shot_neutral
        cal = raw_format.calibration
        gains = getattr(cal, "gains", None)
        if gains is None or getattr(cal, "device_gains", False):
            return (1.0, 1.0, 1.0)
        by = {"R": [], "G": [], "B": []}
        for ch, g in zip(raw_format.cfa, gains):
            by[ch].append(float(g))
        g = sum(by["G"]) / 2.0
        if not (g > 0.0 and by["R"][0] > 0.0 and by["B"][0] > 0.0):
            raise ValueError(f"Dng: AsShotNeutral cannot be derived from Calibration.gains {tuple(gains)} (a zero gain): give as_shot_neutral")
        return (g / by["R"][0], 1.0, g / by["B"][0])

    @staticmethod
    def linearization(raw_format) -> Optional[Tuple[int, ...]]:
        """LinearizationTable: entry c = clamp(rint(curve(c)), 0, 65535) for every code c of the storage, curve(c) formed in double from
        the Pwl's fp32 knots and slopes as rc_raw_calibrate's step 1 states it; None without a Calibration.curve."""
        curve = getattr(raw_format.calibration, "curve", None)
        if curve is None:
            return None
        import numpy as np
        c = np.arange(1 << PRECISION[raw_format.storage], dtype=np.float64)
        x, y, s = (np.asarray(v, np.float64) for v in (curve.x, curve.y, curve.slopes()))
        j = np.clip(np.searchsorted(x, c, side="right") - 1, 0, len(x) - 2)
        lin = y[j] + (c - x[j]) * s[j]
        if lin.max() > 65535.0:
            raise ValueError(f"Dng: the Calibration.curve reaches {lin.max():.6g}: a LinearizationTable entry is a SHORT (at most 65535)")
        return tuple(int(v) for v in np.clip(np.rint(lin), 0, 65535))

    def _tags(self, h2, w2, raw_format, tiles):
        """IFD 0's entries, ascending: (tag, type, count, value bytes)."""
        p = self._precision(raw_format)
        short = lambda *v: struct.pack(f"<{len(v)}H", *v)
        long_ = lambda *v: struct.pack(f"<{len(v)}I", *v)
        text = lambda s: s.encode("ascii") + b"\0"
        if raw_format.cfa not in ("RGGB", "BGGR", "GRBG", "GBRG"):
            raise ValueError(f"Dng: unknown cfa {raw_format.cfa!r}")
        colors = [_COLOR[ch] for ch in raw_format.cfa]
        blacks = raw_format.blacks()
        if raw_format.quad is not None:
            if len(set(blacks)) != 1:
                raise ValueError("Dng: a Quad-Bayer frame needs one black level for all positions (BlackLevelRepeatDim is 2 x 2, the colours "
                                 f"repeat every 4 x 4), got {blacks}")
            pattern = [colors[2 * ((y >> 1) & 1) + ((x >> 1) & 1)] for y in range(4) for x in range(4)]
        else:
            pattern = colors
        if not all(math.isfinite(b) and b >= 0.0 for b in blacks):
            raise ValueError(f"Dng: BlackLevel is a RATIONAL: the black levels must be finite and >= 0, got {blacks}")
        white = float(raw_format.white_level)
        if not (math.isfinite(white) and 1 <= round(white) <= 65535):
            raise ValueError(f"Dng: WhiteLevel must round to 1 .. 65535, got {raw_format.white_level!r}")
        unique = f"{self.make} {self.model}" if self.unique_model is None else self.unique_model
        software = SOFTWARE if self.software is None else self.software
        matrix = XYZ_TO_SRGB if self.color_matrix is None else self.color_matrix
        dim = int(math.isqrt(len(pattern)))
        tags = [(254, _LONG, 1, long_(0)), (256, _LONG, 1, long_(w2)), (257, _LONG, 1, long_(h2)), (258, _SHORT, 1, short(8 if p == 8 else 16)),
                (259, _SHORT, 1, short(7)), (262, _SHORT, 1, short(32803)), (271, _ASCII, len(self.make) + 1, text(self.make)),
                (272, _ASCII, len(self.model) + 1, text(self.model)), (274, _SHORT, 1, short(1)), (277, _SHORT, 1, short(1)), (284, _SHORT, 1, short(1)),
                (305, _ASCII, len(software) + 1, text(software))]
        if self.datetime is not None:
            tags.append((306, _ASCII, 20, text(self.datetime)))
        tags += [(322, _LONG, 1, long_(self.tile[0])), (323, _LONG, 1, long_(self.tile[1])), (324, _LONG, tiles, bytes(4 * tiles)),
                 (325, _LONG, tiles, bytes(4 * tiles)), (33421, _SHORT, 2, short(dim, dim)), (33422, _BYTE, len(pattern), bytes(pattern)),
                 (50706, _BYTE, 4, bytes((1, 4, 0, 0))), (50707, _BYTE, 4, bytes((1, 1, 0, 0))), (50708, _ASCII, len(unique) + 1, text(unique)),
                 (50710, _BYTE, 3, bytes((0, 1, 2))), (50711, _SHORT, 1, short(1))]
        table = self.linearization(raw_format)
        if table is not None:
            tags.append((50712, _SHORT, len(table), short(*table)))
        tags += [(50713, _SHORT, 2, short(2, 2)), (50714, _RATIONAL, 4, b"".join(_rational(b, "black level") for b in blacks)),
                 (50717, _LONG, 1, long_(int(round(white)))), (50721, _SRATIONAL, 9, b"".join(_rational(m, "color_matrix entry", True) for m in matrix)),
                 (50728, _RATIONAL, 3, b"".join(_rational(v, "AsShotNeutral") for v in self.neutral(raw_format))), (50778, _SHORT, 1, short(21))]
        if self.noise_profile is not None:
            tags.append((51041, _DOUBLE, len(self.noise_profile), struct.pack(f"<{len(self.noise_profile)}d", *self.noise_profile)))
        return tags

    def _compose(self, h2, w2, raw_format):
        """(header bytes, offsets_at, counts_at): "II*\\0", the IFD at 8 with its entries ascending, then the values longer than 4 bytes in
        entry order, each on an even offset."""
        self._size(h2, w2)
        tiles = -(-w2 // self.tile[0]) * -(-h2 // self.tile[1])
        tags = self._tags(h2, w2, raw_format, tiles)
        at = 8 + 2 + 12 * len(tags) + 4
        ifd, tail, where = bytearray(struct.pack("<H", len(tags))), bytearray(), {}
        for i, (tag, typ, count, value) in enumerate(tags):
            if len(value) <= 4:
                where[tag] = 8 + 2 + 12 * i + 8
                field = value + bytes(4 - len(value))
            else:
                where[tag] = at + len(tail)
                field = struct.pack("<I", where[tag])
                tail += value + bytes(len(value) & 1)
            ifd += struct.pack("<HHI", tag, typ, count) + field
        ifd += struct.pack("<I", 0)
        return b"II*\0" + struct.pack("<I", 8) + bytes(ifd) + bytes(tail), where[324], where[325]

    def plan(self, h2: int, w2: int, raw_format) -> DngPlan:
        """The DngPlan of an (h2, w2) mosaic that `raw_format` describes.  Raises for what a DNG cannot hold."""
        header, offsets_at, counts_at = self._compose(h2, w2, raw_format)
        tw, th = self.tile
        tx, ty = -(-w2 // tw), -(-h2 // th)
        thb = 58 + 5 * self.components
        default = len(header) + tx * ty * (thb + 2 + 4 * tw * th)
        if default > MAX_FILE:
            raise ValueError(f"Dng: a ({h2}, {w2}) mosaic in {tx * ty} tiles of {self.tile} may need {default} bytes; a file stays below 2^31")
        return DngPlan(len(header), thb, tx, ty, default if self.capacity is None else self.capacity, 4 * tx * ty, offsets_at, counts_at)

    def header(self, h2: int, w2: int, raw_format) -> bytes:
        """The TIFF header and IFD 0 with every tag's value; the entries of TileOffsets and TileByteCounts are zero (the device fills them)."""
        return self._compose(h2, w2, raw_format)[0]

    def tile_header(self, raw_format) -> bytes:
        """SOI .. the end of SOS of a tile's stream (rc_dng_tile_header)."""
        self._precision(raw_format)
        buf, n, d = C.create_string_buffer(80), C.c_size_t(0), self.desc()
        f = _lib.RawFormatDesc(storage=STORAGE_CODE[raw_format.storage])
        _lib.check(_lib.load().rc_dng_tile_header(C.byref(d), C.byref(f), C.cast(buf, C.c_void_p), 80, C.byref(n)), "rc_dng_tile_header")
        return buf.raw[:n.value]


class DngFrames(NamedTuple):
    """forward_mosaic(raw_format=RawFormat(dng=Dng(...))) / ops.raw_dng: `buffer` (B, capacity) uint8 and `lengths` (B,) int64 on the device, the
    bytes each complete file NEEDS; frame b is buffer[b, :lengths[b]], a complete DNG file, when lengths[b] <= capacity.  fmt: the Dng;
    size: (h2, w2)."""
    buffer: object
    lengths: object
    fmt: Dng
    size: Tuple[int, int]

    def _cut(self, b, n, data):
        cap = self.buffer.shape[1]
        if n > cap:
            raise ValueError(f"DngFrames: frame {b} needs {n} bytes, the buffer holds {cap} per frame: encode it with Dng(capacity={n}) or more")
        return data[:n].tobytes()

    def tobytes(self, b: int) -> bytes:
        """Frame b as a complete DNG file.  Synchronises; raises ValueError when the frame did not fit, naming the capacity that would do."""
        n = int(self.lengths[b])
        return self._cut(b, n, self.buffer[b, :min(n, self.buffer.shape[1])].cpu().numpy())

    def files(self):
        """Every frame as bytes (one synchronisation, one copy)."""
        lengths, data = self.lengths.cpu().tolist(), self.buffer.cpu().numpy()
        return [self._cut(b, n, data[b]) for b, n in enumerate(lengths)]
