"""The compressed still forward_mosaic / ops.jpeg_encode return: the `out_format=Jpeg(...)` argument and `Output(format=Jpeg(...))`
(include/realcam_hip.h, rc_jpeg_desc / rc_jpeg_encode).

Pure Python: validation raises ValueError / TypeError and never touches the GPU.  Only `Jpeg.tables` and `Jpeg.header`, which restate
nothing and ask the library's host functions, load it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

from . import _lib

SUBSAMPLINGS = {"420": _lib.RC_JPEG_420, "444": _lib.RC_JPEG_444}
MCU = {"420": 16, "444": 8}
HEADER_BYTES = 613          # SOI, APP0, DQT (two tables), SOF0, DHT (four tables), DRI, SOS: rc_jpeg_plan's header_bytes
MAX_DIM = 65535


def _int(v, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not lo <= v <= hi:
        raise ValueError(f"{name} must be {lo} .. {hi}, got {v!r}")


class JpegPlan(NamedTuple):
    """What an (h, w) frame needs: the header's bytes (SOI .. SOS), the MCU grid, the restart intervals, and the bytes reserved per frame."""
    header_bytes: int
    mcu_cols: int
    mcu_rows: int
    intervals: int
    capacity: int


@dataclass(frozen=True)
class Jpeg:
    """A baseline JFIF still per frame, coded on the device.

    quality      1 .. 100: the IJG scaling of the standard quantisation tables (what libjpeg and Pillow call quality).
    subsampling  "420" (default; MCU 16x16: four Y blocks, Cb, Cr; chroma is the centre-sited 2x2 mean) or "444" (MCU 8x8).
    restart      MCUs per restart interval, 1 .. 65535.  An interval is what one wave codes: a short one means more parallelism and two
                 marker bytes more per interval.
    capacity     bytes reserved per frame, or None: the header + 3 hp wp (444) or 3 hp wp / 2 (420) + 2 per interval + 2, hp / wp the size
                 padded to the MCU -- the raw samples' size, which a frame at quality 100 can still exceed (JpegFrames.tobytes says so).
    Any h, w >= 1 is valid: the frame is padded to whole MCUs by repeating its last row and column.
    """

    quality: int = 90
    subsampling: str = "420"
    restart: int = 8
    capacity: Optional[int] = None

    def __post_init__(self):
        _int(self.quality, "Jpeg.quality", 1, 100)
        if not isinstance(self.subsampling, str) or self.subsampling not in SUBSAMPLINGS:
            raise ValueError(f"Jpeg.subsampling must be one of {sorted(SUBSAMPLINGS)}, got {self.subsampling!r}")
        _int(self.restart, "Jpeg.restart", 1, 65535)
        if self.capacity is not None:
            _int(self.capacity, "Jpeg.capacity", 1, (1 << 62))

    def plan(self, h: int, w: int) -> JpegPlan:
        """The JpegPlan of an (h, w) frame.  Raises for a size a JPEG cannot hold (its SOF0 segment has 16 bits per axis)."""
        _int(h, "Jpeg.plan: h", 1, MAX_DIM)
        _int(w, "Jpeg.plan: w", 1, MAX_DIM)
        mcu = MCU[self.subsampling]
        cols, rows = -(-w // mcu), -(-h // mcu)
        intervals = -(-cols * rows // self.restart)
        area = cols * rows * mcu * mcu
        default = HEADER_BYTES + (3 * area if self.subsampling == "444" else 3 * area // 2) + 2 * intervals + 2
        return JpegPlan(HEADER_BYTES, cols, rows, intervals, default if self.capacity is None else self.capacity)

    def desc(self) -> "_lib.JpegDesc":
        return _lib.JpegDesc(quality=self.quality, subsampling=SUBSAMPLINGS[self.subsampling], restart=self.restart)

    def tables(self):
        """(luma, chroma): the two quantisation tables as (8, 8) uint8 arrays in natural order (rc_jpeg_tables)."""
        import numpy as np
        ql, qc = np.empty(64, np.uint8), np.empty(64, np.uint8)
        _lib.check(_lib.load().rc_jpeg_tables(self.quality, ql.ctypes.data, qc.ctypes.data), "rc_jpeg_tables")
        return ql.reshape(8, 8), qc.reshape(8, 8)

    def header(self, h: int, w: int) -> bytes:
        """The file's bytes from SOI to the end of SOS for an (h, w) frame (rc_jpeg_header)."""
        self.plan(h, w)
        buf, n, d = C.create_string_buffer(HEADER_BYTES), C.c_size_t(0), self.desc()
        _lib.check(_lib.load().rc_jpeg_header(C.byref(d), h, w, C.cast(buf, C.c_void_p), HEADER_BYTES, C.byref(n)), "rc_jpeg_header")
        return buf.raw[:n.value]


class JpegFrames(NamedTuple):
    """forward_mosaic(out_format=Jpeg(...)) / ops.jpeg_encode: `buffer` (B, capacity) uint8 and `lengths` (B,) int64 on the device, the bytes
    each complete file NEEDS; frame b is buffer[b, :lengths[b]], a complete JFIF file, when lengths[b] <= capacity.  fmt: the Jpeg; size: (h, w)."""
    buffer: object
    lengths: object
    fmt: Jpeg
    size: Tuple[int, int]

    def _cut(self, b, n, data):
        cap = self.buffer.shape[1]
        if n > cap:
            raise ValueError(f"JpegFrames: frame {b} needs {n} bytes, the buffer holds {cap} per frame: encode it with Jpeg(capacity={n}) or more")
        return data[:n].tobytes()

    def tobytes(self, b: int) -> bytes:
        """Frame b as a complete JFIF file.  Synchronises; raises ValueError when the frame did not fit, naming the capacity that would do."""
        n = int(self.lengths[b])
        return self._cut(b, n, self.buffer[b, :min(n, self.buffer.shape[1])].cpu().numpy())

    def files(self):
        """Every frame as bytes (one synchronisation, one copy)."""
        lengths, data = self.lengths.cpu().tolist(), self.buffer.cpu().numpy()
        return [self._cut(b, n, data[b]) for b, n in enumerate(lengths)]
