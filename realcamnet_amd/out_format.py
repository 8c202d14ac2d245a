"""The video-encoder surface forward_mosaic / ops.yuv_encode return: the `out_format=OutFormat(...)` argument (include/realcam_hip.h,
rc_out_format / rc_yuv_encode).

Pure Python: validation raises ValueError and never touches the GPU or the library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Tuple

from . import _lib

LAYOUTS = {"nv12": _lib.RC_YUV_NV12, "p010": _lib.RC_YUV_P010, "i420": _lib.RC_YUV_I420}
MATRICES = {"bt601": _lib.RC_MATRIX_BT601, "bt709": _lib.RC_MATRIX_BT709, "bt2020": _lib.RC_MATRIX_BT2020}
RANGES = {"limited": _lib.RC_RANGE_LIMITED, "full": _lib.RC_RANGE_FULL}
SITINGS = {"left": _lib.RC_SITING_LEFT, "center": _lib.RC_SITING_CENTER}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}     # the header's RC_YUV_KR_KB
ELEM_BYTES = {"nv12": 1, "p010": 2, "i420": 1}


def _align_up(v: int, a: int) -> int:
    return -(-v // a) * a


class Plane(NamedTuple):
    """One plane of a frame, in bytes: `rows` rows of `valid_bytes` samples each, `pitch` apart, starting `offset` into the frame;
    `alloc_rows` rows are allocated (the rest, and each row's bytes past valid_bytes, are zero)."""
    name: str
    offset: int
    pitch: int
    rows: int
    valid_bytes: int
    alloc_rows: int


class PlaneLayout(NamedTuple):
    """The numbers a caller hands to the encoder.  pitch: bytes between Y rows (also the first plane's pitch); frame_bytes: one frame,
    and the distance between the frames of a batch; elem_bytes: 1 (uint8) or 2 (uint16)."""
    pitch: int
    planes: Tuple[Plane, ...]
    frame_bytes: int
    elem_bytes: int


class YuvFrames(NamedTuple):
    """forward_mosaic(out_format=OutFormat(...)): `buffer` is the one allocation, (B, frame_elems) uint8 / uint16, frame b being what the
    encoder takes; `planes` are views into it without the padding: Y (B,h,w), then CbCr (B,h/2,w/2,2) for nv12 / p010 or Cb, Cr
    (B,h/2,w/2) for i420."""
    buffer: object
    planes: tuple


def frame_layout(layout: int, pitch: int, rows: int, h: int, w: int) -> PlaneLayout:
    """rc_yuv_encode's surface plan for a packed frame (chroma_offset 0) with the given Y pitch (bytes) and allocated Y rows."""
    es = 2 if layout == _lib.RC_YUV_P010 else 1
    crows = (rows + 1) // 2
    y = Plane("y", 0, pitch, h, w * es, rows)
    if layout == _lib.RC_YUV_I420:
        cp = pitch // 2
        cb = Plane("cb", pitch * rows, cp, h // 2, w // 2, crows)
        cr = Plane("cr", cb.offset + cp * crows, cp, h // 2, w // 2, crows)
        return PlaneLayout(pitch, (y, cb, cr), cr.offset + cp * crows, es)
    c = Plane("cbcr", pitch * rows, pitch, h // 2, w * es, crows)
    return PlaneLayout(pitch, (y, c), c.offset + pitch * crows, es)


@dataclass(frozen=True)
class OutFormat:
    """A Y'CbCr 4:2:0 encoder surface.

    layout         "nv12" (uint8: Y plane, then one plane of interleaved Cb,Cr pairs at half size), "p010" (the same planes as uint16, the
                   10-bit code in the high bits: code << 6), "i420" (uint8: Y, Cb, Cr planes; chroma pitch = pitch / 2).
    matrix         "bt601", "bt709" (default), "bt2020" (its luma coefficients only: the network's result stays sRGB).
    range          "limited" (default: Y 16..235, chroma 16..240, times 4 at 10 bit) or "full".
    chroma_siting  "left" (default; MPEG-2 / H.264 / HEVC) or "center" (JPEG / MPEG-1).
    pitch_align    bytes, a power of two: the Y pitch is the row's bytes rounded up to it (for "i420" to twice it, so that the chroma pitch
                   is aligned too).  A multiple of 16 takes the kernel's 16-byte store path.
    height_align   rows of the Y plane: the chroma plane(s) start pitch * align_up(h, height_align) bytes into the frame.
    """

    layout: str = "nv12"
    matrix: str = "bt709"
    range: str = "limited"
    chroma_siting: str = "left"
    pitch_align: int = 1
    height_align: int = 1

    def __post_init__(self):
        for field, table in (("layout", LAYOUTS), ("matrix", MATRICES), ("range", RANGES), ("chroma_siting", SITINGS)):
            v = getattr(self, field)
            if not isinstance(v, str) or v not in table:
                raise ValueError(f"OutFormat.{field} must be one of {sorted(table)}, got {v!r}")
        pa, ha = self.pitch_align, self.height_align
        if isinstance(pa, bool) or not isinstance(pa, int) or pa < 1 or pa & (pa - 1):
            raise ValueError(f"OutFormat.pitch_align must be a power of two (bytes), got {pa!r}")
        if isinstance(ha, bool) or not isinstance(ha, int) or ha < 1:
            raise ValueError(f"OutFormat.height_align must be a positive number of rows, got {ha!r}")

    @property
    def bits(self) -> int:
        return 10 if self.layout == "p010" else 8

    @property
    def elem_bytes(self) -> int:
        return ELEM_BYTES[self.layout]

    def pitch(self, w: int) -> int:
        """Bytes between Y rows of a frame `w` pixels wide."""
        es = self.elem_bytes
        a = max(self.pitch_align, es)
        return _align_up(w * es, 2 * a if self.layout == "i420" else a)

    def plane_layout(self, h: int, w: int) -> PlaneLayout:
        """The pitch, each plane's offset / rows / valid bytes, and the frame size of an (h, w) frame, in bytes.  Raises ValueError for a
        size 4:2:0 cannot hold."""
        if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int) or h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"4:2:0 needs an even height and width, got ({h!r}, {w!r})")
        pl = frame_layout(LAYOUTS[self.layout], self.pitch(w), _align_up(h, self.height_align), h, w)
        if pl.frame_bytes >= 1 << 31:
            raise ValueError(f"a {self.layout} frame of ({h}, {w}) needs {pl.frame_bytes} bytes: beyond 2 GiB")
        return pl
