"""The video-encoder surface forward_mosaic / ops.yuv_encode return: the `out_format=OutFormat(...)` argument (include/realcam_hip.h,
rc_out_format / rc_yuv_encode).

Pure Python: validation raises ValueError and never touches the GPU or the library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Tuple

from . import _lib

LAYOUTS = {"nv12": _lib.RC_YUV_NV12, "p010": _lib.RC_YUV_P010, "i420": _lib.RC_YUV_I420,
           "nv16": _lib.RC_YUV_NV16, "p210": _lib.RC_YUV_P210, "i422": _lib.RC_YUV_I422, "i210": _lib.RC_YUV_I210, "i010": _lib.RC_YUV_I010,
           "i444": _lib.RC_YUV_I444, "i410": _lib.RC_YUV_I410, "yuy2": _lib.RC_YUV_YUY2, "uyvy": _lib.RC_YUV_UYVY, "y210": _lib.RC_YUV_Y210,
           "v210": _lib.RC_YUV_V210}
MATRICES = {"bt601": _lib.RC_MATRIX_BT601, "bt709": _lib.RC_MATRIX_BT709, "bt2020": _lib.RC_MATRIX_BT2020}
RANGES = {"limited": _lib.RC_RANGE_LIMITED, "full": _lib.RC_RANGE_FULL}
SITINGS = {"left": _lib.RC_SITING_LEFT, "center": _lib.RC_SITING_CENTER}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}     # the header's RC_YUV_KR_KB
# the buffer's element: uint8 or uint16; a v210 row is a byte stream of little-endian dwords, so its buffer is uint8
ELEM_BYTES = {"nv12": 1, "p010": 2, "i420": 1, "nv16": 1, "p210": 2, "i422": 1, "i210": 2, "i010": 2, "i444": 1, "i410": 2, "yuy2": 1, "uyvy": 1,
              "y210": 2, "v210": 1}
SUBSAMPLING = {"nv12": "420", "p010": "420", "i420": "420", "i010": "420", "i444": "444", "i410": "444"}       # every other layout: "422"
BITS = {"p010": 10, "p210": 10, "i210": 10, "i010": 10, "i410": 10, "y210": 10, "v210": 10}                    # every other layout: 8
# how the samples are stored: three planes, Y + interleaved CbCr, one plane of Y0 Cb Y1 Cr / Cb Y0 Cr Y1, or v210's dwords
CONTAINERS = {"nv12": "semi", "p010": "semi", "nv16": "semi", "p210": "semi", "yuy2": "yuyv", "y210": "yuyv", "uyvy": "uyvy", "v210": "v210"}   # every other: "planar"
_NAMES = {v: k for k, v in LAYOUTS.items()}


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
    (B,h/2,w/2) for i420.  The 4:2:2 / 4:4:4 layouts the same with chroma of (h, w/2) / (h, w); yuy2 / uyvy / y210 one (B,h,w/2,4) view in
    memory order; v210 one (B,h,ceil(w/6),4) int32 view of its dwords."""
    buffer: object
    planes: tuple


def frame_layout(layout: int, pitch: int, rows: int, h: int, w: int) -> PlaneLayout:
    """rc_yuv_encode's surface plan for a packed frame (chroma_offset 0) with the given pitch (bytes) and allocated rows of the first
    plane.  A 4:2:0 chroma plane has ceil(rows / 2) allocated rows, a 4:2:2 / 4:4:4 one `rows`."""
    name = _NAMES[layout]
    es, sub, cont = ELEM_BYTES[name], SUBSAMPLING.get(name, "422"), CONTAINERS.get(name, "planar")
    if cont == "v210":
        return PlaneLayout(pitch, (Plane("v210", 0, pitch, h, -(-w // 6) * 16, rows),), pitch * rows, es)
    if cont in ("yuyv", "uyvy"):
        return PlaneLayout(pitch, (Plane(cont, 0, pitch, h, 2 * w * es, rows),), pitch * rows, es)
    crows, ch = ((rows + 1) // 2, h // 2) if sub == "420" else (rows, h)
    y = Plane("y", 0, pitch, h, w * es, rows)
    if cont == "planar":
        cp, cw = (pitch, w) if sub == "444" else (pitch // 2, w // 2)
        cb = Plane("cb", pitch * rows, cp, ch, cw * es, crows)
        cr = Plane("cr", cb.offset + cp * crows, cp, ch, cw * es, crows)
        return PlaneLayout(pitch, (y, cb, cr), cr.offset + cp * crows, es)
    c = Plane("cbcr", pitch * rows, pitch, ch, w * es, crows)
    return PlaneLayout(pitch, (y, c), c.offset + pitch * crows, es)


@dataclass(frozen=True)
class OutFormat:
    """A Y'CbCr encoder surface: 4:2:0, 4:2:2 or 4:4:4, 8 or 10 bit.

    layout         "nv12" (uint8: Y plane, then one plane of interleaved Cb,Cr pairs at half size), "p010" (the same planes as uint16, the
                   10-bit code in the high bits: code << 6), "i420" (uint8: Y, Cb, Cr planes; chroma pitch = pitch / 2).
                   4:2:2 (any height, even width): "nv16" / "p210" (nv12's / p010's planes with chroma on every row), "i422" (yuv422p) and
                   "i210" (yuv422p10le: uint16, the code in the low bits), packed "yuy2" (bytes Y0 Cb Y1 Cr), "uyvy" (Cb Y0 Cr Y1), "y210"
                   (yuy2's order as uint16, code << 6) and "v210" (six pixels in four dwords; pitch = ceil(w / 48) * 128 bytes).
                   "i010" (yuv420p10le: i420 as uint16, low bits).  4:4:4 (any size): "i444" (yuv444p), "i410" (yuv444p10le, low bits).
    matrix         "bt601", "bt709" (default), "bt2020" (its luma coefficients only: the network's result stays sRGB).
    range          "limited" (default: Y 16..235, chroma 16..240, times 4 at 10 bit) or "full".
    chroma_siting  "left" (default; MPEG-2 / H.264 / HEVC) or "center" (JPEG / MPEG-1).  4:4:4 has no chroma step and ignores it.
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
        return BITS.get(self.layout, 8)

    @property
    def subsampling(self) -> str:
        """"420", "422" or "444"."""
        return SUBSAMPLING.get(self.layout, "422")

    @property
    def elem_bytes(self) -> int:
        return ELEM_BYTES[self.layout]

    def pitch(self, w: int) -> int:
        """Bytes between rows of the first plane of a frame `w` pixels wide."""
        es = self.elem_bytes
        a = max(self.pitch_align, es)
        cont = CONTAINERS.get(self.layout, "planar")
        if cont == "v210":
            return _align_up(-(-w // 48) * 128, a)
        if cont in ("yuyv", "uyvy"):
            return _align_up(2 * w * es, a)
        return _align_up(w * es, 2 * a if cont == "planar" and self.subsampling != "444" else a)     # pitch / 2 is the chroma pitch: aligned too

    def plane_layout(self, h: int, w: int) -> PlaneLayout:
        """The pitch, each plane's offset / rows / valid bytes, and the frame size of an (h, w) frame, in bytes.  Raises ValueError for a
        size the layout cannot hold: 4:2:0 needs an even height and width, 4:2:2 an even width."""
        ok = not (isinstance(h, bool) or isinstance(w, bool)) and isinstance(h, int) and isinstance(w, int)
        sub = self.subsampling
        if sub == "420" and (not ok or h < 2 or w < 2 or h % 2 or w % 2):
            raise ValueError(f"4:2:0 needs an even height and width, got ({h!r}, {w!r})")
        if sub == "422" and (not ok or h < 1 or w < 2 or w % 2):
            raise ValueError(f"4:2:2 ({self.layout}) needs an even width, got ({h!r}, {w!r})")
        if not ok or h < 1 or w < 1:
            raise ValueError(f"4:4:4 ({self.layout}) needs a height and width of at least 1, got ({h!r}, {w!r})")
        pl = frame_layout(LAYOUTS[self.layout], self.pitch(w), _align_up(h, self.height_align), h, w)
        if pl.frame_bytes >= 1 << 31:
            raise ValueError(f"a {self.layout} frame of ({h}, {w}) needs {pl.frame_bytes} bytes: beyond 2 GiB")
        return pl
