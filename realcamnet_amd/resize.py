"""Scaled and cropped renditions of forward_mosaic's result: the `Resize` of an `Output` (include/realcam_hip.h, rc_resize_taps / rc_resize).

Pure Python: validation raises ValueError / TypeError and never touches the GPU or the library; only `taps()` calls the library's host
function rc_resize_taps, which holds the one copy of the filter arithmetic.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import InitVar, dataclass
from typing import Optional, Tuple

from . import _lib
from .look import Lut3D
from .jpeg import Jpeg
from .out_format import OutFormat
from .sharpen import Sharpen
from .stats import Stats
from .motion import Motion
from .tone import ToneMap
from .warp import Warp

FILTERS = {"area": _lib.RC_FILTER_AREA, "bilinear": _lib.RC_FILTER_BILINEAR}
MAX_TAPS = _lib.RC_RESIZE_MAX_TAPS
MAX_RATIO = _lib.RC_RESIZE_MAX_RATIO


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_axis(what: str, n: int, m: int) -> None:
    if m > n:
        raise ValueError(f"Resize: {what} {n} -> {m} is an upscale; the stage downscales or keeps the size (1 <= ratio <= {MAX_RATIO})")
    if n > MAX_RATIO * m:
        raise ValueError(f"Resize: {what} {n} -> {m} is a ratio of {n / m:.3g}, above the limit of {MAX_RATIO}")


def axis_taps(n: int, off: int, m: int, filter: str = "area"):
    """The tables of one axis (rc_resize_taps): ROI length n at offset off, output length m -> (first int32 [m], weights float32 [m, T], T)
    as NumPy arrays, T being the axis's longest list; shorter lists are padded with zeros."""
    import numpy as np
    if filter not in FILTERS:
        raise ValueError(f"Resize.filter must be one of {sorted(FILTERS)}, got {filter!r}")
    if not all(_is_int(v) for v in (n, off, m)) or n < 1 or m < 1 or off < 0:
        raise ValueError(f"axis_taps: bad lengths (n, off, m) = {(n, off, m)!r}")
    _check_axis("axis", n, m)
    first = np.empty(m, dtype=np.int32)
    weights = np.empty(m * MAX_TAPS, dtype=np.float32)
    t = C.c_int(0)
    lib = _lib.load()
    if lib.rc_resize_taps(FILTERS[filter], n, off, m, first.ctypes.data, weights.ctypes.data, C.byref(t)) != 0:
        raise ValueError(f"rc_resize_taps({filter!r}, n={n}, off={off}, m={m}): {lib.rc_last_error().decode(errors='replace')}")
    return first, weights[:m * t.value].reshape(m, t.value).copy(), t.value


@dataclass(frozen=True)
class Resize:
    """One rendition's geometry: a window of the cropped network result, downscaled.

    size    (h, w) of the output.
    roi     (y0, x0, rh, rw) in pixels of the cropped network result; None: all of it.
    filter  "area" (fractional coverage: box averaging at integer ratios) or "bilinear" (the antialiased triangle of
            F.interpolate(mode="bilinear", antialias=True)).
    Per axis 1 <= roi / size <= 8: the stage downscales or keeps the size.
    """

    size: Tuple[int, int]
    roi: Optional[Tuple[int, int, int, int]] = None
    filter: str = "area"

    def __post_init__(self):
        sz = self.size
        if not isinstance(sz, (tuple, list)) or len(sz) != 2 or not all(_is_int(v) for v in sz) or min(sz) < 1:
            raise ValueError(f"Resize.size must be (h, w) with positive integers, got {sz!r}")
        object.__setattr__(self, "size", (sz[0], sz[1]))
        if not isinstance(self.filter, str) or self.filter not in FILTERS:
            raise ValueError(f"Resize.filter must be one of {sorted(FILTERS)}, got {self.filter!r}")
        r = self.roi
        if r is not None:
            if not isinstance(r, (tuple, list)) or len(r) != 4 or not all(_is_int(v) for v in r) or r[0] < 0 or r[1] < 0 or r[2] < 1 or r[3] < 1:
                raise ValueError(f"Resize.roi must be (y0, x0, rh, rw) with y0, x0 >= 0 and rh, rw >= 1, got {r!r}")
            object.__setattr__(self, "roi", tuple(r))
            _check_axis("height", r[2], sz[0])
            _check_axis("width", r[3], sz[1])

    def window(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """The ROI (y0, x0, rh, rw) inside an (h, w) frame, checked: inside the frame, and each axis's ratio within 1 .. 8."""
        y0, x0, rh, rw = self.roi if self.roi is not None else (0, 0, h, w)
        if y0 + rh > h or x0 + rw > w:
            raise ValueError(f"Resize.roi {(y0, x0, rh, rw)} lies outside the ({h}, {w}) frame")
        _check_axis("height", rh, self.size[0])
        _check_axis("width", rw, self.size[1])
        return y0, x0, rh, rw

    def taps(self, h: int, w: int):
        """((first_y, wy, Ty), (first_x, wx, Tx)) for an (h, w) frame: axis_taps of the two axes, first indices into the frame."""
        y0, x0, rh, rw = self.window(h, w)
        return axis_taps(rh, y0, self.size[0], self.filter), axis_taps(rw, x0, self.size[1], self.filter)


@dataclass(frozen=True)
class Output:
    """One entry of forward_mosaic(outputs=[...]): an optional Warp of the float result, an optional Resize, an optional ToneMap, an
    optional colour look, an optional Sharpen, then its format.

    format  None (the planar float tensor), "rgb8" / "rgb16" (interleaved uint8 / uint16), an OutFormat (a YuvFrames), a Jpeg (a JpegFrames:
            any size, the evenness rules below are the encoder surfaces' alone: even height and width for 4:2:0, even width for 4:2:2, none for 4:4:4) or a Stats (a FrameStats: the statistics of the frame after this output's own warp / resize / look, in place of a picture)
            or a Motion (a MotionField: the block motion vectors of that frame against the previous call's, in place of a picture).
    resize  None (the result's own size) or a Resize.
    look    None or a Lut3D, applied after the resize and before the encoder (ops.lut3d; with format None the looked tensor is fp32).
    warp    None or a Warp, applied first (ops.warp, fp32): the resize's window and the format then see a frame of warp.size.
    sharpen None or a Sharpen, applied last among the float stages (ops.sharpen, fp32): its thresholds are meant in the values the encoder
            and the viewer see, and nothing resamples or remaps the picture after it.
    tone    None or a ToneMap, applied after the resize and before the look (ops.tone_map, fp32): a show LUT is designed against a normally
            exposed picture, so the scene-adaptive lift comes first.
    The first five are dataclass fields.  `tone` is an init-only parameter kept as an attribute: dataclasses.fields(Output) stays the five
    names callers know, while the constructor (sixth position or keyword), equality, hash, repr and dataclasses.replace all take
    `tone` in.
    """

    format: object = None
    resize: Optional[Resize] = None
    look: Optional[Lut3D] = None
    warp: Optional[Warp] = None
    sharpen: Optional[Sharpen] = None
    tone: InitVar[Optional[ToneMap]] = None

    def __post_init__(self, tone=None):
        f = self.format
        if f is not None and not isinstance(f, (str, OutFormat, Jpeg, Stats, Motion)):
            raise TypeError(f"Output.format must be None, 'rgb8', 'rgb16', an OutFormat, a Jpeg, a Stats or a Motion, got {type(f).__name__}")
        if isinstance(f, str) and f not in ("rgb8", "rgb16"):
            raise ValueError(f"Output.format must be None, 'rgb8', 'rgb16', an OutFormat, a Jpeg, a Stats or a Motion, got {f!r}")
        if self.resize is not None and not isinstance(self.resize, Resize):
            raise TypeError(f"Output.resize must be None or a Resize, got {type(self.resize).__name__}")
        if self.look is not None and not isinstance(self.look, Lut3D):
            raise TypeError(f"Output.look must be None or a Lut3D, got {type(self.look).__name__}")
        if self.warp is not None and not isinstance(self.warp, Warp):
            raise TypeError(f"Output.warp must be None or a Warp, got {type(self.warp).__name__}")
        if self.sharpen is not None and not isinstance(self.sharpen, Sharpen):
            raise TypeError(f"Output.sharpen must be None or a Sharpen, got {type(self.sharpen).__name__}")
        if tone is not None and not isinstance(tone, ToneMap):
            raise TypeError(f"Output.tone must be None or a ToneMap, got {type(tone).__name__}")
        object.__setattr__(self, "tone", tone)
        if isinstance(f, OutFormat) and f.subsampling != "444":          # each layout's own size rule; 4:4:4 takes any size
            odd = (lambda s: s[0] % 2 or s[1] % 2) if f.subsampling == "420" else (lambda s: s[1] % 2)
            needs = "4:2:0 ({}) needs an even height and width" if f.subsampling == "420" else "4:2:2 ({}) needs an even width"
            if self.resize is not None and odd(self.resize.size):
                raise ValueError(f"Output: {needs.format(f.layout)}, Resize.size is {self.resize.size}")
            if self.resize is None and self.warp is not None and odd(self.warp.size):
                raise ValueError(f"Output: {needs.format(f.layout)}, Warp.size is {self.warp.size} and no Resize follows it")

    def _key(self):
        return (self.format, self.resize, self.look, self.warp, self.sharpen, self.tone)

    def __eq__(self, other):
        return self._key() == other._key() if other.__class__ is self.__class__ else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Output(" + ", ".join(f"{n}={v!r}" for n, v in zip(("format", "resize", "look", "warp", "sharpen", "tone"), self._key())) + ")"

    def plan(self, h: int, w: int) -> Tuple[int, int]:
        """The (h, w) this output has for an (h, w) result; every refusal that depends on the frame is raised here, before any launch."""
        if self.warp is not None:
            self.warp.check_source(h, w)
            h, w = self.warp.size
        if self.resize is not None:
            self.resize.window(h, w)
            h, w = self.resize.size
        if self.tone is not None:
            self.tone.check(h, w)
        if isinstance(self.format, OutFormat):
            self.format.plane_layout(h, w)
        if isinstance(self.format, Jpeg):
            self.format.plan(h, w)
        if isinstance(self.format, (Stats, Motion)):
            self.format.check(h, w)
        return h, w
