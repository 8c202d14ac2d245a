"""Geometric correction for forward_mosaic's outputs: `Warp`, a coarse mesh of source positions that ops.warp resamples the float result
through (include/realcam_hip.h, rc_warp) -- lens distortion correction, a 90 degree orientation, a flip.

Pure Python and NumPy: construction and validation raise ValueError / TypeError and never touch the GPU or the library.
"""
from __future__ import annotations

import hashlib
import math
from typing import Optional, Tuple

import numpy as np

from . import _lib

CELLS = tuple(1 << k for k in range(_lib.RC_WARP_MIN_CELL_LOG2, _lib.RC_WARP_MAX_CELL_LOG2 + 1))
INTERPS = {"bilinear": _lib.RC_WARP_BILINEAR, "bicubic": _lib.RC_WARP_BICUBIC}
BORDERS = {"clamp": _lib.RC_WARP_CLAMP, "constant": _lib.RC_WARP_CONSTANT}
MAX_DIM = _lib.RC_WARP_MAX_DIM


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _hw(what: str, v, none_ok: bool = False):
    if v is None and none_ok:
        return None
    if not isinstance(v, (tuple, list)) or len(v) != 2 or not all(_is_int(x) for x in v) or min(v) < 1 or max(v) > MAX_DIM:
        raise ValueError(f"Warp.{what} must be (h, w) with integers in 1 .. {MAX_DIM}{' or None' if none_ok else ''}, got {v!r}")
    return int(v[0]), int(v[1])


def _cell(cell) -> int:
    if not _is_int(cell) or int(cell) not in CELLS:
        raise ValueError(f"Warp.cell must be one of {CELLS}, got {cell!r}")
    return int(cell)


def mesh_shape(size: Tuple[int, int], cell: int) -> Tuple[int, int]:
    """(Gh, Gw) of the mesh of an (oh, ow) output: a node every `cell` pixels and one more, so that the last cell has both its ends."""
    return -(-size[0] // cell) + 1, -(-size[1] // cell) + 1


class Warp:
    """An immutable resampling of the cropped network result through a coarse mesh.

    mesh    array-like (Gh, Gw, 2) fp32, every value finite, Gh = ceil(oh / cell) + 1 and Gw = ceil(ow / cell) + 1: mesh[j, i] = (sx, sy) is
            the source position sampled by output pixel (x, y) = (i cell, j cell), in pixels of the cropped result, an integer at a pixel's
            centre; between nodes the position is interpolated bilinearly.  The last node may lie beyond the output.
    size    (oh, ow) of the output, any size >= 1: upscaling is allowed here.
    cell    8, 16, 32 or 64 output pixels between nodes.
    interp  "bilinear" or "bicubic" (A = -0.75: F.grid_sample's and OpenCV's).
    border  "clamp" (a tap outside the frame reads the nearest pixel) or "constant" (it is `fill`).
    fill    (R, G, B), three finite floats, used by "constant".
    source  None, or the (h, w) of the frame the mesh was made for: Output.plan and ops.warp refuse any other frame.
    Equal and hashed by content (every field and a digest of the mesh's bytes, computed once): a Warp keys the device-mesh cache of
    ops.warp and sits inside the frozen Output.
    """

    __slots__ = ("_mesh", "_size", "_cell", "_interp", "_border", "_fill", "_source", "_digest")

    def __init__(self, mesh, size, cell: int = 16, interp: str = "bilinear", border: str = "clamp", fill=(0, 0, 0), source=None):
        size = _hw("size", size)
        cell = _cell(cell)
        if not isinstance(interp, str) or interp not in INTERPS:
            raise ValueError(f"Warp.interp must be one of {sorted(INTERPS)}, got {interp!r}")
        if not isinstance(border, str) or border not in BORDERS:
            raise ValueError(f"Warp.border must be one of {sorted(BORDERS)}, got {border!r}")
        if not isinstance(fill, (tuple, list)) or len(fill) != 3 or not all(_is_real(v) for v in fill):
            raise TypeError(f"Warp.fill must be three real numbers (R, G, B), got {fill!r}")
        with np.errstate(over="ignore"):
            fill = tuple(float(np.float32(v)) for v in fill)             # as the kernel gets them
        if not all(math.isfinite(v) for v in fill):
            raise ValueError(f"Warp.fill must be finite (within fp32), got {fill!r}")
        source = _hw("source", source, none_ok=True)
        if isinstance(mesh, (str, bytes)) or mesh is None:
            raise TypeError(f"Warp.mesh must be array-like of shape (Gh, Gw, 2), got {type(mesh).__name__}")
        try:
            a = np.asarray(mesh)
        except Exception as e:                                           # ragged lists and the like
            raise TypeError(f"Warp.mesh must be array-like of shape (Gh, Gw, 2): {e}") from None
        if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"Warp.mesh must hold real numbers, got dtype {a.dtype}")
        want = (*mesh_shape(size, cell), 2)
        if a.shape != want:
            raise ValueError(f"Warp.mesh must have shape {want} for size {size} at cell {cell} (ceil(size / cell) + 1 nodes per axis), got {a.shape}")
        with np.errstate(over="ignore"):
            m = np.array(a, dtype=np.float32, order="C", copy=True)      # the private copy; a double beyond fp32 becomes inf and is refused
        if not np.isfinite(m).all():
            raise ValueError("Warp.mesh must be finite (no NaN, no infinity, nothing beyond fp32)")
        m.flags.writeable = False
        h = hashlib.sha256(repr((size, cell, interp, border, fill, source)).encode())
        h.update(m.tobytes())
        for name, v in (("_mesh", m), ("_size", size), ("_cell", cell), ("_interp", interp), ("_border", border), ("_fill", fill), ("_source", source),
                        ("_digest", h.digest())):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("Warp is immutable")

    def __delattr__(self, name):
        raise AttributeError("Warp is immutable")

    mesh = property(lambda self: self._mesh, doc="The (Gh, Gw, 2) fp32 mesh, read-only.")
    size = property(lambda self: self._size)
    cell = property(lambda self: self._cell)
    interp = property(lambda self: self._interp)
    border = property(lambda self: self._border)
    fill = property(lambda self: self._fill)
    source = property(lambda self: self._source)

    def __eq__(self, other):
        if not isinstance(other, Warp):
            return NotImplemented
        return self._digest == other._digest

    def __hash__(self):
        return hash(self._digest)

    def __repr__(self):
        return (f"Warp(size={self._size}, cell={self._cell}, interp={self._interp!r}, border={self._border!r}, fill={self._fill}, source={self._source}, "
                f"sha256={self._digest.hex()[:12]})")

    def check_source(self, h: int, w: int) -> None:
        """Refuse a frame other than the one the mesh was made for."""
        if self._source is not None and self._source != (int(h), int(w)):
            raise ValueError(f"Warp.source is {self._source}: the mesh was made for that frame, not for ({h}, {w})")

    # ---- constructors: float64 throughout, rounded to fp32 once ---------------------------------------------------------------------------
    @classmethod
    def from_function(cls, size, fn, cell: int = 16, **kw) -> "Warp":
        """The mesh of fn(xo, yo) -> (sx, sy), evaluated on float64 arrays (Gh, Gw) of the nodes' output positions xo = i cell, yo = j cell."""
        size, cell = _hw("size", size), _cell(cell)
        if not callable(fn):
            raise TypeError(f"Warp.from_function: fn must be callable, got {type(fn).__name__}")
        gh, gw = mesh_shape(size, cell)
        yo, xo = np.meshgrid(np.arange(gh, dtype=np.float64) * cell, np.arange(gw, dtype=np.float64) * cell, indexing="ij")
        out = fn(xo, yo)
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("Warp.from_function: fn must return the pair (sx, sy)")
        try:
            sx, sy = (np.broadcast_to(np.asarray(v, dtype=np.float64), (gh, gw)) for v in out)
        except (ValueError, TypeError) as e:
            raise ValueError(f"Warp.from_function: fn's results must be real and broadcast to the nodes' shape {(gh, gw)}: {e}") from None
        return cls(np.stack([sx, sy], axis=-1), size, cell, **kw)

    @classmethod
    def identity(cls, size, cell: int = 16, **kw) -> "Warp":
        """Every output pixel samples the source pixel of the same index."""
        return cls.from_function(size, lambda x, y: (x, y), cell, **kw)

    @classmethod
    def rotate90(cls, source, k: int = 1, cell: int = 16, **kw) -> "Warp":
        """torch.rot90(frame, k, dims=(-2, -1)) of an (h, w) source: k quarter turns counter-clockwise; odd k gives a (w, h) output."""
        h, w = _hw("source", source)
        if not _is_int(k):
            raise TypeError(f"Warp.rotate90: k must be an int, got {type(k).__name__}")
        fn = (lambda x, y: (x, y), lambda x, y: (w - 1 - y, x), lambda x, y: (w - 1 - x, h - 1 - y), lambda x, y: (y, h - 1 - x))[int(k) % 4]
        return cls.from_function((w, h) if int(k) % 2 else (h, w), fn, cell, source=(h, w), **kw)

    @classmethod
    def flip(cls, source, horizontal: bool = True, cell: int = 16, **kw) -> "Warp":
        """torch.flip of an (h, w) source along its width (horizontal) or its height."""
        h, w = _hw("source", source)
        fn = (lambda x, y: (w - 1 - x, y)) if horizontal else (lambda x, y: (x, h - 1 - y))
        return cls.from_function((h, w), fn, cell, source=(h, w), **kw)

    @staticmethod
    def lens_function(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, out_fx=None, out_fy=None, out_cx=None, out_cy=None):
        """fn(xo, yo) -> (sx, sy) of the radial-tangential lens model, evaluated forward: the output pixel normalised with the out_*
        intrinsics (default: the source's), distorted, projected with the source intrinsics."""
        vals = dict(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, k3=k3, p1=p1, p2=p2)
        outs = dict(out_fx=fx if out_fx is None else out_fx, out_fy=fy if out_fy is None else out_fy, out_cx=cx if out_cx is None else out_cx,
                    out_cy=cy if out_cy is None else out_cy)
        for name, v in {**vals, **outs}.items():
            if not _is_real(v) or not math.isfinite(v):
                raise ValueError(f"Warp.lens: {name} must be a finite real number, got {v!r}")
        for name in ("fx", "fy"):
            if vals[name] == 0 or outs["out_" + name] == 0:
                raise ValueError(f"Warp.lens: {name} and out_{name} must not be zero")
        ofx, ofy, ocx, ocy = (float(outs[n]) for n in ("out_fx", "out_fy", "out_cx", "out_cy"))

        def fn(xo, yo):
            xn, yn = (xo - ocx) / ofx, (yo - ocy) / ofy
            r2 = xn * xn + yn * yn
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = xn * radial + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
            yd = yn * radial + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
            return fx * xd + cx, fy * yd + cy
        return fn

    @classmethod
    def lens(cls, size, source, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, out_fx=None, out_fy=None, out_cx=None, out_cy=None,
             cell: int = 16, **kw) -> "Warp":
        """Lens distortion correction: the (oh, ow) output is the ideal pinhole image with the out_* intrinsics, the (h, w) source the
        distorted frame with intrinsics fx, fy, cx, cy and coefficients k1, k2, k3 (radial), p1, p2 (tangential) -- OpenCV's model and
        order of terms.  No inversion is needed: the mesh maps output pixels to source positions."""
        return cls.from_function(size, cls.lens_function(fx, fy, cx, cy, k1, k2, k3, p1, p2, out_fx, out_fy, out_cx, out_cy), cell,
                                 source=_hw("source", source), **kw)

    # ---- what a mesh of this cell loses ---------------------------------------------------------------------------------------------------
    def positions(self, xo, yo):
        """(sx, sy) in float64 at output positions xo, yo (arrays, 0 <= xo <= ow - 1, 0 <= yo <= oh - 1; fractions allowed): the mesh's
        bilinear interpolation without fp32's roundings."""
        xo, yo = np.asarray(xo, dtype=np.float64), np.asarray(yo, dtype=np.float64)
        gh, gw = self._mesh.shape[:2]
        i = np.clip(np.floor(xo / self._cell).astype(np.int64), 0, gw - 2)
        j = np.clip(np.floor(yo / self._cell).astype(np.int64), 0, gh - 2)
        u, v = (xo / self._cell - i)[..., None], (yo / self._cell - j)[..., None]
        m = self._mesh.astype(np.float64)
        s = (1 - v) * ((1 - u) * m[j, i] + u * m[j, i + 1]) + v * ((1 - u) * m[j + 1, i] + u * m[j + 1, i + 1])
        return s[..., 0], s[..., 1]

    def residual(self, fn) -> float:
        """The largest distance in source pixels between fn and the mesh's bilinear interpolation, over the cells' centres and the
        midpoints of their edges (those inside the output): what a mesh of this cell loses against fn.  Choose the cell by it."""
        gh, gw = self._mesh.shape[:2]
        half = self._cell / 2.0
        a, b = np.meshgrid(np.arange(2 * gh - 1), np.arange(2 * gw - 1), indexing="ij")            # half-cell steps: both even is a node
        keep = ((a % 2 == 1) | (b % 2 == 1)) & (a * half <= self._size[0] - 1) & (b * half <= self._size[1] - 1)
        if not keep.any():
            return 0.0
        yo, xo = a[keep] * half, b[keep] * half
        sx, sy = self.positions(xo, yo)
        fx, fy = fn(xo, yo)
        return float(np.max(np.hypot(sx - np.asarray(fx, dtype=np.float64), sy - np.asarray(fy, dtype=np.float64))))

    def packed(self) -> np.ndarray:
        """The mesh as rc_warp reads it: (1, Gh, Gw, 2) fp32, contiguous."""
        return np.array(self._mesh[None], order="C")                  # a writable copy: torch.from_numpy wants one
