"""Sensor calibration of forward_mosaic: what stands between the repaired samples and the normalised mosaic the network reads (Pwl, GainMap,
Calibration) -- linearisation, the levels, a flat-field gain map, white-balance gains, a clip (include/realcam_hip.h, rc_raw_calibrate, fixes
the arithmetic).

Pwl is a sensor's companding curve undone, GainMap a camera module's lens-shading calibration (kept on the host, copied to a device once),
Calibration the request: it rides in RawFormat(calibration=...).  Pure Python: validation raises ValueError / TypeError and never touches the
GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# The kernel's lane map (csrc/calibrate.hip): a lane holds LANE_PX consecutive samples of a row, a wave a strip of WAVE_SPAN columns, a block
# BLOCK_SPAN columns of BLOCK_ROWS rows.  Tests place widths and heights on these seams.
LANE_PX = 4
WAVE_SPAN = 64 * LANE_PX
BLOCK_SPAN = 2 * WAVE_SPAN
BLOCK_ROWS = 16
MAX_KNOTS = 16
CELLS = (8, 16, 32, 64, 128)


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _f32(v) -> float:
    with np.errstate(over="ignore"):            # a value past fp32's range becomes inf, which the callers refuse
        return float(np.float32(v))


@dataclass(frozen=True)
class Pwl:
    """A piecewise-linear curve through 2 to 16 knots: the linearisation of companded sensor codes.

    x   strictly increasing, in the storage's own units (codes).
    y   non-decreasing, in linear units -- RawFormat's black_level / white_level are in these units once a curve is set.
    Both are kept as fp32 values (what the kernel is given).  Segment j runs from knot j to knot j + 1 with the slope
    s_j = (y_{j+1} - y_j) / (x_{j+1} - x_j), formed in double and rounded to fp32 once; a sample c takes the last segment whose x_j <= c
    (a sample on a knot: the segment that starts there), and the end segments extrapolate.
    """

    x: Tuple[float, ...]
    y: Tuple[float, ...]

    def __post_init__(self):
        for name in ("x", "y"):
            v = getattr(self, name)
            if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or not all(_number(e) for e in v):
                raise TypeError(f"Pwl.{name} must be a sequence of numbers, got {v!r}")
        if len(self.x) != len(self.y):
            raise ValueError(f"Pwl: x and y must have the same length, got {len(self.x)} and {len(self.y)}")
        if not 2 <= len(self.x) <= MAX_KNOTS:
            raise ValueError(f"Pwl: 2 to {MAX_KNOTS} knots, got {len(self.x)}")
        if not all(math.isfinite(float(e)) for e in tuple(self.x) + tuple(self.y)):
            raise ValueError("Pwl: knots must be finite")
        x, y = tuple(_f32(e) for e in self.x), tuple(_f32(e) for e in self.y)
        if not all(math.isfinite(e) for e in x + y):
            raise ValueError("Pwl: knots must be finite in fp32")
        if not all(b > a for a, b in zip(x, x[1:])):
            raise ValueError(f"Pwl.x must be strictly increasing (as fp32), got {x}")
        if not all(b >= a for a, b in zip(y, y[1:])):
            raise ValueError(f"Pwl.y must be non-decreasing, got {y}")
        object.__setattr__(self, "x", x)
        object.__setattr__(self, "y", y)

    def slopes(self) -> Tuple[float, ...]:
        """s_j of the K - 1 segments, as fp32 values."""
        return tuple(_f32((self.y[j + 1] - self.y[j]) / (self.x[j + 1] - self.x[j])) for j in range(len(self.x) - 1))


def _size(what, size) -> Tuple[int, int]:
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in size):
        raise TypeError(f"{what}: size must be (H2, W2), two ints, got {size!r}")
    h2, w2 = size
    if h2 < 2 or w2 < 2 or h2 % 2 or w2 % 2:
        raise ValueError(f"{what}: a mosaic has an even, positive number of rows and columns, got {(h2, w2)}")
    return h2, w2


def _cell(cell) -> int:
    if not isinstance(cell, int) or isinstance(cell, bool):
        raise TypeError(f"GainMap: cell must be an int, got {cell!r}")
    if cell not in CELLS:
        raise ValueError(f"GainMap: cell must be one of {CELLS}, got {cell}")
    return cell


class GainMap:
    """A flat-field / lens-shading gain map (a DNG GainMap per CFA position): the normalised sample is multiplied by the bilinear
    interpolation of a coarse grid of gains.

    gains   (4, Gh, Gw) fp32, finite: plane p belongs to CFA position p = 2 (y & 1) + (x & 1), i.e. (0,0), (0,1), (1,0), (1,1).  Kept on the
            host, read-only.
    cell    8, 16, 32, 64 or 128: a node sits every `cell` samples of a position's own h x w plane (every 2 cell mosaic samples); node
            (j, i) is at plane sample (j cell, i cell).  A mosaic of (2h, 2w) needs Gh = ceil(h / cell) + 1, Gw = ceil(w / cell) + 1.
    Immutable; compared by identity.  device_gains(device) hands out the device copy, made once per device.
    """

    def __init__(self, gains, cell: int):
        import torch
        cell = _cell(cell)
        if isinstance(gains, np.ndarray):
            gains = torch.from_numpy(gains)
        if not isinstance(gains, torch.Tensor):
            raise TypeError(f"GainMap: gains must be a (4, Gh, Gw) fp32 tensor, got {type(gains).__name__}")
        if gains.dtype != torch.float32:
            raise TypeError(f"GainMap: gains must be fp32, got {gains.dtype}")
        if gains.dim() != 3 or gains.shape[0] != 4 or gains.shape[1] < 2 or gains.shape[2] < 2:
            raise ValueError(f"GainMap: gains must be (4, Gh, Gw) with Gh, Gw >= 2, got {tuple(gains.shape)}")
        gains = gains.detach().cpu().contiguous().clone()
        if not bool(torch.isfinite(gains).all()):
            raise ValueError("GainMap: gains must be finite")
        object.__setattr__(self, "gains", gains)
        object.__setattr__(self, "cell", cell)

    def __setattr__(self, name, value):
        raise AttributeError("GainMap is immutable")

    @staticmethod
    def nodes(size, cell: int) -> Tuple[int, int]:
        """(Gh, Gw) a (H2, W2) mosaic needs at this cell."""
        h2, w2 = _size("GainMap", size)
        cell = _cell(cell)
        return -(-(h2 // 2) // cell) + 1, -(-(w2 // 2) // cell) + 1

    def fits(self, h2: int, w2: int) -> bool:
        return tuple(self.gains.shape[1:]) == self.nodes((int(h2), int(w2)), self.cell)

    @classmethod
    def from_function(cls, size, cell: int, fn) -> "GainMap":
        """size (H2, W2) of the mosaic.  fn(pos, y, x) -> the gain of CFA position pos at the mosaic coordinates y (Gh, 1) and x (1, Gw) of
        that position's nodes (fp64 tensors; y = 2 j cell + (pos >> 1), x = 2 i cell + (pos & 1); the last nodes may lie past the frame)."""
        import torch
        gh, gw = cls.nodes(size, cell)
        planes = []
        for pos in range(4):
            y = (2 * cell * torch.arange(gh, dtype=torch.float64) + (pos >> 1)).view(gh, 1)
            x = (2 * cell * torch.arange(gw, dtype=torch.float64) + (pos & 1)).view(1, gw)
            g = torch.as_tensor(fn(pos, y, x), dtype=torch.float64)
            planes.append(g.expand(gh, gw).to(torch.float32))
        return cls(torch.stack(planes), cell)

    @classmethod
    def radial(cls, size, cell: int, centre=None, coeffs=(0.0,), cos4: Optional[float] = None) -> "GainMap":
        """A radial vignette correction about `centre` (y, x) in mosaic coordinates (default: the middle of the frame):
        gain = (1 + c1 r^2 + c2 r^4 + ...) and, with cos4 = a focal length in mosaic samples, times (1 + (d / cos4)^2)^2 -- the inverse
        of the cos^4 law.  r is the distance d from the centre over the half diagonal.  coeffs: (c1, c2, ...) for every position, or four
        such tuples in CFA-position order (colour shading)."""
        h2, w2 = _size("GainMap.radial", size)
        cy, cx = ((h2 - 1) / 2.0, (w2 - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
        per_pos = [tuple(coeffs)] * 4 if all(_number(c) for c in coeffs) else [tuple(c) for c in coeffs]
        if len(per_pos) != 4 or not all(_number(c) for t in per_pos for c in t):
            raise TypeError(f"GainMap.radial: coeffs must be numbers, or four tuples of numbers, got {coeffs!r}")
        if cos4 is not None and not (_number(cos4) and cos4 > 0 and math.isfinite(cos4)):
            raise ValueError(f"GainMap.radial: cos4 must be a positive focal length, got {cos4!r}")
        half2 = (h2 / 2.0) ** 2 + (w2 / 2.0) ** 2

        def fn(pos, y, x):
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            r2 = d2 / half2
            g, p = 1.0, r2
            for c in per_pos[pos]:
                g = g + float(c) * p
                p = p * r2
            if cos4 is not None:
                g = g * (1.0 + d2 / (float(cos4) ** 2)) ** 2
            return g

        return cls.from_function((h2, w2), cell, fn)

    def device_gains(self, device):
        """The map as a (4, Gh, Gw) fp32 tensor on `device`: uploaded once per device (ops.derived), then kept."""
        import torch
        from . import ops
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return ops.derived(self, ("device_gains", str(device)), (), lambda: self.gains.to(device))

    def __repr__(self):
        return f"GainMap(nodes={tuple(self.gains.shape[1:])}, cell={self.cell})"


@dataclass(frozen=True, eq=False)
class Calibration:
    """What to do to the samples before they are ingested: RawFormat(calibration=Calibration(...)) or ops.raw_calibrate.  In this order,
    each step skipped when it is None; the levels always apply:

    curve    a Pwl: l = y_j + (c - x_j) s_j, the companding undone.  RawFormat's levels are then in the curve's linear units.
    (levels) n = (l - black[pos]) / (white - black[pos]), RawFormat's own, exactly as the ingest forms it.
    shading  a GainMap of the mosaic's node count: n times the bilinear interpolation of the position's plane.
    gains    white-balance / digital gains in CFA-position order (0,0), (0,1), (1,0), (1,1), finite and >= 0: four host numbers, or a
             (1,4) / (B,4) fp32 tensor on the device, which the kernel reads when it runs -- an AWB / AE loop rewrites it in place without
             a host sync and a captured graph sees the new values on replay (its values are not checked).
    clip     (lo, hi), lo < hi: the result is clamped.
    At least one of the four must be set.  Frames holding NaN / Inf are outside the contract.  Compared by identity (a tensor may ride in it).
    """

    curve: Optional[Pwl] = None
    shading: Optional[GainMap] = None
    gains: Optional[object] = None
    clip: Optional[Tuple[float, float]] = None

    def __post_init__(self):
        import torch
        if self.curve is not None and not isinstance(self.curve, Pwl):
            raise TypeError(f"Calibration.curve must be None or a Pwl, got {type(self.curve).__name__}")
        if self.shading is not None and not isinstance(self.shading, GainMap):
            raise TypeError(f"Calibration.shading must be None or a GainMap, got {type(self.shading).__name__}")
        g = self.gains
        if isinstance(g, torch.Tensor):
            if g.dtype != torch.float32:
                raise TypeError(f"Calibration.gains: a tensor must be fp32, got {g.dtype}")
            if g.dim() != 2 or g.shape[1] != 4 or g.shape[0] < 1:
                raise ValueError(f"Calibration.gains: a tensor must be (1,4) or (B,4), got {tuple(g.shape)}")
        elif g is not None:
            if isinstance(g, (str, bytes)) or not hasattr(g, "__len__") or len(g) != 4 or not all(_number(v) for v in g):
                raise TypeError(f"Calibration.gains must be None, four numbers in CFA-position order or a (B,4) tensor, got {g!r}")
            g = tuple(_f32(v) for v in g)
            if not all(math.isfinite(v) and v >= 0.0 for v in g):
                raise ValueError(f"Calibration.gains must be finite and >= 0, got {g}")
            object.__setattr__(self, "gains", g)
        c = self.clip
        if c is not None:
            if isinstance(c, (str, bytes)) or not hasattr(c, "__len__") or len(c) != 2 or not all(_number(v) for v in c):
                raise TypeError(f"Calibration.clip must be None or (lo, hi), got {c!r}")
            c = (_f32(c[0]), _f32(c[1]))
            if not (math.isfinite(c[0]) and math.isfinite(c[1]) and c[0] < c[1]):
                raise ValueError(f"Calibration.clip needs finite lo < hi, got {c}")
            object.__setattr__(self, "clip", c)
        if self.curve is None and self.shading is None and self.gains is None and self.clip is None:
            raise ValueError("Calibration: nothing enabled -- give a curve, shading, gains or clip")

    @property
    def device_gains(self) -> bool:
        """The gains are a device tensor (read by the kernel), not four host numbers."""
        return self.gains is not None and not isinstance(self.gains, tuple)

    def check(self, h2: int, w2: int, batch: Optional[int] = None) -> None:
        """Refuse a gain map whose node count does not fit the mosaic, and a gains tensor with the wrong number of rows."""
        if self.shading is not None and not self.shading.fits(h2, w2):
            want = GainMap.nodes((int(h2), int(w2)), self.shading.cell)
            raise ValueError(f"Calibration: the gain map has {tuple(self.shading.gains.shape[1:])} nodes per position, a {(int(h2), int(w2))} mosaic at "
                             f"cell {self.shading.cell} needs {want}")
        if batch is not None and self.device_gains and self.gains.shape[0] not in (1, int(batch)):
            raise ValueError(f"Calibration.gains: {self.gains.shape[0]} rows for a batch of {int(batch)} (1 or the batch)")
