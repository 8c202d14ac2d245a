"""Lateral chromatic aberration correction of forward_mosaic: the R and B samples of the mosaic resampled inside their own colour's plane
through a coarse mesh of shifts (Aberration) -- the last box of the input side, between the calibration and the ingest
(include/realcam_hip.h, rc_raw_aberration, fixes the arithmetic).

A lens images red and blue at a slightly different magnification than green.  The calibration is a mesh of (dx, dy) per colour, in samples
of the colour's own plane, as chart tools deliver it, or DNG WarpRectilinear's radial terms per plane (Aberration.radial).  Pure Python:
validation raises ValueError / TypeError and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

from .calibration import CELLS, GainMap, _size

# The kernel's tile (csrc/aberration.hip): a lane holds LANE_PX consecutive samples of a row, a block a tile of TILE_CELLS x TILE_CELLS Bayer
# cells (BLOCK_SPAN mosaic columns of BLOCK_ROWS mosaic rows) plus a halo of reach + 2 (bicubic) or reach + 1 (bilinear) plane samples.  Tests
# place widths, heights and shifts on these seams.
LANE_PX = 4
TILE_CELLS = 32
BLOCK_SPAN = 2 * TILE_CELLS
BLOCK_ROWS = 2 * TILE_CELLS
MAX_REACH = 8
INTERPS = ("bilinear", "bicubic")


def _cell(cell) -> int:
    if not isinstance(cell, int) or isinstance(cell, bool):
        raise TypeError(f"Aberration: cell must be an int, got {cell!r}")
    if cell not in CELLS:
        raise ValueError(f"Aberration: cell must be one of {CELLS}, got {cell}")
    return cell


class Aberration:
    """The lateral chromatic aberration calibration of a lens: RawFormat(aberration=Aberration(...)) or ops.raw_aberration.

    red, blue   (Gh, Gw, 2) fp32 arrays (NumPy or torch) of (dx, dy), or None for zeros (that colour is left exactly as it is): output sample
                (Y, X) of the colour's own h x w plane takes the source at (X + dx, Y + dy), in samples of that plane -- one unit is two
                mosaic samples.  Node (j, i) belongs to plane sample (j cell, i cell); a (2h, 2w) mosaic needs Gh = ceil(h / cell) + 1,
                Gw = ceil(w / cell) + 1, which is GainMap's node count.  Between the nodes the shift is interpolated bilinearly.
    cell        8, 16, 32, 64 or 128.
    interp      "bicubic" (A = -0.75, Warp's kernel) or "bilinear".
    reach       max(1, ceil(max |d|)) over all nodes: what the kernel stages around its tile.  A mesh with a non-finite node or a reach
                above 8 is refused here.  G is never moved.
    Immutable; compared by identity.  device_shift(device) hands out the (2, Gh, Gw, 2) device copy, made once per device.
    """

    def __init__(self, red=None, blue=None, cell: int = 32, interp: str = "bicubic"):
        import torch
        cell = _cell(cell)
        if not isinstance(interp, str) or interp not in INTERPS:
            raise ValueError(f"Aberration: interp must be one of {INTERPS}, got {interp!r}")
        if red is None and blue is None:
            raise ValueError("Aberration: give red, blue or both (a colour left None is not moved)")
        planes = []
        for name, m in (("red", red), ("blue", blue)):
            if m is None:
                planes.append(None)
                continue
            if isinstance(m, np.ndarray):
                m = torch.from_numpy(np.ascontiguousarray(m))
            if not isinstance(m, torch.Tensor):
                raise TypeError(f"Aberration: {name} must be None or a (Gh, Gw, 2) fp32 array, got {type(m).__name__}")
            if m.dtype != torch.float32:
                raise TypeError(f"Aberration: {name} must be fp32, got {m.dtype}")
            if m.dim() != 3 or m.shape[2] != 2 or m.shape[0] < 2 or m.shape[1] < 2:
                raise ValueError(f"Aberration: {name} must be (Gh, Gw, 2) with Gh, Gw >= 2, got {tuple(m.shape)}")
            m = m.detach().cpu().contiguous().clone()
            if not bool(torch.isfinite(m).all()):
                raise ValueError(f"Aberration: {name} holds a node that is not finite")
            planes.append(m)
        if planes[0] is not None and planes[1] is not None and planes[0].shape != planes[1].shape:
            raise ValueError(f"Aberration: red and blue must have one node count, got {tuple(planes[0].shape)} and {tuple(planes[1].shape)}")
        shape = next(p.shape for p in planes if p is not None)
        shift = torch.stack([torch.zeros(shape, dtype=torch.float32) if p is None else p for p in planes])
        reach = max(1, int(math.ceil(float(shift.abs().max()))))
        if reach > MAX_REACH:
            raise ValueError(f"Aberration: the largest shift is {float(shift.abs().max()):.3f} samples of a colour's plane; the stage corrects up to "
                             f"{MAX_REACH} (a reach of {reach})")
        object.__setattr__(self, "shift", shift)
        object.__setattr__(self, "cell", cell)
        object.__setattr__(self, "interp", interp)
        object.__setattr__(self, "reach", reach)

    def __setattr__(self, name, value):
        raise AttributeError("Aberration is immutable")

    @property
    def red(self):
        return self.shift[0]

    @property
    def blue(self):
        return self.shift[1]

    @property
    def code(self) -> int:
        from . import _lib
        return _lib.RC_WARP_BICUBIC if self.interp == "bicubic" else _lib.RC_WARP_BILINEAR

    @staticmethod
    def nodes(size, cell: int) -> Tuple[int, int]:
        """(Gh, Gw) a (H2, W2) mosaic needs at this cell: GainMap's."""
        _size("Aberration", size)
        return GainMap.nodes(size, _cell(cell))

    def fits(self, h2: int, w2: int) -> bool:
        return tuple(self.shift.shape[1:3]) == self.nodes((int(h2), int(w2)), self.cell)

    def check(self, h2: int, w2: int) -> None:
        """Refuse a mesh whose node count does not fit the (h2, w2) mosaic."""
        if not self.fits(h2, w2):
            raise ValueError(f"Aberration: the mesh has {tuple(self.shift.shape[1:3])} nodes per colour, a {(int(h2), int(w2))} mosaic at cell "
                             f"{self.cell} needs {self.nodes((int(h2), int(w2)), self.cell)}")

    @classmethod
    def from_function(cls, size, fn, cell: int = 32, interp: str = "bicubic") -> "Aberration":
        """size (H2, W2) of the mosaic.  fn(colour, y, x) -> (dx, dy) of colour "red" / "blue" at the plane coordinates y (Gh, 1) and x
        (1, Gw) of the nodes (fp64 tensors: y = j cell, x = i cell; the last nodes may lie past the plane), in samples of the colour's
        plane; None for a colour that is not moved.  Evaluated in float64, rounded to fp32 once."""
        import torch
        gh, gw = cls.nodes(size, cell)
        y = (cell * torch.arange(gh, dtype=torch.float64)).view(gh, 1)
        x = (cell * torch.arange(gw, dtype=torch.float64)).view(1, gw)
        planes = []
        for colour in ("red", "blue"):
            d = fn(colour, y, x)
            if d is None:
                planes.append(None)
                continue
            dx, dy = d
            dx = torch.as_tensor(dx, dtype=torch.float64).expand(gh, gw)
            dy = torch.as_tensor(dy, dtype=torch.float64).expand(gh, gw)
            planes.append(torch.stack([dx, dy], dim=-1).to(torch.float32))
        return cls(planes[0], planes[1], cell, interp)

    @classmethod
    def radial(cls, size, red=None, blue=None, centre=(0.5, 0.5), cell: int = 32, interp: str = "bicubic") -> "Aberration":
        """DNG WarpRectilinear's radial form per plane: red / blue = (kr0, kr1, kr2, kr3), or None for a plane that is not moved.  With the
        centre (cx, cy) in DNG's normalised coordinates (0 .. 1 across the frame, x first) and r the distance of a photosite from it over
        the largest distance from the centre to a corner, the source lies at radius r (kr0 + kr1 r^2 + kr2 r^4 + kr3 r^6) along the same
        ray.  Evaluated at each node's photosite position in float64, rounded to fp32 once; kr = (1, 0, 0, 0) gives zeros."""
        h2, w2 = _size("Aberration.radial", size)
        for name, k in (("red", red), ("blue", blue)):
            if k is not None and (isinstance(k, (str, bytes)) or not hasattr(k, "__len__") or len(k) != 4
                                  or not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in k)):
                raise TypeError(f"Aberration.radial: {name} must be None or four numbers (kr0, kr1, kr2, kr3), got {k!r}")
        cx, cy = float(centre[0]) * (w2 - 1), float(centre[1]) * (h2 - 1)         # the centre in mosaic samples, as DNG maps 0 .. 1
        rmax = math.sqrt(max(cx, w2 - 1 - cx) ** 2 + max(cy, h2 - 1 - cy) ** 2)
        ks = {"red": red, "blue": blue}

        def fn(colour, y, x):
            k = ks[colour]
            if k is None:
                return None
            # node (j, i) stands for the colour's photosite of cell (j cell, i cell); the half-sample offset of a colour inside its cell is
            # below what the coarse mesh resolves and both colours take the cell's centre
            my, mx = 2.0 * y + 0.5 - cy, 2.0 * x + 0.5 - cx
            r2 = (my * my + mx * mx) / (rmax * rmax)
            f = float(k[0]) + float(k[1]) * r2 + float(k[2]) * r2 * r2 + float(k[3]) * r2 * r2 * r2
            return mx * (f - 1.0) / 2.0, my * (f - 1.0) / 2.0                      # mosaic samples -> samples of the colour's plane

        return cls.from_function((h2, w2), fn, cell, interp)

    def device_shift(self, device):
        """The mesh as a (2, Gh, Gw, 2) fp32 tensor on `device`: uploaded once per device (ops.derived), then kept."""
        import torch
        from . import ops
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return ops.derived(self, ("device_shift", str(device)), (), lambda: self.shift.to(device))

    def __repr__(self):
        return f"Aberration(nodes={tuple(self.shift.shape[1:3])}, cell={self.cell}, interp={self.interp!r}, reach={self.reach})"
