"""RAW-domain 3A statistics of forward_mosaic: what to measure on the sensor mosaic (RawStats) and what comes back (RawFrameStats).

RawStats describes the request -- the code depth, the histogram's bins, the sample value that maps to full scale, the region of interest and
the zone grid in Bayer cells, and the two cell-class thresholds; RawFrameStats holds the two int64 device tensors rc_raw_stats writes
(include/realcam_hip.h fixes the arithmetic) and derives the three control inputs an AE / AWB loop needs from them on the device, so a
measurement can go into Calibration.gains / Exposures.times / Temporal.gain without the host seeing it.  Pure Python: no kernel, no library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

from . import _lib
from .stats import zone_bounds

MAX_GRID = _lib.RC_RAW_STATS_MAX_GRID
MAX_HIST_BITS = _lib.RC_RAW_STATS_MAX_HIST_BITS
SLOTS = ("valid", "sum_r", "sum_g1", "sum_g2", "sum_b", "saturated", "dark", "focus")     # zones[..., k]
COLOURS = ("r", "g1", "g2", "b")                                                            # hist[:, c]: the packed map's slots, Calibration.gains' order


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"RawStats.{name} must be an int, got {v!r}")
    return v


@dataclass(frozen=True)
class RawStats:
    """Histograms and a 3A zone grid of the sensor mosaic per CFA colour: RawFormat(stats=RawStats(...)) or ops.raw_stats(mosaic, fmt, RawStats(...)).

    grid       (gy, gx) zones, 1 .. 64 per axis and at most the measured region's side in cells.
    bits       8 .. 16: the codes are clamp(rint((v - black) S / (top - black)), 0, S) with S = 2**bits - 1.
    hist_bits  6 .. min(bits, 10): a histogram has 2**hist_bits bins, bin = code >> (bits - hist_bits).
    roi        None (the whole frame) or (cy0, cx0, rh, rw) in Bayer cells inside it.
    top        None (the format's white level) or the sample value that maps to S; it must exceed every black level.  With top - black = S
               (black 0, top 1023, bits 10) the codes are the sensor's own.
    sat        None (nothing is saturated) or a code 1 .. S: a cell is saturated if the largest of its four codes is >= sat.
    dark       None (nothing is dark) or a code 0 .. S: a cell that is not saturated is dark if that largest code is <= dark.
    """

    grid: Tuple[int, int] = (16, 16)
    bits: int = 10
    hist_bits: int = 8
    roi: Optional[Tuple[int, int, int, int]] = None
    top: Optional[float] = None
    sat: Optional[int] = None
    dark: Optional[int] = None

    def __post_init__(self):
        if not 8 <= _int("bits", self.bits) <= 16:
            raise ValueError(f"RawStats.bits must lie in 8 .. 16, got {self.bits}")
        if not 6 <= _int("hist_bits", self.hist_bits) <= min(self.bits, MAX_HIST_BITS):
            raise ValueError(f"RawStats.hist_bits must lie in 6 .. min(bits, {MAX_HIST_BITS}), got {self.hist_bits} at bits {self.bits}")
        if not isinstance(self.grid, (tuple, list)) or len(self.grid) != 2:
            raise TypeError(f"RawStats.grid must be (gy, gx), got {self.grid!r}")
        grid = tuple(_int("grid", v) for v in self.grid)
        if not all(1 <= v <= MAX_GRID for v in grid):
            raise ValueError(f"RawStats.grid must lie in 1 .. {MAX_GRID} per axis, got {grid}")
        object.__setattr__(self, "grid", grid)
        if self.roi is not None:
            if not isinstance(self.roi, (tuple, list)) or len(self.roi) != 4:
                raise TypeError(f"RawStats.roi must be None or (cy0, cx0, rh, rw) in cells, got {self.roi!r}")
            roi = tuple(_int("roi", v) for v in self.roi)
            if roi[0] < 0 or roi[1] < 0 or roi[2] < 1 or roi[3] < 1:
                raise ValueError(f"RawStats.roi must have cy0, cx0 >= 0 and rh, rw >= 1, got {roi}")
            if grid[0] > roi[2] or grid[1] > roi[3]:
                raise ValueError(f"RawStats.grid {grid} has more zones than the roi {roi} has cell rows or columns")
            object.__setattr__(self, "roi", roi)
        if self.top is not None:
            if isinstance(self.top, bool) or not isinstance(self.top, (int, float)):
                raise TypeError(f"RawStats.top must be None or a number, got {self.top!r}")
            if not math.isfinite(self.top):
                raise ValueError(f"RawStats.top must be finite, got {self.top!r}")
            object.__setattr__(self, "top", float(self.top))
        if self.sat is not None and not 1 <= _int("sat", self.sat) <= self.codes:
            raise ValueError(f"RawStats.sat must be None or lie in 1 .. {self.codes}, got {self.sat}")
        if self.dark is not None and not -1 <= _int("dark", self.dark) <= self.codes - 1:
            raise ValueError(f"RawStats.dark must be None or lie in -1 .. {self.codes - 1}, got {self.dark}")

    @property
    def codes(self) -> int:
        """2**bits: the number of codes."""
        return 1 << self.bits

    @property
    def bins(self) -> int:
        """2**hist_bits: the length of a histogram."""
        return 1 << self.hist_bits

    @property
    def sat_code(self) -> int:
        return self.codes if self.sat is None else self.sat

    @property
    def dark_code(self) -> int:
        return -1 if self.dark is None else self.dark

    def top_value(self, white_level: float, blacks) -> float:
        """The sample value that maps to S for a format with these levels; refuses one at or below a black level."""
        top = float(white_level) if self.top is None else self.top
        if not math.isfinite(top) or not all(top > float(b) for b in blacks):
            raise ValueError(f"RawStats: top ({top!r}) must be finite and exceed every black level {tuple(blacks)}")
        return top

    def check(self, h_cells: int, w_cells: int) -> Tuple[int, int, int, int]:
        """The region (cy0, cx0, rh, rw) measured in a frame of (h_cells, w_cells) Bayer cells; every refusal that depends on the frame is
        raised here, before any launch."""
        h, w = int(h_cells), int(w_cells)
        if h < 1 or w < 1:
            raise ValueError(f"RawStats: the frame of {(h, w)} cells is empty")
        if 4 * h * w >= 1 << 31:
            raise ValueError(f"RawStats: a mosaic of {(2 * h, 2 * w)} has 2^31 samples or more")
        cy0, cx0, rh, rw = self.roi if self.roi is not None else (0, 0, h, w)
        if cy0 + rh > h or cx0 + rw > w:
            raise ValueError(f"RawStats: the roi {self.roi} lies outside the frame of {(h, w)} cells")
        if self.grid[0] > rh or self.grid[1] > rw:
            raise ValueError(f"RawStats: the grid {self.grid} has more zones than the measured region {(rh, rw)} has cell rows or columns")
        return cy0, cx0, rh, rw


class RawFrameStats:
    """The RAW-domain statistics of a batch of frames (ops.raw_stats, net.raw_stats after forward_mosaic with RawFormat.stats).

    hist   (B, 4, 2**hist_bits) int64 on the device: per colour R, G1 (G of the R row), G2 (G of the B row), B the number of measured
           samples in each bin.
    zones  (B, gy, gx, 8) int64 on the device: per zone the slots of raw_stats.SLOTS -- valid cells, the sums of qR, qG1, qG2, qB over
           them, saturated cells, dark cells, the focus figure (forward-difference gradient energy of the cells' green).
    spec   the RawStats that asked;  roi  the (cy0, cx0, rh, rw) measured, in cells.
    The colour order is Calibration.gains' order, so a result feeds the gains tensor as it is.
    """

    __slots__ = ("hist", "zones", "spec", "roi")

    def __init__(self, hist, zones, spec: RawStats, roi):
        self.hist, self.zones, self.spec, self.roi = hist, zones, spec, tuple(int(v) for v in roi)

    @property
    def zone_pixels(self):
        """(gy, gx) int64 on the host: the cells of each zone, from the geometry alone (slots valid + saturated + dark of any frame)."""
        import torch
        by, bx = zone_bounds(self.roi[2], self.spec.grid[0]), zone_bounds(self.roi[3], self.spec.grid[1])
        rows = torch.tensor([b - a for a, b in zip(by, by[1:])], dtype=torch.int64)
        cols = torch.tensor([b - a for a, b in zip(bx, bx[1:])], dtype=torch.int64)
        return rows[:, None] * cols[None, :]

    def _sums(self):
        import torch
        return self.zones[..., 1:5].sum((1, 2)).to(torch.float64), self.zones[..., 0].sum((1, 2)).to(torch.float64)

    def mean_level(self):
        """(B, 4) float64 on the device, 0 .. 1: per colour the mean code of the valid cells in units of full scale S (what an AE loop holds
        at its set point); 0 where no cell is valid.  No synchronisation."""
        import torch
        s, n = self._sums()
        n = n[:, None] * float(self.spec.codes - 1)
        return torch.where(n == 0, torch.zeros_like(s), s / torch.where(n == 0, torch.ones_like(n), n))

    def awb_gains(self):
        """(B, 4) float32 on the device: grey-world gains (g / sum qR, 1, 1, g / sum qB) over the valid cells with g = (sum qG1 + sum qG2) / 2;
        a colour whose sum is zero keeps the gain 1.  Ready for calibration.gains.copy_(...) or .lerp_(...).  No synchronisation."""
        import torch
        s, _ = self._sums()
        g = ((s[:, 1] + s[:, 2]) * 0.5)[:, None].expand(-1, 4)
        one = torch.ones_like(s)
        gains = torch.where(s == 0, one, g / torch.where(s == 0, one, s))
        gains[:, 1:3] = 1.0
        return gains.to(torch.float32)

    def saturated_fraction(self):
        """(B,) float64 on the device, 0 .. 1: the share of the region's cells that are saturated.  No synchronisation."""
        import torch
        return self.zones[..., 5].sum((1, 2)).to(torch.float64) / float(self.roi[2] * self.roi[3])

    def __repr__(self):
        return f"RawFrameStats(hist={tuple(self.hist.shape)}, zones={tuple(self.zones.shape)}, roi={self.roi}, spec={self.spec!r})"
