"""Frame statistics of forward_mosaic: what to measure (Stats) and what comes back (FrameStats).

Stats describes the request -- the code depth, the luma matrix, the region of interest, the 3A zone grid and the two pixel-class thresholds;
FrameStats holds the two int64 device tensors rc_frame_stats writes (include/realcam_hip.h fixes the arithmetic) and derives the usual
control inputs from them on the device.  Pure Python: no kernel, no library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

from . import _lib
from .out_format import MATRICES

MAX_GRID = _lib.RC_STATS_MAX_GRID
SLOTS = ("valid", "sum_r", "sum_g", "sum_b", "sum_y", "clipped", "dark", "focus")     # zones[..., k]
CHANNELS = ("r", "g", "b", "y")                                                        # hist[:, c]


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"Stats.{name} must be an int, got {v!r}")
    return v


@dataclass(frozen=True)
class Stats:
    """Histograms and a 3A zone grid of a frame, as an output format: Output(Stats(...)) or out_format=Stats(...).

    grid    (gy, gx) zones, 1 .. 64 per axis and at most the measured region's side.
    bits    8 or 10: the codes are clamp(rint(v S), 0, S) with S = 2**bits - 1, the encoders' own.
    matrix  "bt601" / "bt709" / "bt2020": the luma coefficients of the Y histogram, the luma sums and the focus figure.
    roi     None (the whole frame) or (y0, x0, rh, rw) inside it.
    dark    None (nothing is dark) or a luma code 0 .. S: a pixel that is not clipped is dark if qY <= dark.
    clip    None (nothing clips) or a code 1 .. S: a pixel is clipped if max(qR, qG, qB) >= clip.
    """

    grid: Tuple[int, int] = (8, 8)
    bits: int = 8
    matrix: str = "bt709"
    roi: Optional[Tuple[int, int, int, int]] = None
    dark: Optional[int] = None
    clip: Optional[int] = None

    def __post_init__(self):
        if _int("bits", self.bits) not in (8, 10):
            raise ValueError(f"Stats.bits must be 8 or 10, got {self.bits}")
        if not isinstance(self.matrix, str) or self.matrix not in MATRICES:
            raise ValueError(f"Stats.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if not isinstance(self.grid, (tuple, list)) or len(self.grid) != 2:
            raise TypeError(f"Stats.grid must be (gy, gx), got {self.grid!r}")
        grid = tuple(_int("grid", v) for v in self.grid)
        if not all(1 <= v <= MAX_GRID for v in grid):
            raise ValueError(f"Stats.grid must lie in 1 .. {MAX_GRID} per axis, got {grid}")
        object.__setattr__(self, "grid", grid)
        if self.roi is not None:
            if not isinstance(self.roi, (tuple, list)) or len(self.roi) != 4:
                raise TypeError(f"Stats.roi must be None or (y0, x0, rh, rw), got {self.roi!r}")
            roi = tuple(_int("roi", v) for v in self.roi)
            if roi[0] < 0 or roi[1] < 0 or roi[2] < 1 or roi[3] < 1:
                raise ValueError(f"Stats.roi must have y0, x0 >= 0 and rh, rw >= 1, got {roi}")
            if grid[0] > roi[2] or grid[1] > roi[3]:
                raise ValueError(f"Stats.grid {grid} has more zones than the roi {roi} has rows or columns")
            object.__setattr__(self, "roi", roi)
        if self.dark is not None and not -1 <= _int("dark", self.dark) <= self.codes - 1:
            raise ValueError(f"Stats.dark must be None or lie in -1 .. {self.codes - 1}, got {self.dark}")
        if self.clip is not None and not 1 <= _int("clip", self.clip) <= self.codes:
            raise ValueError(f"Stats.clip must be None or lie in 1 .. {self.codes}, got {self.clip}")

    @property
    def codes(self) -> int:
        """2**bits: the length of a histogram."""
        return 1 << self.bits

    @property
    def dark_code(self) -> int:
        return -1 if self.dark is None else self.dark

    @property
    def clip_code(self) -> int:
        return self.codes if self.clip is None else self.clip

    def check(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """The region (y0, x0, rh, rw) measured in an (h, w) frame; every refusal that depends on the frame is raised here, before any launch."""
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"Stats: the frame {(h, w)} is empty")
        if h * w >= 1 << 29:
            raise ValueError(f"Stats: a frame of {(h, w)} has 2^29 samples or more per plane")
        y0, x0, rh, rw = self.roi if self.roi is not None else (0, 0, h, w)
        if y0 + rh > h or x0 + rw > w:
            raise ValueError(f"Stats: the roi {self.roi} lies outside the {(h, w)} frame")
        if self.grid[0] > rh or self.grid[1] > rw:
            raise ValueError(f"Stats: the grid {self.grid} has more zones than the measured region {(rh, rw)} has rows or columns")
        return y0, x0, rh, rw


def zone_bounds(side: int, zones: int):
    """The zones + 1 boundaries of an axis: zone i is positions ceil(i side / zones) .. ceil((i + 1) side / zones) - 1, which are the
    positions p with floor(p zones / side) = i."""
    return [-(-i * side // zones) for i in range(zones + 1)]


class FrameStats:
    """The statistics of a batch of frames (ops.frame_stats, Output(Stats(...))).

    hist   (B, 4, 2**bits) int64 on the device: per channel R, G, B, Y the number of measured pixels with each code.
    zones  (B, gy, gx, 8) int64 on the device: per zone the slots of stats.SLOTS -- valid pixels, the sums of qR, qG, qB over them, the sum
           of qY over all pixels, clipped pixels, dark pixels, the focus figure (forward-difference gradient energy of qY).
    spec   the Stats that asked;  roi  the (y0, x0, rh, rw) measured.
    """

    __slots__ = ("hist", "zones", "spec", "roi")

    def __init__(self, hist, zones, spec: Stats, roi):
        self.hist, self.zones, self.spec, self.roi = hist, zones, spec, tuple(int(v) for v in roi)

    @property
    def zone_pixels(self):
        """(gy, gx) int64 on the host: the pixels of each zone, from the geometry alone (slots valid + clipped + dark of any frame)."""
        import torch
        by, bx = zone_bounds(self.roi[2], self.spec.grid[0]), zone_bounds(self.roi[3], self.spec.grid[1])
        rows = torch.tensor([b - a for a, b in zip(by, by[1:])], dtype=torch.int64)
        cols = torch.tensor([b - a for a, b in zip(bx, bx[1:])], dtype=torch.int64)
        return rows[:, None] * cols[None, :]

    def mean_luma(self):
        """(B,) float64 on the device, 0 .. 1: the mean luma code over the region, in units of full scale.  No synchronisation."""
        import torch
        return self.zones[..., 4].sum((1, 2)).to(torch.float64) / float(self.roi[2] * self.roi[3] * (self.spec.codes - 1))

    def awb_gains(self):
        """(B, 3) float64 on the device: grey-world gains (sum qG / sum qR, 1, sum qG / sum qB) over the valid pixels; a channel whose sum
        is zero keeps the gain 1.  No synchronisation."""
        import torch
        s = self.zones[..., 1:4].sum((1, 2)).to(torch.float64)
        g = s[:, 1:2].expand(-1, 3)
        one = torch.ones_like(s)
        gains = torch.where(s == 0, one, g / torch.where(s == 0, one, s))
        gains[:, 1] = 1.0
        return gains

    def __repr__(self):
        return f"FrameStats(hist={tuple(self.hist.shape)}, zones={tuple(self.zones.shape)}, roi={self.roi}, spec={self.spec!r})"
