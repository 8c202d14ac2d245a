"""RAW noise measurement of forward_mosaic: what to measure on the sensor mosaic (RawNoise) and what comes back (RawNoiseStats).

RawNoise describes the request -- the tile, the code depth, the level bins, the sample value that maps to full scale, the region of interest
in Bayer cells and the two thresholds that spoil a tile; RawNoiseStats holds the two device tensors rc_raw_noise writes
(include/realcam_hip.h fixes the arithmetic) and derives the photon-transfer curve and the noise models of the sensor-side stages from them
on the device, so a calibration can run without the host seeing a frame.  Pure Python: no kernel, no library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from statistics import NormalDist
from typing import Optional, Tuple

from . import _lib

EBINS = _lib.RC_RAW_NOISE_EBINS
MAX_LEVEL_BITS = _lib.RC_RAW_NOISE_MAX_LEVEL_BITS
TILES = (4, 8, 16)
COLOURS = ("r", "g1", "g2", "b")                                                            # hist[:, c]: the packed map's slots, Calibration.gains' order


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"RawNoise.{name} must be an int, got {v!r}")
    return v


def ebin(e: int) -> int:
    """The energy bin of e >= 0 (step 5 of the header): e itself below 16, then 8 bins per octave (a 3-bit mantissa)."""
    if e < 16:
        return e
    k = e.bit_length() - 1
    return 8 * (k - 3) + (e >> (k - 3))


def ebin_range(b: int) -> Tuple[int, int]:
    """The smallest and the largest e of energy bin b."""
    if b < 16:
        return b, b
    shift = b // 8 - 1
    lo = (8 + b % 8) << shift
    return lo, lo + (1 << shift) - 1


def chi2_quantile(q: float, n: int) -> float:
    """The q-quantile of a chi-squared variable with n degrees of freedom (Wilson-Hilferty)."""
    z = NormalDist().inv_cdf(q)
    return n * (1.0 - 2.0 / (9.0 * n) + z * math.sqrt(2.0 / (9.0 * n))) ** 3


@dataclass(frozen=True)
class RawNoise:
    """The noise of the sensor mosaic per CFA colour and level: RawFormat(noise=RawNoise(...)) or ops.raw_noise(mosaic, fmt, RawNoise(...)).

    tile        4, 8 or 16: the region is cut into tiles of tile x tile Bayer cells; a tile gives one energy (tile**2 / 2 pair differences)
                per colour.  Larger tiles estimate better and find fewer flat places.
    bits        8 .. 16: the codes are clamp(rint((v - black) S / (top - black)), -S, S) with S = 2**bits - 1 -- signed: samples below
                black are half of the noise at black.
    level_bits  3 .. 6: 2**level_bits level bins over 0 .. S.
    roi         None (the whole frame) or (cy0, cx0, rh, rw) in Bayer cells inside it, cx0 even; at least one tile each way.
    top         None (the format's white level) or the sample value that maps to S; it must exceed every black level.
    sat         None (S: a tile that holds a full-scale code is not measured) or a code 1 .. S + 1: a sample at or above it spoils its
                tile for its colour -- clipped samples have no noise.  S + 1: nothing does.
    floor       None (nothing does) or a code -S - 1 .. S - 1: a sample at or below it spoils its tile (a sensor that clips at black: 0).
    """

    tile: int = 8
    bits: int = 10
    level_bits: int = 5
    roi: Optional[Tuple[int, int, int, int]] = None
    top: Optional[float] = None
    sat: Optional[int] = None
    floor: Optional[int] = None

    def __post_init__(self):
        if _int("tile", self.tile) not in TILES:
            raise ValueError(f"RawNoise.tile must be 4, 8 or 16, got {self.tile}")
        if not 8 <= _int("bits", self.bits) <= 16:
            raise ValueError(f"RawNoise.bits must lie in 8 .. 16, got {self.bits}")
        if not 3 <= _int("level_bits", self.level_bits) <= MAX_LEVEL_BITS:
            raise ValueError(f"RawNoise.level_bits must lie in 3 .. {MAX_LEVEL_BITS}, got {self.level_bits}")
        if self.roi is not None:
            if not isinstance(self.roi, (tuple, list)) or len(self.roi) != 4:
                raise TypeError(f"RawNoise.roi must be None or (cy0, cx0, rh, rw) in cells, got {self.roi!r}")
            roi = tuple(_int("roi", v) for v in self.roi)
            if roi[0] < 0 or roi[1] < 0 or roi[2] < 1 or roi[3] < 1:
                raise ValueError(f"RawNoise.roi must have cy0, cx0 >= 0 and rh, rw >= 1, got {roi}")
            if roi[1] % 2:
                raise ValueError(f"RawNoise.roi must start on an even cell column (cx0), got {roi}")
            if roi[2] < self.tile or roi[3] < self.tile:
                raise ValueError(f"RawNoise.roi {roi} holds no whole tile of {self.tile} x {self.tile} cells")
            object.__setattr__(self, "roi", roi)
        if self.top is not None:
            if isinstance(self.top, bool) or not isinstance(self.top, (int, float)):
                raise TypeError(f"RawNoise.top must be None or a number, got {self.top!r}")
            if not math.isfinite(self.top):
                raise ValueError(f"RawNoise.top must be finite, got {self.top!r}")
            object.__setattr__(self, "top", float(self.top))
        S = self.codes - 1
        if self.sat is not None and not 1 <= _int("sat", self.sat) <= S + 1:
            raise ValueError(f"RawNoise.sat must be None or lie in 1 .. {S + 1}, got {self.sat}")
        if self.floor is not None and not -S - 1 <= _int("floor", self.floor) <= S - 1:
            raise ValueError(f"RawNoise.floor must be None or lie in {-S - 1} .. {S - 1}, got {self.floor}")

    @property
    def codes(self) -> int:
        """2**bits: S + 1."""
        return 1 << self.bits

    @property
    def levels(self) -> int:
        """2**level_bits: the number of level bins."""
        return 1 << self.level_bits

    @property
    def pairs(self) -> int:
        """tile**2 / 2: the pair differences of a tile and colour, the degrees of freedom of its energy."""
        return self.tile * self.tile // 2

    @property
    def sat_code(self) -> int:
        return self.codes - 1 if self.sat is None else self.sat

    @property
    def floor_code(self) -> int:
        return -self.codes if self.floor is None else self.floor

    def top_value(self, white_level: float, blacks) -> float:
        """The sample value that maps to S for a format with these levels; refuses one at or below a black level."""
        top = float(white_level) if self.top is None else self.top
        if not math.isfinite(top) or not all(top > float(b) for b in blacks):
            raise ValueError(f"RawNoise: top ({top!r}) must be finite and exceed every black level {tuple(blacks)}")
        return top

    def check(self, h_cells: int, w_cells: int) -> Tuple[int, int, int, int]:
        """The region (cy0, cx0, rh, rw) measured in a frame of (h_cells, w_cells) Bayer cells; every refusal that depends on the frame is
        raised here, before any launch."""
        h, w = int(h_cells), int(w_cells)
        if h < 1 or w < 1:
            raise ValueError(f"RawNoise: the frame of {(h, w)} cells is empty")
        if 4 * h * w >= 1 << 31:
            raise ValueError(f"RawNoise: a mosaic of {(2 * h, 2 * w)} has 2^31 samples or more")
        cy0, cx0, rh, rw = self.roi if self.roi is not None else (0, 0, h, w)
        if cy0 + rh > h or cx0 + rw > w:
            raise ValueError(f"RawNoise: the roi {self.roi} lies outside the frame of {(h, w)} cells")
        if rh < self.tile or rw < self.tile:
            raise ValueError(f"RawNoise: the measured region of {(rh, rw)} cells holds no whole tile of {self.tile} x {self.tile} cells")
        return cy0, cx0, rh, rw


class RawNoiseStats:
    """The noise measurement of a batch of frames (ops.raw_noise, net.raw_noise after forward_mosaic with RawFormat.noise).

    hist   (B, 4, L, 320) int32 on the device: per colour R, G1 (G of the R row), G2 (G of the B row), B and per level bin the number of
           valid tiles in each energy bin (raw_noise.ebin).
    level  (B, 4, L) int64 on the device: the sum of the valid tiles' code sums.
    spec   the RawNoise that asked;  roi  the (cy0, cx0, rh, rw) measured, in cells;  unit  four floats in colour order: the sample
           units of one code, (top - black) / S.
    Every method computes with torch on the tensors' device and synchronises nothing.  Frames of a batch that share a sensor setting may
    be pooled: the tables are counts and sums, so hist.sum(0, keepdim=True) and level.sum(0, keepdim=True) are a measurement too.
    """

    __slots__ = ("hist", "level", "spec", "roi", "unit")

    def __init__(self, hist, level, spec: RawNoise, roi, unit):
        self.hist, self.level, self.spec, self.roi = hist, level, spec, tuple(int(v) for v in roi)
        self.unit = tuple(float(v) for v in unit)
        if len(self.unit) != 4:
            raise ValueError(f"RawNoiseStats.unit holds four floats in colour order, got {unit!r}")

    def _unit(self):
        import torch
        return torch.stack([torch.full((), u, dtype=torch.float64, device=self.hist.device) for u in self.unit])      # fills: no upload of a host table

    def tiles(self):
        """(B, 4, L) int64: the valid tiles of each level bin."""
        import torch
        return self.hist.sum(-1, dtype=torch.int64)

    def levels(self):
        """(B, 4, L) float64: the mean level above black of each bin's tiles, in sample units; NaN where a bin is empty."""
        import torch
        n = self.tiles().to(torch.float64) * float(self.spec.tile ** 2)
        return torch.where(n > 0, self.level.to(torch.float64) / n, torch.full_like(n, math.nan)) * self._unit()[:, None]

    def _centres(self):
        """(320,) float64: the middle of each energy bin's range of e, computed on the device."""
        import torch
        b = torch.arange(EBINS, device=self.hist.device, dtype=torch.int64)
        shift = (b // 8 - 1).clamp(min=0)
        lo = torch.where(b < 16, b, (8 + b % 8) << shift).to(torch.float64)
        return lo + ((1 << shift) - 1).to(torch.float64) * 0.5

    def variance(self, quantile: float = 0.1, min_tiles: int = 16):
        """(B, 4, L) float64: the noise variance of each level bin in sample units squared; NaN where a bin has fewer than min_tiles tiles.

        With b the first energy bin at which the cumulative count reaches ceil(quantile tiles) and E the middle of that bin's range of e:
        variance = E / (2 chi2_q(n)) unit^2, n = tile^2 / 2 -- on a flat tile e / (2 sigma^2) is chi-squared with n degrees of freedom, so
        the q-quantile of e is 2 sigma^2 chi2_q(n) (chi2_quantile: Wilson-Hilferty).
        Why a LOW quantile: texture adds to a tile's energy and never takes away, so a textured tile only ever has more energy than a
        flat one at the same level and the low end of a bin's energies belongs to its flat tiles; a mean or a median would measure the
        scene.  The bias: if only a share f < 1 of a bin's tiles is flat and the others lie above, the q-quantile of all tiles is the
        (q / f)-quantile of the flat ones: the estimate is high by chi2_(q/f)(n) / chi2_q(n) -- at q = 0.1, tile 8 (n = 32), f = 0.5: 1.13; f
        = 0.7: 1.06 -- and meaningless once f <= q.  An energy bin is 1/8 octave wide: E is within 6 % of any e of its bin."""
        import torch
        if not 0.0 < float(quantile) < 1.0:
            raise ValueError(f"RawNoiseStats.variance: quantile must lie inside 0 .. 1, got {quantile!r}")
        t = self.tiles()
        need = torch.ceil(t.to(torch.float64) * float(quantile)).clamp(min=1.0)
        cum = self.hist.cumsum(-1, dtype=torch.int64).to(torch.float64)
        b = (cum < need[..., None]).sum(-1).clamp(max=EBINS - 1)
        E = self._centres()[b]
        var = E / (2.0 * chi2_quantile(float(quantile), self.spec.pairs)) * (self._unit() ** 2)[:, None]
        return torch.where(t >= int(min_tiles), var, torch.full_like(var, math.nan))

    @staticmethod
    def _line(x, y, w, dims):
        """Weighted least squares y = a + b x over `dims` (w = 0 where a point does not count): (b, a); one point or one level: b = 0; none: NaN."""
        import torch
        sw, sx, sy = w.sum(dims), (w * x).sum(dims), (w * y).sum(dims)
        sxx, sxy = (w * x * x).sum(dims), (w * x * y).sum(dims)
        den = sw * sxx - sx * sx
        ok = den > 1e-12 * sw * sxx
        slope = torch.where(ok, (sw * sxy - sx * sy) / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
        slope = torch.where(sw > 0, slope, torch.full_like(slope, math.nan))                # no point at all: NaN, as the intercept 0 / 0 is
        return slope, (sy - slope * sx) / sw

    def _points(self, quantile, min_tiles):
        import torch
        var, lev, t = self.variance(quantile, min_tiles), self.levels(), self.tiles().to(torch.float64)
        ok = torch.isfinite(var) & torch.isfinite(lev) & (var > 0)
        zero = torch.zeros_like(var)
        return torch.where(ok, lev, zero), torch.where(ok, var, torch.ones_like(var)), torch.where(ok, t, zero)

    def profile(self, quantile: float = 0.1, min_tiles: int = 16):
        """(4, 2) float64, per colour (gain, offset) of variance = offset + gain level in sample units, pooled over the frames: a weighted
        least-squares line through the bins that have a variance, with weights tiles / variance^2 (the variance of a variance estimate
        goes with its square).  Divided by the white range -- gain / (white - black), offset / (white - black)^2 -- this is DNG's
        NoiseProfile pair (S, O) for that plane.  NaN for a colour without a measured bin; the offset needs dark tiles: a line fitted to
        bright bins alone extrapolates it."""
        import torch
        x, y, t = self._points(quantile, min_tiles)
        gain, offset = self._line(x, y, t / (y * y), (0, 2))
        return torch.stack([gain, offset], -1)

    def temporal_noise(self, quantile: float = 0.1, min_tiles: int = 16):
        """(2,) float64: (n_abs, n_rel) of sqrt(variance) = n_abs + n_rel level in sample units, pooled over colours and frames with
        weights tiles; n_abs is floored at the smallest positive normal fp32 and n_rel at 0 (what Temporal accepts).  After .tolist() this is Temporal(noise=...), and,
        scaled by the number of noise levels to tolerate, Defects(hot=..., cold=...) and Exposures(motion=...)."""
        import torch
        x, y, t = self._points(quantile, min_tiles)
        rel, ab = self._line(x, y.sqrt(), t, (0, 1, 2))
        return torch.stack([ab.clamp(min=float(torch.finfo(torch.float32).smallest_normal)), rel.clamp(min=0.0)])

    def __repr__(self):
        return f"RawNoiseStats(hist={tuple(self.hist.shape)}, level={tuple(self.level.shape)}, roi={self.roi}, spec={self.spec!r})"
