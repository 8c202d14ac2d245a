"""Multi-exposure HDR merge of forward_mosaic: how the E = 2 .. 4 exposures of one scene are delivered and fused into one linear mosaic
(Exposures) in front of the calibration (include/realcam_hip.h, rc_raw_hdr_merge, fixes the arithmetic).

Exposures is the request -- the exposure times, the knee at which a longer exposure fades out, the optional motion cut, the layout -- and
rides in RawFormat(exposures=...).  Pure Python: validation raises ValueError / TypeError and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# The kernel's lane map (csrc/hdr_merge.hip), calibrate.hip's: a lane holds LANE_PX consecutive samples of a row of every exposure, a wave a
# strip of WAVE_SPAN columns, a block BLOCK_SPAN columns of BLOCK_ROWS rows.  Tests place widths and heights on these seams.
LANE_PX = 4
WAVE_SPAN = 64 * LANE_PX
BLOCK_SPAN = 2 * WAVE_SPAN
BLOCK_ROWS = 16
MIN_EXPOSURES, MAX_EXPOSURES = 2, 4
LAYOUTS = ("frames", "lines")


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _f32(v) -> float:
    with np.errstate(over="ignore"):            # a value past fp32's range becomes inf, which the callers refuse
        return float(np.float32(v))


def _pair(name, v, what) -> Tuple[float, float]:
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2 or not all(_number(e) for e in v):
        raise TypeError(f"Exposures.{name} must be {what}, got {v!r}")
    return _f32(v[0]), _f32(v[1])


@dataclass(frozen=True, eq=False)
class Exposures:
    """The E = 2 .. 4 exposures of one scene and how to merge them: RawFormat(exposures=Exposures(...)) or ops.raw_hdr_merge.

    times    the exposure times (or ratios: only their quotients matter), the shortest first: E host numbers, finite, positive and
             strictly increasing, or a (1,E) / (B,E) fp32 tensor on the device, which the kernel reads when it runs -- an AE loop rewrites
             it in place without a host sync and a captured graph sees the new values on replay.  A tensor's values are NOT checked: a
             value <= 0 or rows that are not increasing give an unspecified result (no fault).
    knee     (lo, hi), finite, lo < hi, in the storage's own code units (as the Defects thresholds): a longer exposure's weight is 1 up to
             lo, fades linearly to 0 at hi and stays 0 above -- its saturated samples do not count.  The shortest exposure always counts.
    motion   None, or (t_abs, t_rel), finite and >= 0: a longer exposure is cut where its linear value differs from the shortest one's by
             more than t_abs + t_rel |l_0| (in the shortest exposure's code units).
    layout   "frames": the mosaic tensor is (B, E, 2h, X), whole frames.  "lines": (B,[1,] E 2h, X), row r of exposure e at tensor row
             r E + e (line-interleaved / staggered readout).  X is samples, or the line stride in bytes of a MIPI storage.
    The merged mosaic is linear, fp32 and in the shortest exposure's code units, so RawFormat's levels keep their meaning.  A sample with
    weights w_e = u_e t_e becomes black + sum(w_e l_e) / sum(w_e), l_e = (c_e - black) t_0 / t_e.  Compared by identity (a tensor may ride
    in it).
    """

    times: object
    knee: Tuple[float, float]
    motion: Optional[Tuple[float, float]] = None
    layout: str = "frames"

    def __post_init__(self):
        import torch
        t = self.times
        if isinstance(t, torch.Tensor):
            if t.dtype != torch.float32:
                raise TypeError(f"Exposures.times: a tensor must be fp32, got {t.dtype}")
            if t.dim() != 2 or t.shape[0] < 1 or not MIN_EXPOSURES <= t.shape[1] <= MAX_EXPOSURES:
                raise ValueError(f"Exposures.times: a tensor must be (1,E) or (B,E) with E = {MIN_EXPOSURES} .. {MAX_EXPOSURES}, got {tuple(t.shape)}")
        else:
            if isinstance(t, (str, bytes)) or not hasattr(t, "__len__") or not all(_number(v) for v in t):
                raise TypeError(f"Exposures.times must be {MIN_EXPOSURES} to {MAX_EXPOSURES} numbers or a (B,E) fp32 tensor, got {t!r}")
            if not MIN_EXPOSURES <= len(t) <= MAX_EXPOSURES:
                raise ValueError(f"Exposures.times: {MIN_EXPOSURES} to {MAX_EXPOSURES} exposures, got {len(t)}")
            t = tuple(_f32(v) for v in t)
            if not all(math.isfinite(v) and v > 0.0 for v in t):
                raise ValueError(f"Exposures.times must be finite and positive (as fp32), got {t}")
            if not all(b > a for a, b in zip(t, t[1:])):
                raise ValueError(f"Exposures.times must be strictly increasing (as fp32), the shortest exposure first, got {t}")
            object.__setattr__(self, "times", t)
        k = _pair("knee", self.knee, "(lo, hi)")
        if not (math.isfinite(k[0]) and math.isfinite(k[1]) and k[0] < k[1]):
            raise ValueError(f"Exposures.knee needs finite lo < hi, got {k}")
        object.__setattr__(self, "knee", k)
        if self.motion is not None:
            m = _pair("motion", self.motion, "None or (t_abs, t_rel)")
            if not all(math.isfinite(v) and v >= 0.0 for v in m):
                raise ValueError(f"Exposures.motion: both thresholds must be finite and >= 0, got {m}")
            object.__setattr__(self, "motion", m)
        if not isinstance(self.layout, str):
            raise TypeError(f"Exposures.layout must be one of {LAYOUTS}, got {self.layout!r}")
        if self.layout not in LAYOUTS:
            raise ValueError(f"Exposures.layout must be one of {LAYOUTS}, got {self.layout!r}")

    @property
    def device_times(self) -> bool:
        """The times are a device tensor (read by the kernel), not host numbers."""
        return not isinstance(self.times, tuple)

    @property
    def count(self) -> int:
        """E."""
        return int(self.times.shape[1]) if self.device_times else len(self.times)

    def check(self, h2: int, w2: int, batch: Optional[int] = None) -> None:
        """Refuse a times tensor with the wrong number of rows."""
        if batch is not None and self.device_times and self.times.shape[0] not in (1, int(batch)):
            raise ValueError(f"Exposures.times: {self.times.shape[0]} rows for a batch of {int(batch)} (1 or the batch)")
