"""Output sharpening of forward_mosaic: an unsharp mask on the luma of one output, after its warp, resize and look and before its encoder
or statistics (include/realcam_hip.h, rc_sharpen, fixes the arithmetic).

Sharpen is the request and rides in Output(sharpen=...) or goes to ops.sharpen.  Pure Python: validation raises ValueError / TypeError
and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}          # RC_MATRIX_*: the luma coefficients of RC_YUV_KR_KB
MAX_AMOUNT = 8.0

# The kernel's lane map (csrc/sharpen.hip): a lane holds LANE_PX consecutive pixels of a row, a wave loads WAVE_SPAN columns and produces
# WAVE_OUT of them (strips overlap by one lane at either end, so strip s starts at column s WAVE_OUT), a wave walks a band of BAND_ROWS
# rows.  Tests place widths and heights on these seams.
LANE_PX = 4
WAVE_SPAN = 64 * LANE_PX
WAVE_OUT = WAVE_SPAN - 2 * LANE_PX
BAND_ROWS = 32


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _f32(v) -> float:
    with np.errstate(over="ignore"):            # a value past fp32's range becomes inf, which the caller refuses
        return float(np.float32(v))


@dataclass(frozen=True)
class Sharpen:
    """One output's detail enhancement: Output(sharpen=Sharpen(...)) or ops.sharpen.

    amount     in [0, 8]: the gain on the luma detail (luma minus its binomial blur).  0 leaves the picture alone.
    radius     1 or 2: the 3x3 or the 5x5 binomial.
    core       in [0, 1], in output units: detail below it is left alone, so noise is not sharpened.
    overshoot  in [0, 1], in output units: how far the sharpened luma may leave the range of its 3x3 neighbourhood; 0 means no ringing
               beyond the local extremes.
    matrix     "bt601", "bt709" or "bt2020": the luma coefficients.
    The numbers are kept as the fp32 values the kernel sees.  Hashable and compared by value.
    """

    amount: float = 1.0
    radius: int = 2
    core: float = 0.0
    overshoot: float = 0.0
    matrix: str = "bt709"

    def __post_init__(self):
        for name, hi in (("amount", MAX_AMOUNT), ("core", 1.0), ("overshoot", 1.0)):
            v = getattr(self, name)
            if not _number(v):
                raise TypeError(f"Sharpen.{name} must be a number, got {v!r}")
            v = _f32(v)
            if not (math.isfinite(v) and 0.0 <= v <= hi):
                raise ValueError(f"Sharpen.{name} must be finite and lie in [0, {hi:g}] (as fp32), got {v}")
            object.__setattr__(self, name, v)
        r = self.radius
        if not isinstance(r, (int, np.integer)) or isinstance(r, (bool, np.bool_)):
            raise TypeError(f"Sharpen.radius must be 1 or 2, got {r!r}")
        if r not in (1, 2):
            raise ValueError(f"Sharpen.radius must be 1 or 2, got {r!r}")
        object.__setattr__(self, "radius", int(r))
        if not isinstance(self.matrix, str):
            raise TypeError(f"Sharpen.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if self.matrix not in MATRICES:
            raise ValueError(f"Sharpen.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")

    @property
    def matrix_code(self) -> int:
        """RC_MATRIX_* of the luma coefficients."""
        return MATRICES[self.matrix]
