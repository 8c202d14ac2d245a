"""Local tone mapping of forward_mosaic: contrast-limited adaptive histogram equalisation (CLAHE) on the luma of one output, after its
warp and resize and before its look (include/realcam_hip.h, rc_tone_*, fixes the arithmetic).

ToneMap is the request and rides in Output(tone=...) or goes to ops.tone_map / ops.tone_hist / ops.tone_gains / ops.tone_apply.  Pure
Python: validation raises ValueError / TypeError and never touches the GPU or the library; only `axis()` calls the library's host
function rc_tone_axis, which holds the one copy of the interpolation tables' arithmetic.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib

MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}          # RC_MATRIX_*: the luma coefficients of RC_YUV_KR_KB
MAX_GRID = _lib.RC_TONE_MAX_GRID
BINS = _lib.RC_TONE_BINS
MAX_CLIP = 256.0
MAX_GAIN = 64.0

# The kernels' lane maps (csrc/tone.hip): a lane holds LANE_PX consecutive pixels of a row and a wave WAVE_SPAN columns -- a strip of the
# apply kernel, a piece of a tile's row in the hist kernel; an apply block walks a band of BAND_ROWS rows, a hist block a slab of HIST_ROWS
# rows of one tile.  Tests place widths and heights on these seams.
LANE_PX = 4
WAVE_SPAN = 64 * LANE_PX
BAND_ROWS = 64
HIST_ROWS = 32


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _f32(v) -> float:
    with np.errstate(over="ignore"):            # a value past fp32's range becomes inf, which the caller refuses
        return float(np.float32(v))


def tile_bounds(side: int, tiles: int):
    """The tiles + 1 boundaries of an axis: tile i is positions ceil(i side / tiles) .. ceil((i + 1) side / tiles) - 1."""
    return [-(-i * side // tiles) for i in range(tiles + 1)]


def axis(n: int, g: int):
    """The interpolation tables of one axis (rc_tone_axis): n positions, g tiles -> (idx int32 [n], wt float32 [n]) as NumPy arrays."""
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in (n, g)) or n < 1 or g < 1 or g > MAX_GRID or g > n:
        raise ValueError(f"tone axis: n must be positive and g lie in 1 .. min({MAX_GRID}, n), got (n, g) = {(n, g)!r}")
    idx = np.empty(int(n), dtype=np.int32)
    wt = np.empty(int(n), dtype=np.float32)
    lib = _lib.load()
    if lib.rc_tone_axis(int(n), int(g), idx.ctypes.data, wt.ctypes.data) != 0:
        raise ValueError(f"rc_tone_axis(n={n}, g={g}): {lib.rc_last_error().decode(errors='replace')}")
    return idx, wt


@dataclass(frozen=True)
class ToneMap:
    """One output's local tone mapping: Output(tone=ToneMap(...)) or ops.tone_map.

    grid      (gy, gx) tiles, 1 .. 16 per axis and at most the frame's side.  Each tile owns a table of 256 gains; a pixel interpolates
              between the tables of the four nearest tile centres.
    clip      in [1, 256]: a histogram bin is limited to `clip` times the mean bin count and the excess is spread evenly, which bounds the
              slope of the tile's curve.  1 leaves the tile alone, 256 is plain histogram equalisation.
    strength  in [0, 1]: how far the curve moves from the identity towards the equalised one.  0 leaves the picture alone.
    max_gain  in [1, 64]: the bound on the gain of R, G and B.
    matrix    "bt601", "bt709" or "bt2020": the luma coefficients.
    The numbers are kept as the fp32 values the kernel sees.  Hashable and compared by value.
    """

    grid: Tuple[int, int] = (8, 8)
    clip: float = 2.0
    strength: float = 1.0
    max_gain: float = 8.0
    matrix: str = "bt709"

    def __post_init__(self):
        g = self.grid
        if not isinstance(g, (tuple, list)) or len(g) != 2:
            raise TypeError(f"ToneMap.grid must be (gy, gx), got {g!r}")
        for v in g:
            if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
                raise TypeError(f"ToneMap.grid must hold two ints, got {g!r}")
        g = (int(g[0]), int(g[1]))
        if not all(1 <= v <= MAX_GRID for v in g):
            raise ValueError(f"ToneMap.grid must lie in 1 .. {MAX_GRID} per axis, got {g}")
        object.__setattr__(self, "grid", g)
        for name, lo, hi in (("clip", 1.0, MAX_CLIP), ("strength", 0.0, 1.0), ("max_gain", 1.0, MAX_GAIN)):
            v = getattr(self, name)
            if not _number(v):
                raise TypeError(f"ToneMap.{name} must be a number, got {v!r}")
            v = _f32(v)
            if not (math.isfinite(v) and lo <= v <= hi):
                raise ValueError(f"ToneMap.{name} must be finite and lie in [{lo:g}, {hi:g}] (as fp32), got {v}")
            object.__setattr__(self, name, v)
        if not isinstance(self.matrix, str):
            raise TypeError(f"ToneMap.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if self.matrix not in MATRICES:
            raise ValueError(f"ToneMap.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")

    @property
    def matrix_code(self) -> int:
        """RC_MATRIX_* of the luma coefficients."""
        return MATRICES[self.matrix]

    @property
    def clip_q8(self) -> int:
        """rint(clip 256), half to even: 256 .. 65536, the clip limit as the kernel takes it."""
        return int(np.rint(np.float64(self.clip) * 256.0))

    def check(self, h: int, w: int) -> Tuple[int, int]:
        """(h, w) of the frame, checked against the grid; every refusal that depends on the frame is raised here, before any launch."""
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"ToneMap: the frame {(h, w)} is empty")
        if h * w >= 1 << 29:
            raise ValueError(f"ToneMap: a frame of {(h, w)} has 2^29 samples or more per plane")
        if self.grid[0] > h or self.grid[1] > w:
            raise ValueError(f"ToneMap: the grid {self.grid} has more tiles than the frame {(h, w)} has rows or columns")
        return h, w
