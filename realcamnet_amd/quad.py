"""Quad-Bayer (tetracell) sensors of forward_mosaic: how the frame becomes an ordinary Bayer mosaic (QuadBayer) in front of every other
stage (include/realcam_hip.h, rc_raw_quad, fixes the arithmetic).

Each colour of the Bayer cell covers a 2x2 block of photosites: with RawFormat(quad=QuadBayer(...)) the format's `cfa` names the colours
of the four 2x2 blocks of the 4x4 tile.  Pure Python: validation raises ValueError / TypeError and never touches the GPU or the library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

# The remosaic kernel's lane map (csrc/quad.hip): a lane holds LANE_PX consecutive samples of a row (one quad period), a wave produces
# WAVE_SPAN columns (62 lanes; the other two hold the halo) of WAVE_ROWS rows, a block BLOCK_SPAN columns of BLOCK_ROWS rows (two strips,
# two row bands).  Tests place widths, heights and bright samples on these seams.
LANE_PX = 4
WAVE_SPAN = 62 * LANE_PX
BLOCK_SPAN = 2 * WAVE_SPAN
WAVE_ROWS = 16
BLOCK_ROWS = 2 * WAVE_ROWS
MODES = ("remosaic", "bin")


@dataclass(frozen=True)
class QuadBayer:
    """What a Quad-Bayer sensor delivered and how to read it: RawFormat(quad=QuadBayer(...)) or ops.raw_quad.

    mode    "remosaic": the full-resolution quad mosaic (B,[1,]H,X) -> a Bayer mosaic (B,H,W) of the same size: a site whose colour is
            already the wanted one is kept, the others are interpolated from the nearest samples of the wanted colour along the row, the
            column (the smoother of the two where both have it) or the diagonal square.  uint16 for the u8 / u16 / mipi10 / mipi12
            storages, the tensor's own dtype for float.
            "bin": -> the mean of each 2x2 same-colour block, a Bayer mosaic (B,H/2,W/2), fp32 for every storage.
    The result has the format's cfa and levels; H and W must be multiples of 4.  A factory defect map (Defects.map) cannot follow: it
    addresses photosites that the remosaic has mixed or the binning has merged; the dynamic hot / cold tests run on the Bayer result.
    Frames holding NaN / Inf are outside the contract.
    """

    mode: str = "remosaic"

    def __post_init__(self):
        if not isinstance(self.mode, str) or self.mode not in MODES:
            raise ValueError(f"QuadBayer.mode must be one of {MODES}, got {self.mode!r}")

    @property
    def code(self) -> int:
        from . import _lib
        return _lib.RC_QUAD_BIN if self.mode == "bin" else _lib.RC_QUAD_REMOSAIC

    def out_size(self, h: int, w: int) -> Tuple[int, int]:
        """Check the sensor frame's size (H, W) and return the size of the Bayer mosaic that leaves the stage."""
        h, w = int(h), int(w)
        if h < 4 or w < 4 or h % 4 or w % 4:
            raise ValueError(f"QuadBayer: the quad tile is 4x4 -- the frame's height and width must be multiples of 4 and at least 4, got {(h, w)}")
        return (h // 2, w // 2) if self.mode == "bin" else (h, w)
