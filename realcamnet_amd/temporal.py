"""Temporal noise reduction of forward_mosaic: a motion-adaptive recursive filter on the mosaic, between the repair / merge and the
calibration (include/realcam_hip.h, rc_raw_temporal, fixes the arithmetic).

Temporal is the request -- the noise model, the weight of a new frame, the ramp, the exposure gain, the state -- and rides in
RawFormat(temporal=...).  TemporalState holds the last filtered mosaic from one call to the next.  TemporalMotion (Temporal(motion=...))
asks for motion compensation: block vectors are estimated on the luma proxy of the frame and of the state (rc_raw_motion_pyramid,
rc_motion_search) and the filter reads the state displaced by them (rc_raw_temporal_mc).  Pure Python: validation raises ValueError /
TypeError and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# The kernel's lane map (csrc/temporal_kernel.hpp): a lane holds LANE_PX consecutive samples of a row, a wave loads WAVE_SPAN columns and produces
# WAVE_OUT of them (strips overlap by one lane at either end, so strip s starts at column s WAVE_OUT), a block holds BLOCK_STRIPS strips of
# BLOCK_ROWS rows.  Tests place widths and heights on these seams.
LANE_PX = 4
WAVE_SPAN = 64 * LANE_PX
WAVE_OUT = WAVE_SPAN - 2 * LANE_PX
BLOCK_STRIPS = 2
BLOCK_ROWS = 32


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _f32(v) -> float:
    with np.errstate(over="ignore"):            # a value past fp32's range becomes inf, which the callers refuse
        return float(np.float32(v))


class TemporalState:
    """What the filter carries from one forward_mosaic call to the next: `frame`, the last filtered mosaic (B,2h,2w) fp32 on the device, or
    None.  reset() drops it (a scene cut): the next call returns its decoded frame.  One state serves one stream (or the B streams of a
    batch); a call whose frame has another shape or device than the state starts over.  With Temporal(motion=...), `field` is the last
    call's level-0 vectors (B,by,bx,4) int32 -- (dx, dy, cost, texture) per block, in Bayer cells, after the texture / cost mask -- or None
    (a call that started over, or no motion)."""

    def __init__(self):
        self.frame = None
        self.field = None
        self._spare = None                       # the buffer the call after next writes: forward_mosaic swaps the two
        self._pyramids = None                    # Temporal(motion=...): the frame's and the state's pyramid buffers, rewritten by every call

    def reset(self) -> None:
        self.frame = None
        self.field = None

    def pyramids(self, shapes, like):
        """The two sets of uint8 pyramid buffers for these level shapes on `like`'s device: the ones kept when they fit, new ones otherwise."""
        import torch
        kept = self._pyramids
        if kept is None or not all(len(p) == len(shapes) and all(t.dtype == torch.uint8 and tuple(t.shape) == tuple(s) and t.device == like.device
                                                                 for t, s in zip(p, shapes)) for p in kept):
            self._pyramids = tuple([like.new_empty(tuple(s), dtype=torch.uint8) for s in shapes] for _ in range(2))
        return self._pyramids

    def matches(self, shape, device) -> bool:
        """The state continues a frame of this (B,2h,2w) shape on this device."""
        f = self.frame
        return f is not None and tuple(f.shape) == tuple(int(s) for s in shape) and f.device == device


@dataclass(frozen=True)
class TemporalMotion:
    """Motion compensation of the temporal filter: Temporal(motion=TemporalMotion(...)).  The estimator is Motion's -- hierarchical block
    matching -- on the 8-bit luma proxy of the mosaic (one code per Bayer cell), so every size here is in cells (a cell is 2 x 2 samples).

    levels       1 .. 4 pyramid levels.
    block        8, 16 or 32 cells: the matching block at every level, and the block whose vector displaces the state.
    search       1 .. 8: the range of the full search at the coarsest level, in that level's cells.
    refine       0 .. 2: the range around the doubled vector of the level above, at every finer level.
    min_texture  >= 0: a block whose texture is below it keeps a zero vector (a flat block matches anywhere).
    max_sad      None or >= 0: a block whose cost is above it keeps a zero vector (nothing in range matched).
    The reach is about (search 2^(levels-1) + refine (2^(levels-1) - 1)) cells per axis.
    """

    levels: int = 3
    block: int = 16
    search: int = 4
    refine: int = 1
    min_texture: int = 0
    max_sad: Optional[int] = None

    def __post_init__(self):
        self.spec()                                                   # levels, block, search, refine: Motion's own refusals
        for name in ("min_texture", "max_sad"):
            v = getattr(self, name)
            if v is None and name == "max_sad":
                continue
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"TemporalMotion.{name} must be an int{' or None' if name == 'max_sad' else ''}, got {v!r}")
            if v < 0:
                raise ValueError(f"TemporalMotion.{name} must be >= 0, got {v}")

    def spec(self):
        """The Motion that ops.motion_estimate takes for these levels, block and ranges."""
        from .motion import Motion
        try:
            return Motion(levels=self.levels, block=self.block, search=self.search, refine=self.refine)
        except (TypeError, ValueError) as e:
            raise type(e)(str(e).replace("Motion.", "TemporalMotion.")) from None

    def check(self, h: int, w: int) -> Tuple[int, int]:
        """(by, bx), the grid of vectors of a frame of (h, w) cells; refuses a frame whose coarsest level holds no whole block."""
        try:
            return self.spec().check(h, w)
        except ValueError as e:
            raise ValueError(str(e).replace("Motion:", "TemporalMotion:") + " (sizes in Bayer cells)") from None


@dataclass(frozen=True, eq=False)
class Temporal:
    """The temporal filter's request: RawFormat(temporal=Temporal(...)) or ops.raw_temporal.

    noise    (n_abs, n_rel) in the storage's own code units: the expected noise level of a sample is n_abs + n_rel max(p - black, 0).
             n_abs finite and > 0, n_rel finite and >= 0.
    alpha    in (0, 1]: the weight of the new frame where nothing moves.
    ramp     finite and > 1: at an activity (the mean |frame - state| over the same-colour 3x3 neighbourhood) of `ramp` noise levels the new
             frame passes unchanged; between 1 and ramp the weight rises linearly from alpha to 1.
    gain     None, one host number (finite and > 0), or a (1,1) / (B,1) fp32 tensor on the device: this frame's exposure over the previous
             frame's, so an AE step does not read as motion.  The kernel reads a tensor when it runs -- a loop rewrites it in place without a
             host sync and a captured graph sees the new value on replay.  A tensor's values are NOT checked.
    state    a TemporalState; forward_mosaic requires it (ops.raw_temporal takes the previous frame as an argument and ignores it).
    motion   None, or a TemporalMotion: forward_mosaic estimates block vectors between the frame and the state and filters against the
             displaced state, so a pan or a hand-held shot is filtered like a static scene (ops.raw_temporal takes vectors as an argument
             and ignores it).
    The B frames of a call are B independent streams, not B consecutive frames.  Compared by identity (a tensor and a state ride in it).
    """

    noise: Tuple[float, float]
    alpha: float = 0.125
    ramp: float = 3.0
    gain: object = None
    state: Optional[TemporalState] = None
    motion: Optional[TemporalMotion] = None

    def __post_init__(self):
        import torch
        if self.motion is not None and not isinstance(self.motion, TemporalMotion):
            raise TypeError(f"Temporal.motion must be None or a TemporalMotion, got {type(self.motion).__name__}")
        v = self.noise
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2 or not all(_number(e) for e in v):
            raise TypeError(f"Temporal.noise must be (n_abs, n_rel), got {v!r}")
        nz = (_f32(v[0]), _f32(v[1]))
        if not (math.isfinite(nz[0]) and nz[0] > 0.0 and math.isfinite(nz[1]) and nz[1] >= 0.0):
            raise ValueError(f"Temporal.noise: n_abs must be finite and > 0, n_rel finite and >= 0 (as fp32), got {nz}")
        object.__setattr__(self, "noise", nz)
        for name in ("alpha", "ramp"):
            if not _number(getattr(self, name)):
                raise TypeError(f"Temporal.{name} must be a number, got {getattr(self, name)!r}")
            object.__setattr__(self, name, _f32(getattr(self, name)))
        if not 0.0 < self.alpha <= 1.0:
            raise ValueError(f"Temporal.alpha must lie in (0, 1] (as fp32), got {self.alpha}")
        if not (math.isfinite(self.ramp) and self.ramp > 1.0):
            raise ValueError(f"Temporal.ramp must be finite and > 1 (as fp32), got {self.ramp}")
        g = self.gain
        if isinstance(g, torch.Tensor):
            if g.dtype != torch.float32:
                raise TypeError(f"Temporal.gain: a tensor must be fp32, got {g.dtype}")
            if g.dim() != 2 or g.shape[0] < 1 or g.shape[1] != 1:
                raise ValueError(f"Temporal.gain: a tensor must be (1,1) or (B,1), got {tuple(g.shape)}")
        elif g is not None:
            if not _number(g):
                raise TypeError(f"Temporal.gain must be None, a number or a (B,1) fp32 tensor, got {g!r}")
            g = _f32(g)
            if not (math.isfinite(g) and g > 0.0):
                raise ValueError(f"Temporal.gain must be finite and > 0 (as fp32), got {g}")
            object.__setattr__(self, "gain", g)
        if self.state is not None and not isinstance(self.state, TemporalState):
            raise TypeError(f"Temporal.state must be None or a TemporalState, got {type(self.state).__name__}")

    @property
    def device_gain(self) -> bool:
        """The gain is a device tensor (read by the kernel), not a host number or None."""
        return self.gain is not None and not isinstance(self.gain, float)

    def params(self) -> Tuple[float, float, float, float]:
        """n_abs, n_rel, alpha, ramp."""
        return self.noise + (self.alpha, self.ramp)

    def check(self, h2: int, w2: int, batch: Optional[int] = None) -> None:
        """Refuse a gain tensor with the wrong number of rows, and with `motion` a frame too small for its coarsest level."""
        if self.motion is not None:
            self.motion.check(int(h2) // 2, int(w2) // 2)
        if batch is not None and self.device_gain and self.gain.shape[0] not in (1, int(batch)):
            raise ValueError(f"Temporal.gain: {self.gain.shape[0]} rows for a batch of {int(batch)} (1 or the batch)")
