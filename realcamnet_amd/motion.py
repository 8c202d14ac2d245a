"""Motion estimation of forward_mosaic: what to estimate (Motion), what is carried between calls (MotionState), what comes back (MotionField)
and a global stabiliser that turns fields into meshes for ops.warp (Stabilizer).

The estimator is hierarchical block matching on the 8-bit luma code of the planar result: rc_motion_pyramid and rc_motion_search
(include/realcam_hip.h fixes the arithmetic).  Pure Python and torch: no kernel, no library; validation raises ValueError / TypeError
before any launch.  MotionField's and Stabilizer's methods are plain tensor arithmetic without a host synchronisation and work on CPU
tensors as well.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

from . import _lib
from .out_format import MATRICES

BLOCKS = (8, 16, 32)
MAX_LEVELS, MAX_RANGE, MAX_REFINE = _lib.RC_MOTION_MAX_LEVELS, _lib.RC_MOTION_MAX_RANGE, 2
SLOTS = ("dx", "dy", "cost", "texture")                   # vectors[..., k]


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int, got {v!r}")
    return v


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number, got {v!r}")
    return float(v)


class MotionState:
    """What the estimator carries from one forward_mosaic call to the next: `levels`, the last frame's pyramid (a list of uint8 device
    tensors) or None.  reset() drops it (a scene cut): the next call estimates its frame against itself.  One state serves one stream (or
    the B streams of a batch); a call whose frame has another shape or device than the state starts over."""

    def __init__(self):
        self.levels = None
        self._spare = None                       # the buffers the call after next writes: forward_mosaic swaps the two sets

    def reset(self) -> None:
        self.levels = None

    @staticmethod
    def _fits(levels, shapes, device) -> bool:
        return levels is not None and len(levels) == len(shapes) and all(tuple(t.shape) == s and t.device == device for t, s in zip(levels, shapes))

    def matches(self, shapes, device) -> bool:
        """The state continues a frame whose pyramid has these level shapes on this device."""
        return self._fits(self.levels, shapes, device)


@dataclass(frozen=True, eq=False)
class Motion:
    """Block motion vectors of a frame against the previous one, as an output format: Output(Motion(...)) or out_format=Motion(...).

    levels  1 .. 4 pyramid levels; level k halves level k - 1 (2 x 2 rounded means of the luma code).
    block   8, 16 or 32: the matching block, at every level.
    search  1 .. 8: the range of the full search at the coarsest level, in that level's pixels.
    refine  0 .. 2: the range around the doubled vector of the level above, at every finer level.
    matrix  "bt601" / "bt709" / "bt2020": the luma coefficients.
    state   None (the frame is estimated against itself: zero vectors, zero cost, the real texture) or a MotionState.
    The reach is about (search 2^(levels-1) + refine (2^(levels-1) - 1)) pixels per axis.  Compared by identity (a state rides in it).
    """

    levels: int = 3
    block: int = 16
    search: int = 4
    refine: int = 1
    matrix: str = "bt709"
    state: Optional[MotionState] = None

    def __post_init__(self):
        if not 1 <= _int("Motion.levels", self.levels) <= MAX_LEVELS:
            raise ValueError(f"Motion.levels must lie in 1 .. {MAX_LEVELS}, got {self.levels}")
        if _int("Motion.block", self.block) not in BLOCKS:
            raise ValueError(f"Motion.block must be one of {BLOCKS}, got {self.block}")
        if not 1 <= _int("Motion.search", self.search) <= MAX_RANGE:
            raise ValueError(f"Motion.search must lie in 1 .. {MAX_RANGE}, got {self.search}")
        if not 0 <= _int("Motion.refine", self.refine) <= MAX_REFINE:
            raise ValueError(f"Motion.refine must lie in 0 .. {MAX_REFINE}, got {self.refine}")
        if not isinstance(self.matrix, str) or self.matrix not in MATRICES:
            raise ValueError(f"Motion.matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if self.state is not None and not isinstance(self.state, MotionState):
            raise TypeError(f"Motion.state must be None or a MotionState, got {type(self.state).__name__}")

    def level_shapes(self, batch: int, h: int, w: int):
        """The pyramid's level shapes [(B, h >> k, w >> k), ...] of an (h, w) frame."""
        return [(int(batch), int(h) >> k, int(w) >> k) for k in range(self.levels)]

    def check(self, h: int, w: int) -> Tuple[int, int]:
        """(by, bx), the grid of vectors of an (h, w) frame; every refusal that depends on the frame is raised here, before any launch."""
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"Motion: the frame {(h, w)} is empty")
        if h * w >= 1 << 29:
            raise ValueError(f"Motion: a frame of {(h, w)} has 2^29 samples or more")
        top = self.levels - 1
        if (h >> top) < self.block or (w >> top) < self.block:
            raise ValueError(f"Motion: level {top} of a {(h, w)} frame is {(h >> top, w >> top)}, smaller than one block of {self.block}")
        return h // self.block, w // self.block


class MotionField:
    """The motion of a batch of frames (ops.motion_estimate, Output(Motion(...))).

    vectors  (B, by, bx, 4) int32 on the device: per block of level 0 (dx, dy, cost, texture) -- the block's content sits at (x + dx, y + dy) of
             the reference frame; cost is the sum of absolute luma-code differences there, texture the block's own gradient sum.
    spec     the Motion that asked;  frame  the (h, w) estimated;  levels  the per-level results, levels[k] of pyramid level k (levels[0] is
             `vectors`).
    """

    __slots__ = ("vectors", "spec", "frame", "levels")

    def __init__(self, vectors, spec: Motion, frame, levels):
        self.vectors, self.spec, self.frame, self.levels = vectors, spec, tuple(int(v) for v in frame), tuple(levels)

    def valid(self, min_texture: int = 0, max_sad: Optional[int] = None):
        """(B, by, bx) bool: the blocks with texture >= min_texture and cost <= max_sad (None: any cost).  No synchronisation."""
        ok = self.vectors[..., 3] >= int(min_texture)
        return ok if max_sad is None else ok & (self.vectors[..., 2] <= int(max_sad))

    def global_shift(self, min_texture: int = 0, max_sad: Optional[int] = None):
        """(B, 2) int64 (dx, dy): per component the lower median over the valid blocks, 0 for a frame with none.  No synchronisation."""
        import torch
        v = self.vectors
        b = v.shape[0]
        ok = self.valid(min_texture, max_sad).reshape(b, -1, 1)
        d = v[..., :2].reshape(b, -1, 2).to(torch.int64)
        big = torch.iinfo(torch.int64).max
        ranked = torch.where(ok, d, torch.full_like(d, big)).sort(dim=1).values        # the valid ones first, ascending
        n = ok.sum(dim=1)                                                              # (B, 1)
        at = ((n - 1).clamp(min=0) // 2).expand(b, 2).unsqueeze(1)                     # the lower median's rank
        med = ranked.gather(1, at).squeeze(1)
        return torch.where(n > 0, med, torch.zeros_like(med))

    def mesh(self, size: Optional[Tuple[int, int]] = None, cell: int = 16, shift=None):
        """(B, Gh, Gw, 2) fp32 for ops.warp(y, mesh, size=size, cell=cell): node (j, i) = (i cell + sx, j cell + sy) with (sx, sy) = shift,
        a (B, 2) tensor (default: global_shift()).  size defaults to the frame.  No synchronisation."""
        import torch
        oh, ow = (int(s) for s in (self.frame if size is None else size))
        cell = _int("mesh: cell", cell)
        if oh < 1 or ow < 1 or cell < 1:
            raise ValueError(f"mesh: size {(oh, ow)} and cell {cell} must be positive")
        shift = self.global_shift() if shift is None else shift
        if shift.dim() != 2 or shift.shape[1] != 2 or shift.shape[0] not in (1, self.vectors.shape[0]):
            raise ValueError(f"mesh: shift must be (B, 2) or (1, 2), got {tuple(shift.shape)}")
        dev = self.vectors.device
        gh, gw = -(-oh // cell) + 1, -(-ow // cell) + 1
        xs = torch.arange(gw, device=dev, dtype=torch.float32) * cell
        ys = torch.arange(gh, device=dev, dtype=torch.float32) * cell
        base = torch.stack((xs[None, :].expand(gh, gw), ys[:, None].expand(gh, gw)), dim=-1)
        return base[None] + shift.to(device=dev, dtype=torch.float32)[:, None, None, :]

    def __repr__(self):
        return f"MotionField(vectors={tuple(self.vectors.shape)}, frame={self.frame}, spec={self.spec!r})"


class Stabilizer:
    """A global (translation) stabiliser: MotionFields in, meshes for ops.warp out.  Device state c (the camera's accumulated position)
    and s (its smoothed path), both (B, 2) fp32; nothing is synchronised.

    alpha      0 .. 1: how fast the smoothed path follows the camera.  1 follows at once (the identity mesh); 0 never (every frame is
               locked to the first).
    max_shift  >= 0: the correction is clamped to +- max_shift pixels per axis.
    update(field, size=None, cell=16, min_texture=0, max_sad=None) -> mesh:
        d = field.global_shift(...);  c <- c - d  (content at x in this frame sat at x + d in the last one);  s <- s + alpha (c - s);
        e = clamp(c - s, +- max_shift);  mesh = field.mesh(size, cell, shift=e).
    reset() starts over; a field of another batch or device does too.
    """

    def __init__(self, alpha: float = 0.1, max_shift: float = 64):
        self.alpha, self.max_shift = _number("Stabilizer.alpha", alpha), _number("Stabilizer.max_shift", max_shift)
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"Stabilizer.alpha must lie in 0 .. 1, got {alpha!r}")
        if not 0.0 <= self.max_shift < float("inf"):
            raise ValueError(f"Stabilizer.max_shift must be finite and >= 0, got {max_shift!r}")
        self.c = self.s = None

    def reset(self) -> None:
        self.c = self.s = None

    def update(self, field: MotionField, size=None, cell: int = 16, min_texture: int = 0, max_sad: Optional[int] = None):
        import torch
        if not isinstance(field, MotionField):
            raise TypeError(f"Stabilizer.update: field must be a MotionField, got {type(field).__name__}")
        d = field.global_shift(min_texture, max_sad).to(torch.float32)
        if self.c is None or self.c.shape != d.shape or self.c.device != d.device:
            self.c, self.s = torch.zeros_like(d), torch.zeros_like(d)
        self.c = self.c - d
        self.s = self.s + self.alpha * (self.c - self.s)
        e = (self.c - self.s).clamp(-self.max_shift, self.max_shift)
        return field.mesh(size, cell, shift=e)
