"""Defective-pixel correction of forward_mosaic: which samples to repair (DefectMap, Defects) in front of the ingest
(include/realcam_hip.h, rc_raw_defects, fixes the arithmetic).

DefectMap is the factory map: one bit per mosaic sample, kept on the host and copied to a device once.  Defects is the request -- the map,
the dynamic hot / cold thresholds, whether the counts are wanted -- and rides in RawFormat(defects=...).  Pure Python: validation raises
ValueError / TypeError and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# The kernel's lane map (csrc/defects.hip): a lane holds LANE_PX consecutive samples of a row, a wave corrects WAVE_SPAN columns (62 lanes;
# the other two hold the halo), a block BLOCK_SPAN columns of BLOCK_ROWS rows.  Tests place widths, heights and defects on these seams.
LANE_PX = 4
WAVE_SPAN = 62 * LANE_PX
BLOCK_SPAN = 2 * WAVE_SPAN
BLOCK_ROWS = 64
COUNTS = ("mapped", "hot", "cold")               # counts[:, k]


def _size(size) -> Tuple[int, int]:
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in size):
        raise TypeError(f"DefectMap: size must be (H2, W2), two ints, got {size!r}")
    h2, w2 = size
    if h2 < 2 or w2 < 2 or h2 % 2 or w2 % 2:
        raise ValueError(f"DefectMap: a mosaic has an even, positive number of rows and columns, got {(h2, w2)}")
    return h2, w2


class DefectMap:
    """The static defect map of a sensor: one bit per mosaic sample, set = do not trust this photosite.

    words   (H2, ceil(W2 / 32)) uint32 on the host, read-only: sample (y, x) is bit x & 31 of words[y, x >> 5] (rc_raw_defects' layout);
            bits past W2 are zero.
    Immutable; equal and hashed by size and content.  device_words(device) hands out the device copy, made once per device.
    """

    def __init__(self, size, words: np.ndarray):
        h2, w2 = _size(size)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if words.shape != (h2, -(-w2 // 32)):
            raise ValueError(f"DefectMap: words must be {(h2, -(-w2 // 32))} for size {(h2, w2)}, got {words.shape}")
        if w2 % 32 and (words[:, -1] >> np.uint32(w2 % 32)).any():
            raise ValueError("DefectMap: bits past the last column must be zero")
        words.setflags(write=False)
        object.__setattr__(self, "size", (h2, w2))
        object.__setattr__(self, "words", words)
        object.__setattr__(self, "count", int(np.unpackbits(words.view(np.uint8)).sum()))
        object.__setattr__(self, "_hash", hash(((h2, w2), words.tobytes())))

    def __setattr__(self, name, value):
        raise AttributeError("DefectMap is immutable")

    @classmethod
    def from_coords(cls, size, coords) -> "DefectMap":
        """size (H2, W2) of the mosaic; coords: (y, x) pairs in mosaic coordinates, duplicates allowed."""
        h2, w2 = _size(size)
        words = np.zeros((h2, -(-w2 // 32)), dtype=np.uint32)
        for c in coords:
            if not isinstance(c, (tuple, list)) or len(c) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in c):
                raise TypeError(f"DefectMap.from_coords: a coordinate is (y, x), two ints, got {c!r}")
            y, x = int(c[0]), int(c[1])
            if not (0 <= y < h2 and 0 <= x < w2):
                raise ValueError(f"DefectMap.from_coords: {(y, x)} lies outside the {(h2, w2)} mosaic")
            words[y, x >> 5] |= np.uint32(1 << (x & 31))
        return cls((h2, w2), words)

    @classmethod
    def from_mask(cls, mask) -> "DefectMap":
        """mask: a (H2, W2) bool tensor (or array), True = defective.  A device tensor is copied to the host once, here."""
        import torch
        if isinstance(mask, torch.Tensor):
            if mask.dtype != torch.bool:
                raise TypeError(f"DefectMap.from_mask: expected a bool mask, got {mask.dtype}")
            mask = mask.detach().cpu().numpy()
        mask = np.asarray(mask)
        if mask.dtype != np.bool_:
            raise TypeError(f"DefectMap.from_mask: expected a bool mask, got {mask.dtype}")
        if mask.ndim != 2:
            raise ValueError(f"DefectMap.from_mask: expected (H2, W2), got {mask.shape}")
        h2, w2 = _size(tuple(int(v) for v in mask.shape))
        padded = np.zeros((h2, -(-w2 // 32) * 32), dtype=np.uint8)
        padded[:, :w2] = mask
        words = np.packbits(padded.reshape(h2, -1, 32), axis=-1, bitorder="little").view("<u4").reshape(h2, -1)
        return cls((h2, w2), words)

    def mask(self):
        """The map as a (H2, W2) bool tensor on the host."""
        import torch
        h2, w2 = self.size
        bits = np.unpackbits(self.words.astype("<u4").view(np.uint8).reshape(h2, -1), axis=-1, bitorder="little")[:, :w2]
        return torch.from_numpy(bits.astype(np.bool_))

    @property
    def pitch_bytes(self) -> int:
        return 4 * self.words.shape[1]

    def device_words(self, device):
        """The bitmap as an (H2, ceil(W2 / 32)) int32 tensor on `device`: uploaded once per device (ops.derived), then kept -- a video loop
        makes no host-to-device copy."""
        import torch
        from . import ops
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return ops.derived(self, ("device_words", str(device)), (), lambda: torch.from_numpy(self.words.view(np.int32).copy()).to(device))

    def __eq__(self, other):
        return isinstance(other, DefectMap) and self.size == other.size and np.array_equal(self.words, other.words)

    def __hash__(self):
        return self._hash

    def __repr__(self):
        return f"DefectMap(size={self.size}, count={self.count})"


def _threshold(name, t) -> Optional[Tuple[float, float]]:
    if t is None:
        return None
    if not isinstance(t, (tuple, list)) or len(t) != 2:
        raise TypeError(f"Defects.{name} must be None or (t_abs, t_rel), got {t!r}")
    if not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in t):
        raise TypeError(f"Defects.{name} must hold two numbers, got {t!r}")
    t = (float(t[0]), float(t[1]))
    if not all(math.isfinite(v) and v >= 0.0 for v in t):
        raise ValueError(f"Defects.{name}: both thresholds must be finite and >= 0, got {t}")
    return t


@dataclass(frozen=True)
class Defects:
    """What to repair on the mosaic before it is ingested: RawFormat(defects=Defects(...)) or ops.raw_defects.

    map     None or a DefectMap of the mosaic's size: its samples are replaced from the nearest good samples of the same colour (the
            mean of the pair, of H / V / D1 / D2, that differs least; a single neighbour where no pair is whole).
    hot     None or (t_abs, t_rel): a sample that exceeds the maximum hi of its good same-colour ring by more than
            t_abs + t_rel max(hi - black, 0) becomes hi.
    cold    None or (t_abs, t_rel): a sample below the ring's minimum lo by more than t_abs + t_rel max(lo - black, 0) becomes lo.
    counts  also return (B, 3) int64 on the device: samples replaced from the map, as hot, as cold (defects.COUNTS).
    Thresholds are in the storage's own units, as RawFormat's levels: counts for u8 / u16 / mipi10 / mipi12, the float scale for float.
    Single pass: neighbours are always source samples.  Frames holding NaN / Inf are outside the contract.
    """

    map: Optional[DefectMap] = None
    hot: Optional[Tuple[float, float]] = None
    cold: Optional[Tuple[float, float]] = None
    counts: bool = False

    def __post_init__(self):
        if self.map is not None and not isinstance(self.map, DefectMap):
            raise TypeError(f"Defects.map must be None or a DefectMap, got {type(self.map).__name__}")
        object.__setattr__(self, "hot", _threshold("hot", self.hot))
        object.__setattr__(self, "cold", _threshold("cold", self.cold))
        if not isinstance(self.counts, bool):
            raise TypeError(f"Defects.counts must be a bool, got {self.counts!r}")
        if self.map is None and self.hot is None and self.cold is None:
            raise ValueError("Defects: nothing enabled -- give a map, hot or cold")

    def check(self, h2: int, w2: int) -> None:
        """Refuse a map made for another mosaic size."""
        if self.map is not None and self.map.size != (int(h2), int(w2)):
            raise ValueError(f"Defects: the map is for a {self.map.size} mosaic, the frame is {(int(h2), int(w2))}")

    @property
    def flags(self) -> int:
        from . import _lib
        return (_lib.RC_DEFECT_HOT if self.hot is not None else 0) | (_lib.RC_DEFECT_COLD if self.cold is not None else 0)

    def thresholds(self) -> Tuple[float, float, float, float]:
        return (self.hot or (0.0, 0.0)) + (self.cold or (0.0, 0.0))
