"""How a sensor frame is laid out: the `raw_format=` argument of forward_mosaic / ops.raw_ingest (include/realcam_hip.h, rc_raw_format).

Pure Python: validation raises ValueError and never touches the GPU or the library.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

from . import _lib

CFAS = {"RGGB": _lib.RC_CFA_RGGB, "BGGR": _lib.RC_CFA_BGGR, "GRBG": _lib.RC_CFA_GRBG, "GBRG": _lib.RC_CFA_GBRG}
STORAGES = ("float", "u16", "u8", "mipi10", "mipi12")
PACKED_BITS = {"mipi10": 10, "mipi12": 12}
# packed slot k (0 R, 1 G of the R row, 2 G of the B row, 3 B) <- cell position (row * 2 + col) of that colour in the 2x2 cell
SLOT_POS = {"RGGB": (0, 1, 2, 3), "BGGR": (3, 2, 1, 0), "GRBG": (1, 0, 3, 2), "GBRG": (2, 3, 0, 1)}


@dataclass(frozen=True)
class RawFormat:
    """A sensor frame's layout and levels.

    cfa          colour of mosaic cell positions (0,0), (0,1), (1,0), (1,1): "RGGB" (default), "BGGR", "GRBG", "GBRG".  The packed map
                 keeps the RGGB slot meaning; each slot reads its colour's position in the same 2x2 cell.
    storage      "float" (the tensor's own fp32 / bf16 / fp16), "u16" (LSB-aligned counts), "u8", "mipi10", "mipi12" (MIPI CSI-2
                 packed lines: a (B,[1,]2h,line_bytes) uint8 tensor, bytes past a line's samples ignored).
    width        mosaic width 2w in samples; required for the MIPI storages (the tensor's last dimension is the line stride).
    black_level  one float, or four in CFA-position order (DNG BlackLevel order).
    white_level  must exceed every black level.
    exposures    None, or an Exposures: the tensor holds E = 2 .. 4 exposures of each frame, (B,E,2h,X) for its layout "frames" or
                 (B,[1,]E 2h,X) line-interleaved for "lines", and forward_mosaic merges them (ops.raw_hdr_merge) into one linear fp32
                 mosaic in the shortest exposure's code units -- after the defects stage, which then runs per exposure, and in front of
                 the calibration.  The levels are the shortest exposure's; a calibration must not carry a curve (the merge needs linear
                 samples), and layout "lines" takes no defects (de-interleave first).
    defects      None, or a Defects: forward_mosaic repairs the mosaic (ops.raw_defects: a static map and / or hot / cold thresholds, in
                 this storage's own units) before it ingests it.  A map must have the mosaic's size.
    temporal     None, or a Temporal: forward_mosaic runs the motion-adaptive recursive temporal filter (ops.raw_temporal, one launch) on
                 the linear sensor codes -- after the repair / the merge and in front of the calibration -- against the last filtered
                 frame, which its TemporalState carries from call to call (the B frames of a call are B streams).  The noise model is in
                 this storage's own code units and uses these black levels; a calibration must not carry a curve (the noise model needs
                 linear samples).  Temporal(motion=TemporalMotion(...)) compensates camera motion: block vectors are estimated on the
                 mosaic's luma proxy and the filter reads the state displaced by them.
    quad         None, or a QuadBayer: the sensor is Quad-Bayer (tetracell) -- `cfa` then names the colours of the four 2x2 blocks of the 4x4
                 tile (sample (y,x) has colour cfa[2 ((y>>1)&1) + ((x>>1)&1)]) and forward_mosaic first turns the frame into an ordinary
                 Bayer mosaic with this cfa and these levels (ops.raw_quad, one launch: mode "remosaic" at full size, "bin" at half size),
                 in front of every other stage -- per exposure with Exposures(layout="frames").  Height and width must be multiples of
                 4; validate then returns the size of what leaves the stage, and the other stages are checked against it.  It takes no
                 Exposures(layout="lines") (de-interleave first) and no Defects.map (the map addresses photosites that the stage mixes
                 or merges; hot / cold thresholds are fine).
    noise        None, or a RawNoise: forward_mosaic measures the noise of the mosaic that enters the temporal filter (or the calibration, or
                 the ingest, where there is none) -- after quad, merge and repair, and IN FRONT of the filter, whose Temporal.noise
                 describes exactly this frame -- with ops.raw_noise (one launch: per CFA colour and level bin a histogram of tile
                 energies) and leaves the RawNoiseStats in net.raw_noise; its temporal_noise() is the (n_abs, n_rel) a Temporal takes.
                 A measurement changes nothing the other stages do: every other op ignores the field.  The region and the tile are
                 checked against the cell size (h, w) of what leaves the quad stage; RawNoise.top defaults to white_level.
    calibration  None, or a Calibration: forward_mosaic then runs ops.raw_calibrate (a linearisation curve, these levels, a flat-field gain
                 map, white-balance gains, a clip) after the defects stage and ingests its fp32 result.  With a curve, black_level and
                 white_level are in the curve's linear units.  A gain map must have the node count the mosaic needs.
    stats        None, or a RawStats: forward_mosaic measures the mosaic that enters the calibration (or the ingest, where there is none) --
                 after quad, repair, merge and temporal, in linear black-subtracted codes and in front of the gains -- with ops.raw_stats
                 (one launch: per CFA colour a code histogram and a 3A zone grid in Bayer cells) and leaves the RawFrameStats in
                 net.raw_stats.  A measurement changes nothing the other stages do: every other op ignores the field.  The region and
                 the grid are checked against the cell size (h, w) of what leaves the quad stage; RawStats.top defaults to white_level.
    aberration   None, or an Aberration: forward_mosaic corrects the lens's lateral chromatic aberration (ops.raw_aberration, one launch)
                 behind the calibration and in front of the ingest: every R and every B sample is resampled inside its own colour's
                 h x w plane through a coarse mesh of shifts, G is kept, and the ingest reads the fp32 result with the same CFA and
                 levels.  Behind the calibration because a curve must be undone before samples are interpolated, and because the gain
                 map, the temporal state and a Defects.map address photosites.  The mesh must have the node count the mosaic that leaves
                 the quad stage needs.
    dng          None, or a Dng: forward_mosaic also writes the mosaic AS DELIVERED -- in front of quad, repair and every other stage -- as one
                 DNG raw still per frame (ops.raw_dng, three launches, no state: allowed under graph capture) and leaves the DngFrames in
                 net.raw_dng.  The file is the sensor's data; its tags carry what this format knows: the CFA phase (a 4x4 pattern with quad),
                 the levels, a Calibration.curve as LinearizationTable, host-number Calibration.gains as AsShotNeutral.  Nothing else
                 changes: every other op ignores the field.  Storage u16, u8, mipi10 or mipi12 (a DNG holds sensor codes), and no
                 exposures (write each exposure with ops.raw_dng on the (B E, 2h, X) view).  net.raw_dng holds the last call that wrote
                 it: a later call without the field leaves it as it is (as net.raw_noise and net.raw_stats).
    """

    cfa: str = "RGGB"
    storage: str = "float"
    width: Optional[int] = None
    black_level: Union[float, Tuple[float, float, float, float]] = 0.0
    white_level: float = 1.0
    dng: Optional[object] = None
    aberration: Optional[object] = None
    quad: Optional[object] = None
    noise: Optional[object] = None
    temporal: Optional[object] = None
    stats: Optional[object] = None
    exposures: Optional[object] = None
    defects: Optional[object] = None
    calibration: Optional[object] = None

    @property
    def packed(self) -> bool:
        return self.storage in PACKED_BITS

    def blacks(self) -> Tuple[float, float, float, float]:
        b = self.black_level
        if isinstance(b, (int, float)):
            return (float(b),) * 4
        return tuple(float(v) for v in b)

    def min_line_bytes(self, width: int) -> int:
        """Bytes of one MIPI-packed line of `width` samples."""
        return math.ceil(width * PACKED_BITS[self.storage] / 8)

    def _one_exposure(self, shape: Tuple[int, ...]) -> Tuple[int, ...]:
        """With exposures set: check the tensor's shape against the layout and return the shape (B, 2h, X) of ONE exposure; also the
        refusals that depend on the other fields."""
        from .exposures import Exposures
        ex = self.exposures
        if not isinstance(ex, Exposures):
            raise TypeError(f"RawFormat.exposures must be None or an Exposures, got {type(ex).__name__}")
        e = ex.count
        if ex.layout == "frames":
            if len(shape) != 4 or min(shape) < 1:
                raise ValueError(f"mosaic must be (B,E,2h,X) for Exposures(layout='frames'), got {shape}")
            if shape[1] != e:
                raise ValueError(f"mosaic holds {shape[1]} exposures (B,E,2h,X), Exposures.times has {e}")
            one = (shape[0],) + shape[2:]
        else:
            if len(shape) == 4 and shape[1] == 1:
                shape = (shape[0],) + shape[2:]
            if len(shape) != 3 or min(shape) < 1:
                raise ValueError(f"mosaic must be (B,[1,]E 2h,X) for Exposures(layout='lines'), got {shape}")
            if shape[1] % (2 * e):
                raise ValueError(f"line-interleaved mosaic of {e} exposures needs a multiple of {2 * e} rows (E 2h), got {shape[1]}")
            one = (shape[0], shape[1] // e, shape[2])
            if self.defects is not None:
                raise ValueError("Exposures(layout='lines') takes no defects: the defects stage reads whole frames -- de-interleave the lines "
                                 "into (B,E,2h,X) first")
            if self.quad is not None:
                raise ValueError("Exposures(layout='lines') takes no quad: the quad stage reads whole frames -- de-interleave the lines "
                                 "into (B,E,H,X) first")
        if self.calibration is not None and getattr(self.calibration, "curve", None) is not None:
            raise ValueError("a Calibration.curve cannot follow exposures: the merge needs linear samples -- linearise each exposure first")
        return one

    def validate(self, mosaic_shape: Sequence[int]) -> Tuple[int, int]:
        """Check this format against a mosaic tensor's shape (B,[1,]2h,X); returns the mosaic size (2h, 2w).  X is 2w for the sample
        storages and the line stride in bytes for the MIPI ones.  With exposures set the tensor is (B,E,2h,X) or (B,[1,]E 2h,X) (its layout)
        and the size returned is that of one exposure.  With quad set the size returned is that of the Bayer mosaic the quad stage hands on:
        (H, W), or (H/2, W/2) for mode "bin".  Raises ValueError."""
        if self.cfa not in CFAS:
            raise ValueError(f"RawFormat.cfa must be one of {sorted(CFAS)}, got {self.cfa!r}")
        if self.storage not in STORAGES:
            raise ValueError(f"RawFormat.storage must be one of {STORAGES}, got {self.storage!r}")
        b = self.black_level
        if not isinstance(b, (int, float)):
            if isinstance(b, (str, bytes)) or not hasattr(b, "__len__") or len(b) != 4 or not all(isinstance(v, (int, float)) for v in b):
                raise ValueError(f"RawFormat.black_level must be a float or four floats in CFA-position order, got {b!r}")
        if not isinstance(self.white_level, (int, float)) or not all(float(self.white_level) > v for v in self.blacks()):
            raise ValueError(f"RawFormat.white_level ({self.white_level!r}) must exceed every black level {self.blacks()}")
        shape = tuple(int(s) for s in mosaic_shape)
        if self.exposures is not None:
            shape = self._one_exposure(shape)
        if len(shape) == 4 and shape[1] == 1:
            shape = (shape[0],) + shape[2:]
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"mosaic must be (B,[1,]2h,X), got {tuple(mosaic_shape)}")
        _, h2, x = shape
        if h2 % 2:
            raise ValueError(f"mosaic height must be even, got {h2}")
        if self.packed:
            if self.width is None:
                raise ValueError(f"RawFormat.width is required for storage {self.storage!r}")
            w2 = self.width
        else:
            w2 = x if self.width is None else self.width
            if w2 != x:
                raise ValueError(f"RawFormat.width {self.width} does not match the mosaic width {x}")
        if not isinstance(w2, int) or w2 < 2 or w2 % 2:
            raise ValueError(f"mosaic width must be a positive even number of samples, got {w2!r}")
        if self.storage == "mipi10" and w2 % 4:
            raise ValueError(f"RAW10 packs 4 samples in 5 bytes: the mosaic width must be a multiple of 4, got {w2}")
        if self.packed and x < self.min_line_bytes(w2):
            raise ValueError(f"{self.storage} line of {w2} samples needs {self.min_line_bytes(w2)} bytes, the tensor's lines have {x}")
        if self.quad is not None:
            from .quad import QuadBayer
            if not isinstance(self.quad, QuadBayer):
                raise ValueError(f"RawFormat.quad must be None or a QuadBayer, got {type(self.quad).__name__}")
            if getattr(self.defects, "map", None) is not None:
                raise ValueError("a Defects.map cannot follow quad: the map addresses photosites that the remosaic has mixed or the binning "
                                 "has merged -- use the dynamic hot / cold tests, which run on the Bayer result")
            h2, w2 = self.quad.out_size(h2, w2)                # from here on: the Bayer mosaic that leaves the quad stage
        if self.exposures is not None:
            self.exposures.check(h2, w2, shape[0])
        if self.defects is not None:
            from .defects import Defects
            if not isinstance(self.defects, Defects):
                raise TypeError(f"RawFormat.defects must be None or a Defects, got {type(self.defects).__name__}")
            self.defects.check(h2, w2)
        if self.temporal is not None:
            from .temporal import Temporal
            if not isinstance(self.temporal, Temporal):
                raise TypeError(f"RawFormat.temporal must be None or a Temporal, got {type(self.temporal).__name__}")
            if self.calibration is not None and getattr(self.calibration, "curve", None) is not None:
                raise ValueError("a Calibration.curve cannot follow temporal: the noise model needs linear samples -- linearise the frame first")
            self.temporal.check(h2, w2, shape[0])
        if self.noise is not None:
            from .raw_noise import RawNoise
            if not isinstance(self.noise, RawNoise):
                raise TypeError(f"RawFormat.noise must be None or a RawNoise, got {type(self.noise).__name__}")
            self.noise.check(h2 // 2, w2 // 2)
            self.noise.top_value(self.white_level, self.blacks())
        if self.stats is not None:
            from .raw_stats import RawStats
            if not isinstance(self.stats, RawStats):
                raise TypeError(f"RawFormat.stats must be None or a RawStats, got {type(self.stats).__name__}")
            self.stats.check(h2 // 2, w2 // 2)
            self.stats.top_value(self.white_level, self.blacks())
        if self.calibration is not None:
            from .calibration import Calibration
            if not isinstance(self.calibration, Calibration):
                raise TypeError(f"RawFormat.calibration must be None or a Calibration, got {type(self.calibration).__name__}")
            self.calibration.check(h2, w2, shape[0])
        if self.aberration is not None:
            from .aberration import Aberration
            if not isinstance(self.aberration, Aberration):
                raise TypeError(f"RawFormat.aberration must be None or an Aberration, got {type(self.aberration).__name__}")
            self.aberration.check(h2, w2)
        if self.dng is not None:
            from .dng import PRECISION, Dng
            if not isinstance(self.dng, Dng):
                raise TypeError(f"RawFormat.dng must be None or a Dng, got {type(self.dng).__name__}")
            if self.storage not in PRECISION:
                raise ValueError(f"RawFormat.dng: a DNG holds sensor codes: storage must be one of {sorted(PRECISION)}, got {self.storage!r}")
            if self.exposures is not None:
                raise ValueError("RawFormat.dng cannot go with exposures: a file holds one exposure -- write each with ops.raw_dng on the "
                                 "(B E, 2h, X) view of the frames as delivered, with exposures=None")
        return h2, w2
