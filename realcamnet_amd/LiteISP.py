"""HIP-backed mirror of the reference ISP nets on the RAW->sRGB path (upstream models/LiteISP.py).

Class names, constructor signatures, attribute names (=> state_dict keys) and forward() contracts
follow the reference:
    x = [raw (B,4,H,W), cond (B,4,h,w), coord (B,2,H,W)]  ->  sRGB (B,3,2H,2W)
`forward` is the drop-in entry; `forward_mosaic` adds the ingest step the paper's figure shows in
front of it (Bayer unshuffle + pad_to_multiple_of_16 + crop), which upstream never published.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import networks as N
from . import ops
from .groupmix import GMA_Block, SUPPORTED_DTYPES
from ._lib import RC_OUT_NCHW, RC_OUT_PIXEL_SHUFFLE2
from .jpeg import Jpeg
from .out_format import OutFormat
from .stats import Stats
from .motion import Motion
from .resize import Output


def color_block(in_filters, out_filters, normalization=False):
    """Conv1x1 -> AvgPool(3,2,1) -> LeakyReLU(0.2) [-> InstanceNorm(affine)]; upstream LiteISP.py:23-30.
    The pooling/activation/norm modules are structural (they pin the Sequential indices and hold the
    affine parameters); execution is rc_color_block / rc_instance_stats."""
    layers = [N.Conv2d(in_filters, out_filters, 1, stride=1, padding=0),
              nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=True),
              nn.LeakyReLU(0.2)]
    if normalization:
        layers.append(nn.InstanceNorm2d(out_filters, affine=True))
    return layers


def pad_to_multiple_of_16(x):
    """Zero-pad NCHW x bottom/right to H,W % 16 == 0 (upstream LiteISP.py:84-105), on the device."""
    b, c, h, w = x.shape
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    return ops.to_nchw(ops.to_nhwc(x, pad_hw=(hp, wp))), (h, w)


def remove_padding(x_padded, original_size):
    """Crop the 2x output to 2*orig (upstream LiteISP.py:108-128)."""
    h, w = original_size
    return x_padded[:, :, :min(2 * h, x_padded.shape[-2]), :min(2 * w, x_padded.shape[-1])]


class Color_Condition_GFM(nn.Module):
    """Global colour prior (upstream LiteISP.py:345-361)."""

    def __init__(self, in_channels=4, out_c=32):
        super().__init__()
        self.model = nn.Sequential(
            *color_block(in_channels, 16, normalization=True),
            *color_block(16, 32, normalization=True),
            *color_block(32, 64, normalization=True),
            *color_block(64, 128, normalization=True),
            *color_block(128, 128),
            nn.Dropout(p=0.5),
            N.Conv2d(128, out_c, 1, stride=1, padding=0),
            nn.AdaptiveAvgPool2d(1),
        )

    def _vec(self, cond: torch.Tensor) -> torch.Tensor:
        """(B,4,h,w) NCHW cond image -> (B,out_c) fp32 vector; eval semantics (Dropout = identity)."""
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        m = self.model
        x, norm, stats = cond, None, None
        for blk in range(5):
            i = 4 * blk
            x = ops.color_block(x, m[i], norm, stats)
            if blk < 4:
                norm = m[i + 3]
                stats = ops.instance_stats(x, norm.eps)
            else:
                norm, stats = None, None
        return ops.color_head(x, m[20])

    def forward(self, img_input):
        v = self._vec(img_input)
        return v.to(img_input.dtype).view(v.shape[0], v.shape[1], 1, 1)


class Lens_Shading_Correction(N.HipModule):
    """4x Conv1x1 with LeakyReLU(0.1) between (upstream LiteISP.py:363-378)."""

    def __init__(self, in_channels=2, out_c=32, nf=32):
        super().__init__()
        self.model = N.Sequential(
            N.Conv2d(in_channels, nf, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            N.Conv2d(nf, nf, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            N.Conv2d(nf, nf, 1, 1),
            nn.LeakyReLU(negative_slope=0.1, inplace=True),
            N.Conv2d(nf, out_c, 1, 1),
        )

    def _nhwc(self, a):
        mods = list(self.model)
        convs, acts = mods[0::2], mods[1::2]
        if (all(isinstance(m, N.Conv2d) for m in convs) and all(isinstance(m, nn.LeakyReLU) for m in acts) and
                len(mods) == 2 * len(convs) - 1):
            slopes = [float(m.negative_slope) for m in acts]
            y = ops.lsc_chain(self, a)                          # all four layers in one launch, activations in registers
            if y is not None:
                return y
            if ops.pointwise_chain_ok(a, convs, slopes):       # the LDS-slab form (kept for rc_pointwise_chain48's callers)
                return ops.pointwise_chain(a, convs, slopes[0])
        return self.model._nhwc(a)


class Res_GFM(nn.Module):
    """GFT block (upstream LiteISP.py:537-559): conv0 -> f*scale+shift+f -> LeakyReLU(0.01) -> conv1 + x.
    Tuple in / tuple out so it chains inside Sequential like upstream."""

    def __init__(self, in_nc=32, chan=32, cond_c=32, out_nc=32, nf=64):
        super().__init__()
        self.conv0 = N.Conv2d(in_nc, chan, 3, 1, 1)
        self.conv1 = N.Conv2d(chan, chan, 3, 1, 1)
        self.GFM_scale_conv0 = nn.Linear(cond_c, nf)
        self.GFM_scale_conv1 = nn.Linear(nf, chan)
        self.GFM_shift_conv0 = nn.Linear(cond_c, nf)
        self.GFM_shift_conv1 = nn.Linear(nf, chan)
        self.out_nc = chan
        self.act = nn.LeakyReLU(inplace=True)

    def _nhwc(self, x):
        a, vec = x
        scale = ops.gfm_vector(vec, self.GFM_scale_conv0, self.GFM_scale_conv1)
        shift = ops.gfm_vector(vec, self.GFM_shift_conv0, self.GFM_shift_conv1)
        slope = float(self.act.negative_slope)
        if 0.0 <= slope <= 1.0 and ops.conv_pair_ok(a, self.conv0, self.conv1):
            return ops.conv_pair(a, self.conv0, self.conv1, act="leaky", slope=slope, film=(scale, shift), residual=a), vec
        f = self.conv0._nhwc(a, film=(scale, shift), act="leaky", slope=slope)
        return self.conv1._nhwc(f, residual=a), vec

    def forward(self, x):
        y, vec = self._nhwc((ops.to_nhwc(x[0]), x[1]))
        return ops.to_nchw(y), vec


class CB(nn.Module):
    """Conv1x1 -> AvgPool(3,2,1) -> LeakyReLU(0.2) [-> InstanceNorm(affine)] as a module (upstream LiteISP.py:215-230); executed
    inside Color_Condition_GFM_LFM through rc_color_block / rc_instance_stats like color_block()."""

    def __init__(self, in_filters, out_filters, normalization=False):
        super().__init__()
        self.conv = N.Conv2d(in_filters, out_filters, 1, stride=1, padding=0)
        self.pooling = nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=True)
        self.act = nn.LeakyReLU(0.2)
        self.normalization = normalization
        if normalization:
            self.norm = nn.InstanceNorm2d(out_filters, affine=True)

    def forward(self, x):
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        y = ops.color_block(x, self.conv)                       # fp32 NCHW like the colour branch
        return ops.instance_norm(y, self.norm) if self.normalization else y


class SFTLayer(nn.Module):
    """x0 * (scale(cond) + 1) + shift(cond), two 1x1-conv pairs on the condition MAP (upstream LiteISP.py:293-305)."""

    def __init__(self, cond_c=32, out_nc=64, nf=32):
        super().__init__()
        self.SFT_scale_conv0 = N.Conv2d(cond_c, nf, 1)
        self.SFT_scale_conv1 = N.Conv2d(nf, out_nc, 1)
        self.SFT_shift_conv0 = N.Conv2d(cond_c, nf, 1)
        self.SFT_shift_conv1 = N.Conv2d(nf, out_nc, 1)

    def _nhwc(self, x):
        fea, cond = x
        scale = self.SFT_scale_conv1._nhwc(self.SFT_scale_conv0._nhwc(cond, act="leaky", slope=0.1))
        shift = self.SFT_shift_conv1._nhwc(self.SFT_shift_conv0._nhwc(cond, act="leaky", slope=0.1))
        return ops.sft_apply(fea, scale, shift)                 # fea*scale + shift + fea

    def forward(self, x):
        return ops.to_nchw(self._nhwc((ops.to_nhwc(x[0]), ops.to_nhwc(x[1]))))


class GFMLayer(nn.Module):
    """x0 * scale(vec) + shift(vec) + x0 with two Linear pairs on the global vector (upstream LiteISP.py:308-321)."""

    def __init__(self, cond_c=32, out_nc=64, nf=32):
        super().__init__()
        self.GFM_scale_conv0 = nn.Linear(cond_c, nf)
        self.GFM_scale_conv1 = nn.Linear(nf, out_nc)
        self.GFM_shift_conv0 = nn.Linear(cond_c, nf)
        self.GFM_shift_conv1 = nn.Linear(nf, out_nc)
        self.out_nc = out_nc

    def _nhwc(self, x):
        fea, vec = x
        scale = ops.gfm_vector(vec, self.GFM_scale_conv0, self.GFM_scale_conv1)
        shift = ops.gfm_vector(vec, self.GFM_shift_conv0, self.GFM_shift_conv1)
        return ops.film_apply(fea, scale, shift)

    def forward(self, x):
        return ops.to_nchw(self._nhwc((ops.to_nhwc(x[0]), x[1])))


class Res_GFM_LFM(nn.Module):
    """Global (vector) + local (map) modulation block (upstream LiteISP.py:601-620): x0 + conv2(lfm(lrelu0.1(conv1(gfm(x0, vec))), map));
    triple in / triple out so it chains inside Sequential like upstream."""

    def __init__(self, cond_c=32, out_nc=32, nf=64):
        super().__init__()
        self.gfm = GFMLayer(cond_c=cond_c, out_nc=out_nc, nf=nf)
        self.conv1 = N.Conv2d(out_nc, out_nc, 3, 1, 1)
        self.lfm = SFTLayer(cond_c=cond_c, out_nc=out_nc, nf=out_nc)
        self.conv2 = N.Conv2d(out_nc, out_nc, 3, 1, 1)

    def _nhwc(self, x):
        a, vec, cmap = x
        f = self.conv1._nhwc(self.gfm._nhwc((a, vec)), act="leaky", slope=0.1)
        return self.conv2._nhwc(self.lfm._nhwc((f, cmap)), residual=a), vec, cmap

    def forward(self, x):
        y, vec, cmap = self._nhwc((ops.to_nhwc(x[0]), x[1], ops.to_nhwc(x[2])))
        return ops.to_nchw(y), vec, x[2]


class Color_Condition_GFM_LFM(nn.Module):
    """Global colour vector from the cond image + a local condition map from the RAW patch (upstream LiteISP.py:501-534)."""

    def __init__(self, in_channels=4, GFM_out_c=32, LFM_out_c=32):
        super().__init__()
        self.downblocks = nn.ModuleList([CB(in_channels, 16, True), CB(16, 32, True), CB(32, 64, True), CB(64, 128, True),
                                         CB(128, 256, True), CB(256, 384, False)])
        self.global_vector = nn.Sequential(nn.Dropout(p=0.8), N.Conv2d(384, GFM_out_c, 1, stride=1, padding=0), nn.AdaptiveAvgPool2d(1))
        # upstream builds a 3-layer cond_first and then overwrites the attribute with a single conv (:524-529); the RNG stream of the
        # discarded layers is consumed all the same, so they are constructed (and dropped) here too
        self.cond_first = nn.Sequential(N.Conv2d(in_channels, LFM_out_c, 3, 1, 1), nn.LeakyReLU(0.1, True), N.Conv2d(LFM_out_c, LFM_out_c, 1),
                                        nn.LeakyReLU(0.1, True), N.Conv2d(LFM_out_c, LFM_out_c, 1), nn.LeakyReLU(0.1, True))
        self.cond_first = nn.Sequential(N.Conv2d(in_channels, LFM_out_c, 3, 1, 1))

    def _run(self, global_raw, local_nhwc):
        """global_raw NCHW (B,4,h,w) -> vector (B,GFM_out_c) fp32; local_nhwc (B,H,W,4) -> local map NHWC (B,H,W,LFM_out_c)."""
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        x, norm, stats = ops._req(global_raw, "cond"), None, None
        for blk in self.downblocks:
            x = ops.color_block(x, blk.conv, norm, stats)
            if blk.normalization:
                norm, stats = blk.norm, ops.instance_stats(x, blk.norm.eps)
            else:
                norm, stats = None, None
        return ops.color_head(x, self.global_vector[1]), self.cond_first[0]._nhwc(local_nhwc)

    def forward(self, global_raw, local_patch):
        vec, lfm = self._run(global_raw, ops.to_nhwc(local_patch))
        return vec.to(global_raw.dtype).view(vec.shape[0], vec.shape[1], 1, 1), ops.to_nchw(lfm)


def _quad(mosaic, raw_format):
    """raw_format.quad (a QuadBayer): the sensor is Quad-Bayer.  ops.raw_quad (one launch) turns the frame -- every exposure of it, with
    Exposures(layout="frames"): (B,E,...) viewed as (B E,...) -- into an ordinary Bayer mosaic of the same cfa and levels: remosaiced at full
    size, or binned to half size (fp32).  Returns that mosaic and the format that describes it; every later stage reads it as it would a
    Bayer sensor's frame."""
    h2, w2 = raw_format.validate(mosaic.shape)                # every refusal, before any launch; the size of what leaves the stage
    one = dataclasses.replace(raw_format, exposures=None, defects=None, temporal=None, calibration=None, aberration=None)
    if raw_format.exposures is not None:                      # layout "frames": validate refuses "lines"
        b, e = mosaic.shape[0], mosaic.shape[1]
        out = ops.raw_quad(mosaic.reshape((b * e,) + tuple(mosaic.shape[2:])), one).view(b, e, h2, w2)
    else:
        out = ops.raw_quad(mosaic, one)
    storage = "float" if raw_format.quad.mode == "bin" or raw_format.storage == "float" else "u16"
    return out, dataclasses.replace(raw_format, quad=None, storage=storage, width=None)


def _merge_exposures(net, mosaic, raw_format):
    """raw_format.exposures (an Exposures): the tensor holds E exposures of each frame.  The defects stage, when asked for, runs on every
    exposure (layout "frames": (B,E,...) viewed as (B E,...); net.defect_counts is then (B,E,3)); ops.raw_hdr_merge (one launch) fuses them
    into one linear fp32 mosaic in the shortest exposure's code units.  Returns that mosaic and the format that describes it: storage
    "float", the same CFA and levels, the calibration kept for the next stage."""
    h2, w2 = raw_format.validate(mosaic.shape)                # also: "lines" with defects, a curve with exposures
    ex = raw_format.exposures
    if raw_format.defects is not None:
        b, e = mosaic.shape[0], ex.count
        one = dataclasses.replace(raw_format, exposures=None, calibration=None, temporal=None, aberration=None)
        fixed = ops.raw_defects(mosaic.reshape((b * e,) + tuple(mosaic.shape[2:])), one)
        if raw_format.defects.counts:
            fixed, counts = fixed
            net.__dict__["defect_counts"] = counts.view(b, e, 3)
        mosaic = fixed.view(b, e, h2, w2)
        raw_format = dataclasses.replace(raw_format, storage="float" if raw_format.storage == "float" else "u16", width=None, defects=None)
    merged = ops.raw_hdr_merge(mosaic, dataclasses.replace(raw_format, temporal=None))
    return merged, dataclasses.replace(raw_format, storage="float", width=None, exposures=None, defects=None)


def _temporal(mosaic, raw_format):
    """raw_format.temporal (a Temporal): ops.raw_temporal (one launch) filters the frame -- repaired and merged by now -- against the last
    filtered mosaic its TemporalState holds, and the result becomes the state: two buffers that swap from call to call.  An empty state, or
    one of another shape or device, starts over (the result is the decoded frame, state.field is None).  With Temporal(motion=...) and a
    state that continues, the block vectors of the frame against the state come first (_temporal_vectors), the filter reads the state
    displaced by them (still one launch) and state.field keeps them.  Returns the filtered fp32 mosaic and the format that describes it:
    storage "float", the same CFA and levels, the calibration kept for the next stage."""
    h2, w2 = raw_format.validate(mosaic.shape)
    st = raw_format.temporal.state
    shape = (mosaic.shape[0], h2, w2)
    prev = st.frame if st.matches(shape, mosaic.device) else None
    out = st._spare
    if out is None or out is prev or tuple(out.shape) != shape or out.device != mosaic.device:
        out = None
    tm = raw_format.temporal.motion
    st.field = None
    if tm is not None and prev is not None:
        st.field = _temporal_vectors(mosaic, raw_format, prev, st)
    st.frame, st._spare = ops.raw_temporal(mosaic, raw_format, prev=prev, out=out, vectors=st.field, block=16 if tm is None else tm.block), prev
    return st.frame, dataclasses.replace(raw_format, storage="float", width=None, defects=None, exposures=None, temporal=None)


def _temporal_vectors(mosaic, raw_format, prev, st):
    """Temporal(motion=TemporalMotion(...)) with a state that continues: the block vectors (B,by,bx,4) int32 of the frame against the state,
    in Bayer cells.  The luma-proxy pyramids of the frame and of the state (ops.raw_motion_pyramid, one launch each, into buffers the
    TemporalState keeps; the state is read as float storage with the frame's levels and Temporal.gain as its gain), ops.motion_estimate
    (`levels` launches), and the vectors of blocks with too little texture or too high a cost set to zero on the device: no host sync."""
    t = raw_format.temporal
    tm, spec = t.motion, t.motion.spec()
    b, h2, w2 = prev.shape
    of_frame, of_state = st.pyramids(spec.level_shapes(b, h2 // 2, w2 // 2), prev)
    cur = ops.raw_motion_pyramid(mosaic, raw_format, tm.levels, out=of_frame)
    state_format = dataclasses.replace(raw_format, storage="float", width=None, defects=None, exposures=None, aberration=None)
    ref = ops.raw_motion_pyramid(prev, state_format, tm.levels, gain=t.gain, out=of_state)
    field = ops.motion_estimate(cur, ref, spec)
    v = field.vectors
    if tm.min_texture > 0 or tm.max_sad is not None:
        v[..., :2] *= field.valid(tm.min_texture, tm.max_sad)[..., None]
    return v


def _temporal_check(raw_format):
    """What forward_mosaic asks of a temporal format before any stage runs."""
    from .temporal import Temporal, TemporalState
    t = raw_format.temporal
    if not isinstance(t, Temporal):
        raise TypeError(f"RawFormat.temporal must be None or a Temporal, got {type(t).__name__}")
    if not isinstance(t.state, TemporalState):
        raise ValueError("forward_mosaic: RawFormat.temporal needs a state (Temporal(state=TemporalState())): the filter carries the last "
                         "filtered frame from one call to the next")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("forward_mosaic with RawFormat.temporal cannot be captured: it swaps its state buffers between calls and a graph "
                           "would replay one direction of the swap forever.  Capture ops.raw_temporal(mosaic, raw_format, prev=, out=) on "
                           "explicit buffers instead")


def _ingest(net, mosaic, cond, dt, pad_to, black_level, white_level, cond_hw, raw_format=None):
    """Front end shared by every forward_mosaic: packed NHWC RAW (+ the cond image when the caller did not bring one).
    raw_format (a RawFormat): the sensor's CFA phase / storage / levels, decoded by the one-launch rc_raw_ingest_fmt.
    raw_format.defects (a Defects): the mosaic is repaired first (ops.raw_defects, one launch) and the ingest then reads the corrected,
    unpacked mosaic with the same CFA and levels; with defects.counts the (B,3) counts of this call are left in net.defect_counts.
    raw_format.calibration (a Calibration): the samples (repaired first, when defects is set too: its thresholds apply to the codes as
    delivered) are then linearised, normalised with the format's levels, flat-fielded, white-balanced and clipped by ops.raw_calibrate (one
    launch) into an fp32 mosaic, and the ingest reads that with storage "float" and levels 0 / 1: the packed RAW and the cond image are
    rounded to the network's type once, by the ingest, as without a calibration.
    raw_format.exposures (an Exposures): the tensor holds E exposures of each frame; they are repaired one by one and merged first
    (_merge_exposures), and the calibration and the ingest then read the merged fp32 mosaic with the same levels.
    raw_format.temporal (a Temporal): the repaired / merged frame is filtered against the last call's result (_temporal) in front of the
    calibration.
    raw_format.quad (a QuadBayer): a Quad-Bayer sensor's frame is remosaiced or binned to a Bayer mosaic first (_quad), and everything
    else reads that.  The order is quad, merge (with its per-exposure repair), repair, temporal, calibration, ingest.
    raw_format.stats (a RawStats): the mosaic that enters the calibration (or the ingest, where there is none) is measured by ops.raw_stats
    (one launch, no state: allowed under graph capture) in the format the preceding stage left -- the frame as delivered, unpacked uint16
    behind a repair, fp32 behind a merge or the filter -- and the RawFrameStats of this call is left in net.raw_stats, the way
    net.defect_counts is.  Nothing else changes.  Other taps are the op on its own; per-exposure statistics are ops.raw_stats on the
    (B E, 2h, X) view of the frame as delivered.
    raw_format.noise (a RawNoise): the mosaic that enters the temporal filter (or, without one, the next stage) is measured by
    ops.raw_noise (one launch, no state: allowed under graph capture) behind quad, merge and repair and IN FRONT of the filter -- the frame
    whose noise Temporal.noise describes; behind the filter that noise is gone -- and the RawNoiseStats of this call is left in
    net.raw_noise.  Nothing else changes.  Per-exposure noise is ops.raw_noise on the (B E, 2h, X) view of the frame as delivered.
    raw_format.aberration (an Aberration): the last box in front of the ingest.  ops.raw_aberration (one launch, no state: allowed under
    graph capture) resamples the R and B samples of the mosaic the calibration left (or, without one, of the frame as the preceding stage
    left it) inside their own colour's plane and keeps G; the ingest reads its fp32 result with the same CFA and levels.  The order is
    quad, merge, repair, noise tap, temporal, stats tap, calibration, aberration, ingest.
    raw_format.dng (a Dng): before anything else the mosaic AS DELIVERED is written as one DNG raw still per frame (ops.raw_dng, three
    launches, no state: allowed under graph capture) and the DngFrames of this call is left in net.raw_dng.  Nothing else changes.  As with
    net.raw_noise and net.raw_stats, a later call without the field leaves the attribute as it is: it holds the last call that wrote it.
    A cond the caller supplies is used as it is: it is NOT corrected and NOT calibrated."""
    if raw_format is not None and raw_format.dng is not None:
        net.__dict__["raw_dng"] = ops.raw_dng(mosaic, raw_format)
        raw_format = dataclasses.replace(raw_format, dng=None)
    need_cond = hasattr(net, "classifier") and cond is None and not getattr(net, "cond_from_raw", False)
    if raw_format is not None and raw_format.temporal is not None:
        _temporal_check(raw_format)
    if raw_format is not None and raw_format.quad is not None:
        mosaic, raw_format = _quad(mosaic, raw_format)
    if raw_format is not None and raw_format.exposures is not None:
        mosaic, raw_format = _merge_exposures(net, mosaic, raw_format)
    if raw_format is not None and raw_format.defects is not None:
        fixed = ops.raw_defects(mosaic, dataclasses.replace(raw_format, temporal=None))
        if raw_format.defects.counts:
            fixed, net.__dict__["defect_counts"] = fixed
        mosaic = fixed
        raw_format = dataclasses.replace(raw_format, storage="float" if raw_format.storage == "float" else "u16", width=None, defects=None)
    if raw_format is not None and raw_format.noise is not None:
        net.__dict__["raw_noise"] = ops.raw_noise(mosaic, raw_format)
        raw_format = dataclasses.replace(raw_format, noise=None)
    if raw_format is not None and raw_format.temporal is not None:
        mosaic, raw_format = _temporal(mosaic, raw_format)
    if raw_format is not None and raw_format.stats is not None:
        net.__dict__["raw_stats"] = ops.raw_stats(mosaic, raw_format)
        raw_format = dataclasses.replace(raw_format, stats=None)
    if raw_format is not None and raw_format.calibration is not None:
        mosaic = ops.raw_calibrate(mosaic, raw_format, dtype=torch.float32)
        raw_format = dataclasses.replace(raw_format, storage="float", width=None, black_level=0.0, white_level=1.0, defects=None, calibration=None)
    if raw_format is not None and raw_format.aberration is not None:
        mosaic = ops.raw_aberration(mosaic, raw_format)
        raw_format = dataclasses.replace(raw_format, storage="float", width=None, aberration=None)
    if raw_format is not None:
        a, c = ops.raw_ingest(mosaic, dtype=dt, pad_to=pad_to, black_level=black_level, white_level=white_level, cond_hw=cond_hw,
                              raw_format=raw_format)
        return a, (c if need_cond else cond)
    if need_cond or black_level != 0.0 or white_level != 1.0 or mosaic.dtype == torch.uint16:
        a, c = ops.raw_ingest(mosaic, dtype=dt, pad_to=pad_to, black_level=black_level, white_level=white_level, cond_hw=cond_hw)
        return a, (c if need_cond else cond)
    return ops.bayer_unshuffle(mosaic, dtype=dt, pad_to=pad_to), cond


def _mosaic_hw(mosaic, raw_format):
    """(2h, 2w) of the frame: the tensor's last two dimensions, or for MIPI-packed lines the height and raw_format.width; with
    raw_format.exposures, one exposure's."""
    if raw_format is None:
        return mosaic.shape[-2], mosaic.shape[-1]
    return raw_format.validate(mosaic.shape)


_OUT_BITS = {None: None, "rgb8": 8, "rgb16": 16}


def _out_bits(out_format):
    """What _encode does with the result: None (as it is), 8 / 16 (interleaved RGB), the OutFormat itself (an encoder surface), the Jpeg itself (compressed
    stills), the Stats itself (frame statistics) or the Motion itself (motion vectors)."""
    if isinstance(out_format, (OutFormat, Jpeg, Stats, Motion)):
        return out_format
    if out_format is not None and not isinstance(out_format, str):
        raise TypeError(f"out_format must be None, 'rgb8', 'rgb16', an OutFormat, a Jpeg, a Stats or a Motion, got {type(out_format).__name__}")
    if out_format not in _OUT_BITS:
        raise ValueError(f"out_format must be None, 'rgb8', 'rgb16', an OutFormat, a Jpeg, a Stats or a Motion, got {out_format!r}")
    return _OUT_BITS[out_format]


def _encode(y, bits):
    """out_format: the planar float sRGB (B,3,2h,2w) as it is, interleaved (B,2h,2w,3) uint8 / uint16 (rc_rgb_encode), a YuvFrames
    holding one Y'CbCr 4:2:0 / 4:2:2 / 4:4:4 surface per frame (rc_yuv_encode), a JpegFrames holding one JFIF file per frame (rc_jpeg_encode), a
    FrameStats (rc_frame_stats) or a MotionField (_motion)."""
    if bits is None:
        return y
    if isinstance(bits, Motion):
        return _motion(y, bits)
    if isinstance(bits, Stats):
        return ops.frame_stats(y, bits)
    if isinstance(bits, Jpeg):
        return ops.jpeg_encode(y, bits)
    return ops.yuv_encode(y, bits) if isinstance(bits, OutFormat) else ops.rgb_encode(y, bits)


def _motion(y, motion):
    """A Motion as a format: the luma pyramid of the frame (ops.motion_pyramid, one launch) is estimated (ops.motion_estimate, one launch
    per level) against the pyramid the Motion's state holds from the last call, and becomes the state: two sets of buffers that swap from
    call to call.  With no state, an empty one, or one of another shape or device, the frame is estimated against itself: zero vectors,
    zero cost, the real texture."""
    st = motion.state
    if st is None:
        cur = ops.motion_pyramid(y, motion.levels, motion.matrix)
        return ops.motion_estimate(cur, cur, motion)
    shapes = [tuple(s) for s in motion.level_shapes(y.shape[0], y.shape[2], y.shape[3])]
    prev = st.levels if st.matches(shapes, y.device) else None
    out = st._spare
    if out is None or out is prev or not st._fits(out, shapes, y.device):
        out = None
    cur = ops.motion_pyramid(y, motion.levels, motion.matrix, out=out)
    field = ops.motion_estimate(cur, cur if prev is None else prev, motion)
    st.levels, st._spare = cur, prev
    return field


def _motion_check(motion, hw):
    """What forward_mosaic asks of a Motion format before any stage runs."""
    if hw is not None:
        motion.check(*hw)
    if motion.state is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("forward_mosaic with a Motion that has a state cannot be captured: it swaps its pyramid buffers between calls and a "
                           "graph would replay one direction of the swap forever.  Capture ops.motion_pyramid(y, levels, out=) and "
                           "ops.motion_estimate(cur_levels, ref_levels, motion) on explicit buffers instead")


def _plan_outputs(outputs, out_format, hw):
    """forward_mosaic(outputs=[Output, ...]) checked before any launch: None, or the tuple of Outputs for an (h, w) result."""
    if outputs is None:
        if isinstance(out_format, Motion):
            _motion_check(out_format, hw)
        if isinstance(out_format, Stats):
            out_format.check(*hw)                         # the refusals that depend on the frame, as Output.plan raises them
        if isinstance(out_format, Jpeg):
            out_format.plan(*hw)
        return None
    if out_format is not None:
        raise ValueError("give either out_format or outputs, not both (an Output carries its own format)")
    if not isinstance(outputs, (list, tuple)):
        raise TypeError(f"outputs must be a list of Output, got {type(outputs).__name__}")
    for o in outputs:
        if not isinstance(o, Output):
            raise TypeError(f"outputs must be a list of Output, got an entry of type {type(o).__name__}")
        o.plan(*hw)
        if isinstance(o.format, Motion):
            _motion_check(o.format, None)                 # plan has checked the frame this output's stages leave
    return tuple(outputs)


def _emit(y, bits, outs):
    """The single result of the out_format route, or the list of renditions of `outs` in the order given: each an optional ops.warp (fp32)
    of the one float result, then an optional ops.resize (fp32), then an optional local tone mapping (ops.tone_map, fp32: three launches),
    then an optional colour look (ops.lut3d, fp32), then an optional sharpening (ops.sharpen, fp32), then the encoders of _encode."""
    if outs is None:
        return _encode(y, bits)
    res = []
    for o in outs:
        t = y if o.warp is None else ops.warp(y, o.warp)
        t = t if o.resize is None else ops.resize(t, o.resize)
        if o.tone is not None:
            t = ops.tone_map(t, o.tone)
        if o.look is not None:
            t = ops.lut3d(t, o.look)
        if o.sharpen is not None:
            t = ops.sharpen(t, o.sharpen)
        res.append(_encode(t, _out_bits(o.format)))
    return res


class _DwtUNet(nn.Module):
    """Shared trunk of the LiteISPNet family (upstream LiteISP.py:2019-2032, 2397-2409): Haar-DWT U-Net with RCAGroups; optional
    colour prior + Res_GFM modulation in front of each encoder level, optional lens-shading gain on the head."""

    output_dtype: Optional[torch.dtype] = None  # None: same as the parameters (reference semantics)
    cond_from_raw = False                       # LiteISPNet_GFMresize feeds the packed RAW itself to the colour prior

    def _build(self, ch_1, ch_2, ch_3, cond_c=None, lsc=False, nf=None, n_blocks=4):
        """Modules in the reference's construction order ([classifier], head, [lsc], [encoder_modulation i], down i, ..., tail),
        so torch.manual_seed(0) reproduces the reference's seed-0 parameters.  nf: Res_GFM hidden widths per level."""
        if cond_c is not None:
            self.classifier = Color_Condition_GFM(in_channels=4, out_c=cond_c)
        self.head = N.seq(N.conv(4, ch_1, mode='C'))
        if lsc:
            self.lsc = Lens_Shading_Correction(in_channels=2, out_c=ch_1, nf=ch_1)

        def gfm(i, c):
            if cond_c is not None:
                setattr(self, f"encoder_modulation{i}", N.seq(Res_GFM(in_nc=c, chan=c, cond_c=cond_c, out_nc=c, nf=nf[i - 1])))

        gfm(1, ch_1)
        self.down1 = N.seq(N.conv(ch_1, ch_1, mode='C'), N.RCAGroup(in_channels=ch_1, out_channels=ch_1, nb=n_blocks),
                           N.conv(ch_1, ch_1, mode='C'), N.DWTForward(ch_1))
        gfm(2, ch_1 * 4)
        self.down2 = N.seq(N.conv(ch_1 * 4, ch_1, mode='C'), N.RCAGroup(in_channels=ch_1, out_channels=ch_1, nb=n_blocks),
                           N.DWTForward(ch_1))
        gfm(3, ch_1 * 4)
        self.down3 = N.seq(N.conv(ch_1 * 4, ch_2, mode='C'), N.RCAGroup(in_channels=ch_2, out_channels=ch_2, nb=n_blocks),
                           N.DWTForward(ch_2))
        gfm(4, ch_2 * 4)
        self.middle = N.seq(N.conv(ch_2 * 4, ch_3, mode='C'), N.RCAGroup(in_channels=ch_3, out_channels=ch_3, nb=n_blocks),
                            N.RCAGroup(in_channels=ch_3, out_channels=ch_3, nb=n_blocks), N.conv(ch_3, ch_2 * 4, mode='C'))
        self.up3 = N.seq(N.DWTInverse(ch_2 * 4), N.RCAGroup(in_channels=ch_2, out_channels=ch_2, nb=n_blocks),
                         N.conv(ch_2, ch_1 * 4, mode='C'))
        self.up2 = N.seq(N.DWTInverse(ch_1 * 4), N.RCAGroup(in_channels=ch_1, out_channels=ch_1, nb=n_blocks),
                         N.conv(ch_1, ch_1 * 4, mode='C'))
        self.up1 = N.seq(N.DWTInverse(ch_1 * 4), N.RCAGroup(in_channels=ch_1, out_channels=ch_1, nb=n_blocks),
                         N.conv(ch_1, ch_1, mode='C'))
        self.tail = N.seq(N.conv(ch_1, ch_1 * 4, mode='C'), nn.PixelShuffle(upscale_factor=2), N.conv(ch_1, 3, mode='C'))

    def _act_dtype(self) -> torch.dtype:
        return self.head.weight.dtype

    def _refine_d1(self, d1):
        return d1

    def _check(self, raw):
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        if raw.dim() != 4 or raw.shape[1] != 4:
            raise ValueError(f"raw must be (B,4,H,W), got {tuple(raw.shape)}")
        if raw.shape[2] % 8 or raw.shape[3] % 8:
            raise ValueError(f"packed RAW H,W must be multiples of 8 (3 Haar levels), got {raw.shape[2]}x{raw.shape[3]}; "
                             "use forward_mosaic()/pad_to_multiple_of_16 for other sizes")

    def _front(self, a, cond, coord_nhwc):
        """head(raw) [* (lsc(coord) + 1)] and the colour-prior vector (None without a classifier)."""
        def head():
            if not hasattr(self, "lsc"):
                return self.head._nhwc(a)
            h = ops.lsc_chain(self.lsc, coord_nhwc, self.head, a)       # h = head(raw) * (lsc + 1), one launch when 48-wide bf16
            return h if h is not None else self.head._nhwc(a, mul_plus1=self.lsc._nhwc(coord_nhwc))

        if not hasattr(self, "classifier"):
            return head(), None
        # the colour prior is a chain of ~10 tiny launches on the (small) cond image: on a side stream it runs under the head conv
        cond = ops._req(cond, "cond")
        vec, h = ops.fork_join(lambda: self.classifier._vec(cond), head, [cond])
        return h, vec

    def _trunk(self, h, vec, crop_hw=None):
        mod = (lambda i, t: getattr(self, f"encoder_modulation{i}")._nhwc((t, vec))[0]) if vec is not None else (lambda i, t: t)
        h = mod(1, h)
        d1 = self._refine_d1(self.down1._nhwc(h))
        d2 = self.down2._nhwc(mod(2, d1))
        d3 = self.down3._nhwc(mod(3, d2))
        m = self.middle._nhwc(mod(4, d3), residual=d3)
        u3 = self.up3._nhwc(m, residual=d2)
        u2 = self.up2._nhwc(u3, residual=d1)
        u1 = self.up1._nhwc(u2, residual=h)
        if ops.tail_fold_ok(u1, self.tail[0], self.tail[2]):          # no activation between the two tail convs: one folded 5x5 launch + border ring
            return ops.tail_fold(u1, self.tail[0], self.tail[2], crop_hw=crop_hw, out_dtype=self.output_dtype)
        t = self.tail[0]._nhwc(u1, out_mode=RC_OUT_PIXEL_SHUFFLE2)
        return self.tail[2]._nhwc(t, out_mode=RC_OUT_NCHW, crop_hw=crop_hw, out_dtype=self.output_dtype)

    def forward(self, x: Sequence[torch.Tensor]):
        """x = [raw (B,4,H,W), cond (B,4,h,w), coord (B,2,H,W)] (nets without a prior / lens shading ignore those entries, as
        upstream does) -> sRGB (B,3,2H,2W)."""
        raw = x if isinstance(x, torch.Tensor) else x[0]
        self._check(raw)
        dt = self._act_dtype()
        coord_nhwc = None
        if hasattr(self, "lsc"):
            coord = x[2]
            if coord.shape[0] != raw.shape[0] or coord.shape[1] != 2 or coord.shape[2:] != raw.shape[2:]:
                raise ValueError(f"coord must be (B,2,H,W) matching raw, got {tuple(coord.shape)}")
            coord_nhwc = ops.to_nhwc(coord, dtype=dt)
        cond = (raw if self.cond_from_raw else x[1]) if hasattr(self, "classifier") else None
        h, vec = self._front(ops.to_nhwc(raw, dtype=dt), cond, coord_nhwc)
        return self._trunk(h, vec)

    def forward_mosaic(self, mosaic, cond=None, coord=None, pad_to: int = 16, black_level: float = 0.0, white_level: float = 1.0,
                       cond_hw=(256, 256), raw_format=None, out_format=None, outputs=None):
        """Bayer mosaic (B,1,2h,2w), cond (B,4,hc,wc), coord (B,2,h,w) -> sRGB (B,3,2h,2w).
        RAW and coord are zero-padded bottom/right to a multiple of `pad_to` (reference convention,
        upstream LiteISP.py:84-105) and the output is cropped back.  cond=None on a net with a colour prior: the fused ingest
        kernel (ops.raw_ingest) also produces cond = bilinear resize of the normalised packed RAW to `cond_hw`.
        raw_format (a RawFormat): the sensor frame's CFA phase, storage (MIPI RAW10 / RAW12 lines: (B,[1,]2h,line_bytes) uint8) and
        per-position levels.  out_format "rgb8" / "rgb16": the result as interleaved (B,2h,2w,3) uint8 / uint16; an OutFormat: a YuvFrames
        (one encoder surface per frame -- NV12 / P010 / I420, or a 4:2:2 / 4:4:4 / planar 10-bit / packed / v210 layout of OutFormat -- and views of its planes); a Stats: a FrameStats (the histograms and the 3A zone
        grid of the result, ops.frame_stats, in place of a picture); a Jpeg: a JpegFrames (one baseline JFIF file per frame, coded on the
        device, ops.jpeg_encode); a Motion: a MotionField (the block motion vectors of the result against the previous call's result, kept in
        the Motion's state; ops.motion_pyramid and ops.motion_estimate, in place of a picture).
        outputs [Output(format, resize, look, warp), ...] instead of out_format: one network pass, then per Output, in this order, an optional
        geometric correction (a Warp: ops.warp, fp32 out, whose size is the frame the next stages see), an optional scaled / cropped
        rendition (ops.resize, fp32) and an optional colour look (a Lut3D: ops.lut3d, fp32) in its own format; returns the list in the
        order given."""
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        bits = _out_bits(out_format)
        dt = self._act_dtype()
        mh, mw = _mosaic_hw(mosaic, raw_format)
        outs = _plan_outputs(outputs, out_format, (mh, mw))
        a, cond = _ingest(self, mosaic, cond, dt, pad_to, black_level, white_level, cond_hw, raw_format)
        b, hp, wp, _ = a.shape
        co = None
        if hasattr(self, "lsc"):
            if coord is None or coord.shape[-2:] != (mh // 2, mw // 2):
                raise ValueError("coord must be at packed resolution (h, w)")
            co = ops.to_nhwc(coord, dtype=dt, pad_hw=(hp, wp))
        if hasattr(self, "classifier") and self.cond_from_raw:
            cond = ops.to_nchw(a)                             # the padded packed RAW, as upstream's x[0]
        h, vec = self._front(a, cond, co)
        return _emit(self._trunk(h, vec, crop_hw=(mh, mw)), bits, outs)


class LiteISPNet(_DwtUNet):
    """upstream LiteISP.py:2322-2412 (reads only x[0])."""

    def __init__(self):
        super().__init__()
        self._build(64, 128, 128)


class LiteISPNet_GFM_LSC(_DwtUNet):
    """upstream LiteISP.py:1924-2035 -- the net the reference's __main__ builds."""

    def __init__(self):
        super().__init__()
        self._build(48, 128, 128, cond_c=32, lsc=True, nf=(48, 48, 48, 128))


class LiteISPNet_LSC(_DwtUNet):
    """upstream LiteISP.py:1710-1805: the 48-channel trunk with the lens-shading gain only (x[1] is ignored)."""

    def __init__(self):
        super().__init__()
        self._build(48, 128, 128, lsc=True)


class LiteISPNet_GFM(_DwtUNet):
    """upstream LiteISP.py:1809-1920: 64-channel trunk, colour prior (cond_c = 64) + Res_GFM modulation, no lens shading."""

    def __init__(self):
        super().__init__()
        self._build(64, 128, 128, cond_c=64, nf=(64, 64, 64, 128))


class LiteISPNet_GFMresize(_DwtUNet):
    """upstream LiteISP.py:2414-2520: as LiteISPNet_GFM with cond_c = 32, wider GFM MLPs, and the colour prior reading the packed
    RAW x[0] itself (:2496)."""
    cond_from_raw = True

    def __init__(self):
        super().__init__()
        self._build(64, 128, 128, cond_c=32, nf=(128, 256, 256, 512))


class _StridedUNet(nn.Module):
    """Shared body of the ISPUNet / ResUNet family (upstream LiteISP.py:963-1380, 2038-2146): widths chan,
    2chan, 4chan, 8chan; Conv2d(c, 2c, 2, 2) down-samplers; Conv1x1(c, 2c, bias=False) + PixelShuffle(2) up-samplers; RCAGroups of
    2 (middle: 4) blocks; optionally m_blocks Res_GFM per level on the way down AND up and the lens-shading gain on the intro.
    Modules are created in the reference's order ([classifier], intro, [lsc], [encoder_modulation1], encoder1, down1, ...), so the
    seed-0 parameters and the state_dict keys are identical."""

    output_dtype: Optional[torch.dtype] = None

    cond_from_raw = False        # ISPUNet_GFM_crop: the colour prior reads the packed RAW x[0] itself (upstream :928)
    coord_in_intro = False       # ISPUNet_GFM_LSC1: coord is concatenated to the RAW in front of a 6-channel intro conv (upstream :1497)
    skips = True                 # ISPUNet_GFM_LSC_noskip: no additive skips and no modulation on the way up (upstream :2626-2650)

    def _build(self, chan=32, cond_c=None, lsc=False, m_blocks=2, lsc_nf=None, intro_in=4, dec_gfm=True):
        n_blocks = 2
        if cond_c is not None:
            self.classifier = Color_Condition_GFM(in_channels=4, out_c=cond_c)

        def gfm(name, c):
            if cond_c is not None:
                setattr(self, name, N.seq(*[Res_GFM(in_nc=c, chan=c, cond_c=cond_c, out_nc=c, nf=c * 2) for _ in range(m_blocks)]))

        def lrelu():
            return nn.LeakyReLU(negative_slope=1e-1, inplace=True)

        self.intro = N.seq(N.Conv2d(intro_in, chan, 3, 1, 1))
        if lsc:
            self.lsc = Lens_Shading_Correction(in_channels=2, out_c=chan, nf=chan if lsc_nf is None else lsc_nf)
        gfm("encoder_modulation1", chan)
        self.encoder1 = N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down1 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        gfm("encoder_modulation2", chan)
        self.encoder2 = N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down2 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        gfm("encoder_modulation3", chan)
        self.encoder3 = N.seq(N.Conv2d(chan, chan, 3, 1, 1), N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks),
                              N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down3 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        gfm("middle_modulation", chan)
        self.middle = N.seq(N.Conv2d(chan, chan, 3, 1, 1), N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks * 2),
                            N.Conv2d(chan, chan, 3, 1, 1))
        for i in (3, 2, 1):
            setattr(self, f"up{i}", N.seq(N.Conv2d(chan, chan * 2, 1, bias=False), nn.PixelShuffle(2)))
            chan = chan // 2
            if dec_gfm:
                gfm(f"decoder_modulation{i}", chan)
            setattr(self, f"decoder{i}", N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.conv(chan, chan, mode='C')))
        self.tail = N.seq(N.conv(chan, chan * 4, mode='C'), nn.PixelShuffle(upscale_factor=2), N.conv(chan, 3, mode='C'))

    def _act_dtype(self) -> torch.dtype:
        return self.intro.weight.dtype

    def _run(self, a, cond, coord_nhwc, crop_hw=None):
        if self.coord_in_intro:                                          # intro(torch.cat([x[0], x[2]], dim=1)) as conv(raw) + conv(coord)
            w_raw, w_co = ops.split_conv_input_views(self.intro, (4, 2))
            intro = ops.conv2d(coord_nhwc, w_co, residual=ops.conv2d(a, w_raw))
        elif hasattr(self, "lsc"):
            intro = ops.lsc_chain(self.lsc, coord_nhwc, self.intro, a) if self.lsc.model[0].out_channels == self.intro.out_channels else None
            if intro is None:                                            # intro(raw) * (lsc + 1); lsc_chain fuses it for equal widths
                intro = self.intro._nhwc(a, mul_plus1=self.lsc._nhwc(coord_nhwc))
        else:
            intro = self.intro._nhwc(a)
        has_gfm = hasattr(self, "classifier")
        vec = self.classifier._vec(ops._req(cond, "cond")) if has_gfm else None

        def gfm(name, t):
            return getattr(self, name)._nhwc((t, vec))[0] if (has_gfm and hasattr(self, name)) else t

        def dec(i, t, skip):
            t = getattr(self, f"up{i}")._nhwc(t)
            if not self.skips:
                return getattr(self, f"decoder{i}")._nhwc(t)
            if has_gfm and hasattr(self, f"decoder_modulation{i}"):
                return ops.add(gfm(f"decoder_modulation{i}", getattr(self, f"decoder{i}")._nhwc(t)), skip)
            return getattr(self, f"decoder{i}")._nhwc(t, residual=skip)            # decoder's last conv takes the skip add

        d1 = self.down1._nhwc(self.encoder1._nhwc(gfm("encoder_modulation1", intro)))
        d2 = self.down2._nhwc(self.encoder2._nhwc(gfm("encoder_modulation2", d1)))
        d3 = self.down3._nhwc(self.encoder3._nhwc(gfm("encoder_modulation3", d2)))
        m = self.middle._nhwc(gfm("middle_modulation", d3), residual=d3 if self.skips else None)
        u1 = dec(1, dec(2, dec(3, m, d2), d1), intro)
        if ops.tail_fold_ok(u1, self.tail[0], self.tail[2]):          # no activation between the two tail convs: one folded 5x5 launch + border ring
            return ops.tail_fold(u1, self.tail[0], self.tail[2], crop_hw=crop_hw, out_dtype=self.output_dtype)
        t = self.tail[0]._nhwc(u1, out_mode=RC_OUT_PIXEL_SHUFFLE2)
        return self.tail[2]._nhwc(t, out_mode=RC_OUT_NCHW, crop_hw=crop_hw, out_dtype=self.output_dtype)

    def forward(self, x: Sequence[torch.Tensor]):
        raw = x if isinstance(x, torch.Tensor) else x[0]
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        if raw.dim() != 4 or raw.shape[1] != 4 or raw.shape[2] % 8 or raw.shape[3] % 8:
            raise ValueError(f"raw must be (B,4,H,W) with H,W multiples of 8 (three stride-2 levels), got {tuple(raw.shape)}")
        dt = self._act_dtype()
        co = None
        if hasattr(self, "lsc") or self.coord_in_intro:
            coord = x[2]
            if coord.shape[0] != raw.shape[0] or coord.shape[1] != 2 or coord.shape[2:] != raw.shape[2:]:
                raise ValueError(f"coord must be (B,2,H,W) matching raw, got {tuple(coord.shape)}")
            co = ops.to_nhwc(coord, dtype=dt)
        cond = (raw if self.cond_from_raw else x[1]) if hasattr(self, "classifier") else None
        return self._run(ops.to_nhwc(raw, dtype=dt), cond, co)

    def forward_mosaic(self, mosaic, cond=None, coord=None, pad_to: int = 16, black_level: float = 0.0, white_level: float = 1.0,
                       cond_hw=(256, 256), raw_format=None, out_format=None, outputs=None):
        """Bayer mosaic (B,1,2h,2w), cond, coord (B,2,h,w) -> sRGB (B,3,2h,2w) with the unshuffle / pad16 / crop front end
        (cond=None, raw_format, out_format, outputs: see _DwtUNet.forward_mosaic)."""
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        bits = _out_bits(out_format)
        dt = self._act_dtype()
        mh, mw = _mosaic_hw(mosaic, raw_format)
        outs = _plan_outputs(outputs, out_format, (mh, mw))
        a, cond = _ingest(self, mosaic, cond, dt, pad_to, black_level, white_level, cond_hw, raw_format)
        b, hp, wp, _ = a.shape
        co = None
        if hasattr(self, "lsc") or self.coord_in_intro:
            if coord is None or coord.shape[-2:] != (mh // 2, mw // 2):
                raise ValueError("coord must be at packed resolution (h, w)")
            co = ops.to_nhwc(coord, dtype=dt, pad_hw=(hp, wp))
        if hasattr(self, "classifier") and self.cond_from_raw:
            cond = ops.to_nchw(a)                             # the padded packed RAW, as upstream's x[0]
        return _emit(self._run(a, cond, co, crop_hw=(mh, mw)), bits, outs)


class ISPUNet_GFM_LSC(_StridedUNet):
    """upstream LiteISP.py:1228-1380: colour prior + Res_GFM on both sides + lens shading."""

    def __init__(self, cond_c=32, chan=32, m_blocks=2):
        super().__init__()
        self._build(chan=chan, cond_c=cond_c, lsc=True, m_blocks=m_blocks)


class ISPUNet_GFM(_StridedUNet):
    """upstream LiteISP.py:963-1110: ISPUNet_GFM_LSC without the lens-shading branch (x[2] is ignored)."""

    def __init__(self):
        super().__init__()
        self._build(chan=32, cond_c=32, lsc=False, m_blocks=2)


class ISPUNet_LSC(_StridedUNet):
    """upstream LiteISP.py:1113-1225: the strided U-Net with the lens-shading gain only (x[1] is ignored)."""

    def __init__(self):
        super().__init__()
        self._build(chan=32, cond_c=None, lsc=True)


class ResUNet(_StridedUNet):
    """upstream LiteISP.py:2038-2146: the bare strided U-Net (reads only x[0])."""

    def __init__(self):
        super().__init__()
        self._build(chan=32)


class ISPUNet_GFM_crop(_StridedUNet):
    """upstream LiteISP.py:811-960: ISPUNet_GFM at 64 channels, cond_c = 64, one Res_GFM per level, and the colour prior reading the
    packed RAW x[0] itself (:928) -- "its own crop as the global condition"."""
    cond_from_raw = True

    def __init__(self):
        super().__init__()
        self._build(chan=64, cond_c=64, lsc=False, m_blocks=1)


class ISPUNet_GFM_LSC1(_StridedUNet):
    """upstream LiteISP.py:1382-1532: the position code is concatenated to the RGGB planes (intro = Conv2d(6, 32, 3)) instead of going
    through a Lens_Shading_Correction branch."""
    coord_in_intro = True

    def __init__(self):
        super().__init__()
        self._build(chan=32, cond_c=32, lsc=False, m_blocks=2, intro_in=6)


class ISPUNet_GFM_LSC_noskip(_StridedUNet):
    """upstream LiteISP.py:2522-2652: ISPUNet_GFM_LSC with one Res_GFM per level on the way down only, no additive skips (middle,
    decoders) and a lens-shading MLP of hidden width lsc_c."""
    skips = False

    def __init__(self, cond_c=32, lsc_c=32):
        super().__init__()
        self._build(chan=32, cond_c=cond_c, lsc=True, m_blocks=1, lsc_nf=lsc_c, dec_gfm=False)


class ISPUNet_GFM_LFM(nn.Module):
    """upstream LiteISP.py:1535-1707: the strided U-Net with GLOBAL + LOCAL modulation -- Color_Condition_GFM_LFM gives a colour vector
    (from x[1]) and a condition map (3x3 conv of the packed RAW x[0]); CondNet1..4 bring the map to the four resolutions; every level's
    Res_GFM_LFM applies GFMLayer (vector) and SFTLayer (map).  Same construction order and attribute names as upstream."""

    output_dtype: Optional[torch.dtype] = None

    def __init__(self, cond_c=32, n_blocks=2, modulation_blocks=1, chan=32):
        super().__init__()
        self.cond_c = cond_c
        self.classifier = Color_Condition_GFM_LFM(in_channels=4, GFM_out_c=cond_c, LFM_out_c=cond_c)
        self.chan, self.n_blocks, self.modulation_blocks = chan, n_blocks, modulation_blocks

        def mod(c):
            return N.seq(*[Res_GFM_LFM(cond_c=cond_c, out_nc=c, nf=c * 2) for _ in range(modulation_blocks)])

        def lrelu():
            return nn.LeakyReLU(negative_slope=1e-1, inplace=True)

        self.intro = N.seq(N.Conv2d(4, chan, 3, 1, 1))
        self.encoder_modulation1 = mod(chan)
        self.encoder1 = N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down1 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        self.encoder_modulation2 = mod(chan)
        self.encoder2 = N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down2 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        self.encoder_modulation3 = mod(chan)
        self.encoder3 = N.seq(N.Conv2d(chan, chan, 3, 1, 1), N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks),
                              N.Conv2d(chan, chan, 3, 1, 1), lrelu())
        self.down3 = N.Conv2d(chan, chan * 2, 2, 2)
        chan = chan * 2
        self.middle_modulation = mod(chan)
        self.middle = N.seq(N.Conv2d(chan, chan, 3, 1, 1), N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks * 2),
                            N.Conv2d(chan, chan, 3, 1, 1))
        for i in (3, 2, 1):
            setattr(self, f"up{i}", N.seq(N.Conv2d(chan, chan * 2, 1, bias=False), nn.PixelShuffle(2)))
            chan = chan // 2
            setattr(self, f"decoder_modulation{i}", mod(chan))
            setattr(self, f"decoder{i}", N.seq(N.RCAGroup(in_channels=chan, out_channels=chan, nb=n_blocks), N.conv(chan, chan, mode='C')))
        self.tail = N.seq(N.conv(chan, chan * 4, mode='C'), nn.PixelShuffle(upscale_factor=2), N.conv(chan, 3, mode='C'))
        c = cond_c
        self.CondNet1 = N.Sequential(N.Conv2d(c, c, 1), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 1))
        self.CondNet2 = N.Sequential(N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 1))
        self.CondNet3 = N.Sequential(N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 1))
        self.CondNet4 = N.Sequential(N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True),
                                     N.Conv2d(c, c, 2, 2), nn.LeakyReLU(0.1, True), N.Conv2d(c, c, 1))

    def _act_dtype(self) -> torch.dtype:
        return self.intro.weight.dtype

    def _run(self, a, cond, crop_hw=None):
        intro = self.intro._nhwc(a)
        vec, lfm = self.classifier._run(cond, a)
        l1, l2, l4, l8 = (getattr(self, f"CondNet{i}")._nhwc(lfm) for i in (1, 2, 3, 4))

        def mod(name, t, cmap):
            return getattr(self, name)._nhwc((t, vec, cmap))[0]

        d1 = self.down1._nhwc(self.encoder1._nhwc(mod("encoder_modulation1", intro, l1)))
        d2 = self.down2._nhwc(self.encoder2._nhwc(mod("encoder_modulation2", d1, l2)))
        d3 = self.down3._nhwc(self.encoder3._nhwc(mod("encoder_modulation3", d2, l4)))
        m = self.middle._nhwc(mod("middle_modulation", d3, l8), residual=d3)
        u3 = ops.add(mod("decoder_modulation3", self.decoder3._nhwc(self.up3._nhwc(m)), l4), d2)
        u2 = ops.add(mod("decoder_modulation2", self.decoder2._nhwc(self.up2._nhwc(u3)), l2), d1)
        u1 = ops.add(mod("decoder_modulation1", self.decoder1._nhwc(self.up1._nhwc(u2)), l1), intro)
        if ops.tail_fold_ok(u1, self.tail[0], self.tail[2]):          # no activation between the two tail convs: one folded 5x5 launch + border ring
            return ops.tail_fold(u1, self.tail[0], self.tail[2], crop_hw=crop_hw, out_dtype=self.output_dtype)
        t = self.tail[0]._nhwc(u1, out_mode=RC_OUT_PIXEL_SHUFFLE2)
        return self.tail[2]._nhwc(t, out_mode=RC_OUT_NCHW, crop_hw=crop_hw, out_dtype=self.output_dtype)

    def forward(self, x: Sequence[torch.Tensor]):
        raw, cond = x[0], x[1]
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        if raw.dim() != 4 or raw.shape[1] != 4 or raw.shape[2] % 8 or raw.shape[3] % 8:
            raise ValueError(f"raw must be (B,4,H,W) with H,W multiples of 8 (three stride-2 levels), got {tuple(raw.shape)}")
        return self._run(ops.to_nhwc(raw, dtype=self._act_dtype()), cond)

    def forward_mosaic(self, mosaic, cond=None, coord=None, pad_to: int = 16, black_level: float = 0.0, white_level: float = 1.0,
                       cond_hw=(256, 256), raw_format=None, out_format=None, outputs=None):
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        bits = _out_bits(out_format)
        mh, mw = _mosaic_hw(mosaic, raw_format)
        outs = _plan_outputs(outputs, out_format, (mh, mw))
        a, cond = _ingest(self, mosaic, cond, self._act_dtype(), pad_to, black_level, white_level, cond_hw, raw_format)
        return _emit(self._run(a, cond, crop_hw=(mh, mw)), bits, outs)


class LiteISPNet_GFM_LSC_GMA(LiteISPNet_GFM_LSC):
    """BUILD-DEFINED composition for BASELINE.json config 3 ("4K RAW->sRGB with GroupMix attention").

    Upstream defines GMA_Block (models/groupmix.py:274-299, copy at models/raw2bit.py:117-142) but wires it into
    no full model -- only the smoke test `test_gma` (models/raw2bit.py:4361-4367) instantiates it.  This class
    attaches one GMA_Block(dim=80, heads=8) as a residual refinement of the H/2-level feature d1 (192 ch):
        d1 <- d1 + gma_out( GMA_Block( gma_in(d1) ) ),   gma_in: Conv1x1 192->80, gma_out: Conv1x1 80->192
    i.e. N = (H/2)(W/2) tokens (522 240 at 4K), the placement SURVEY.md section 8d names.  Everything else is
    LiteISPNet_GFM_LSC unchanged (the extra modules are constructed last, so the base parameters keep the
    reference's seed-0 values).  oracle/liteisp_oracle.py restates the same composition for parity."""

    def __init__(self, gma_dim: int = 80, gma_heads: int = 8):
        super().__init__()
        c1 = self.down1[3].weight.shape[0]            # 4 * ch_1 = 192
        self.gma_in = N.Conv2d(c1, gma_dim, 1, 1, 0)
        self.gma = GMA_Block(gma_dim, gma_heads)
        self.gma_out = N.Conv2d(gma_dim, c1, 1, 1, 0)

    def _act_dtype(self) -> torch.dtype:
        dt = super()._act_dtype()
        ops.require_dtype(self.head.weight, SUPPORTED_DTYPES, type(self).__name__)     # the GroupMix block has no fp16 kernels: refused before any launch
        return dt

    def _refine_d1(self, d1):
        return self.gma._nhwc(d1, pre=self.gma_in, post=(self.gma_out, d1))          # gma_in + ConvPosEnc in the block's first launch, gma_out(GMA(.)) + d1 in its last
