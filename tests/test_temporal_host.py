"""Temporal noise reduction (Temporal / TemporalState / rc_raw_temporal), CPU side: the restatement (tests/temporal_ref.py) against a scalar
loop with explicit per-op fp32 rounding on a 6 x 6 frame, its three exact identities, the 2 x 2 frame, the variance it removes measured
against theory, the branch shares of the GPU branch test's input, validation, the refusals of the other front-end ops, the C entry's
bad-argument table, a FakeTensorMode trace and the kernels' resources."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd.calibration import Calibration, Pwl
from realcamnet_amd.exposures import Exposures
from realcamnet_amd.temporal import Temporal, TemporalState
from temporal_ref import F32, TAPS, blacks_of, branch_shares, restated_temporal

# ---- 1. a 6 x 6 frame by a scalar loop ------------------------------------------------------------------------------------------------------
# Integer codes c and a fractional state s: the top-left 4 x 4 differs from its state by well under a noise level (u <= 1), the right two
# columns by a few noise levels (the ramp), the bottom two rows by far more (u >= ramp).  Every tap fallback of a 6 x 6 frame is live: rows
# 0, 1, 4, 5 and columns 0, 1, 4, 5 each lack one neighbour.
HAND_C = [[260, 300, 341, 282, 423, 364], [305, 346, 287, 428, 269, 310], [350, 291, 432, 273, 314, 455],
          [295, 436, 277, 318, 459, 300], [440, 281, 322, 463, 304, 345], [285, 326, 467, 308, 349, 390]]
HAND_D = [[0.5, -0.75, 1.25, -0.375, 7.5, -9.25], [-1.0, 0.625, -0.25, 1.125, -8.75, 6.5], [0.875, -0.5, 0.375, -1.375, 9.125, -7.625],
          [-0.125, 1.0, -0.875, 0.75, -6.25, 8.875], [70.5, -81.25, 64.75, -90.125, 77.5, -68.0], [-75.25, 66.5, -88.0, 72.375, -61.75, 84.625]]
HAND_BLACKS, HAND_PARAMS, HAND_GAIN = (64.0, 66.0, 62.0, 65.0), (3.0, 0.0078125, 0.1875, 3.5), 1.0078125


def hand_frame():
    c = torch.tensor(HAND_C, dtype=F32).unsqueeze(0)
    return c, torch.sub(c, torch.tensor(HAND_D, dtype=F32).unsqueeze(0))


def scalar_loop(c, s, blacks, params, gain=None):
    """The header's arithmetic, one sample at a time, every operation on numpy fp32 scalars (each is rounded to fp32 on its own); slope and
    1 / 9 are formed in double and rounded once.  c, s: (H, W) lists of numbers -> ((H, W) list of floats, (H, W) list of u)."""
    f = np.float32
    h, w = len(c), len(c[0])
    n_abs, n_rel, alpha, ramp = (f(v) for v in params)
    slope, ninth = f((1.0 - float(alpha)) / (float(ramp) - 1.0)), f(1.0 / 9.0)
    p = [[f(s[y][x]) if gain is None else f(blacks[2 * (y & 1) + (x & 1)]) + (f(s[y][x]) - f(blacks[2 * (y & 1) + (x & 1)])) * f(gain) for x in range(w)] for y in range(h)]
    e = [[abs(f(c[y][x]) - p[y][x]) for x in range(w)] for y in range(h)]
    out, us = [[0.0] * w for _ in range(h)], [[0.0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            acc = None
            for dy, dx in TAPS:
                ty = y + dy if 0 <= y + dy < h else y
                tx = x + dx if 0 <= x + dx < w else x
                acc = e[ty][tx] if acc is None else f(acc + e[ty][tx])
            b = f(blacks[2 * (y & 1) + (x & 1)])
            t = f(n_abs + f(n_rel * max(f(p[y][x] - b), f(0.0))))
            u = f(f(acc * ninth) / t)
            d = f(f(c[y][x]) - p[y][x])
            if u >= ramp:
                o = f(c[y][x])
            else:
                k = alpha if u <= f(1.0) else f(alpha + f(f(u - f(1.0)) * slope))
                o = f(p[y][x] + f(k * d))
            out[y][x], us[y][x] = float(o), float(u)
    return out, us


def hand_out(gain=None):
    c, s = hand_frame()
    return scalar_loop(c[0].tolist(), s[0].tolist(), HAND_BLACKS, HAND_PARAMS, gain)


def test_restatement_equals_the_scalar_loop_on_the_6x6_frame():
    c, s = hand_frame()
    for gain in (None, HAND_GAIN):
        want, us = hand_out(gain)
        got, info = restated_temporal(c, s, blacks_of(HAND_BLACKS, 6, 6), HAND_PARAMS, gain, details=True)
        assert got.dtype == F32 and got[0].tolist() == want and info["u"][0].tolist() == us
        assert bool((torch.tensor(us)[:2, :2] <= 1.0).all()) and bool((torch.tensor(us)[4:] >= 3.5).all())              # with the gain too
    _, us = hand_out()
    u = torch.tensor(us)
    assert bool((u[:2, :2] <= 1.0).all()) and bool(((u[:4, 4:] > 1.0) & (u[:4, 4:] < 3.5)).any()) and bool((u[4:] >= 3.5).all())     # all three branches
    out = torch.tensor(hand_out()[0])
    assert torch.equal(out[4:], torch.tensor(HAND_C, dtype=F32)[4:])                   # u >= ramp: the new frame exactly
    assert not torch.equal(out[:4], torch.tensor(HAND_C, dtype=F32)[:4])
    # a tensor gain, one row per frame: frame 1's gain of 1 is not the same as no gain only in its rounding, and here it is exact
    two = restated_temporal(c.expand(2, 6, 6), s.expand(2, 6, 6), blacks_of(HAND_BLACKS, 6, 6), HAND_PARAMS, torch.tensor([[HAND_GAIN], [1.0]]))
    assert two[0].tolist() == hand_out(HAND_GAIN)[0] and two[1].tolist() == hand_out(1.0)[0]


# ---- 2. the three exact identities, and the smallest frame -----------------------------------------------------------------------------------
def codes(b, h, w, seed, lo=64, hi=4096):
    return torch.randint(lo, hi, (b, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def far_state(c, blacks, params, seed):
    """A state that differs from the frame c (int32 codes) by more than ramp t everywhere, t taken at the state's own level: fp32."""
    g = torch.Generator().manual_seed(seed)
    n_abs, n_rel, _, ramp = params
    sign = torch.where(torch.rand(c.shape, generator=g) < 0.5, -1.0, 1.0)
    reach = 4096.0 + max(blacks)                                                   # |p - b| stays below this
    step = 1.25 * ramp * (n_abs + n_rel * reach) + torch.rand(c.shape, generator=g) * 16.0
    return (c.to(torch.float64) + sign * step).to(F32)


def test_the_three_identities_on_the_restatement():
    blacks, params = (64.0, 60.0, 68.0, 66.0), (6.0, 0.03125, 0.125, 3.0)
    c = codes(2, 10, 14, 1)
    cf, plane = c.to(F32), blacks_of(blacks, 10, 14)
    assert torch.equal(restated_temporal(cf, None, plane, params), cf)                                  # a reset
    assert torch.equal(restated_temporal(cf, cf.clone(), plane, params), cf)                            # a frame equal to its state
    s = far_state(c, blacks, params, 2)
    out, info = restated_temporal(cf, s, plane, params, details=True)
    assert bool((info["u"] >= 3.0).all()) and torch.equal(out, cf)                                      # motion everywhere
    assert not torch.equal(restated_temporal(cf, cf + 1.5, plane, params), cf)                          # and otherwise it does filter


def test_a_2x2_frame_takes_the_centre_nine_times():
    c = torch.tensor([[[300.0, 310.0], [320.0, 330.0]]])
    s = torch.tensor([[[301.25, 307.5], [320.0, 333.625]]])
    params = (2.0, 0.015625, 0.25, 4.0)
    out, info = restated_temporal(c, s, blacks_of((64.0,) * 4, 2, 2), params, details=True)
    want, us = scalar_loop(c[0].tolist(), s[0].tolist(), (64.0,) * 4, params)
    assert out[0].tolist() == want and info["u"][0].tolist() == us
    e = (c - s).abs()
    acc = e.clone()
    for _ in range(8):
        acc = torch.add(acc, e)                                                    # nine equal taps, added one by one
    t = 2.0 + 0.015625 * (s - 64.0)
    assert torch.equal(info["u"], torch.div(torch.mul(acc, torch.tensor(1.0 / 9.0, dtype=torch.float64).to(F32)), t))
    for shape in ((2, 4), (4, 2)):                                                 # one axis has neighbours, the other has none
        cc = codes(1, shape[0], shape[1], 3).to(F32)
        ss = cc + torch.linspace(-3.0, 3.0, shape[0] * shape[1]).reshape(1, *shape)
        assert restated_temporal(cc, ss, blacks_of((64.0,) * 4, *shape), params)[0].tolist() == scalar_loop(cc[0].tolist(), ss[0].tolist(), (64.0,) * 4, params)[0]


# ---- 3. what the stage is for ---------------------------------------------------------------------------------------------------------------
def test_static_scene_noise_variance_falls_to_alpha_over_two_minus_alpha():
    """out = p + alpha (c - p) with white noise of variance v in c is a first-order recursion whose output noise has the variance
    v alpha / (2 - alpha) once the start has decayed ((1 - alpha)^(2 N) = 0.75^80 = 1e-10 here).  The residual of the last frame is M =
    128 x 128 independent Gaussian samples, so its sample variance has the relative standard error sqrt(2 / (M - 1)) = 0.01105; the input
    variance is taken over all N M samples and adds sqrt(2 / (N M)) = 0.0017.  The margin is four standard errors of their sum in
    quadrature: 4 sqrt(0.01105^2 + 0.0017^2) = 0.0447.  sigma = 4 against a noise level of 64: the activity, a mean of nine |d| with
    E|d| < 1.2 sigma, never reaches t, which the test asserts (every sample takes u <= 1)."""
    g = torch.Generator().manual_seed(7)
    h = w = 128
    n, alpha, sigma = 40, 0.25, 4.0
    params = (64.0, 0.0, alpha, 3.0)
    ys, xs = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    scene = (800.0 + 3.0 * ys + 2.0 * xs).unsqueeze(0)
    plane = blacks_of((64.0,) * 4, h, w)
    state, noise_sq, u_max = None, 0.0, 0.0
    for _ in range(n):
        noise = torch.randn(1, h, w, generator=g, dtype=torch.float64) * sigma
        noise_sq += float((noise ** 2).sum())
        state, info = restated_temporal((scene + noise).to(F32), state, plane, params, details=True)
        if info is not None:
            u_max = max(u_max, float(info["u"].max()))
    assert 0.0 < u_max <= 1.0
    v_in = noise_sq / (n * h * w)
    v_out = float(((state.double() - scene) ** 2).mean())
    ratio, theory = v_out / v_in, alpha / (2.0 - alpha)
    margin = 4.0 * (2.0 / (h * w - 1) + 2.0 / (n * h * w)) ** 0.5
    assert round(margin, 4) == 0.0447
    assert abs(ratio / theory - 1.0) <= margin, (ratio, theory)


# ---- 4. the input of the GPU branch test ------------------------------------------------------------------------------------------------------
BRANCH_SHAPE, BRANCH_SEED = (2, 66, 260), 171


def scale_of(kind):
    return {"u16": 65536.0, "u8": 256.0, "mipi10": 1024.0, "mipi12": 4096.0}.get(kind, 1.0)


def request_of(kind, alpha=0.1875, ramp=3.0, **kw):
    """The noise model every GPU test uses, in the storage's code units: 1 / 256 of full scale plus 1 / 64 of the level."""
    return Temporal(noise=(scale_of(kind) / 256.0, 0.015625), alpha=alpha, ramp=ramp, **kw)


def stream_of(kind, b, h, w, seed, blacks, request=None):
    """A frame of storage `kind` on the host -- (B,H,W) int32 counts, or floats of the storage's dtype -- and a fractional fp32 state for
    it.  The state differs from the frame by uniform noise whose reach is fixed per 8 x 8 tile at 1, 4 or 16 noise levels, a third of
    the tiles each, so the activity sits below one noise level, on the ramp and past it in comparable shares."""
    g = torch.Generator().manual_seed(seed)
    s = scale_of(kind)
    t = request_of(kind) if request is None else request
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    black = torch.tensor(blacks, dtype=torch.float64)[2 * (ys & 1) + (xs & 1)] * s
    c = black + torch.rand(b, h, w, generator=g, dtype=torch.float64) * (0.75 * s)
    if kind in ("u16", "u8", "mipi10", "mipi12"):
        c = c.round().clamp(0, s - 1).to(torch.int32)
        cf = c.to(torch.float64)
    else:
        c = c.clamp(0.0, 1.0).to({"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[kind])
        cf = c.to(torch.float64)
    level = t.noise[0] + t.noise[1] * (cf - black).clamp_min(0.0)
    tiles = torch.randint(0, 3, (b, -(-h // 8), -(-w // 8)), generator=g)
    reach = torch.tensor([1.0, 4.0, 16.0], dtype=torch.float64)[tiles].repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :w]
    state = cf + (2.0 * torch.rand(b, h, w, generator=g, dtype=torch.float64) - 1.0) * reach * level
    return c, state.to(F32)


BRANCH_BLACKS = (0.0625, 0.0703125, 0.05859375, 0.06640625)


def test_the_gpu_branch_tests_input_holds_every_branch_in_the_restatement():
    for kind in ("u16", "mipi12", "fp32", "u8"):
        b, h, w = BRANCH_SHAPE
        c, state = stream_of(kind, b, h, w, BRANCH_SEED, BRANCH_BLACKS)
        t = request_of(kind)
        _, info = restated_temporal(c.to(F32), state, blacks_of(tuple(v * scale_of(kind) for v in BRANCH_BLACKS), h, w), t.params(), details=True)
        shares = branch_shares(info)
        assert abs(sum(shares) - 1.0) < 1e-6 and min(shares) >= 0.1, (kind, shares)


# ---- 5. validation --------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def test_temporal_validation():
    st = TemporalState()
    t = Temporal(noise=(4, 0.25), alpha=0.125, ramp=3, gain=2, state=st)
    assert t.noise == (4.0, 0.25) and t.alpha == 0.125 and t.ramp == 3.0 and t.gain == 2.0 and t.state is st and not t.device_gain
    assert t.params() == (4.0, 0.25, 0.125, 3.0)
    assert Temporal((0.1, 0.0)).noise == (float(np.float32(0.1)), 0.0) and Temporal((1, 0), alpha=0.1).alpha == float(np.float32(0.1))   # the fp32 values the kernel gets
    d = Temporal((1, 0))
    assert (d.alpha, d.ramp, d.gain, d.state) == (0.125, 3.0, None, None) and Temporal((1, 0), alpha=1.0).alpha == 1.0
    assert d != Temporal((1, 0)) and d == d                                              # compared by identity
    for bad in ((0.0, 0.0), (-1.0, 0.0), (1.0, -0.5), (INF, 0.0), (1.0, INF), (NAN, 0.0), (1.0, NAN), (1e-46, 0.0), (1e39, 0.0)):
        with pytest.raises(ValueError, match="noise"):
            Temporal(noise=bad)
    for bad in (1.0, (1.0,), (1.0, 0.0, 0.0), ("1", 0.0), (True, 0.0), None, torch.ones(2)):
        with pytest.raises(TypeError, match="noise"):
            Temporal(noise=bad)
    for bad in (0.0, -0.5, 1.0 + 1e-6, 2.0, NAN, INF, 1e-46):
        with pytest.raises(ValueError, match="alpha"):
            Temporal((1, 0), alpha=bad)
    for bad in (1.0, 0.5, 1.0 + 1e-9, -3.0, NAN, INF, 1e39):
        with pytest.raises(ValueError, match="ramp"):
            Temporal((1, 0), ramp=bad)
    for name in ("alpha", "ramp"):
        for bad in ("1", None, True, (0.5,), torch.ones(())):
            with pytest.raises(TypeError, match=name):
                Temporal((1, 0), **{name: bad})
    for bad in (0.0, -1.0, NAN, INF, 1e-46, torch.ones(2), torch.ones(2, 2), torch.ones(0, 1), torch.ones(1, 1, 1)):
        with pytest.raises(ValueError, match="gain"):
            Temporal((1, 0), gain=bad)
    for bad in ("2", True, (2.0,), torch.ones(2, 1, dtype=torch.float64), torch.ones(2, 1, dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match="gain"):
            Temporal((1, 0), gain=bad)
    g = torch.ones(3, 1)
    held = Temporal((1, 0), gain=g)
    assert held.device_gain and held.gain is g                                             # used in place, never copied
    held.check(8, 8, 3)
    Temporal((1, 0), gain=torch.ones(1, 1)).check(8, 8, 5)
    with pytest.raises(ValueError, match="rows"):
        held.check(8, 8, 2)
    for bad in (1, "state", torch.ones(1, 2, 2), TemporalState):
        with pytest.raises(TypeError, match="state"):
            Temporal((1, 0), state=bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.alpha = 0.5
    assert {"Temporal", "TemporalState"} <= set(M.__all__) and M.Temporal is Temporal and M.TemporalState is TemporalState and "raw_temporal" in M.torch_ops.SCHEMAS
    assert "NOT checked" in Temporal.__doc__                                               # a gain tensor is trusted, and the docstring says so


def test_temporal_state_restarts_on_another_shape_or_device():
    st = TemporalState()
    assert st.frame is None and not st.matches((1, 4, 4), torch.device("cpu"))
    st.frame = torch.zeros(2, 4, 6)
    assert st.matches((2, 4, 6), torch.device("cpu")) and st.matches(torch.Size((2, 4, 6)), st.frame.device)
    for shape in ((1, 4, 6), (2, 6, 4), (2, 4, 8), (2, 4), (2, 1, 4, 6)):
        assert not st.matches(shape, torch.device("cpu"))
    assert not st.matches((2, 4, 6), torch.device("cuda", 0)) and not st.matches((2, 4, 6), torch.device("meta"))
    st.reset()
    assert st.frame is None and not st.matches((2, 4, 6), torch.device("cpu"))
    st.reset()                                                                              # an empty state resets too


def test_raw_format_with_temporal_validation():
    assert "temporal" in [f.name for f in dataclasses.fields(M.RawFormat)] and M.RawFormat().temporal is None and "Temporal" in M.RawFormat.__doc__
    fmt = M.RawFormat(storage="mipi12", width=20, black_level=256.0, white_level=4095.0, temporal=Temporal((8.0, 0.03), state=TemporalState()))
    assert fmt.validate((2, 18, 30)) == (18, 20) and fmt.validate((2, 1, 18, 33)) == (18, 20)
    with pytest.raises(TypeError, match="Temporal"):
        M.RawFormat(temporal=(8.0, 0.03)).validate((1, 8, 8))
    with pytest.raises(ValueError, match="curve cannot follow temporal"):
        dataclasses.replace(fmt, calibration=Calibration(curve=Pwl((0, 1), (0, 1)))).validate((2, 18, 30))
    assert dataclasses.replace(fmt, calibration=Calibration(gains=(2, 1, 1, 1.5))).validate((2, 18, 30)) == (18, 20)
    rows = dataclasses.replace(fmt, temporal=Temporal((8.0, 0.03), gain=torch.ones(3, 1)))
    assert rows.validate((3, 18, 30)) == (18, 20)
    with pytest.raises(ValueError, match="rows"):
        rows.validate((2, 18, 30))
    both = M.RawFormat(storage="u16", white_level=4095.0, temporal=Temporal((8.0, 0.03)), exposures=Exposures((1, 4), (3000, 3500)))
    assert both.validate((2, 2, 8, 12)) == (8, 12)                                         # the merge runs in front


def test_the_other_front_end_ops_refuse_a_format_with_temporal():
    fmt = M.RawFormat(storage="u16", white_level=4095.0, temporal=Temporal((8.0, 0.03), state=TemporalState()))
    x = torch.zeros(1, 4, 4, dtype=torch.uint16)
    order = r"ops.raw_defects, ops.raw_hdr_merge, ops.raw_temporal, ops.raw_calibrate, ops.raw_ingest"
    for call in (lambda: M.ops.raw_ingest(x, dtype=torch.float32, raw_format=fmt), lambda: M.ops.raw_defects(x, fmt, M.Defects(hot=(1.0, 0.0))),
                 lambda: M.ops.raw_calibrate(x, fmt, Calibration(gains=(1, 1, 1, 1))),
                 lambda: M.ops.raw_hdr_merge(torch.zeros(1, 2, 4, 4, dtype=torch.uint16), fmt, Exposures((1, 4), (3000, 3500)))):
        with pytest.raises(ValueError, match=order):
            call()
    with pytest.raises(ValueError, match="raw_defects"):                                   # the filter alone does not repair
        M.ops.raw_temporal(x, dataclasses.replace(fmt, defects=M.Defects(hot=(1.0, 0.0))))
    with pytest.raises(ValueError, match="merge first"):                                   # nor merge
        M.ops.raw_temporal(torch.zeros(1, 2, 4, 4, dtype=torch.uint16), dataclasses.replace(fmt, exposures=Exposures((1, 4), (3000, 3500))))
    with pytest.raises(ValueError, match="curve"):
        M.ops.raw_temporal(x, dataclasses.replace(fmt, calibration=Calibration(curve=Pwl((0, 1), (0, 1)))))
    with pytest.raises(TypeError, match="Temporal"):
        M.ops.raw_temporal(x, M.RawFormat(storage="u16"))                                  # nothing asked for
    with pytest.raises(TypeError, match="RawFormat"):
        M.ops.raw_temporal(x, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                             # a CPU tensor: refused, not computed elsewhere
        M.ops.raw_temporal(x, fmt)


# ---- 6. traces ----------------------------------------------------------------------------------------------------------------------------
def test_fake_trace_of_the_op_and_of_forward_mosaic():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                st = TemporalState()
                t = Temporal((8.0, 0.03), gain=torch.empty(2, 1, dtype=torch.float32), state=st)
                fmt = M.RawFormat(storage="mipi12", cfa="GRBG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=4095.0, temporal=t)
                frames = torch.empty(2, 144, 313, dtype=torch.uint8)
                first = M.ops.raw_temporal(frames, fmt)
                assert first.shape == (2, 144, 208) and first.dtype == torch.float32 and first.device.type == "cuda"
                out = torch.empty(2, 144, 208, dtype=torch.float32)
                assert M.ops.raw_temporal(frames, fmt, prev=first, out=out) is out
                padded = torch.empty(2, 144, 256, dtype=torch.float32)[..., :208]                  # rows 256 apart, frames 144 rows apart
                assert M.ops.raw_temporal(frames, fmt, prev=padded, out=out) is out
                half = M.ops.raw_temporal(torch.empty(1, 8, 12, dtype=torch.float16), M.RawFormat(temporal=Temporal((0.004, 0.01))))
                assert half.shape == (1, 8, 12) and half.dtype == torch.float32
                with pytest.raises(TypeError, match="uint8"):
                    M.ops.raw_temporal(torch.empty(2, 144, 313, dtype=torch.uint16), fmt)
                with pytest.raises(ValueError, match="rows"):
                    M.ops.raw_temporal(torch.empty(3, 144, 313, dtype=torch.uint8), fmt)
                for bad in (torch.empty(2, 144, 206, dtype=torch.float32), torch.empty(1, 144, 208, dtype=torch.float32), torch.empty(2, 144, 208, dtype=torch.bfloat16),
                            torch.empty(2, 144, 416, dtype=torch.float32)[..., ::2], torch.empty(2, 150, 208, dtype=torch.float32)[:, :144]):
                    with pytest.raises(ValueError, match="prev must"):
                        M.ops.raw_temporal(frames, fmt, prev=bad)
                    with pytest.raises(ValueError, match="out must"):
                        M.ops.raw_temporal(frames, fmt, prev=first, out=bad)
                with pytest.raises(TypeError, match="prev must be a tensor"):
                    M.ops.raw_temporal(frames, fmt, prev=st)
                # the whole front end: defects, the filter, the calibration, the ingest; the state is kept and swapped
                full = dataclasses.replace(fmt, defects=M.Defects(hot=(24.0, 0.1), counts=True), calibration=Calibration(gains=torch.empty(2, 4, dtype=torch.float32), clip=(0.0, 1.0)))
                net = M.LiteISPNet_GFM_LSC().eval()
                coord = torch.empty(2, 2, 72, 104)
                seen = []
                for _ in range(3):
                    with torch.no_grad():
                        y = net.forward_mosaic(frames, None, coord, raw_format=full)
                    assert y.shape == (2, 3, 144, 208) and y.dtype == torch.bfloat16 and net.defect_counts.shape == (2, 3)
                    assert st.frame.shape == (2, 144, 208) and st.frame.dtype == torch.float32
                    seen.append(st.frame)
                assert seen[0] is not seen[1] and seen[2] is seen[0]                               # two buffers, swapped
                st.reset()
                assert st.frame is None
                ex = dataclasses.replace(fmt, exposures=Exposures((1, 4, 16), (3000, 3500)))
                with torch.no_grad():
                    y = net.forward_mosaic(torch.empty(2, 3, 144, 313, dtype=torch.uint8), None, coord, raw_format=ex)
                assert y.shape == (2, 3, 144, 208) and st.frame.shape == (2, 144, 208)
                with pytest.raises(ValueError, match="needs a state"):
                    net.forward_mosaic(frames, None, coord, raw_format=dataclasses.replace(fmt, temporal=Temporal((8.0, 0.03))))
                with pytest.raises(ValueError, match="curve"):
                    net.forward_mosaic(frames, None, coord, raw_format=dataclasses.replace(fmt, calibration=Calibration(curve=Pwl((0, 1), (0, 1)))))
    finally:
        torch.set_default_dtype(old)


# ---- 7. C ABI and kernels -------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # non-null, aligned addresses that are never dereferenced: every case below fails before anything is enqueued
PREV, DST = FAKE + (1 << 16), FAKE + (1 << 17)       # a frame of the default shape holds 8 rows of 64 bytes


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("empty", dict(h=0), b"bad shape"), ("no columns", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("black nan", dict(black=(64.0, NAN, 64.0, 64.0)), b"black"), ("black inf", dict(black=(64.0, 64.0, 64.0, INF)), b"black"),
    ("reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"), ("flags", dict(flags=4), b"flags"), ("flags < 0", dict(flags=-1), b"flags"),
    ("no state", dict(prev=None), b"no state"), ("no state, host gain", dict(prev=None, flags=_lib.RC_TNR_GAIN, gain=2.0), b"no state"),
    ("dst is prev", dict(dst=PREV), b"overlaps"), ("dst inside prev", dict(dst=PREV + 256), b"overlaps"), ("dst ends in prev", dict(dst=PREV - 256), b"overlaps"),
    ("dst's last row in prev", dict(dst=PREV - 448 - 60), b"overlaps"), ("prev's last row in dst", dict(dst=PREV + 448 + 60), b"overlaps"),
    ("padded dst over prev", dict(dst=PREV - 900, dst_pitch=128), b"overlaps"), ("padded prev over dst", dict(dst=PREV + 1024, prev_pitch=160), b"overlaps"),
    ("batch of prev over dst", dict(b=3, dst=PREV + 1024), b"overlaps"),
    ("dst pitch short", dict(dst_pitch=60), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=66), b"dst pitch"), ("dst misaligned", dict(dst=DST + 2), b"dst misaligned"),
    ("prev pitch short", dict(prev_pitch=60), b"prev pitch"), ("prev pitch odd", dict(prev_pitch=70), b"prev pitch"), ("prev misaligned", dict(prev=PREV + 2), b"prev misaligned"),
    ("rows too far apart", dict(h=1 << 19, line_bytes=4096, dst=1 << 40), b"2 GiB"), ("dst frame too large", dict(h=1 << 19, dst_pitch=4096, dst=1 << 40), b"2 GiB"),
    ("prev frame too large", dict(h=1 << 19, prev_pitch=4096, dst=1 << 40), b"2 GiB"),
    ("gain batch 2 of 3", dict(b=3, dst=DST, gain_ptr=FAKE, gain_batch=2), b"gain_batch"), ("gain batch 0", dict(gain_ptr=FAKE, gain_batch=0), b"gain_batch"),
    ("gain batch without tensor", dict(gain_batch=1), b"gain_batch"), ("gain misaligned", dict(gain_ptr=FAKE + 2, gain_batch=1), b"4-byte"),
    ("gain both ways", dict(flags=_lib.RC_TNR_GAIN, gain=2.0, gain_ptr=FAKE, gain_batch=1), b"both ways"),
    ("gain zero", dict(flags=_lib.RC_TNR_GAIN, gain=0.0), b"gain must be finite"), ("gain negative", dict(flags=_lib.RC_TNR_GAIN, gain=-1.0), b"gain must be finite"),
    ("gain nan", dict(flags=_lib.RC_TNR_GAIN, gain=NAN), b"gain must be finite"), ("gain inf", dict(flags=_lib.RC_TNR_GAIN, gain=INF), b"gain must be finite"),
    ("noise_abs zero", dict(noise=(0.0, 0.0)), b"noise_abs"), ("noise_abs negative", dict(noise=(-1.0, 0.0)), b"noise_abs"), ("noise_abs nan", dict(noise=(NAN, 0.0)), b"noise_abs"),
    ("noise_abs inf", dict(noise=(INF, 0.0)), b"noise_abs"), ("noise_rel negative", dict(noise=(1.0, -0.5)), b"noise_rel"), ("noise_rel nan", dict(noise=(1.0, NAN)), b"noise_rel"),
    ("noise_rel inf", dict(noise=(1.0, INF)), b"noise_rel"), ("parameters are checked on a reset too", dict(flags=_lib.RC_TNR_RESET, prev=None, noise=(0.0, 0.0)), b"noise_abs"),
    ("alpha zero", dict(alpha=0.0), b"alpha"), ("alpha negative", dict(alpha=-0.5), b"alpha"), ("alpha above one", dict(alpha=1.5), b"alpha"), ("alpha nan", dict(alpha=NAN), b"alpha"),
    ("ramp one", dict(ramp=1.0), b"ramp"), ("ramp below one", dict(ramp=0.5), b"ramp"), ("ramp nan", dict(ramp=NAN), b"ramp"), ("ramp inf", dict(ramp=INF), b"ramp"),
])
def test_raw_temporal_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, prev=PREV, prev_pitch=0, gain_ptr=None, gain_batch=0, dst=DST, dst_pitch=0, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0,
              line_bytes=0, width=0, black=(64.0,) * 4, flags=0, noise=(4.0, 0.03125), alpha=0.125, ramp=3.0, gain=0.0, reserved=(0, 0, 0, 0), fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=0.0,
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.TemporalDesc(flags=kw["flags"], noise_abs=kw["noise"][0], noise_rel=kw["noise"][1], alpha=kw["alpha"], ramp=kw["ramp"], gain=kw["gain"],
                          reserved=(C.c_int32 * 4)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_temporal(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["prev"], kw["prev_pitch"], kw["gain_ptr"],
                               kw["gain_batch"], kw["dst"], kw["dst_pitch"], kw["b"], kw["h"], kw["w"], None) == -1, case           # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_raw_temporal_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_temporal", "rc_temporal_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_temporal_desc_size() == C.sizeof(_lib.TemporalDesc) == 40
    header = _lib.HEADER.read_text()
    assert f"#define RC_TNR_RESET {_lib.RC_TNR_RESET}" in header and f"#define RC_TNR_GAIN {_lib.RC_TNR_GAIN}" in header
    t = M.temporal
    assert (t.LANE_PX, t.WAVE_SPAN, t.WAVE_OUT, t.BLOCK_STRIPS, t.BLOCK_ROWS) == (4, 256, 248, 2, 32)
    src = (_lib.PKG / "csrc" / "temporal_kernel.hpp").read_text()                  # the constants the GPU tests place their seams on
    assert ("kTnrPx = 4" in src and "kTnrSpan = 64 * kTnrPx" in src and "kTnrOut = kTnrSpan - 2 * kTnrPx" in src and "kTnrRows = 32" in src
            and "kTnrStrips = kTnrWaves / 2" in src and "kTnrWaves = 4" in src)
    for name in ("temporal.hip", "temporal_mc.hip"):                               # one lane map: neither file defines a constant of its own
        assert not re.search(r"\bk(Tnr|Tmc)\w* *=[^=]", (_lib.PKG / "csrc" / name).read_text()), name


def test_raw_temporal_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "temporal.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "raw_temporal" in k}
    assert len(mine) == 7, sorted(mine)                    # fp32, bf16, fp16, u16, u8, RAW10, RAW12 sources
    assert all(v["tu"] == "temporal.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 72 and v["sgprs"] <= 102 for v in mine.values())     # 7 waves per SIMD: two rows of the window live in registers
    assert all(v["lds"] == 0 for v in mine.values())
    assert not [k for k, v in res.items() if v["tu"] == "temporal.hip" and k not in mine]
