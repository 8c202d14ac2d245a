"""CPU: output sharpening (include/realcam_hip.h rc_sharpen; realcamnet_amd/sharpen.py).  The elementwise torch restatement of the
header's arithmetic that the GPU tests use as their yardstick (sharpen_ref.py), checked here against a scalar fp32 loop, its exact
properties, the float64 bound and what the stage is for; Sharpen's validation; Output(sharpen=...) and every refusal made before a launch;
the C ABI's argument checks; the kernels' resources; fake-tensor traces."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32
from sharpen_ref import blurred_step, bound, luma_coefficients, restated_parts, restated_sharpen, sharpen_source

PARAMS = (dict(amount=1.5, core=1 / 64, overshoot=0.0), dict(amount=8.0, core=0.0, overshoot=1 / 32))
BIG = (1, 3, 400, 500)          # 200 000 pixels: the CPU checks' source


def clamped(y, crop=None):
    """Step 1 alone: NaN -> 0, clamped to [0, 1], fp32."""
    h, w = crop if crop is not None else y.shape[2:]
    return torch.nan_to_num(y[:, :, :h, :w].float(), nan=0.0, posinf=1.0, neginf=0.0).clamp(0, 1)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------
def scalar_sharpen(y, sp):
    """The header's steps for one (3,h,w) fp32 frame as a double loop over pixels, every operation on numpy.float32 scalars (one rounding
    each), the taps clamped per axis."""
    f = np.float32
    _, h, w = y.shape
    kr, kg, kb = (f(k) for k in luma_coefficients(sp.matrix))
    amount, core, over = f(sp.amount), f(sp.core), f(sp.overshoot)
    R = sp.radius

    def unit(v):
        return f(min(v, f(1))) if v > 0 else f(0)                           # NaN compares false: 0

    c = np.array([[[unit(y[p, i, j]) for j in range(w)] for i in range(h)] for p in range(3)], dtype=f)
    L = np.empty((h, w), f)
    for i in range(h):
        for j in range(w):
            L[i, j] = f(f(f(kr * c[0, i, j]) + f(kg * c[1, i, j])) + f(kb * c[2, i, j]))

    def binom(t):
        if R == 1:
            return f(f(t(-1) + t(1)) + f(f(2) * t(0)))
        return f(f(f(f(t(-2) + t(2)) + f(f(2) * t(0))) + f(f(4) * t(0))) + f(f(4) * f(t(-1) + t(1))))

    cy, cx = (lambda i: min(max(i, 0), h - 1)), (lambda j: min(max(j, 0), w - 1))
    S = np.empty((h, w), f)
    for i in range(h):
        for j in range(w):
            S[i, j] = binom(lambda d: L[i, cx(j + d)])
    out = np.empty((3, h, w), f)
    for i in range(h):
        for j in range(w):
            T = binom(lambda d: S[cy(i + d), j])
            blur = f(T * f(2.0 ** (-4 * R)))
            d = f(L[i, j] - blur)
            cc = max(f(abs(d) - core), f(0))
            e = f(amount * f(np.copysign(cc, d)))
            taps = [L[cy(i + dy), cx(j + dx)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            lo, hi = min(taps), max(taps)
            t = f(L[i, j] + e)
            t = min(t, f(hi + over))
            t = max(t, f(lo - over))
            e2 = f(t - L[i, j])
            for p in range(3):
                out[p, i, j] = min(max(f(c[p, i, j] + e2), f(0)), f(1))
    return out


@pytest.mark.parametrize("radius", (1, 2))
def test_restatement_equals_a_scalar_fp32_loop(radius):
    """Frames narrower and shorter than the halo, so every border case of both axes is walked."""
    with np.errstate(invalid="ignore", over="ignore"):
        for k, hw in enumerate(((1, 1), (1, 5), (5, 1), (2, 3), (7, 9))):
            for q, kw in enumerate(PARAMS):
                sp = M.Sharpen(radius=radius, matrix=("bt709", "bt601", "bt2020")[(k + q) % 3], **kw)
                for quantised in (False, True):
                    y = sharpen_source((1, 3) + hw, None, torch.float32, quantised, seed=k)
                    want = scalar_sharpen(y[0].numpy(), sp)
                    got = restated_sharpen(y, sp)[0].numpy()
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hw, kw, quantised)


def test_binomial_of_a_constant_is_exact():
    """The order of additions of step 3: every partial sum of a constant neighbourhood is a power of two times the value."""
    g = torch.Generator().manual_seed(11)
    v = torch.rand(2000, generator=g)
    y = v.view(2000, 1, 1, 1).expand(2000, 3, 5, 5).contiguous()
    for radius in (1, 2):
        p = restated_parts(y, M.Sharpen(radius=radius))
        assert torch.equal(p["blur"], p["L"]) and (p["d"] == 0).all()


@pytest.mark.parametrize("radius", (1, 2))
def test_exact_properties_of_the_restatement(radius):
    big = sharpen_source(BIG)
    want = clamped(big)
    # amount = 0 and core = 1 return the clamped input
    for sp in (M.Sharpen(0.0, radius, 0.0, 0.5), M.Sharpen(0, radius, 1 / 64, 0.0), M.Sharpen(8.0, radius, 1.0, 1.0), M.Sharpen(1.5, radius, 1, 0.0, "bt601")):
        assert torch.equal(restated_sharpen(big, sp), want), sp
    # a frame whose planes are each constant returns the clamped input, whatever the amount, radius and overshoot
    for vals in ((0.25, 0.5, 0.75), (1.3, -0.2, 0.1), (float("nan"), 0.6, float("inf")), (1e-3, 0.999, 0.3333)):
        y = torch.tensor(vals).view(1, 3, 1, 1).expand(2, 3, 9, 13).contiguous()
        for amount in (0.5, 1.5, 8.0):
            for over in (0.0, 1 / 32, 1.0):
                assert torch.equal(restated_sharpen(y, M.Sharpen(amount, radius, 0.0, over)), clamped(y)), (vals, amount, over)
    # every output is finite and lies in [0, 1]
    for kw in PARAMS:
        for y in (big, sharpen_source((2, 3, 40, 72), (37, 71), torch.bfloat16, True)):
            out = restated_sharpen(y, M.Sharpen(radius=radius, **kw), (37, 71) if y.shape[0] == 2 else None)
            assert torch.isfinite(out).all() and out.min() >= 0 and out.max() <= 1


@pytest.mark.parametrize("radius", (1, 2))
def test_without_overshoot_the_luma_stays_in_its_local_range(radius):
    for quantised in (False, True):
        y = sharpen_source(BIG, None, torch.float32, quantised)
        p = restated_parts(y, M.Sharpen(8.0, radius, 0.0, 0.0))
        t = p["L"] + p["e2"]
        assert (p["t"] >= p["lo"]).all() and (p["t"] <= p["hi"]).all()
        slack = 2.0 ** -23                                                   # e2 = t - L and L + e2 round once each below 2
        assert (t >= p["lo"] - slack).all() and (t <= p["hi"] + slack).all()
        assert (p["e"].abs() > (p["e2"].abs() + 0.01)).any()                 # and the limit did bite somewhere


def test_a_softened_edge_gets_steeper_and_keeps_its_range():
    y = blurred_step()
    slope = lambda t: (t[..., 1:] - t[..., :-1]).abs().max().item()
    before = slope(y)
    for radius, amount in ((2, 1.5), (1, 1.5), (2, 8.0)):
        out = restated_sharpen(y, M.Sharpen(amount, radius, 0.0, 0.0))
        print(f"radius {radius}, amount {amount}: largest slope {before:.4f} -> {slope(out):.4f}")
        assert slope(out) > before
        assert out.min() == y.min() and out.max() == y.max()                 # no overshoot: the value range is unchanged
        assert (out[..., 1:] >= out[..., :-1]).all()                         # and the edge is still monotonic
    assert torch.equal(restated_sharpen(y, M.Sharpen(0.0)), y)


@pytest.mark.parametrize("radius", (1, 2))
def test_restatement_within_the_rounding_bound_of_float64(radius):
    y = sharpen_source(BIG)
    for amount in (0.5, 2.0, 8.0):
        for core, over in ((0.0, 1.0), (1 / 64, 1 / 32)):
            sp = M.Sharpen(amount, radius, core, over)
            a, b = restated_sharpen(y, sp), restated_sharpen(y, sp, dtype=torch.float64)
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == y.shape
            err = (a.double() - b).abs().max().item()
            print(f"radius {radius}, amount {amount}, core {core:g}, overshoot {over:g}: max |fp32 - fp64| = {err * 2 ** 24:.2f} x 2^-24, bound {bound(sp) * 2 ** 24:.2f} x 2^-24")
            assert err <= bound(sp)


# ---- 2. Sharpen ---------------------------------------------------------------------------------------------------------------------------------
def test_sharpen_validation_equality_and_immutability():
    s = M.Sharpen()
    assert (s.amount, s.radius, s.core, s.overshoot, s.matrix) == (1.0, 2, 0.0, 0.0, "bt709") and s.matrix_code == _lib.RC_MATRIX_BT709
    assert s == M.Sharpen(1, 2, 0, 0, "bt709") and hash(s) == hash(M.Sharpen(1.0)) and s != M.Sharpen(1.0, 1) and len({s, M.Sharpen(), M.Sharpen(2.0)}) == 2
    assert M.Sharpen(0.1).amount == float(np.float32(0.1)) and M.Sharpen(np.float32(0.3), np.int64(1)).radius == 1           # kept as the kernel sees them
    assert [M.Sharpen(matrix=m).matrix_code for m in ("bt601", "bt709", "bt2020")] == [_lib.RC_MATRIX_BT601, _lib.RC_MATRIX_BT709, _lib.RC_MATRIX_BT2020]
    assert M.Sharpen(8, 1, 1, 1).amount == 8.0 and "Sharpen" in M.__all__
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.amount = 2.0
    for name, bads in (("amount", (-0.1, 8.5, float("nan"), float("inf"), 1e40)), ("core", (-1e-3, 1.01, float("nan"))), ("overshoot", (-1.0, 1.5, float("-inf")))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                M.Sharpen(**{name: bad})
        for bad in (True, "1", None, [1.0], 1j):
            with pytest.raises(TypeError, match=name):
                M.Sharpen(**{name: bad})
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match="radius"):
            M.Sharpen(radius=bad)
    for bad in (True, 2.0, "2", None):
        with pytest.raises(TypeError, match="radius"):
            M.Sharpen(radius=bad)
    for bad in ("bt.709", "BT709", ""):
        with pytest.raises(ValueError, match="matrix"):
            M.Sharpen(matrix=bad)
    for bad in (1, None, b"bt709"):
        with pytest.raises(TypeError, match="matrix"):
            M.Sharpen(matrix=bad)


# ---- 3. Output, ops and forward_mosaic: refusals before any launch -----------------------------------------------------------------------------
def test_output_carries_a_sharpen():
    sp = M.Sharpen(1.5, 2, 1 / 64)
    nv12 = M.OutFormat("nv12")
    assert dataclasses.fields(M.Output)[-1].name == "sharpen" and [f.name for f in dataclasses.fields(M.Output)] == ["format", "resize", "look", "warp", "sharpen"]
    o = M.Output(nv12, M.Resize((36, 52)), None, None, sp)
    assert o.sharpen is sp and o == M.Output(nv12, M.Resize((36, 52)), sharpen=M.Sharpen(1.5, 2, 1 / 64)) and hash(o) == hash(M.Output(nv12, M.Resize((36, 52)), sharpen=sp))
    assert o != M.Output(nv12, M.Resize((36, 52))) and M.Output().sharpen is None and M.Output("rgb8").sharpen is None
    assert M.Output(None, sharpen=sp).plan(71, 153) == (71, 153) and o.plan(72, 104) == (36, 52) and M.Output(None, sharpen=sp).plan(1, 1) == (1, 1)
    for bad in (1.5, "sharp", (sp,), dict(amount=1.0), M.Resize((2, 2))):
        with pytest.raises(TypeError, match="sharpen"):
            M.Output(nv12, sharpen=bad)
    with pytest.raises(ValueError):
        M.Output(nv12, sharpen=sp).plan(71, 154)                              # a sharpen does not lift the encoder's own conditions


def test_plan_outputs_with_the_field_set():
    from realcamnet_amd.LiteISP import _plan_outputs
    sp = M.Sharpen()
    nv12 = M.OutFormat("nv12")
    ladder = [M.Output(nv12), M.Output(nv12, M.Resize((72, 104)), sharpen=sp), M.Output(M.Stats(grid=(4, 4)), M.Resize((36, 52)), sharpen=sp), M.Output(None, sharpen=sp)]
    assert _plan_outputs(ladder, None, (144, 208)) == tuple(ladder) and _plan_outputs(None, nv12, (144, 208)) is None
    with pytest.raises(ValueError, match="either"):
        _plan_outputs(ladder, nv12, (144, 208))
    with pytest.raises(TypeError):
        _plan_outputs([sp], None, (144, 208))
    with pytest.raises(ValueError):
        _plan_outputs([M.Output(nv12, M.Resize((200, 104)), sharpen=sp)], None, (144, 208))       # an upscale, refused as before
    with pytest.raises(ValueError):
        _plan_outputs([M.Output(M.Stats(grid=(64, 64)), M.Resize((36, 52)), sharpen=sp)], None, (144, 208))


def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    sp = M.Sharpen(1.5)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.sharpen(torch.zeros(1, 3, 8, 8), sp)                              # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError, match="Sharpen"):
        ops.sharpen(torch.zeros(1, 3, 8, 8), 1.5)
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for crop in ((81, 160), (80, 161), (0, 160), (80, 0)):
                with pytest.raises(ValueError, match="crop"):
                    ops.sharpen(y, sp, crop_hw=crop)
            with pytest.raises(ValueError):
                ops.sharpen(torch.empty(2, 4, 80, 160), sp)
            with pytest.raises(ValueError):
                ops.sharpen(torch.empty(3, 80, 160), sp)
            with pytest.raises(ValueError):
                ops.sharpen(torch.empty(0, 3, 80, 160), sp)
            with pytest.raises(ValueError, match="out_dtype"):
                ops.sharpen(y.to(torch.bfloat16), sp, out_dtype=torch.float16)
            with pytest.raises(ValueError, match="out_dtype"):
                ops.sharpen(y, sp, out_dtype=torch.bfloat16)
            with pytest.raises(TypeError):
                ops.sharpen(y.to(torch.float64), sp)
            with pytest.raises(TypeError):
                ops.sharpen(y, "sharp")
            with pytest.raises(TypeError):
                ops.sharpen(y, None)
            out = ops.sharpen(y.to(torch.bfloat16), sp, crop_hw=(70, 153))
            assert out.shape == (2, 3, 70, 153) and out.dtype == torch.float32 and out.device.type == "cuda"
            assert ops.sharpen(y.to(torch.float16), sp, out_dtype=torch.float16).dtype == torch.float16
            assert ops.sharpen(y.to(torch.bfloat16), sp, out_dtype=torch.bfloat16).dtype == torch.bfloat16
            assert ops.sharpen(torch.empty(1, 3, 1, 1), M.Sharpen(radius=1)).shape == (1, 3, 1, 1)
            t = torch.ops.realcam.sharpen(torch.empty(3, 3, 80, 160, dtype=torch.float16), 2, 1, 1.5, 0.0, 0.0, 70, 150, torch.float32)
            assert t.shape == (3, 3, 70, 150) and t.dtype == torch.float32
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            nv12 = M.OutFormat("nv12")
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12, outputs=[M.Output(nv12, sharpen=sp)])
                for bad in ([M.Output(nv12, M.Resize((34, 34)), sharpen=sp)], [M.Output(None, M.Resize((2, 16)), sharpen=sp)]):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, outputs=[sp])
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(None, sharpen=sp)])


def test_fake_trace_of_sharpened_ladders():
    """forward_mosaic(outputs=[...sharpen...]) under FakeTensorMode: the shapes, dtypes and device planned, for a DWT net and a strided net."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                sp = M.Sharpen(1.5, 2, 1 / 64)
                ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.OutFormat("nv12"), M.Resize((72, 104)), look=M.Lut3D.identity(17), sharpen=sp),
                          M.Output("rgb8", M.Resize((36, 52), filter="bilinear"), sharpen=M.Sharpen(radius=1)), M.Output(None, sharpen=sp),
                          M.Output(M.Stats(grid=(4, 4)), M.Resize((72, 104)), sharpen=sp)]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c, d, e = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                    assert isinstance(a, M.YuvFrames) and a.planes[0].shape == (2, 144, 208)
                    assert isinstance(b, M.YuvFrames) and b.planes[0].shape == (2, 72, 104) and b.planes[1].shape == (2, 36, 52, 2)
                    assert c.shape == (2, 36, 52, 3) and c.dtype == torch.uint8
                    assert d.shape == (2, 3, 144, 208) and d.dtype == torch.float32 and d.device.type == "cuda"        # a sharpened float output is fp32
                    assert isinstance(e, M.FrameStats) and e.zones.shape == (2, 4, 4, 8)
    finally:
        torch.set_default_dtype(old)


# ---- 4. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null dst", dict(dst=None), b"null"), ("null desc", dict(desc=None), b"null"),
    ("bad source dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("bad output dtype", dict(sdt=RC_BF16, ddt=RC_F16), b"dtype"), ("unknown output dtype", dict(ddt=7), b"dtype"),
    ("fp32 into bf16", dict(ddt=RC_BF16), b"dtype"),
    ("radius 0", dict(radius=0), b"radius"), ("radius 3", dict(radius=3), b"radius"), ("matrix -1", dict(matrix=-1), b"matrix"), ("matrix 3", dict(matrix=3), b"matrix"),
    ("amount nan", dict(amount=NAN), b"amount"), ("amount inf", dict(amount=INF), b"amount"), ("amount < 0", dict(amount=-0.5), b"amount"), ("amount > 8", dict(amount=8.5), b"amount"),
    ("core nan", dict(core=NAN), b"core"), ("core < 0", dict(core=-0.1), b"core"), ("core > 1", dict(core=1.5), b"core"),
    ("overshoot nan", dict(overshoot=NAN), b"overshoot"), ("overshoot < 0", dict(overshoot=-INF), b"overshoot"), ("overshoot > 1", dict(overshoot=2.0), b"overshoot"),
    ("h > H", dict(h=17), b"exceeds"), ("w > W", dict(w=17), b"exceeds"), ("empty", dict(w=0), b"empty"), ("no rows", dict(h=0), b"empty"), ("no frames", dict(b=0), b"empty"),
    ("src misaligned", dict(src=FAKE + 2), b"misaligned"), ("dst misaligned", dict(sdt=RC_BF16, ddt=RC_BF16, dst=(1 << 24) + 1), b"misaligned"),
    ("2 GiB of fp32 planes", dict(H=16384, W=16384, h=8, w=8), b"2 GiB"), ("2 GiB of output planes", dict(H=16384, W=16384, h=16384, w=16384, sdt=RC_BF16), b"2 GiB"),
    ("in place", dict(dst=FAKE), b"overlaps"), ("dst inside src", dict(dst=FAKE + 16 * 16 * 4), b"overlaps"),
])
def test_sharpen_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, dst=1 << 24, ddt=RC_F32, desc=True, radius=2, matrix=1, amount=1.0, core=0.0, overshoot=0.0, b=1, H=16, W=16, h=8, w=8)
    kw.update(kwargs)
    d = _lib.SharpenDesc(radius=kw["radius"], matrix=kw["matrix"], amount=kw["amount"], core=kw["core"], overshoot=kw["overshoot"])
    lib = _lib.load()
    rc = lib.rc_sharpen(kw["src"], kw["sdt"], kw["dst"], kw["ddt"], C.byref(d) if kw["desc"] else None, kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None)
    assert rc == -1, case                                                    # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_sharpen_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_sharpen", "rc_sharpen_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert lib.rc_sharpen_desc_size() == C.sizeof(_lib.SharpenDesc) == 20
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                    # additive: the version stays
    assert "sharpen" in M.torch_ops.SCHEMAS
    from realcamnet_amd import sharpen
    assert sharpen.MATRICES == {"bt601": _lib.RC_MATRIX_BT601, "bt709": _lib.RC_MATRIX_BT709, "bt2020": _lib.RC_MATRIX_BT2020}


def test_sharpen_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build, sharpen
    assert "sharpen.hip" in build.SOURCES
    src = (_lib.PKG / "csrc" / "sharpen.hip").read_text()                          # the constants the GPU tests place their seams on
    assert f"kShPx = {sharpen.LANE_PX}," in src and "kShSpan = 64 * kShPx;" in src and "kShOut = kShSpan - 2 * kShPx;" in src and f"kShRows = {sharpen.BAND_ROWS};" in src
    assert (sharpen.WAVE_SPAN, sharpen.WAVE_OUT) == (256, 248)
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "sharpen_kernel" in k}
    assert len(mine) == 10, sorted(mine)                                     # fp32 -> fp32; bf16 / fp16 -> fp32 or themselves; each at radius 1 and 2
    assert all(v["tu"] == "sharpen.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0) or v.get("lds", 0)]
    assert not [k for k, v in res.items() if v["tu"] == "sharpen.hip" and k not in mine]
    print({k: (v["vgprs"], v.get("sgprs")) for k, v in mine.items()})
