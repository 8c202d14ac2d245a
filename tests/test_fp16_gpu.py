"""GPU (-m gpu): fp16 (torch.float16, RC_F16) on the ISP path -- what `net.half()` means upstream: fp16 parameters and activations, fp32 accumulation,
fp32 reductions / FiLM / gate / colour-prior vectors, fp16 output unless output_dtype says otherwise.
Gates: integer-valued convolutions bit for bit; per block max|err| <= 4e-3 * max|ref|; end to end PSNR >= 70 dB against the reference and >= the bf16 PSNR
of the same fixture + 12 dB (fp16 keeps 3 more mantissa bits than bf16)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import networks as N
from realcamnet_amd import ops
from conftest import net_name_of, golden_names, load_golden, rel_err, seed0_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
H16 = torch.float16
F16_TOL = 4e-3


def put(mod, sd, dt=H16):
    mod.load_state_dict(sd, strict=True)
    return mod.to(device=DEV, dtype=dt).eval()


def run(mod, *xs, dt=H16):
    with torch.no_grad():
        y = mod(*[x.to(DEV, dt) if isinstance(x, torch.Tensor) else x for x in xs])
    torch.cuda.synchronize()
    return y


_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        net = getattr(M, name)()
        net.load_state_dict(seed0_state_dict(name), strict=True)
        _NETS[key] = net.to(device=DEV, dtype=dt).eval()
    return _NETS[key]


# ---- convolutions on integer data ------------------------------------------------------------------------
def _int_conv(cin, cout, ksz, seed, wlo=-2, whi=3, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    c = N.Conv2d(cin, cout, ksz, 1, ksz // 2)
    with torch.no_grad():
        c.weight.copy_(torch.randint(wlo, whi, c.weight.shape, generator=g).float() / scale)
        c.bias.copy_(torch.randint(wlo, whi, c.bias.shape, generator=g).float())
    return c, g


@pytest.mark.parametrize("persist", [1, 2, 3, 0])
@pytest.mark.parametrize("shape", [(48, 48, 16, 40, 3), (48, 48, 9, 33, 3), (48, 3, 8, 32, 3), (4, 48, 24, 70, 3), (32, 32, 21, 70, 3), (32, 64, 9, 33, 3), (32, 3, 16, 40, 3),
                                   (64, 64, 8, 40, 3), (96, 48, 8, 32, 3), (48, 48, 8, 32, 1), (2, 48, 10, 34, 1),
                                   (128, 64, 16, 40, 3), (192, 192, 9, 33, 3), (192, 48, 24, 70, 3), (128, 128, 37, 100, 3)])
def test_f16_conv_exact_on_small_integer_data(hip, persist, shape):
    """Every product and partial sum exactly representable: the fp16 conv equals F.conv2d bit for bit (single- and multi-chunk forms, every persist mode)."""
    cin, cout, h, w, ksz = shape
    c, g = _int_conv(cin, cout, ksz, cin * 1000 + cout)
    x = torch.randint(-2, 3, (2, cin, h, w), generator=g).float() / 2
    ref = F.conv2d(x, c.weight.detach(), c.bias.detach(), padding=ksz // 2)
    assert hip.rc_debug_set(b"persist", persist) == 0
    try:
        with torch.no_grad():
            y = c.to(DEV, H16)(x.to(DEV, H16))
    finally:
        hip.rc_debug_set(b"persist", 1)
    assert y.dtype == H16 and torch.equal(y.float().cpu(), ref)


@pytest.mark.parametrize("shape", [(48, 48, 3, 16, 40), (32, 32, 3, 21, 70), (48, 192, 3, 9, 33), (4, 48, 3, 24, 70), (48, 48, 1, 10, 34), (192, 48, 3, 8, 32)])
def test_f16_stores_round_to_nearest_even(hip, shape):
    """Integer outputs in (2048, 8192), where fp16 keeps only every 2nd / 4th integer: the stored value is F.conv2d(...).half() (round-to-nearest-even,
    ties included), which a truncating pack (v_cvt_pkrtz) or a bf16 pack would miss."""
    cin, cout, ksz, h, w = shape
    taps = cin * ksz * ksz
    c, g = _int_conv(cin, cout, ksz, 7 * cin + cout)
    lo = max(0, round(4000 / (2 * taps) - 1.5))                # mean output ~4000: weights 1..3, inputs lo..lo+3
    x = torch.randint(lo, lo + 4, (2, cin, h, w), generator=g).float()
    with torch.no_grad():
        c.weight.copy_(torch.randint(1, 4, c.weight.shape, generator=g).float())
        c.bias.copy_(torch.randint(0, 4, c.bias.shape, generator=g).float())
    ref = F.conv2d(x, c.weight.detach(), c.bias.detach(), padding=ksz // 2)
    inside = (ref > 2048) & (ref < 8192)
    assert inside.float().mean() > 0.5 and (ref[inside] != ref[inside].half().float()).float().mean() > 0.3     # most values must round
    with torch.no_grad():
        y = c.to(DEV, H16)(x.to(DEV, H16)).cpu()
    assert torch.equal(y[inside], ref[inside].half())


def test_f16_folded_tail_and_conv_dwt_equal_their_two_launch_routes(hip):
    """The two fused forms fp16 shares with bf16: the folded 5x5 tail equals the two tail convolutions on integer data (exact there), and
    conv -> DWT in one launch (RC_OUT_NHWC_DWT) equals rc_conv2d + rc_dwt_forward bit for bit."""
    for c_in in (48, 32):
        tail = N.seq(N.conv(c_in, 4 * c_in, mode="C"), torch.nn.PixelShuffle(2), N.conv(c_in, 3, mode="C"))
        g = torch.Generator().manual_seed(c_in)
        with torch.no_grad():
            for m in (tail[0], tail[2]):
                m.weight.copy_(torch.randint(-1, 2, m.weight.shape, generator=g).float() / 4)
                m.bias.copy_(torch.randint(-1, 2, m.bias.shape, generator=g).float() / 4)
        tail = tail.to(DEV, H16).eval()
        x = (torch.randint(-2, 3, (2, 20, 36, c_in), generator=g).float() / 2).to(DEV, H16)
        with torch.no_grad():
            assert ops.tail_fold_ok(x, tail[0], tail[2])
            y = ops.tail_fold(x, tail[0], tail[2])
            two = tail[2]._nhwc(tail[0]._nhwc(x, out_mode=ops.RC_OUT_PIXEL_SHUFFLE2), out_mode=ops.RC_OUT_NCHW)
        assert y.dtype == H16 and torch.equal(y, two), c_in
    for c in (48, 32):
        g = torch.Generator().manual_seed(11 * c)
        conv = N.Conv2d(c, c, 3, 1, 1).to(DEV, H16).eval()
        dwt = N.DWTForward(c).to(DEV, H16).eval()
        for (B, H, W) in ((1, 8, 32), (2, 22, 70), (1, 130, 260)):
            x = torch.randn(B, H, W, c, generator=g).to(DEV, H16)
            res = torch.randn(B, H, W, c, generator=g).to(DEV, H16)
            for kw in (dict(), dict(act="relu"), dict(act="leaky", slope=0.1), dict(residual=res)):
                assert ops.conv_dwt_ok(x, conv, dwt, kw.get("act"), kw.get("slope", 0.0), residual="residual" in kw)
                with torch.no_grad():
                    want = ops.dwt_forward(ops.conv2d(x, conv, **kw), dwt)
                    got = ops.conv2d(x, conv, out_mode=ops.RC_OUT_NHWC_DWT, **kw)
                assert got.dtype == H16 and torch.equal(got, want), (c, B, H, W, list(kw))


def test_f16_layout_and_ingest_kernels(hip):
    """bayer unshuffle, the fused RAW ingest (uint16 counts with levels, cond from RAW) and NCHW <-> NHWC in fp16: the torch .half() of the fp32 results."""
    g = torch.Generator().manual_seed(3)
    mosaic = torch.rand(2, 1, 2 * 21, 2 * 35, generator=g)
    a32 = ops.bayer_unshuffle(mosaic.to(DEV), dtype=torch.float32, pad_to=16)
    a16 = ops.bayer_unshuffle(mosaic.to(DEV), dtype=H16, pad_to=16)
    assert a16.dtype == H16 and torch.equal(a16, a32.half())
    counts = torch.randint(0, 1024, (2, 1, 2 * 21, 2 * 35), generator=g).to(torch.uint16)
    p32, c32 = ops.raw_ingest(counts.to(DEV), dtype=torch.float32, pad_to=16, black_level=64.0, white_level=1023.0, cond_hw=(24, 40))
    p16, c16 = ops.raw_ingest(counts.to(DEV), dtype=H16, pad_to=16, black_level=64.0, white_level=1023.0, cond_hw=(24, 40))
    assert torch.equal(p16, p32.half()) and torch.equal(c16, c32.half())
    x = torch.randn(2, 48, 13, 37, generator=g).to(DEV)
    for src in (x, x.to(torch.bfloat16), x.half()):
        n = ops.to_nhwc(src, dtype=H16)
        assert n.dtype == H16 and torch.equal(n, ops.to_nhwc(src, dtype=torch.float32).half())
    n = ops.to_nhwc(x.half(), dtype=H16)
    assert torch.equal(ops.to_nchw(n), x.half()) and torch.equal(ops.to_nchw(n, dtype=torch.float32), x.half().float())


# ---- golden block fixtures ---------------------------------------------------------------------------------
def test_f16_blocks_vs_reference(hip):
    L = M.LiteISP
    checks = []

    def chk(name, y, ref):
        checks.append((name, rel_err(y.float().cpu(), ref)))

    g = load_golden("block_dwt_forward")
    chk("dwt_forward", run(put(N.DWTForward(16), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_dwt_inverse")
    chk("dwt_inverse", run(put(N.DWTInverse(64), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_dwt_forward_anyc")
    chk("dwt_forward_anyc", run(put(N.DWTForward_(), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_dwt_inverse_anyc")
    chk("dwt_inverse_anyc", run(put(N.DWTInverse_(), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_conv3x3_16_32")
    chk("conv3x3_16_32", run(put(N.conv(16, 32, mode="C"), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_conv_crc_48")
    chk("conv_crc_48", run(put(N.conv(48, 48, mode="CRC"), g["sd"]), g["x"]), g["y"])
    old = ops.FUSE_GATE, ops.EARLY_GATE
    for schedule in ("early", "staged", "unfused"):
        ops.EARLY_GATE, ops.FUSE_GATE = schedule == "early", schedule != "unfused"
        try:
            g = load_golden("block_rcab_32")
            chk("rcab_32 " + schedule, run(put(N.RCABlock(32, 32), g["sd"]), g["x"]), g["y"])
            g = load_golden("block_rcag_32_nb4")
            chk("rcag_32 " + schedule, run(put(N.RCAGroup(32, 32, nb=4), g["sd"]), g["x"]), g["y"])
            g = load_golden("block_rcag_48_nb2")
            chk("rcag_48 " + schedule, run(put(N.RCAGroup(48, 48, nb=2), g["sd"]), g["x"]), g["y"])
        finally:
            ops.FUSE_GATE, ops.EARLY_GATE = old
    g = load_golden("block_calayer_32")
    chk("calayer_32", run(put(N.CALayer(32, 16), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_res_gfm_48")
    mod = put(L.Res_GFM(48, 48, 32, 48, 48), g["sd"])
    with torch.no_grad():
        chk("res_gfm_48", mod((g["x"].to(DEV, H16), g["v"].to(DEV)))[0], g["y"])
    g = load_golden("block_lsc_48")
    chk("lsc_48", run(put(L.Lens_Shading_Correction(2, 48, 48), g["sd"]), g["x"]), g["y"])
    g = load_golden("block_color_condition")
    mod = put(L.Color_Condition_GFM(4, 32), g["sd"])
    with torch.no_grad():
        v = mod._vec(g["x"].to(DEV, H16))
    assert v.dtype == torch.float32                      # the prior's vector stays fp32
    chk("color_condition", v, g["y"])
    g = load_golden("block_res_gfm_lfm_64")
    mod = put(L.Res_GFM_LFM(cond_c=32, out_nc=64, nf=128), g["sd"])
    with torch.no_grad():
        chk("res_gfm_lfm_64", mod((g["x"].to(DEV, H16), g["v"].to(DEV), g["cmap"].to(DEV, H16)))[0], g["y"])
    g = load_golden("block_sftlayer_32")
    mod = put(L.SFTLayer(32, 32, 32), g["sd"])
    with torch.no_grad():
        chk("sftlayer_32", mod((g["x"].to(DEV, H16), g["cmap"].to(DEV, H16))), g["y"])
    g = load_golden("block_gfmlayer_128")
    mod = put(L.GFMLayer(32, 128, 256), g["sd"])
    with torch.no_grad():
        chk("gfmlayer_128", mod((g["x"].to(DEV, H16), g["v"].to(DEV))), g["y"])
    g = load_golden("block_color_condition_gfm_lfm")
    mod = put(L.Color_Condition_GFM_LFM(4, 32, 32), g["sd"])
    with torch.no_grad():
        vec, lfm = mod(g["x"].to(DEV, H16), g["local"].to(DEV, H16))
    chk("color_condition_gfm_lfm vec", vec.flatten(1), g["y"])
    chk("color_condition_gfm_lfm lfm", lfm, g["lfm"])
    g = load_golden("block_tail_16")
    tail = put(N.seq(N.conv(16, 64, mode="C"), torch.nn.PixelShuffle(2), N.conv(16, 3, mode="C")), g["sd"])
    with torch.no_grad():
        a = ops.to_nhwc(g["x"].to(DEV, H16))
        chk("tail_16", tail[2]._nhwc(tail[0]._nhwc(a, out_mode=ops.RC_OUT_PIXEL_SHUFFLE2), out_mode=ops.RC_OUT_NCHW), g["y"])
    torch.cuda.synchronize()
    print("\n".join(f"[fp16 block] {n}: max|err| / max|ref| = {e:.2e}" for n, e in checks))
    assert all(e <= F16_TOL for _, e in checks), [(n, e) for n, e in checks if e > F16_TOL]


# ---- end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", golden_names("e2e_"))
def test_f16_end_to_end_vs_reference_golden(hip, fixture):
    g = load_golden(fixture)
    name = net_name_of(fixture)
    p = {}
    for dt in (torch.bfloat16, H16):
        net = net_on_gpu(name, dt)
        with torch.no_grad():
            y = net([g["raw"].to(DEV, dt), g["cond"].to(DEV, dt), g["coord"].to(DEV, dt)])
        torch.cuda.synchronize()
        assert y.shape == g["y"].shape and y.dtype == dt
        assert torch.isfinite(y).all()
        p[dt] = O.psnr(y.float().cpu(), g["y"])
    print(f"[fp16 e2e] {fixture}: fp16 {p[H16]:.1f} dB, bf16 {p[torch.bfloat16]:.1f} dB")
    assert p[H16] >= 70.0, p
    assert p[H16] >= p[torch.bfloat16] + 12.0, p


def test_f16_output_dtype_fp32(hip):
    g = load_golden("e2e_LiteISPNet_GFM_LSC_64x64")
    net = getattr(M, "LiteISPNet_GFM_LSC")()
    net.load_state_dict(seed0_state_dict("LiteISPNet_GFM_LSC"), strict=True)
    net = net.to(DEV, H16).eval()
    x = [g["raw"].to(DEV, H16), g["cond"].to(DEV, H16), g["coord"].to(DEV, H16)]
    with torch.no_grad():
        y16 = net(x)
        net.output_dtype = torch.float32
        y32 = net(x)
    assert y16.dtype == H16 and y32.dtype == torch.float32
    assert torch.equal(y32.half(), y16)                  # the same accumulator values, rounded once at the store
    assert O.psnr(y32.cpu(), g["y"]) >= 70.0


@pytest.mark.parametrize("name", ["LiteISPNet", "LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"])
def test_f16_ragged_uint16_mosaic_with_levels_vs_oracle(hip, name):
    """B=3 uint16 sensor counts (black 64, white 1023) through the fused ingest, padded to 16 and cropped back, against the oracle on the normalised
    RAW (>= 70 dB); a frame run alone equals the same frame inside the batch bit for bit; cond from RAW (cond=None) against the fp32 GPU path."""
    g = torch.Generator().manual_seed(7)
    h, w = 44, 70
    counts = torch.randint(64, 1024, (3, 1, 2 * h, 2 * w), generator=g).to(torch.uint16)
    norm = (counts.float() - 64.0) / (1023.0 - 64.0)
    cond = torch.rand(3, 4, 32, 48, generator=g)
    coord = O.make_coord(3, h, w)
    with torch.no_grad():
        ref = O.run_padded(name, seed0_state_dict(name), O.bayer_unshuffle(norm), cond, coord)
        net = net_on_gpu(name, H16)
        kw = dict(black_level=64.0, white_level=1023.0)
        y = net.forward_mosaic(counts.to(DEV), cond.to(DEV, H16), coord.to(DEV, H16), **kw)
        y1 = net.forward_mosaic(counts[1:2].to(DEV), cond[1:2].to(DEV, H16), coord[1:2].to(DEV, H16), **kw)
    torch.cuda.synchronize()
    assert y.shape == ref.shape == (3, 3, 2 * h, 2 * w) and y.dtype == H16
    p = O.psnr(y.float().cpu(), ref)
    print(f"[fp16 mosaic] {name}: {p:.1f} dB")
    assert p >= 70.0, p
    assert torch.equal(y1[0], y[1])
    if hasattr(net, "classifier"):
        with torch.no_grad():
            a = net.forward_mosaic(counts.to(DEV), None, coord.to(DEV, H16), **kw)
            b = net_on_gpu(name, torch.float32).forward_mosaic(counts.to(DEV), None, coord.to(DEV), **kw)
        assert O.psnr(a.float().cpu(), b.cpu()) >= 70.0


def test_f16_run_to_run_stable_and_graph_replay_equals_eager(hip):
    g = load_golden("e2e_LiteISPNet_GFM_LSC_64x64")
    net = net_on_gpu("LiteISPNet_GFM_LSC", H16)
    x = [g["raw"].to(DEV, H16), g["cond"].to(DEV, H16), g["coord"].to(DEV, H16)]
    with torch.no_grad():
        a = net(x).clone()
        b = net(x).clone()
    assert torch.equal(a, b)
    gr = torch.Generator().manual_seed(5)
    mosaic = torch.rand(2, 1, 96, 160, generator=gr).to(DEV, H16)
    cond = torch.rand(2, 4, 32, 32, generator=gr).to(DEV, H16)
    coord = O.make_coord(2, 48, 80).to(DEV, H16)
    fwd = lambda m, c, co: net.forward_mosaic(m, c, co)
    with torch.no_grad():
        eager = fwd(mosaic, cond, coord).clone()
    gf = M.GraphedCall(fwd)
    for _ in range(2):
        out = gf(mosaic, cond, coord)
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_out_of_scope_modules_refuse_f16_before_launching(hip):
    """The GroupMix net and the RAW codec have no fp16 kernels: TypeError naming the dtypes they support, and nothing is launched."""
    import realcamnet_amd.raw2bit as R2B
    log = []

    class _Log(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if str(func).startswith("realcam"):
                log.append(str(func))
            return func(*args, **(kwargs or {}))

    torch.manual_seed(0)
    gma = M.LiteISPNet_GFM_LSC_GMA().eval().to(DEV, H16)
    codec = R2B.raw_compression_tcm_final().eval().to(DEV, H16)
    raw = torch.rand(1, 4, 32, 32, device=DEV, dtype=H16)
    cond = torch.rand(1, 4, 32, 32, device=DEV, dtype=H16)
    coord = torch.rand(1, 2, 32, 32, device=DEV, dtype=H16)
    mosaic = torch.rand(1, 1, 256, 256, device=DEV, dtype=H16)
    with _Log():
        with pytest.raises(TypeError, match="fp32 / bf16"):
            gma([raw, cond, coord])
        with pytest.raises(TypeError, match="fp32 / bf16"):
            gma.forward_mosaic(mosaic[..., :64, :64], cond, coord)
        with pytest.raises(TypeError, match="fp32 / bf16"):
            codec.forward_mosaic(mosaic, cond, ops.make_coord(1, 128, 128, device=DEV, dtype=H16))
        with pytest.raises(TypeError, match="fp32 / bf16"):
            codec.compress([torch.rand(1, 4, 128, 128, device=DEV, dtype=H16), cond, torch.rand(1, 2, 128, 128, device=DEV, dtype=H16)])
    torch.cuda.synchronize()
    assert log == [], log


def test_f16_4k_frame_vs_the_fp32_gpu_path(hip):
    """One 4K LiteISPNet_GFM_LSC frame (packed 1088 x 1920 -> 2176 x 3840 sRGB), fp16 and bf16 against the fp32 GPU output of the same frame."""
    g = torch.Generator().manual_seed(4)
    h, w = 1088, 1920
    mosaic = torch.rand(1, 1, 2 * h, 2 * w, generator=g)
    cond = torch.rand(1, 4, 256, 256, generator=g)
    coord = O.make_coord(1, h, w)
    outs = {}
    for dt in (torch.float32, torch.bfloat16, H16):
        net = net_on_gpu("LiteISPNet_GFM_LSC", dt)
        with torch.no_grad():
            outs[dt] = net.forward_mosaic(mosaic.to(DEV, dt), cond.to(DEV, dt), coord.to(DEV, dt)).float()
        torch.cuda.synchronize()
    ref = outs[torch.float32].cpu()
    p16, pb = O.psnr(outs[H16].cpu(), ref), O.psnr(outs[torch.bfloat16].cpu(), ref)
    print(f"[fp16 4K] fp16 {p16:.1f} dB, bf16 {pb:.1f} dB vs the fp32 GPU path")
    assert torch.isfinite(outs[H16]).all()
    assert p16 >= pb + 12.0, (p16, pb)
