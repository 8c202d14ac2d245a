"""GPU: every streaming (pointwise.hip) and reduction (cond.hip) kernel alone, against the yardsticks of tests/streaming_ref.py.

Data movement: equal bit patterns.  Arithmetic without transcendentals: torch.equal with the fp32 restatement AND inside the rounding window of the float64
reference.  Sigmoid: the rounding window with the allowance for the device's exp (streaming_ref.SIGMOID_ULPS).  Reductions / small MLPs: the fp32 window on real-valued data, bit
equality on small-integer data (every partial sum exact in any order), and the same bits from a second call.

Coverage (entry point, storage dtypes it accepts, the test that runs it in each of them; a host test checks this table against the header):

    rc_bayer_unshuffle              f32,bf16,f16      test_bayer_unshuffle_every_dtype_pair
    rc_raw_ingest                   f32,bf16,f16      test_raw_ingest_restated
    rc_nchw_to_nhwc                 f32,bf16,f16      test_nchw_to_nhwc_both_kernels_every_dtype_pair
    rc_nhwc_to_nchw                 f32,bf16,f16      test_nhwc_to_nchw_with_crop_every_dtype_pair
    rc_gate_residual                f32,bf16,f16      test_gate_residual_and_add
    rc_film_apply                   f32,bf16,f16      test_film_apply
    rc_sigmoid_gate_add             f32,bf16,f16      test_sigmoid_gate_add
    rc_subsample2                   f32,bf16,f16      test_subsample2
    rc_upsample_bilinear2           f32,bf16,f16      test_upsample_bilinear2
    rc_sft_apply                    f32,bf16,f16      test_sft_apply
    rc_space_to_depth2              f32,bf16,f16      test_space_to_depth2_vector_and_scalar_route
    rc_pixel_shuffle2               f32,bf16,f16      test_pixel_shuffle2_both_layouts
    rc_pixel_shuffle2_nchw          f32,bf16,f16      test_pixel_shuffle2_both_layouts
    rc_square                       f32,bf16          test_square_and_gdn_apply
    rc_gdn_apply                    f32,bf16          test_square_and_gdn_apply
    rc_channel_copy                 f32,bf16          test_channel_copy_with_offsets_on_both_sides
    rc_channel_concat               f32,bf16          test_channel_concat
    rc_dwt_forward                  f32,bf16,f16      test_dwt_forward
    rc_dwt_inverse                  f32,bf16,f16      test_dwt_inverse
    rc_tail_ring_gather             f32,bf16,f16      test_tail_ring_gather
    rc_tail_ring_scatter            f32,bf16,f16      test_tail_ring_scatter_touches_the_ring_only
    rc_channel_sums_slots           -                 test_channel_sums
    rc_channel_sums                 f32,bf16,f16      test_channel_sums
    rc_ca_gate                      f32               test_ca_gate_one_and_two_stage
    rc_ca_gate_ahead_scratch_floats -                 test_ca_gate_ahead
    rc_ca_gate_ahead                f32,bf16,f16      test_ca_gate_ahead
    rc_color_block                  f32,bf16,f16      test_color_block
    rc_instance_stats               f32               test_instance_stats_and_norm
    rc_instance_norm                f32               test_instance_stats_and_norm
    rc_color_head                   f32               test_color_head
    rc_gfm_vector                   f32               test_gfm_vector
"""
import pytest
import torch

import streaming_ref as R
from realcamnet_amd import _lib, ops
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

pytestmark = pytest.mark.gpu

_R = torch.ops.realcam
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
RC = {F32: RC_F32, BF16: RC_BF16, F16: RC_F16}
DT = [pytest.param(v, id=k) for k, v in R.DTYPES.items()]
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16), (BF16, F16)]       # RC_DISPATCH_2; (F16, BF16) has no kernel


def dev(*ts):
    out = tuple(None if t is None else t.cuda() for t in ts)
    return out if len(out) > 1 else out[0]


def host(t):
    torch.cuda.synchronize()
    return t.cpu()


def assert_bits(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = R.int_view(got.contiguous()) != R.int_view(want.contiguous())
    assert not bad.any(), f"{what}: {bad.sum().item()} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def assert_arith(got, restate, ref64, slack, dtype, what):
    got = host(got)
    assert got.shape == restate.shape and got.dtype == restate.dtype, what
    ne = ~((got == restate) | (got.isnan() & restate.isnan()))
    assert not ne.any(), \
        f"{what}: {ne.sum().item()} of {ne.numel()} differ from the fp32 restatement, first at {ne.nonzero()[0].tolist()}: {got[ne][0].item()} vs {restate[ne][0].item()}"
    sign = (R.int_view(got.contiguous()) != R.int_view(restate.contiguous())) & ~got.isnan()
    assert not sign.any(), f"{what}: {sign.sum().item()} zeros carry another sign than the restatement's, first at {sign.nonzero()[0].tolist()}"
    assert_window(got, ref64, slack, dtype, what)


def assert_window(got, ref64, slack, dtype, what):
    got = host(got)
    ok = R.within_rounding(got, ref64, slack, dtype)
    assert ok.all(), f"{what}: {(~ok).sum().item()} of {ok.numel()} outside the rounding window, first at {(~ok).nonzero()[0].tolist()}"


def refused(name):
    return pytest.raises(_lib.HipError, match=name)


# ---- data movement -----------------------------------------------------------------------------------------------------------------------------------------
def test_bayer_unshuffle_every_dtype_pair(hip):
    for ti, to in PAIRS:
        for b, h, w, pad in ((1, 1, 1, 1), (3, 2, 3, 1), (1, 3, 5, 4), (3, 7, 2, 16), (1, 16, 19, 1), (1, 17, 16, 16)):
            m = R.packing_values((b, 2 * h, 2 * w), 11 + h).to(ti)
            hp, wp = -(-h // pad) * pad, -(-w // pad) * pad
            assert_bits(_R.bayer_unshuffle(dev(m), to, pad), R.ref64_bayer_unshuffle(m, to, hp, wp), f"bayer {ti}->{to} B{b} {h}x{w} pad {pad}")
    with refused("rc_bayer_unshuffle"):
        _R.bayer_unshuffle(dev(torch.zeros(1, 2, 2, dtype=F16)), BF16, 1)


def test_nchw_to_nhwc_both_kernels_every_dtype_pair(hip):
    for ti, to in PAIRS:
        for b, c, h, w, hp, wp in ((1, 1, 1, 1, 1, 1), (3, 3, 2, 3, 2, 3), (1, 4, 7, 5, 16, 16), (3, 4, 16, 19, 16, 32),        # c <= 4: one thread per pixel
                                   (1, 5, 1, 1, 1, 1), (3, 33, 3, 2, 4, 4), (1, 48, 7, 33, 16, 48), (3, 64, 6, 8, 6, 8), (1, 8, 2, 65, 3, 65)):    # 32 x 32 transpose tiles
            x = R.packing_values((b, c, h, w), 21 + c).to(ti)
            assert_bits(_R.nchw_to_nhwc(dev(x), to, hp, wp), R.ref64_nchw_to_nhwc(x, to, hp, wp), f"nchw_to_nhwc {ti}->{to} B{b} c{c} {h}x{w} -> {hp}x{wp}")
    with refused("bad dtype"):
        _R.nchw_to_nhwc(dev(torch.zeros(1, 8, 2, 2, dtype=F16)), BF16, 2, 2)


def test_nhwc_to_nchw_with_crop_every_dtype_pair(hip):
    for ti, to in PAIRS:
        for b, c, H, W, h, w in ((1, 1, 1, 1, 1, 1), (3, 3, 2, 3, 2, 3), (1, 4, 16, 16, 7, 5), (3, 33, 4, 4, 3, 2), (1, 48, 16, 48, 7, 33), (3, 64, 6, 8, 6, 8),
                                 (1, 8, 3, 65, 2, 65)):
            a = R.packing_values((b, H, W, c), 31 + c).to(ti)
            assert_bits(_R.nhwc_to_nchw(dev(a), to, h, w), R.ref64_nhwc_to_nchw(a, to, h, w), f"nhwc_to_nchw {ti}->{to} B{b} c{c} {H}x{W} -> {h}x{w}")
    with refused("bad dtype"):
        _R.nhwc_to_nchw(dev(torch.zeros(1, 2, 2, 8, dtype=F16)), BF16, 2, 2)


def pattern_cases(dtype, seed, channels=None):
    for i, (b, h, w) in enumerate(R.EW_SHAPES):
        for c in (channels or R.chans(dtype)):
            yield f"B{b} {h}x{w} c{c}", R.raw_patterns((b, h, w, c), dtype, seed + 100 * i + c)


@pytest.mark.parametrize("dtype", DT)
def test_subsample2(hip, dtype):
    for label, x in pattern_cases(dtype, 40):
        assert_bits(ops.subsample2(dev(x)), R.ref64_subsample2(x), f"subsample2 {label}")
    with refused("rc_subsample2"):
        ops.subsample2(dev(torch.zeros(1, 2, 2, R.vec_unit(dtype) + 1, dtype=dtype)))
    with pytest.raises(ValueError):
        ops.subsample2(dev(torch.zeros(4, 4, 8, dtype=dtype)))


@pytest.mark.parametrize("dtype", DT)
def test_space_to_depth2_vector_and_scalar_route(hip, dtype):
    u = R.vec_unit(dtype)
    for label, x in pattern_cases(dtype, 50, channels=[u, 3 * u, 48, 64, 1, 3, u + 1, 2 * u - 1]):      # c % U != 0: the element-wise kernel
        assert_bits(ops.space_to_depth2(dev(x)), R.ref64_space_to_depth2(x), f"space_to_depth2 {label}")
    # a misaligned base pointer with a whole-vector channel count also takes the element-wise kernel
    x = R.raw_patterns((1, 5, 6, u), dtype, 59)
    buf = torch.zeros(x.numel() + 1, dtype=dtype, device="cuda")
    buf[1:] = dev(x).reshape(-1)
    out = torch.empty(1, 3, 3, 4 * u, dtype=dtype, device="cuda")
    assert buf[1:].data_ptr() % 16 != 0
    assert hip.rc_space_to_depth2(buf[1:].data_ptr(), out.data_ptr(), RC[dtype], 1, 5, 6, u, None) == 0
    assert_bits(out, R.ref64_space_to_depth2(x), "space_to_depth2 misaligned source")
    with pytest.raises(ValueError):
        ops.space_to_depth2(dev(torch.zeros(4, 8, dtype=dtype)))


@pytest.mark.parametrize("dtype", DT)
def test_pixel_shuffle2_both_layouts(hip, dtype):
    u = R.vec_unit(dtype)
    for label, x in pattern_cases(dtype, 60, channels=[4, 12, 4 * u, 4 * 48, 4 * 3]):
        assert_bits(ops.pixel_shuffle2(dev(x)), R.ref64_pixel_shuffle2(x), f"pixel_shuffle2 {label}")
        assert_bits(ops.pixel_shuffle2_nchw(dev(x)), R.ref64_pixel_shuffle2_nchw(x), f"pixel_shuffle2_nchw {label}")
    for fn in (ops.pixel_shuffle2, ops.pixel_shuffle2_nchw):
        with pytest.raises(ValueError):
            fn(dev(torch.zeros(1, 2, 2, 6, dtype=dtype)))


def _channel_copy(hip, src, s0, dst, d0, n):
    return hip.rc_channel_copy(src.data_ptr(), src.shape[-1], s0, dst.data_ptr(), dst.shape[-1], d0, n, src.numel() // src.shape[-1], RC[src.dtype], None)


@pytest.mark.parametrize("dtype", DT)
def test_channel_copy_with_offsets_on_both_sides(hip, dtype):
    u = R.vec_unit(dtype)
    if dtype == F16:
        s, d = dev(torch.zeros(4, 16, dtype=dtype)), dev(torch.zeros(4, 16, dtype=dtype))
        assert _channel_copy(hip, s, 0, d, 0, 8) == -1 and b"rc_channel_copy: bad dtype" in hip.rc_last_error()
        with refused("rc_channel_copy"):
            ops.channel_slice(s, 0, 8)
        return
    for i, (b, h, w) in enumerate(R.EW_SHAPES):
        for cs, s0, cd, d0, n in ((u, 0, u, 0, u), (4 * u, u, 3 * u, 2 * u, u), (48 + u, u, 64, 2 * u, 48), (64, 3 * u, 64 + 2 * u, u, 64 - 3 * u), (6 * u, 3 * u, 4 * u, u, 3 * u)):
            src, dst = R.raw_patterns((b, h, w, cs), dtype, 70 + i), R.raw_patterns((b, h, w, cd), dtype, 71 + i)       # the destination's own content is the sentinel
            out = dev(dst).clone()
            assert _channel_copy(hip, dev(src), s0, out, d0, n) == 0, hip.rc_last_error()
            assert_bits(out, R.ref64_channel_copy(src, s0, dst, d0, n), f"channel_copy B{b} {h}x{w} {cs}[{s0}:+{n}] -> {cd}[{d0}:]")
        x = R.raw_patterns((b, h, w, 6 * u), dtype, 72 + i)
        assert_bits(ops.channel_slice(dev(x), 2 * u, 3 * u), x[..., 2 * u:5 * u].contiguous(), "channel_slice")


@pytest.mark.parametrize("dtype", DT)
def test_channel_concat(hip, dtype):
    u = R.vec_unit(dtype)
    if dtype == F16:
        with refused("rc_channel_concat"):
            ops.channel_concat([dev(torch.zeros(1, 2, 2, 8, dtype=dtype))] * 2)
        return
    for i, (b, h, w) in enumerate(R.EW_SHAPES):
        for widths in ((u,), (u, u), (3 * u, u, 48), (64, u, u, 2 * u, u, 3 * u), (u,) * 8, (2 * u, u, u, u, u, u, u, 48), (u,) * 9):      # 9 parts: one rc_channel_copy each
            parts = [R.raw_patterns((b, h, w, c), dtype, 80 + 10 * i + k) for k, c in enumerate(widths)]
            assert_bits(ops.channel_concat([dev(p) for p in parts]), R.ref64_channel_concat(parts), f"concat B{b} {h}x{w} {widths}")


@pytest.mark.parametrize("dtype", DT)
def test_tail_ring_gather(hip, dtype):
    u = R.vec_unit(dtype)
    for b, h, w in ((1, 2, 2), (3, 2, 3), (1, 3, 2), (3, 7, 5), (1, 16, 19), (2, 33, 4)):
        for c in (u, 3 * u, 48, 64):
            x = R.raw_patterns((b, h, w, c), dtype, 90 + h)
            rows, cols = _R.tail_ring_gather(dev(x))
            wr, wc = R.ref64_tail_ring_gather(x)
            assert_bits(rows, wr, f"ring rows B{b} {h}x{w} c{c}")
            assert_bits(cols, wc, f"ring cols B{b} {h}x{w} c{c}")
    with refused("rc_tail_ring_gather"):
        _R.tail_ring_gather(dev(torch.zeros(1, 1, 4, u, dtype=dtype)))


@pytest.mark.parametrize("dtype", DT)
def test_tail_ring_scatter_touches_the_ring_only(hip, dtype):
    for b, co, H, W in ((1, 1, 2, 2), (3, 3, 2, 3), (1, 3, 7, 5), (3, 4, 16, 19)):
        for oh, ow in ((2 * H, 2 * W), (2 * H - 1, 2 * W), (2 * H, 2 * W - 1), (2 * H - 1, 2 * W - 3), (1, 2 * W), (2 * H, 1), (2, 2)):
            if ow < 1 or oh < 1:
                continue
            rows, cols = R.raw_patterns((2 * b, co, 4, 2 * W), dtype, 100 + H), R.raw_patterns((2 * b, co, 4, 2 * H), dtype, 101 + H)
            out = R.raw_patterns((b, co, oh, ow), dtype, 102 + oh)                                      # sentinel: arbitrary bits that must survive
            got = dev(out).clone()
            _R.tail_ring_scatter(got, dev(rows), dev(cols), H, W)
            want = R.ref64_tail_ring_scatter(out, rows, cols, H, W)
            assert_bits(got, want, f"ring scatter B{b} co{co} {H}x{W} -> {oh}x{ow}")
            if oh > 2 and ow > 2:
                assert R.same_bits(want[:, :, 1:-1, 1:-1], out[:, :, 1:-1, 1:-1])
    with refused("rc_tail_ring_scatter"):
        _R.tail_ring_scatter(dev(torch.zeros(1, 3, 9, 4, dtype=dtype)), dev(torch.zeros(2, 3, 4, 8, dtype=dtype)), dev(torch.zeros(2, 3, 4, 8, dtype=dtype)), 4, 4)


# ---- arithmetic without transcendentals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_gate_residual_and_add(hip, dtype):
    for label, (r, x) in R.map_cases(dtype, 2, 100):
        b, c = r.shape[0], r.shape[3]
        g = R.per_image(b, c, 7)
        for xx in (x, None):
            got = ops.gate_residual(dev(r), dev(g), dev(xx))
            assert_arith(got, R.restate32_gate_residual(r, g, xx), R.ref64_gate_residual(r, g, xx), R.slack64_gate_residual(r, g, xx), dtype,
                         f"gate_residual {label} x={'yes' if xx is not None else 'no'}")
        one = torch.ones(b, c)
        assert_arith(ops.add(dev(r), dev(x)), R.restate32_gate_residual(r, one, x), r.double() + x.double(), R.slack64_gate_residual(r, one, x), dtype, f"add {label}")
    with refused("rc_gate_residual"):
        _R.gate_residual(dev(torch.zeros(1, 2, 2, R.vec_unit(dtype) + 1, dtype=dtype)), dev(torch.zeros(1, R.vec_unit(dtype) + 1)), None)


@pytest.mark.parametrize("dtype", DT)
def test_film_apply(hip, dtype):
    for label, (x,) in R.map_cases(dtype, 1, 150):
        b, c = x.shape[0], x.shape[3]
        s, t = R.per_image(b, c, 8), R.per_image(b, c, 9)
        assert_arith(ops.film_apply(dev(x), dev(s), dev(t)), R.restate32_film_apply(x, s, t), R.ref64_film_apply(x, s, t), R.slack64_film_apply(x, s, t), dtype, f"film {label}")


@pytest.mark.parametrize("dtype", DT)
def test_sft_apply(hip, dtype):
    for label, (x, s, t, i) in R.map_cases(dtype, 4, 200):
        for idn in (i, None):
            assert_arith(ops.sft_apply(dev(x), dev(s), dev(t), dev(idn)), R.restate32_sft_apply(x, s, t, idn), R.ref64_sft_apply(x, s, t, idn),
                         R.slack64_sft_apply(x, s, t, idn), dtype, f"sft {label} identity={'yes' if idn is not None else 'no'}")


@pytest.mark.parametrize("dtype", DT)
def test_square_and_gdn_apply(hip, dtype):
    if dtype == F16:
        z = dev(torch.ones(1, 2, 2, 8, dtype=dtype))
        with refused("rc_square"):
            ops.square(z)
        with refused("rc_gdn_apply"):
            ops.gdn_apply(z, z, False)
        return
    for label, (x, s, i) in R.map_cases(dtype, 3, 250):
        assert_arith(ops.square(dev(x)), R.restate32_square(x), R.ref64_square(x), R.slack64_square(x), dtype, f"square {label}")
        n = s.abs().float().clamp_min(2.0 ** -8).to(dtype)
        for inv in (False, True):
            for idn in (i, None):
                assert_arith(ops.gdn_apply(dev(x), dev(n), inv, dev(idn)), R.restate32_gdn_apply(x, n, inv, idn), R.ref64_gdn_apply(x, n, inv, idn),
                             R.slack64_gdn_apply(x, n, inv, idn), dtype, f"gdn {label} inverse={inv} identity={'yes' if idn is not None else 'no'}")


@pytest.mark.parametrize("dtype", DT)
def test_upsample_bilinear2(hip, dtype):
    for label, (x,) in R.map_cases(dtype, 1, 300, span=4):                                              # H == 1 and W == 1 among the shapes
        assert_arith(ops.upsample_bilinear2(dev(x)), R.restate32_upsample_bilinear2(x), R.ref64_upsample_bilinear2(x), R.slack64_upsample_bilinear2(x), dtype,
                     f"upsample {label}")
    with pytest.raises(ValueError):
        ops.upsample_bilinear2(dev(torch.zeros(4, 4, 8, dtype=dtype)))


def _dwt(hip, fn, x, out_shape, taps, uniform):
    out = torch.empty(out_shape, dtype=x.dtype, device="cuda")
    b, h, w, c = x.shape
    assert getattr(hip, fn)(x.data_ptr(), out.data_ptr(), taps.data_ptr(), int(uniform), RC[x.dtype], b, h, w, c, None) == 0, hip.rc_last_error()
    return out


@pytest.mark.parametrize("dtype", DT)
def test_dwt_forward(hip, dtype):
    for label, (x,) in R.map_cases(dtype, 1, 400, shapes=R.EVEN_SHAPES, span=4):
        b, h, w, c = x.shape
        shape = (b, h // 2, w // 2, 4 * c)
        haar, rnd = R.haar_taps(c), R.random_taps(c, 5)
        ref, slack = R.ref64_dwt_forward(x, haar), R.slack64_dwt_forward(x, haar)
        assert_arith(_R.haar_dwt(dev(x), dev(haar), True), R.restate32_dwt_forward(x, haar, True), ref, slack, dtype, f"dwt uniform {label}")
        assert_arith(_dwt(hip, "rc_dwt_forward", dev(x), shape, dev(haar), 0), R.restate32_dwt_forward(x, haar, False), ref, slack, dtype, f"dwt haar taps per channel {label}")
        assert_arith(_R.haar_dwt(dev(x), dev(rnd), True), R.restate32_dwt_forward(x, rnd, False), R.ref64_dwt_forward(x, rnd), R.slack64_dwt_forward(x, rnd), dtype,
                     f"dwt random taps {label}")
    with refused("rc_dwt_forward"):
        _R.haar_dwt(dev(torch.zeros(1, 3, 4, 8, dtype=dtype)), dev(R.haar_taps(8)), True)


@pytest.mark.parametrize("dtype", DT)
def test_dwt_inverse(hip, dtype):
    for label, (x,) in R.map_cases(dtype, 1, 500, channels=[4 * c for c in R.chans(dtype)], span=4):
        b, h, w, c4 = x.shape
        c = c4 // 4
        shape = (b, 2 * h, 2 * w, c)
        haar, rnd = R.haar_taps(c), R.random_taps(c, 6)
        ref, slack = R.ref64_dwt_inverse(x, haar), R.slack64_dwt_inverse(x, haar)
        assert_arith(_R.haar_idwt(dev(x), dev(haar), True), R.restate32_dwt_inverse(x, haar, True), ref, slack, dtype, f"idwt uniform {label}")
        assert_arith(_dwt(hip, "rc_dwt_inverse", dev(x), shape, dev(haar), 0), R.restate32_dwt_inverse(x, haar, False), ref, slack, dtype, f"idwt haar taps per channel {label}")
        assert_arith(_R.haar_idwt(dev(x), dev(rnd), True), R.restate32_dwt_inverse(x, rnd, False), R.ref64_dwt_inverse(x, rnd), R.slack64_dwt_inverse(x, rnd), dtype,
                     f"idwt random taps {label}")
    with refused("rc_dwt_inverse"):
        _R.haar_idwt(dev(torch.zeros(1, 2, 2, 2 * R.vec_unit(dtype), dtype=dtype)), dev(R.haar_taps(8)), True)


@pytest.mark.parametrize("dtype", DT)
def test_raw_ingest_restated(hip, dtype):
    for label, m, h, w, pad, ch, cw, black, white in R.raw_ingest_cases(dtype):
        packed, cond = _R.raw_ingest(dev(m), dtype, pad, black, white, ch, cw)
        pk, cd = R.raw_ingest_yardsticks(m, dtype, h, w, pad, ch, cw, black, white)
        assert_arith(packed, *pk, dtype, f"raw_ingest packed {label}")
        assert_arith(cond, *cd, dtype, f"raw_ingest cond {label}")


# ---- transcendental ------------------------------------------------------------------------------------------------------------------------------------------
def _sigmoid_inputs(dtype):
    for label, (a, b, i) in R.map_cases(dtype, 3, 600, span=4):           # |b| < 32: exp neither overflows nor reaches the subnormal range
        yield label, a, b, i


def test_sigmoid_factor_error_is_inside_the_allowance(hip):
    """Measures the device's 1 / (1 + expf(-z)) against float64 on the sigmoid tests' own arguments (a = 1, identity = 0: the output IS the factor), as a relative
    error in units of 2^-23, prints the maximum and holds it to the recorded one; streaming_ref.SIGMOID_ULPS is twice the recorded maximum, rounded up."""
    def rel(z):
        got = host(ops.sigmoid_gate_add(dev(torch.ones_like(z)), dev(z), dev(torch.zeros_like(z)))).double()
        ref = torch.sigmoid(z.double())
        return ((got - ref).abs() / ref).max().item() * 2.0 ** 23
    worst = 0.0
    for dtype in (F32, BF16, F16):
        for label, a, b, i in _sigmoid_inputs(dtype):
            worst = max(worst, rel(b.float()))
    worst = max(worst, rel(R.values((4096,), F32, 3, span=5)))           # and the range of the gates' pre-activations
    print(f"\n[sigmoid factor] measured max relative error {worst:.3f} x 2^-23; recorded {R.SIGMOID_ULPS_MEASURED}, allowed {R.SIGMOID_ULPS}")
    assert worst <= R.SIGMOID_ULPS_MEASURED and R.SIGMOID_ULPS == 3.0


@pytest.mark.parametrize("dtype", DT)
def test_sigmoid_gate_add(hip, dtype):
    for label, a, b, i in _sigmoid_inputs(dtype):
        assert_window(ops.sigmoid_gate_add(dev(a), dev(b), dev(i)), R.ref64_sigmoid_gate_add(a, b, i), R.slack64_sigmoid_gate_add(a, b, i), dtype, f"sigmoid_gate_add {label}")


# ---- reductions and small MLPs -------------------------------------------------------------------------------------------------------------------------------
def twice(fn):
    """The result of fn() and the check that a second call returns the same bits (fixed summation order)."""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert R.same_bits(host(x), host(y)), "a second call returned other bits"
    return a


@pytest.mark.parametrize("dtype", DT)
def test_channel_sums(hip, dtype):
    u = R.vec_unit(dtype)
    cases = [(1, 1, 1, u), (3, 1, 1, 48), (1, 64, 64, 48), (3, 64, 64, 3 * u), (1, 241, 17, 48), (3, 17, 241, 64), (1, 1025, 1024, u), (2, 37, 29, 256 * u)]
    for b, h, w, c in cases:                                              # n_pix = 1, 4096, 4097, 1049600 (> 256 x 4096)
        n = h * w
        assert hip.rc_channel_sums_slots(n) == R.channel_sums_layout(n)[0]
        x = R.values((b, h, w, c), dtype, 800 + c, span=3)
        got = twice(lambda: ops.channel_sums(dev(x)))
        assert_window(got, R.ref64_channel_sums(x), R.slack64_channel_sums(x), F32, f"channel_sums B{b} {h}x{w} c{c}")
        xi = R.small_ints((b, h, w, c), 801 + c, dtype=dtype)
        assert_bits(ops.channel_sums(dev(xi)), R.ref64_channel_sums(xi).float(), f"channel_sums ints B{b} {h}x{w} c{c}")
    with refused("rc_channel_sums"):
        ops.channel_sums(dev(torch.zeros(1, 2, 2, 257 * u, dtype=dtype)))
    with pytest.raises(ValueError):
        ops.channel_sums(dev(torch.zeros(4, 4, 8, dtype=dtype)))


def _mlp(c, cr, seed):
    return (R.values((cr, c), F32, seed, span=1, specials=False) / c ** 0.5, R.values((cr,), F32, seed + 1, span=1, specials=False),
            R.values((c, cr), F32, seed + 2, span=1, specials=False), R.values((c,), F32, seed + 3, span=1, specials=False))


def test_ca_gate_one_and_two_stage(hip):
    for b in (1, 3):
        for n_tiles in (1, 128, 129, 300):                                # > 128: the fold kernel first, in place
            for c, cr in ((48, 1), (48, 4), (64, 4), (64, 20), (320, 20), (320, 1)):
                hw = 4096
                sums = R.values((b, n_tiles, c), F32, 900 + n_tiles + c, span=4) * 64
                w0, b0, w1, b1 = _mlp(c, cr, 910 + c + cr)
                what = f"ca_gate B{b} tiles {n_tiles} c{c} cr{cr}"
                got = twice(lambda: _R.ca_gate(dev(sums).clone(), hw, *dev(w0, b0, w1, b1)))
                assert_window(got, R.ref64_ca_gate(sums, hw, w0, b0, w1, b1), R.slack64_ca_gate(sums, hw, w0, b0, w1, b1), F32, what)
                si = R.small_ints((b, n_tiles, c), 901 + n_tiles + c)      # exact sums: the same bits as from the pre-folded total in ONE tile
                total = si.sum(1, keepdim=True)
                assert_bits(_R.ca_gate(dev(si).clone(), hw, *dev(w0, b0, w1, b1)), host(_R.ca_gate(dev(total).clone(), hw, *dev(w0, b0, w1, b1))), what + " ints")
    assert hip.rc_ca_gate(4096, 1, 4, 20000, 2, 1.0, 4096, 4096, 4096, 4096, 4096, None) == -1 and b"rc_ca_gate" in hip.rc_last_error()


def _tile_sums(t, n_tiles):
    """Per-tile channel sums (B,n_tiles,C) of an NHWC map: any split of the pixels into n_tiles groups serves (the kernel only adds them up)."""
    b, h, w, c = t.shape
    flat = t.double().reshape(b, h * w, c)
    per = -(-h * w // n_tiles)
    flat = torch.nn.functional.pad(flat, (0, 0, 0, per * n_tiles - h * w))
    return flat.reshape(b, n_tiles, per, c).sum(2).float()


@pytest.mark.parametrize("dtype", DT)
def test_ca_gate_ahead(hip, dtype):
    for b, h, w in ((1, 1, 1), (3, 2, 3), (1, 5, 7), (3, 16, 8), (1, 33, 20)):
        for c, cr, n_tiles in ((48, 4, 1), (64, 20, 129), (8, 1, 7)):
            g = torch.Generator().manual_seed(950 + h + c)
            t = (torch.randint(-127, 128, (b, h, w, c), generator=g).float() / 64).to(dtype)            # multiples of 2^-6 below 2: exact in every dtype, tile sums exact in fp32
            sums = _tile_sums(t, n_tiles)
            w2 = R.values((c, c, 3, 3), F32, 951 + c, span=1, specials=False) / (3 * c ** 0.5)
            b2 = R.values((c,), F32, 952 + c, span=1, specials=False)
            w0, b0, w1, b1 = _mlp(c, cr, 953 + c)
            w2t = w2.permute(1, 2, 3, 0).contiguous()
            assert hip.rc_ca_gate_ahead_scratch_floats(b, c) == b * 36 * c
            for bias in (b2, None):
                what = f"ca_gate_ahead B{b} {h}x{w} c{c} cr{cr} tiles {n_tiles} bias={'yes' if bias is not None else 'no'}"
                got = twice(lambda: _R.ca_gate_ahead(dev(sums).clone(), dev(t), dev(w2t), dev(bias), *dev(w0, b0, w1, b1))[0])
                assert_window(got, R.ref64_ca_gate_ahead(t, w2, bias, w0, b0, w1, b1), R.slack64_ca_gate_ahead(t, n_tiles, w2, bias, w0, b0, w1, b1), F32, what)
    # integers, H*W a power of two: every sum is exact, so the gate equals rc_ca_gate of the materialised conv output's exact sums bit for bit
    for b, h, w, c, cr, n_tiles in ((3, 16, 8, 48, 4, 129), (1, 8, 16, 64, 20, 5)):
        t = R.small_ints((b, h, w, c), 960, 2, dtype)
        w2, b2 = R.small_ints((c, c, 3, 3), 961, 2), R.small_ints((c,), 962, 2)
        w0, b0, w1, b1 = _mlp(c, cr, 963)
        conv_sums = R.ref64_conv_tile_sums(t, w2, b2)
        assert conv_sums.abs().max() < 2 ** 24
        got = _R.ca_gate_ahead(dev(_tile_sums(t, n_tiles)), dev(t), dev(w2.permute(1, 2, 3, 0).contiguous()), dev(b2), *dev(w0, b0, w1, b1))[0]
        assert_bits(got, host(_R.ca_gate(dev(conv_sums.float()), h * w, *dev(w0, b0, w1, b1))), f"ca_gate_ahead ints B{b} {h}x{w} c{c}")


@pytest.mark.parametrize("dtype", DT)
def test_color_block(hip, dtype):
    for b in (1, 3):
        for cin, cout in ((4, 8), (64, 128), (256, 48)):
            for h, w in ((1, 1), (2, 7), (7, 2), (16, 33), (33, 16), (1, 16)):
                x = R.values((b, cin, h, w), dtype, 1000 + cin + h, span=3)
                wgt = R.values((cout, cin), F32, 1001 + cin, span=1, specials=False) / cin ** 0.5
                bias = R.values((cout,), F32, 1002 + cin, span=1, specials=False)
                mean, rstd = R.values((b, cin), F32, 1003, span=1), R.values((b, cin), F32, 1004, span=1, specials=False).abs()
                gm, bt = R.values((cin,), F32, 1005, span=1, specials=False), R.values((cin,), F32, 1006, span=1)
                for norm in ((None, None, None, None), (mean, rstd, gm, bt)):
                    what = f"color_block B{b} {cin}->{cout} {h}x{w} norm={'yes' if norm[0] is not None else 'no'}"
                    got = twice(lambda: _R.color_block(dev(x), dev(wgt), dev(bias), *dev(*norm)))
                    assert_window(got, R.ref64_color_block(x, wgt, bias, *norm), R.slack64_color_block(x, wgt, bias, *norm), F32, what)
                xi, wi, bi = R.small_ints((b, cin, h, w), 1007 + h, 8, dtype), R.small_ints((cout, cin), 1008, 3), R.small_ints((cout,), 1009, 3)
                assert_bits(_R.color_block(dev(xi), dev(wi), dev(bi), None, None, None, None), R.restate32_color_block_ints(xi, wi, bi),
                            f"color_block ints B{b} {cin}->{cout} {h}x{w}")
    with refused("rc_color_block"):
        _R.color_block(dev(torch.zeros(1, 4, 2, 2, dtype=dtype)), dev(torch.zeros(4, 4)), dev(torch.zeros(4)), dev(torch.zeros(1, 4)), None, None, None)


@pytest.mark.parametrize("dtype", DT)
def test_color_block_cout_slices_do_not_change_the_bits(hip, dtype):
    """One image of an 8 x 8 output is ONE pixel tile, so the launcher cuts cout into slices to fill the chip; inside 512 such images there are enough tiles and it
    does not.  Same sums in the same order: image 0 must come out bit for bit the same."""
    cin, cout = 64, 128
    x = R.values((512, cin, 16, 16), F32, 1100, span=3, specials=False).to(dtype)
    wgt, bias = R.values((cout, cin), F32, 1101, span=1, specials=False) / 8, R.values((cout,), F32, 1102, span=1, specials=False)
    xd = dev(x)
    whole = _R.color_block(xd, dev(wgt), dev(bias), None, None, None, None)
    alone = _R.color_block(xd[:1].contiguous(), dev(wgt), dev(bias), None, None, None, None)
    assert_bits(alone, host(whole)[:1].contiguous(), "color_block image 0 alone vs inside a batch of 512")
    assert_window(alone, R.ref64_color_block(x[:1], wgt, bias), R.slack64_color_block(x[:1], wgt, bias), F32, "color_block 8x8 output")


def test_instance_stats_and_norm(hip):
    for label, x, y, m32, r32, gm, bt in R.instance_cases():
        b, c, hw = x.shape[0], x.shape[1], x.shape[3]
        mean, rstd = twice(lambda: ops.instance_stats(dev(x), 1e-5))
        rm, rr = R.ref64_instance_stats(x, 1e-5)
        em, er = R.slack64_instance_stats(x, 1e-5)
        assert_window(mean, rm, em, F32, f"instance mean {label}")
        assert_window(rstd, rr, er, F32, f"instance rstd {label}")
        xi = R.integer_mean_map(b, c, hw)
        mi, ri = ops.instance_stats(dev(xi), 1e-5)
        wm, wr = R.restate32_instance_stats_ints(xi, 1e-5)
        assert_bits(mi, wm, f"instance mean ints {label}")
        assert_bits(ri, wr, f"instance rstd ints {label}")
        # the normalisation with GIVEN statistics (per plane, differing between the images)
        assert_arith(_R.instance_norm(dev(y), *dev(m32, r32, gm, bt)), R.restate32_instance_norm(y, m32, r32, gm, bt), R.ref64_instance_norm(y, m32, r32, gm, bt),
                     R.slack64_instance_norm(y, m32, r32, gm, bt), F32, f"instance_norm {label}")
    for bad in (torch.zeros(2, 8, 16), torch.zeros(2, 8, 4, 4, dtype=BF16), torch.zeros(2, 8, 4, 4, dtype=F16)):
        with pytest.raises(ValueError):
            ops.instance_stats(dev(bad))


class _Conv1x1:
    def __init__(self, w, b):
        self.weight, self.bias = torch.nn.Parameter(w.cuda()[:, :, None, None]), torch.nn.Parameter(b.cuda())


def test_color_head(hip):
    for b in (1, 3):
        for cin, cout in ((4, 3), (64, 64)):
            for hw in (1, 255, 256, 257, 1000):
                x = R.values((b, cin, 1, hw), F32, 1300 + hw, span=3)
                wgt, bias = R.values((cout, cin), F32, 1301, span=1, specials=False), R.values((cout,), F32, 1302, span=1)
                conv = _Conv1x1(wgt, bias)
                got = twice(lambda: ops.color_head(dev(x), conv))
                assert_window(got, R.ref64_color_head(x, wgt, bias), R.slack64_color_head(x, wgt, bias), F32, f"color_head B{b} {cin}->{cout} hw{hw}")
                xi, wi, bi = R.small_ints((b, cin, 1, hw), 1303, 8), R.small_ints((cout, cin), 1304, 3), R.small_ints((cout,), 1305, 3)
                assert_bits(_R.color_head(dev(xi), dev(wi), dev(bi)), R.restate32_color_head_ints(xi, wi, bi), f"color_head ints B{b} {cin}->{cout} hw{hw}")
    for bad in (torch.zeros(2, 64, 16), torch.zeros(2, 64, 4, 4, dtype=BF16), torch.zeros(2, 8, 4, 4)):
        with pytest.raises(ValueError):
            ops.color_head(dev(bad), conv)


def test_gfm_vector(hip):
    for label, v, w0, b0, w1, b1 in R.gfm_cases():
        got = twice(lambda: _R.gfm_vector(*dev(v, w0, b0, w1, b1)))
        what = f"gfm_vector {label}"
        assert_arith(got, R.restate32_gfm_vector(v, w0, b0, w1, b1), R.ref64_gfm_vector(v, w0, b0, w1, b1), R.slack64_gfm_vector(v, w0, b0, w1, b1), F32, what)
        vi, wi0, bi0, wi1, bi1 = (R.small_ints(t.shape, 1405 + k, 3) for k, t in enumerate((v, w0, b0, w1, b1)))
        assert_bits(_R.gfm_vector(*dev(vi, wi0, bi0, wi1, bi1)), R.restate32_gfm_vector(vi, wi0, bi0, wi1, bi1), what + " ints")
    assert hip.rc_gfm_vector(4096, 1, 9000, 9000, 8, 4096, 4096, 4096, 4096, 4096, None) == -1 and b"rc_gfm_vector" in hip.rc_last_error()


# ---- the grid-stride loops ------------------------------------------------------------------------------------------------------------------------------------
def _pointwise_runs(hip, dtype):
    """One case of every pointwise.hip entry point that sizes its launch with grid_for, at least two trips of the 768 threads each: name -> callable returning its output tensors."""
    u = R.vec_unit(dtype)
    dt2 = dtype if dtype != F16 else BF16                                 # the entry points without fp16 kernels run in bf16
    u2 = R.vec_unit(dt2)
    x, s, t, i = (dev(R.values((2, 18, 22, 6 * u), dtype, 1500 + k, span=3)) for k in range(4))
    x2, s2, i2 = (dev(R.values((2, 18, 22, 6 * u2), dt2, 1510 + k, span=3)) for k in range(3))
    n2 = s2.abs().float().clamp_min(2.0 ** -8).to(dt2)
    g, sh = dev(R.per_image(2, 6 * u, 1), R.per_image(2, 6 * u, 2))
    mosaic = dev(R.values((2, 60, 76), F32, 1520, span=2).abs().to(dtype))
    nchw = dev(R.values((2, 3, 50, 70), dtype, 1521))
    odd = dev(R.values((2, 17, 21, u + 1), dtype, 1522))
    haar, rnd = dev(R.haar_taps(6 * u), R.random_taps(6 * u, 3))
    xi = dev(R.values((2, 18, 22, 8 * u), dtype, 1523))
    rows, cols = dev(R.values((4, 3, 4, 400), dtype, 1524), R.values((4, 3, 4, 600), dtype, 1525))

    def scatter():
        out = torch.full((2, 3, 600, 399), 7.0, dtype=dtype, device="cuda")
        _R.tail_ring_scatter(out, rows, cols, 300, 200)
        return out

    def copy():
        out = torch.full((2, 18, 22, 8 * u2), 7.0, dtype=dt2, device="cuda")
        assert _channel_copy(hip, x2, 2 * u2, out, u2, 3 * u2) == 0
        return out
    return {
        "bayer_unshuffle": lambda: _R.bayer_unshuffle(mosaic, dtype, 16), "raw_ingest": lambda: _R.raw_ingest(mosaic, dtype, 16, 0.0, 1.0, 40, 56),
        "nchw_to_nhwc": lambda: _R.nchw_to_nhwc(nchw, dtype, 64, 80),          # c <= 4; the 32 x 32 tile kernels of both directions launch fixed 3-D grids (no grid_for)
        "gate_residual": lambda: _R.gate_residual(x, g, s), "film_apply": lambda: _R.film_apply(x, g, sh), "sigmoid_gate_add": lambda: _R.sigmoid_gate_add(x, s, i),
        "subsample2": lambda: _R.subsample2(x), "upsample_bilinear2": lambda: _R.upsample_bilinear2(x), "sft_apply": lambda: _R.sft_apply(x, s, t, i),
        "space_to_depth2": lambda: _R.space_to_depth2(x), "space_to_depth2 scalar": lambda: _R.space_to_depth2(odd),
        "pixel_shuffle2": lambda: _R.pixel_shuffle2(x), "pixel_shuffle2_nchw": lambda: _R.pixel_shuffle2_nchw(x),
        "square": lambda: _R.square(x2), "gdn_apply": lambda: _R.gdn_apply(x2, n2, False, i2), "gdn_apply inverse": lambda: _R.gdn_apply(x2, n2, True, None),
        "channel_copy": copy, "channel_concat": lambda: _R.channel_concat([x2, s2, i2]),
        "dwt_forward": lambda: _R.haar_dwt(x, haar, True), "dwt_forward taps": lambda: _R.haar_dwt(x, rnd, True),
        "dwt_inverse": lambda: _R.haar_idwt(xi, dev(R.haar_taps(2 * u)), True), "dwt_inverse taps": lambda: _R.haar_idwt(xi, dev(R.random_taps(2 * u, 4)), True),
        "tail_ring_gather": lambda: _R.tail_ring_gather(x), "tail_ring_scatter": scatter,
    }


@pytest.mark.parametrize("dtype", DT)
def test_grid_stride_loops_give_the_one_shot_bits(hip, dtype):
    """rc_debug_set("pw_grid_cap", 3): every pointwise.hip kernel runs its items through the grid-stride loop of 3 blocks (768 threads) and must return the bits of
    the one-shot launch."""
    runs = _pointwise_runs(hip, dtype)
    assert hip.rc_debug_get(b"pw_grid_cap") == 1 << 22
    one_shot = {k: fn() for k, fn in runs.items()}
    torch.cuda.synchronize()
    try:
        assert hip.rc_debug_set(b"pw_grid_cap", 3) == 0 and hip.rc_debug_get(b"pw_grid_cap") == 3
        looped = {k: fn() for k, fn in runs.items()}
        torch.cuda.synchronize()
    finally:
        hip.rc_debug_set(b"pw_grid_cap", 0)
    assert hip.rc_debug_get(b"pw_grid_cap") == 1 << 22
    for k in runs:
        a, b = one_shot[k], looped[k]
        for p, q in zip(a if isinstance(a, (tuple, list)) else (a,), b if isinstance(b, (tuple, list)) else (b,)):
            assert p.numel() >= 768 * 2, (k, p.numel())
            assert_bits(q, host(p), f"grid-stride {k}")
