"""CPU: the yardsticks of tests/streaming_ref.py against each other and against torch functionals (so that they are known good before a GPU run), the argument
checks of every streaming / reduction entry point, and the coverage table of test_streaming_gpu.py against the header."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = [pytest.param(v, id=k) for k, v in R.DTYPES.items()]


def _inside(restate, ref64, slack, dtype, what):
    ok = R.within_rounding(restate, ref64, slack, dtype)
    assert ok.all(), f"{what}: {(~ok).sum().item()} of {ok.numel()} outside, worst {((restate.double() - ref64).abs() - slack).max().item():.3e}"


# ---- within_rounding itself ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_within_rounding_accepts_both_neighbours_of_a_tie_and_rejects_two_steps(dtype):
    base = torch.tensor([1.25, -3.0, 0.15625, 1000.0, -1.5 * 2.0 ** -10], dtype=dtype)       # no powers of two: the spacing is the same on both sides
    nxt = (R.int_view(base) + 1).view(dtype)                              # the next representable value away from zero
    step = nxt.double() - base.double()
    tie = base.double() + step / 2                                        # exactly between two representable values
    zero = torch.zeros_like(tie)
    eps = step.abs() * 2.0 ** -10                                         # resolvable in fp32, the first of the two casts
    assert R.within_rounding(base, tie, eps, dtype).all() and R.within_rounding(nxt, tie, eps, dtype).all()
    two = (base.double() + 2 * step).to(dtype)
    back = (base.double() - step).to(dtype)
    assert not R.within_rounding(two, base.double(), step.abs() * 0.25, dtype).any()
    assert not R.within_rounding(two, tie, eps, dtype).any() and not R.within_rounding(back, tie, eps, dtype).any()
    assert R.within_rounding(base, base.double(), zero, dtype).all() and not R.within_rounding(nxt, base.double(), zero, dtype).any()


# ---- restatements inside the rounding window of the float64 references -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_restatements_of_the_per_image_kernels(dtype):
    for label, (r, x) in R.map_cases(dtype, 2, 100):
        b, c = r.shape[0], r.shape[3]
        g, s = R.per_image(b, c, 7), R.per_image(b, c, 8)
        for xx in (x, None):
            _inside(R.restate32_gate_residual(r, g, xx), R.ref64_gate_residual(r, g, xx), R.slack64_gate_residual(r, g, xx), dtype, f"gate_residual {label}")
        _inside(R.restate32_film_apply(x, g, s), R.ref64_film_apply(x, g, s), R.slack64_film_apply(x, g, s), dtype, f"film {label}")
        xd, gd = x.double(), g.double().reshape(b, 1, 1, c)
        assert torch.equal(R.ref64_gate_residual(r, g, x), torch.addcmul(xd, r.double(), gd))
        assert torch.allclose(R.ref64_film_apply(x, g, s), torch.addcmul(xd + s.double().reshape(b, 1, 1, c), xd, gd), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dtype", DT)
def test_restatements_of_the_elementwise_kernels(dtype):
    for label, (x, s, t, i) in R.map_cases(dtype, 4, 200):
        for idn in (i, None):
            _inside(R.restate32_sft_apply(x, s, t, idn), R.ref64_sft_apply(x, s, t, idn), R.slack64_sft_apply(x, s, t, idn), dtype, f"sft {label}")
        assert torch.equal(R.ref64_sft_apply(x, s, t, None), torch.addcmul(t.double(), x.double(), s.double()) + x.double())
        _inside(R.restate32_square(x), R.ref64_square(x), R.slack64_square(x), dtype, f"square {label}")
        assert torch.equal(R.ref64_square(x), torch.square(x.double()))
        n = s.abs().float().clamp_min(2.0 ** -8).to(dtype)
        for inv in (False, True):
            for idn in (i, None):
                _inside(R.restate32_gdn_apply(x, n, inv, idn), R.ref64_gdn_apply(x, n, inv, idn), R.slack64_gdn_apply(x, n, inv, idn), dtype, f"gdn {label}")
        assert torch.allclose(R.ref64_gdn_apply(x, n, False, None), x.double() / torch.sqrt(n.double()), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dtype", DT)
def test_restatement_of_the_bilinear_upsampling(dtype):
    for label, (x,) in R.map_cases(dtype, 1, 300, span=4):
        _inside(R.restate32_upsample_bilinear2(x), R.ref64_upsample_bilinear2(x), R.slack64_upsample_bilinear2(x), dtype, f"upsample {label}")


@pytest.mark.parametrize("dtype", DT)
def test_restatements_of_the_haar_transforms(dtype):
    for label, (x,) in R.map_cases(dtype, 1, 400, shapes=R.EVEN_SHAPES, span=4):
        c = x.shape[3]
        for taps, uni in ((R.haar_taps(c), True), (R.haar_taps(c), False), (R.random_taps(c, 5), False)):
            _inside(R.restate32_dwt_forward(x, taps, uni), R.ref64_dwt_forward(x, taps), R.slack64_dwt_forward(x, taps), dtype, f"dwt {label}")
    for label, (x,) in R.map_cases(dtype, 1, 500, channels=[4 * c for c in R.chans(dtype)], span=4):
        c = x.shape[3] // 4
        for taps, uni in ((R.haar_taps(c), True), (R.haar_taps(c), False), (R.random_taps(c, 6), False)):
            _inside(R.restate32_dwt_inverse(x, taps, uni), R.ref64_dwt_inverse(x, taps), R.slack64_dwt_inverse(x, taps), dtype, f"idwt {label}")
    # the Haar pair is orthonormal: the inverse of the forward transform returns the input (float64)
    x = R.values((2, 4, 6, 8), torch.float32, 1)
    assert torch.allclose(R.ref64_dwt_inverse(R.ref64_dwt_forward(x, R.haar_taps(8)), R.haar_taps(8)), x.double(), rtol=0, atol=1e-12)


def test_instance_norm_yardsticks_agree_with_the_functional():
    for hw in ((1, 1), (15, 17), (16, 16), (1, 257), (25, 40)):
        x = R.values((3, 5, *hw), torch.float32, 600 + hw[1], span=3)
        gm, bt = R.values((5,), torch.float32, 1, span=1, specials=False), R.values((5,), torch.float32, 2, span=1, specials=False)
        mean, rstd = R.ref64_instance_stats(x, 1e-5)
        ref = R.ref64_instance_norm(x, mean, rstd, gm, bt)
        if hw != (1, 1):
            assert torch.allclose(ref, F.instance_norm(x.double(), weight=gm.double(), bias=bt.double(), eps=1e-5), rtol=1e-10, atol=1e-10)
        m32, r32 = mean.float(), rstd.float()
        _inside(R.restate32_instance_norm(x, m32, r32, gm, bt), R.ref64_instance_norm(x, m32, r32, gm, bt), R.slack64_instance_norm(x, m32, r32, gm, bt),
                torch.float32, f"instance_norm {hw}")
        e_m, e_r = R.slack64_instance_stats(x, 1e-5)                       # a plain fp32 evaluation lies inside the statistics' slack
        v32, mm32 = torch.var_mean(x, dim=(2, 3), unbiased=False)
        assert ((mm32.double() - mean).abs() <= e_m).all() and (((v32 + 1e-5).rsqrt().double() - rstd).abs() <= e_r).all()


@pytest.mark.parametrize("dtype", DT)
def test_restatement_of_raw_ingest(dtype):
    for label, m, h, w, pad, ch, cw, black, white in R.raw_ingest_cases(dtype):
        pk, cd = R.raw_ingest_yardsticks(m, dtype, h, w, pad, ch, cw, black, white)
        _inside(*pk, dtype, f"raw_ingest packed {label}")
        _inside(*cd, dtype, f"raw_ingest cond {label}")
        if (h, w) == (ch, cw):                                            # same size: the resize is the identity
            assert torch.allclose(cd[1], pk[1][:, :h, :w].permute(0, 3, 1, 2), rtol=0, atol=1e-12)


def test_restatements_of_instance_norm_and_gfm_vector_on_the_gpu_tests_inputs():
    for label, x, y, m32, r32, gm, bt in R.instance_cases():
        _inside(R.restate32_instance_norm(y, m32, r32, gm, bt), R.ref64_instance_norm(y, m32, r32, gm, bt), R.slack64_instance_norm(y, m32, r32, gm, bt),
                torch.float32, f"instance_norm {label}")
    for label, v, w0, b0, w1, b1 in R.gfm_cases():
        _inside(R.restate32_gfm_vector(v, w0, b0, w1, b1), R.ref64_gfm_vector(v, w0, b0, w1, b1), R.slack64_gfm_vector(v, w0, b0, w1, b1), torch.float32, f"gfm {label}")
        assert torch.allclose(R.ref64_gfm_vector(v, w0, b0, w1, b1),
                              torch.addmm(b1.double(), F.leaky_relu(torch.addmm(b0.double(), v.double(), w0.double().T), 0.1), w1.double().T), rtol=1e-12, atol=1e-12)


def test_integer_restatements_agree_with_the_float64_references():
    x = R.small_ints((2, 64, 7, 9), 1, dtype=torch.bfloat16)
    w, b = R.small_ints((32, 64), 2, 3), R.small_ints((32,), 3, 3)
    got, ref = R.restate32_color_block_ints(x, w, b), R.ref64_color_block(x, w, b)
    assert ((got.double() - ref).abs() <= R.slack64_color_block(x, w, b)).all()
    xh = R.small_ints((2, 16, 5, 51), 4)
    assert ((R.restate32_color_head_ints(xh, w[:, :16], b).double() - R.ref64_color_head(xh, w[:, :16], b)).abs() <= R.slack64_color_head(xh, w[:, :16], b)).all()
    v = R.values((3, 40), torch.float32, 5, span=2)
    w0, b0, w1, b1 = (R.values(s, torch.float32, 6 + i, span=1) for i, s in enumerate(((300, 40), (300,), (70, 300), (70,))))
    assert ((R.restate32_gfm_vector(v, w0, b0, w1, b1).double() - R.ref64_gfm_vector(v, w0, b0, w1, b1)).abs() <= R.slack64_gfm_vector(v, w0, b0, w1, b1)).all()
    xs = R.integer_mean_map(2, 3, 1000)
    m, r = R.restate32_instance_stats_ints(xs, 1e-5)
    m64, r64 = R.ref64_instance_stats(xs, 1e-5)
    e_m, e_r = R.slack64_instance_stats(xs, 1e-5)
    assert ((m.double() - m64).abs() <= e_m).all() and ((r.double() - r64).abs() <= e_r).all()


def test_movement_references_against_other_functionals():
    for dtype in R.DTYPES.values():
        x = R.raw_patterns((2, 5, 7, 16), dtype, 1)
        xi = R.int_view(x)
        assert R.same_bits(R.ref64_subsample2(x), F.max_pool2d(xi.permute(0, 3, 1, 2).double(), 1, 2).permute(0, 2, 3, 1).to(xi.dtype).view(dtype))
        s2d = R.ref64_space_to_depth2(x)
        assert s2d.shape == (2, 3, 4, 64)
        for ph in range(4):                                               # phase ph = 2i + j of the zero-padded map, by slicing
            padded = F.pad(xi, (0, 0, 0, 1, 0, 1))
            assert torch.equal(R.int_view(s2d)[..., ph * 16:(ph + 1) * 16], padded[:, (ph >> 1)::2, (ph & 1)::2])
        ps = R.ref64_pixel_shuffle2(x)                                    # (2,10,14,4): out[2y+i][2x+j][k] = in[y][x][4k + 2i + j]
        for i in range(2):
            for j in range(2):
                assert torch.equal(R.int_view(ps)[:, i::2, j::2], xi[..., 2 * i + j::4])
        assert R.same_bits(R.ref64_pixel_shuffle2_nchw(x), ps.permute(0, 3, 1, 2).contiguous())
        assert R.same_bits(R.ref64_space_to_depth2(R.ref64_pixel_shuffle2(x)[..., :1].contiguous()).reshape(2, 5, 7, 4), x[..., :4].contiguous())
    # the ring scatter against a per-pixel loop
    out = torch.full((2, 3, 7, 10), -7.0)
    rows, cols = R.values((4, 3, 4, 10), torch.float32, 1), R.values((4, 3, 4, 8), torch.float32, 2)
    for oh, ow in ((8, 10), (7, 10), (8, 9), (5, 3)):
        o = torch.full((2, 3, oh, ow), -7.0)
        want = o.clone()
        for b in range(2):
            for y in range(oh):
                for xx in range(ow):
                    if y == 0:
                        want[b, :, y, xx] = rows[b, :, 0, xx]
                    elif y == oh - 1 and oh == 8:
                        want[b, :, y, xx] = rows[2 + b, :, 3, xx]
                    elif xx == 0:
                        want[b, :, y, xx] = cols[b, :, 0, y]
                    elif xx == ow - 1 and ow == 10:
                        want[b, :, y, xx] = cols[2 + b, :, 3, y]
        assert torch.equal(R.ref64_tail_ring_scatter(o, rows, cols, 4, 5), want), (oh, ow)
    del out


def test_channel_sum_layout_and_reference():
    assert [R.channel_sums_layout(n) for n in (1, 4096, 4097, 1049600)] == [(1, 1), (1, 4096), (2, 2049), (256, 4100)]
    lib = _lib.load()
    for n in (1, 4095, 4096, 4097, 8193, 1048576, 1048577, 1049600):
        assert lib.rc_channel_sums_slots(n) == R.channel_sums_layout(n)[0]
    x = R.values((2, 70, 60, 8), torch.bfloat16, 3)
    ref = R.ref64_channel_sums(x)
    assert ref.shape == (2, 2, 8) and torch.allclose(ref.sum(1), F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), 1)[:, :, 0, 0] * 4200, rtol=1e-12)


def test_ca_gate_ahead_reference_equals_the_closed_form():
    """The gate-ahead identity the kernel relies on (the mean of a zero-padded 3x3 convolution from the input's total, border lines and corners), in float64."""
    t = R.values((2, 5, 6, 8), torch.float32, 1, span=2).double()
    w2 = R.values((8, 8, 3, 3), torch.float32, 2, span=1).double()
    tot = t.sum((1, 2))
    r0, r1, q0, q1 = t[:, 0].sum(1), t[:, -1].sum(1), t[:, :, 0].sum(1), t[:, :, -1].sum(1)
    k = {(0, 0): t[:, 0, 0], (0, 2): t[:, 0, -1], (2, 0): t[:, -1, 0], (2, 2): t[:, -1, -1]}
    mean = torch.zeros(2, 8, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            s = tot.clone()
            if dy == 0: s = s - r1
            if dy == 2: s = s - r0
            if dx == 0: s = s - q1
            if dx == 2: s = s - q0
            if dy != 1 and dx != 1: s = s + k[(2 - dy, 2 - dx)]
            mean += s @ w2[:, :, dy, dx].T
    assert torch.allclose(mean[:, None], R.ref64_conv_tile_sums(t, w2, None), rtol=1e-12, atol=1e-12)


# ---- argument checks (no GPU: every call must be refused before a launch) ----------------------------------------------------------------------------------
P, Q = 4096, 4100          # dummy device pointers: 16-byte aligned / not


def _bad_calls():
    f, h = RC_F32, RC_BF16
    ew = lambda name, n_ptr, tail_ok: [(name, (*[P] * n_ptr, *tail_ok))]
    t = []
    # (entry point, arguments); every line one fault
    for dt, u in ((f, 4), (h, 8), (RC_F16, 8)):
        t += [("rc_gate_residual", (Q, P, P, P, dt, 1, 4, 2 * u, None)), ("rc_gate_residual", (P, P, Q, P, dt, 1, 4, 2 * u, None)),
              ("rc_gate_residual", (P, P, P, Q, dt, 1, 4, 2 * u, None)), ("rc_gate_residual", (P, P, P, P, dt, 1, 4, u + 1, None)),
              ("rc_gate_residual", (P, P, P, P, dt, 1, 4, 0, None)), ("rc_gate_residual", (P, P, P, P, dt, 0, 4, u, None)),
              ("rc_gate_residual", (P, P, P, P, dt, 1, 0, u, None)),
              ("rc_film_apply", (Q, P, P, P, dt, 1, 4, u, None)), ("rc_film_apply", (P, P, P, Q, dt, 1, 4, u, None)),
              ("rc_film_apply", (P, P, P, P, dt, 1, 4, u - 1, None)), ("rc_film_apply", (P, P, P, P, dt, 1, 0, u, None)),
              ("rc_film_apply", (P, P, P, P, dt, 1, 4, 0, None)),
              ("rc_sigmoid_gate_add", (P, Q, P, P, dt, 4 * u, None)), ("rc_sigmoid_gate_add", (P, P, P, P, dt, u + 2, None)),
              ("rc_sigmoid_gate_add", (P, P, P, P, dt, 0, None)),
              ("rc_subsample2", (Q, P, dt, 1, 4, 4, u, None)), ("rc_subsample2", (P, P, dt, 1, 4, 4, u + 1, None)), ("rc_subsample2", (P, P, dt, 1, 0, 4, u, None)),
              ("rc_subsample2", (P, P, dt, 1, 4, 4, 0, None)),
              ("rc_upsample_bilinear2", (P, Q, dt, 1, 4, 4, u, None)), ("rc_upsample_bilinear2", (P, P, dt, 1, 4, 4, u // 2, None)),
              ("rc_upsample_bilinear2", (P, P, dt, 1, 4, 0, u, None)), ("rc_upsample_bilinear2", (P, P, dt, 0, 4, 4, u, None)),
              ("rc_sft_apply", (P, P, Q, P, P, dt, 4 * u, None)), ("rc_sft_apply", (P, P, P, Q, P, dt, 4 * u, None)), ("rc_sft_apply", (P, P, P, P, P, dt, u + 1, None)),
              ("rc_sft_apply", (P, P, P, P, P, dt, 0, None)),
              ("rc_space_to_depth2", (P, P, dt, 1, 0, 4, u, None)), ("rc_space_to_depth2", (P, P, dt, 1, 4, 4, 0, None)), ("rc_space_to_depth2", (None, P, dt, 1, 4, 4, u, None)),
              ("rc_pixel_shuffle2", (P, P, dt, 1, 4, 0, 4, None)), ("rc_pixel_shuffle2", (P, P, dt, 1, 4, 4, 0, None)), ("rc_pixel_shuffle2", (P, None, dt, 1, 4, 4, 4, None)),
              ("rc_pixel_shuffle2_nchw", (P, P, dt, 0, 4, 4, 4, None)), ("rc_pixel_shuffle2_nchw", (P, P, dt, 1, 4, 4, 0, None)),
              ("rc_dwt_forward", (Q, P, P, 1, dt, 1, 4, 4, u, None)), ("rc_dwt_forward", (P, Q, P, 1, dt, 1, 4, 4, u, None)),
              ("rc_dwt_forward", (P, P, P, 1, dt, 1, 4, 4, 0, None)), ("rc_dwt_forward", (P, P, P, 0, dt, 1, 4, 4, u + 4, None) if u == 8 else (P, P, P, 0, dt, 1, 4, 4, 6, None)),
              ("rc_dwt_forward", (P, P, P, 1, dt, 1, 4, 3, u, None)), ("rc_dwt_forward", (P, P, P, 1, dt, 1, 0, 4, u, None)),
              ("rc_dwt_inverse", (Q, P, P, 1, dt, 1, 4, 4, 4 * u, None)), ("rc_dwt_inverse", (P, Q, P, 1, dt, 1, 4, 4, 4 * u, None)),
              ("rc_dwt_inverse", (P, P, P, 1, dt, 1, 4, 4, 0, None)), ("rc_dwt_inverse", (P, P, P, 1, dt, 1, 4, 4, 2 * u, None)),
              ("rc_dwt_inverse", (P, P, P, 1, dt, 1, 0, 4, 4 * u, None)),
              ("rc_tail_ring_gather", (Q, P, P, dt, 1, 4, 4, u, None)), ("rc_tail_ring_gather", (P, P, Q, dt, 1, 4, 4, u, None)),
              ("rc_tail_ring_gather", (P, P, P, dt, 1, 4, 4, u + 1, None)), ("rc_tail_ring_gather", (P, P, P, dt, 1, 1, 4, u, None)),
              ("rc_tail_ring_gather", (P, P, P, dt, 1, 4, 4, 0, None)),
              ("rc_tail_ring_scatter", (P, P, P, dt, 1, 3, 4, 4, 9, 8, None)), ("rc_tail_ring_scatter", (P, P, P, dt, 1, 3, 1, 4, 2, 8, None)),
              ("rc_tail_ring_scatter", (P, P, P, dt, 1, 0, 4, 4, 8, 8, None)), ("rc_tail_ring_scatter", (P, P, P, dt, 1, 3, 4, 4, 8, 0, None)),
              ("rc_channel_sums", (Q, dt, 1, 16, u, P, None)), ("rc_channel_sums", (P, dt, 1, 16, u + 1, P, None)), ("rc_channel_sums", (P, dt, 1, 0, u, P, None)),
              ("rc_channel_sums", (P, dt, 1, 16, 0, P, None)), ("rc_channel_sums", (P, dt, 1, 16, 257 * u, P, None)), ("rc_channel_sums", (P, dt, 70000, 16, u, P, None)),
              ("rc_ca_gate_ahead", (P, 1, 4, 8, 2, P, dt, 0, 4, P, P, P, P, P, P, P, P, None)), ("rc_ca_gate_ahead", (P, 1, 4, 2000, 2, P, dt, 4, 4, P, P, P, P, P, P, P, P, None)),
              ("rc_ca_gate_ahead", (P, 1, 0, 8, 2, P, dt, 4, 4, P, P, P, P, P, P, P, P, None)), ("rc_ca_gate_ahead", (P, 1, 4, 8, 2, P, dt, 4, 4, P, P, P, P, P, P, None, P, None)),
              ("rc_color_block", (P, dt, P, 1, 0, 8, 4, 4, P, P, None, None, None, None, None)), ("rc_color_block", (P, dt, P, 1, 600, 8, 4, 4, P, P, None, None, None, None, None)),
              ("rc_color_block", (P, dt, P, 1, 8, 8, 4, 4, P, P, P, None, P, P, None)), ("rc_color_block", (P, dt, P, 1, 8, 8, 0, 4, P, P, None, None, None, None, None)),
              ("rc_bayer_unshuffle", (P, dt, Q, dt, 1, 4, 4, 4, 4, None)), ("rc_bayer_unshuffle", (P, dt, P, dt, 1, 4, 4, 3, 4, None)),
              ("rc_bayer_unshuffle", (P, dt, P, dt, 1, 0, 4, 4, 4, None)),
              ("rc_raw_ingest", (P, dt, Q, P, dt, 1, 4, 4, 4, 4, 2, 2, 0.0, 1.0, None)), ("rc_raw_ingest", (P, dt, P, P, dt, 1, 4, 4, 4, 4, 2, 2, 1.0, 1.0, None)),
              ("rc_raw_ingest", (P, dt, P, P, dt, 1, 4, 4, 4, 4, 0, 2, 0.0, 1.0, None)),
              ("rc_nchw_to_nhwc", (P, dt, P, dt, 1, 0, 4, 4, 4, 4, None)), ("rc_nchw_to_nhwc", (P, dt, P, dt, 1, 8, 4, 4, 3, 4, None)),
              ("rc_nchw_to_nhwc", (P, dt, P, dt, 70000, 8, 4, 4, 4, 4, None)),
              ("rc_nhwc_to_nchw", (P, dt, P, dt, 1, 8, 4, 4, 5, 4, None)), ("rc_nhwc_to_nchw", (P, dt, P, dt, 1, 8, 4, 4, 0, 4, None)),
              ("rc_nhwc_to_nchw", (None, dt, P, dt, 1, 8, 4, 4, 4, 4, None))]
    for dt, u in ((f, 4), (h, 8)):
        t += [("rc_square", (Q, P, dt, 4 * u, None)), ("rc_square", (P, P, dt, u - 1, None)), ("rc_square", (P, P, dt, 0, None)),
              ("rc_gdn_apply", (P, Q, P, P, dt, 0, 4 * u, None)), ("rc_gdn_apply", (P, P, Q, P, dt, 1, 4 * u, None)), ("rc_gdn_apply", (P, P, P, P, dt, 0, u + 1, None)),
              ("rc_gdn_apply", (P, P, P, P, dt, 0, 0, None)),
              ("rc_channel_copy", (Q, 4 * u, 0, P, 4 * u, 0, u, 16, dt, None)), ("rc_channel_copy", (P, 4 * u, 0, Q, 4 * u, 0, u, 16, dt, None)),
              ("rc_channel_copy", (P, 4 * u, 1, P, 4 * u, 0, u, 16, dt, None)), ("rc_channel_copy", (P, 4 * u, 0, P, 4 * u, 0, u + 1, 16, dt, None)),
              ("rc_channel_copy", (P, 4 * u, 3 * u, P, 4 * u, 0, 2 * u, 16, dt, None)), ("rc_channel_copy", (P, 4 * u, 0, P, 4 * u, 3 * u, 2 * u, 16, dt, None)),
              ("rc_channel_copy", (P, 4 * u, 0, P, 4 * u, 0, 0, 16, dt, None)), ("rc_channel_copy", (P, 4 * u, 0, P, 4 * u, 0, u, 0, dt, None)),
              ("rc_channel_copy", (P, 4 * u, -u, P, 4 * u, 0, u, 16, dt, None))]
    for dt, u in ((f, 4), (h, 8), (RC_F16, 8)):         # a misaligned pointer in EVERY operand position of the kernels that read or write uint4
        for name, n_ptr, tail in (("rc_sigmoid_gate_add", 4, (dt, 4 * u, None)), ("rc_subsample2", 2, (dt, 1, 4, 4, u, None)), ("rc_upsample_bilinear2", 2, (dt, 1, 4, 4, u, None)),
                                  ("rc_sft_apply", 5, (dt, 4 * u, None)), ("rc_tail_ring_gather", 3, (dt, 1, 4, 4, u, None))) + \
                                 ((("rc_square", 2, (dt, 4 * u, None)), ("rc_gdn_apply", 4, (dt, 0, 4 * u, None))) if dt != RC_F16 else ()):
            for k in range(n_ptr):
                t.append((name, (*[Q if j == k else P for j in range(n_ptr)], *tail)))
    # dtypes an entry point has no kernels for
    t += [("rc_square", (P, P, RC_F16, 16, None)), ("rc_gdn_apply", (P, P, P, P, RC_F16, 0, 16, None)), ("rc_channel_copy", (P, 16, 0, P, 16, 0, 8, 16, RC_F16, None)),
          ("rc_gate_residual", (P, P, P, P, 2, 1, 4, 8, None)), ("rc_film_apply", (P, P, P, P, 7, 1, 4, 8, None)), ("rc_subsample2", (P, P, 2, 1, 4, 4, 8, None)),
          ("rc_dwt_forward", (P, P, P, 1, 2, 1, 4, 4, 8, None)), ("rc_channel_sums", (P, 2, 1, 16, 8, P, None)), ("rc_color_block", (P, 2, P, 1, 8, 8, 4, 4, P, P, None, None, None, None, None))]
    # fp32-only reductions
    t += [("rc_ca_gate", (P, 0, 4, 8, 2, 1.0, P, P, P, P, P, None)), ("rc_ca_gate", (P, 1, 0, 8, 2, 1.0, P, P, P, P, P, None)), ("rc_ca_gate", (P, 1, 4, 0, 2, 1.0, P, P, P, P, P, None)),
          ("rc_ca_gate", (P, 1, 4, 8, 0, 1.0, P, P, P, P, P, None)), ("rc_ca_gate", (P, 1, 4, 20000, 2, 1.0, P, P, P, P, P, None)), ("rc_ca_gate", (P, 70000, 4, 8, 2, 1.0, P, P, P, P, P, None)),
          ("rc_ca_gate", (P, 1, 4, 8, 2, 1.0, None, P, P, P, P, None)),
          ("rc_instance_stats", (P, P, P, 1, 0, 16, 1e-5, None)), ("rc_instance_stats", (P, P, P, 1, 4, 0, 1e-5, None)), ("rc_instance_stats", (P, None, P, 1, 4, 16, 1e-5, None)),
          ("rc_instance_norm", (P, P, P, P, P, P, 0, 4, 16, None)), ("rc_instance_norm", (P, P, P, P, P, P, 1, 4, 0, None)), ("rc_instance_norm", (P, P, P, P, None, P, 1, 4, 16, None)),
          ("rc_color_head", (P, P, 1, 0, 4, 16, P, P, None)), ("rc_color_head", (P, P, 1, 4, 4, 0, P, P, None)), ("rc_color_head", (P, P, 1, 4, 4, 16, None, P, None)),
          ("rc_gfm_vector", (P, 1, 0, 8, 8, P, P, P, P, P, None)), ("rc_gfm_vector", (P, 1, 8, 0, 8, P, P, P, P, P, None)), ("rc_gfm_vector", (P, 1, 8, 8, 0, P, P, P, P, P, None)),
          ("rc_gfm_vector", (P, 1, 9000, 9000, 8, P, P, P, P, P, None)), ("rc_gfm_vector", (P, 1, 8, 8, 8, P, P, P, P, None, None))]
    return t


def test_bad_arguments_of_the_streaming_entry_points_are_refused_before_any_launch():
    lib = _lib.load()
    calls = _bad_calls()
    assert len({n for n, _ in calls}) >= 28
    for name, args in calls:
        lib.rc_bayer_unshuffle(None, 0, None, 0, 1, 4, 4, 4, 4, None)       # leaves another entry point's message behind
        code = getattr(lib, name)(*args)
        msg = lib.rc_last_error().decode()
        assert code == -1 and name in msg, (name, args, code, msg)          # RC_ERR_INVALID from the entry point's own check, not a failed launch (RC_ERR_HIP)


def test_bad_arguments_of_channel_concat():
    import ctypes as C
    lib = _lib.load()

    def call(ptrs, widths, n, dst, pixels, dt):
        pa = (C.c_void_p * 8)(*ptrs, *[None] * (8 - len(ptrs)))
        wa = (C.c_int * 8)(*widths, *[0] * (8 - len(widths)))
        return lib.rc_channel_concat(pa, wa, n, dst, pixels, dt, None)
    for args in (([P, Q], [8, 8], 2, P, 16, RC_BF16), ([P, P], [8, 12], 2, P, 16, RC_BF16), ([P, P], [8, 0], 2, P, 16, RC_BF16), ([P, P], [4, 4], 2, Q, 16, RC_F32),
                 ([P], [8], 0, P, 16, RC_BF16), ([P] * 8, [8] * 8, 9, P, 16, RC_BF16), ([P], [8], 1, P, 0, RC_BF16), ([P, None], [8, 8], 2, P, 16, RC_BF16),
                 ([P], [8], 1, P, 16, RC_F16)):
        assert call(*args) == -1 and b"rc_channel_concat" in lib.rc_last_error(), args


# ---- the coverage table of the GPU file --------------------------------------------------------------------------------------------------------------------
def test_every_streaming_entry_point_is_in_the_gpu_files_coverage_table():
    """The rc_ functions that pointwise.hip and cond.hip define, as far as the public header declares them, each have a row in the docstring of
    test_streaming_gpu.py, and the test that row names exists."""
    header = open(os.path.join(ROOT, "include", "realcam_hip.h")).read()
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    defined = set()
    for tu in ("pointwise.hip", "cond.hip"):
        src = open(os.path.join(ROOT, "realcamnet_amd", "csrc", tu)).read()
        defined |= set(re.findall(r"^(?:int|size_t) (rc_[a-z0-9_]+)\(", src, flags=re.M))
    assert len(defined) == 31 and defined <= declared, sorted(defined - declared)
    gpu = open(os.path.join(ROOT, "tests", "test_streaming_gpu.py")).read()
    doc = gpu.split('"""')[1]
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", gpu, flags=re.M))
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(rc_[a-z0-9_]+)\s+\S+\s+(test_[a-z0-9_]+)", doc, flags=re.M)}
    assert set(rows) == defined, (sorted(defined - set(rows)), sorted(set(rows) - defined))
    assert all(t in tests for t in rows.values()), sorted(t for t in rows.values() if t not in tests)
    called = set(re.findall(r"\b(rc_[a-z0-9_]+)\b", gpu.split('"""', 2)[2])) | {"rc_" + n for n in re.findall(r"\b(?:_R|ops)\.([a-z0-9_]+)\(", gpu)}
    alias = {"rc_haar_dwt": "rc_dwt_forward", "rc_haar_idwt": "rc_dwt_inverse", "rc_channel_slice": "rc_channel_copy"}
    called = {alias.get(n, n) for n in called}
    assert defined - {"rc_channel_sums_slots", "rc_ca_gate_ahead_scratch_floats"} <= called, sorted(defined - called)


def test_ops_wrappers_refuse_what_is_not_a_4d_map():
    """Needs no GPU: a CPU tensor is refused by _req first, so the rank check is reached through a meta-free path -- the wrappers are called with the device check patched out."""
    from realcamnet_amd import ops
    real = ops._req
    ops._req = lambda t, name: t
    try:
        class Conv:
            weight = torch.zeros(3, 8, 1, 1)
        for fn, bad in ((ops.subsample2, torch.zeros(4, 4, 8)), (ops.upsample_bilinear2, torch.zeros(2, 4, 4, 4, 8)), (ops.space_to_depth2, torch.zeros(16)),
                        (ops.channel_sums, torch.zeros(4, 4, 8)), (ops.instance_stats, torch.zeros(2, 8, 16)), (ops.instance_stats, torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)),
                        (lambda x: ops.color_head(x, Conv), torch.zeros(2, 8, 16)), (lambda x: ops.color_head(x, Conv), torch.zeros(2, 4, 4, 4))):
            with pytest.raises(ValueError):
                fn(bad)
    finally:
        ops._req = real


def test_taps_uniform_verdict_cannot_be_inherited_by_a_later_tensor():
    """torch_ops._taps_uniform caches its verdict per (address, version).  A freed taps tensor's address goes to the next allocation of that size, which then inherited
    the verdict (random per-channel taps ran through the UNIFORM kernel).  The cache entry must keep the judged tensor alive, so no later tensor can sit there."""
    from realcamnet_amd import torch_ops
    torch_ops._UNIFORM.clear()
    haar = R.haar_taps(8).clone()
    ptr = haar.data_ptr()
    assert torch_ops._taps_uniform(haar) == 1
    del haar
    later = [R.random_taps(8, k).clone() for k in range(64)]
    assert all(t.data_ptr() != ptr for t in later)
    assert all(torch_ops._taps_uniform(t) == 0 for t in later)
    t = R.haar_taps(8).clone()
    assert torch_ops._taps_uniform(t) == 1
    t[5, 0, 1, 1] = 3.0                                                    # an in-place edit bumps the version: judged again
    assert torch_ops._taps_uniform(t) == 0
