"""No GPU: the yardsticks of tests/codec_ref.py against the oracle (oracle/tcm_oracle.py, oracle/entropy_oracle.py) and against each other; the CPU side of the
sharpness condition; argument checks of every codec entry point; the coverage table of test_codec_gpu.py against the header."""
import os
import re

import pytest
import torch

import codec_ref as C
import entropy_oracle as E
import tcm_oracle as TO
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CPU_CAP = 0.001


def inside(val, ref, slack, dtype):
    return bool(C.within_rounding(val, ref, slack, dtype).all())


def cpu_share(pipe, what):
    """pipe(model, dtype) -> (value, bound): round_to(model64) lies inside the window, and the CPU fp32 restatement of the same inputs differs from it in <= 0.1 % of the
    bf16 values."""
    ref, slack = pipe(False, F64)
    model = pipe(True, F64)[0]
    assert bool(torch.isfinite(slack).all()), what
    assert inside(C.round_to(model, BF16), ref, slack, BF16), what
    share, diff, adjacent = C.flip_share(pipe(True, F32)[0].to(BF16), model)
    print(f"[cpu flip share] {what}: {100 * share:.4f} %")
    assert share <= CPU_CAP, (what, share)


# ---- window attention ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [8, 4])
def test_attention_reference_is_the_oracles_wmsa(ws):
    """wmsa64 on qkv = embedding(x) equals oracle/tcm_oracle.wmsa (models/tcm.py:179-206) with an identity output layer, W and SW, in float64: to 1e-12 of the largest value."""
    shapes = C.WS8_SHAPES if ws == 8 else C.WS4_SHAPES
    for si, (b, H, W) in enumerate(shapes):
        for hd, nh in ((8, 3), (16, 1), (32, 3)):
            c = hd * nh
            g = torch.Generator().manual_seed(100 * ws + si + hd)
            sd = {"m.embedding_layer.weight": torch.randn(3 * c, c, generator=g, dtype=F64) / c ** 0.5, "m.embedding_layer.bias": torch.randn(3 * c, generator=g, dtype=F64),
                  "m.relative_position_params": 0.4 * torch.randn(nh, 2 * ws - 1, 2 * ws - 1, generator=g, dtype=F64),
                  "m.linear.weight": torch.eye(c, dtype=F64), "m.linear.bias": torch.zeros(c, dtype=F64)}
            x = torch.randn(b, H, W, c, generator=g, dtype=F64)
            qkv = torch.nn.functional.linear(x, sd["m.embedding_layer.weight"], sd["m.embedding_layer.bias"])
            for typ, shift in (("W", 0), ("SW", ws // 2)):
                want = TO.wmsa(sd, "m", x, hd, ws, typ)
                got, slack = C.wmsa64(qkv, sd["m.relative_position_params"], hd, ws, shift, False)
                assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (ws, (b, H, W), hd, nh, typ)
                assert bool(torch.isfinite(slack).all()) and bool((slack > 0).all())


@pytest.mark.parametrize("ws", [8, 4])
def test_exact_attention_expectations_are_what_the_float64_reference_rounds_to(ws):
    """uniform_expected (a pooling) and one_hot_expected (index arithmetic) equal the float64 attention of the same inputs, in float64 and hence after rounding to
    either storage dtype; the integer codes make every mean a bf16 value; the cases cover all seven one-hot positions."""
    shapes = C.WS8_SHAPES if ws == 8 else C.WS4_SHAPES
    si, hits = 0, {}
    for (b, H, W) in shapes:
        for hd, nh in C.HEADS:
            for shift in (0, ws // 2):
                c = hd * nh
                qkv = C.exact_qkv(b, H, W, c, ws, 7000 + si, F32)
                v = qkv[..., 2 * c:]
                assert torch.equal(v.to(BF16).float(), v)
                uni = C.uniform_expected(v, ws, shift)
                assert torch.equal(C.wmsa64(qkv, torch.zeros(nh, 2 * ws - 1, 2 * ws - 1), hd, ws, shift, False)[0], uni), (ws, (b, H, W), hd, nh, shift)
                assert torch.equal(C.round_to(uni, BF16).double(), uni)
                rel, pos = C.one_hot_tables(nh, ws, si)
                one = C.one_hot_expected(v, ws, shift, pos, hd)
                for mfma in (False, True):
                    assert torch.equal(C.wmsa64(qkv, rel, hd, ws, shift, mfma, model=True)[0], one), (ws, (b, H, W), hd, nh, shift, pos)
                for h, p in enumerate(pos):                                  # (a corner's only query / key pair can lie across the wrap of a one-window map: then nothing differs)
                    hits[p] = hits.get(p, 0) + int((one[..., h * hd:(h + 1) * hd] != uni[..., h * hd:(h + 1) * hd]).any())
                si += 1
    assert len(hits) == len(C.ONE_HOT) and all(n >= 4 for n in hits.values()), hits


@pytest.mark.parametrize("ws", [8, 4])
def test_exact_attention_values_tell_every_channel_apart(ws):
    """v_codes encodes (image, pixel, channel): no two channels of a map carry the same expectation, so exchanging two channels -- inside a head or across heads --
    changes uniform_expected and one_hot_expected; and no two images or neighbouring pixels do."""
    shapes = [(3, 24, 40, 96, 32), (3, 24, 40, 24, 8), (1, 64, 64, 64, 8)] if ws == 8 else [(3, 12, 28, 96, 32), (3, 12, 28, 24, 8)]
    for (b, H, W, c, hd) in shapes:
        v = C.v_codes(b, H, W, c, ws)
        for shift in (0, ws // 2):
            rel, pos = C.one_hot_tables(c // hd, ws, 3)
            for name, exp in (("uniform", C.uniform_expected(v, ws, shift)), ("one-hot", C.one_hot_expected(v, ws, shift, pos, hd))):
                cols = exp.reshape(-1, c).t()
                same = (cols[:, None, :] == cols[None, :, :]).all(-1)
                assert int(same.sum()) == c, (ws, name, (b, H, W, c), shift, same.nonzero()[:4].tolist())
                for i, j in ((0, 1), (2, 7), (hd - 1, 0)):                    # the permutation itself, inside head 0
                    perm = list(range(c)); perm[i], perm[j] = perm[j], perm[i]
                    assert not torch.equal(exp[..., perm], exp), (ws, name, i, j)
                if b > 1:
                    assert not torch.equal(exp[0], exp[1])
                assert not torch.equal(exp[:, ws:], exp[:, :-ws]) and not torch.equal(exp[:, :, ws:], exp[:, :, :-ws])


def test_big_attention_maps_follow_the_launchers_rule():
    for cus in (256, 304, 64):
        maps = C.wmsa_big_maps(cus)
        assert [C.wmsa_per_wave(b * (H // 8) * (W // 8), 8, cus) for (b, H, W) in maps] == [4, 8]
        assert all(C.wmsa_per_wave(b * (H // 8) * (W // 8), n, cus) == 2 for (b, H, W) in C.WS8_SHAPES for n in (1, 3))
    assert C.wmsa_big_maps(256) == [(2, 256, 256), (1, 512, 512)]


@pytest.mark.parametrize("ws", [8, 4])
def test_attention_models_are_inside_their_windows_and_sharp_on_the_cpu(ws):
    b, H, W = (C.WS8_SHAPES if ws == 8 else C.WS4_SHAPES)[-1]
    si = (len(C.WS8_SHAPES if ws == 8 else C.WS4_SHAPES) - 1) * len(C.HEADS) * 2
    for hd, nh in C.HEADS:
        for shift in (0, ws // 2):
            qkv, rel = C.wmsa_sharp_inputs(b, H, W, hd * nh, nh, ws, 7200 + si)
            signed = C.wmsa_real_inputs(b, H, W, hd * nh, nh, ws, 7200 + si, BF16)[0]
            for mfma in ((True, False) if ws == 8 else (False,)):
                assert inside(C.round_to(C.wmsa64(signed, rel, hd, ws, shift, mfma, model=True)[0], BF16), *C.wmsa64(signed, rel, hd, ws, shift, mfma), BF16)
                cpu_share(lambda model, dtype: C.wmsa64(qkv, rel, hd, ws, shift, mfma, model, dtype), f"window_attention ws{ws} hd{hd} heads{nh} shift{shift} mfma={mfma}")
            si += 1


# ---- token chains -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_chain_models_are_inside_their_windows_and_sharp_on_the_cpu():
    for c in (32, 64):
        x, g, b, eps, w1, b1, w2, b2 = C.sharp_inputs_ln_mlp(c)
        cpu_share(lambda model, dtype: C.ln_mlp64(x, g, b, eps, w1, b1, w2, b2, model, dtype), f"ln_mlp c{c}")
        for cout in (32, 96, 192, 512):
            x, g, b, eps, w, bias = C.sharp_inputs_ln_linear(c, cout)
            cpu_share(lambda model, dtype: C.ln_linear64(x, g, b, eps, w, bias, model, dtype), f"ln_linear c{c} cout{cout}")
    for c in (64, 128):
        x, idn, gam, beta = C.sharp_inputs_gdn(c)
        for inverse in (False, True):
            for ii in (idn, None):
                cpu_share(lambda model, dtype: C.gdn64(x, ii, gam, beta, inverse, model, dtype), f"gdn_chain c{c} inverse={inverse} identity={ii is not None}")
        a, a2, bb, res, w, bias = C.sharp_inputs_cat_linear(c)
        for aa, rr, bi in ((a2, res, bias), (None, res, bias), (a2, None, bias), (a2, res, None), (None, None, None)):
            cpu_share(lambda model, dtype: C.cat_linear64(a, aa, bb, rr, w, bi, model, dtype), f"cat_linear c{c} a_add={aa is not None} residual={rr is not None} bias={bi is not None}")


def test_ln_linear_values_off_by_two_ulps_are_cancelling_ones_and_few():
    """The CPU fp32 restatement of rc_ln_linear's sharpness inputs: a value that is not adjacent to the model's lies where ONE flipped LayerNorm output exceeds the
    element's own ulp (codec_ref.cancelling), within ln_linear_one_flip plus one ulp, at most ceil(NON_ADJACENT_SHARE x elements) times, and never at c = 64: what
    test_codec_gpu.assert_sharp allows the kernel at c = 32 and nowhere else."""
    import math
    for c in (32, 64):
        for cout in (32, 96, 192, 512):
            x, g, b, eps, w, bias = C.sharp_inputs_ln_linear(c, cout)
            ref, slack = C.ln_linear64(x, g, b, eps, w, bias)
            model = C.ln_linear64(x, g, b, eps, w, bias, model=True)[0]
            cpu = C.ln_linear64(x, g, b, eps, w, bias, model=True, dtype=F32)[0].to(BF16)
            share, diff, adjacent = C.flip_share(cpu, model)
            far = diff & ~adjacent & (ref.abs() > slack)
            one = C.ln_linear_one_flip(x, g, b, eps, w)
            print(f"[cpu non-adjacent] ln_linear c{c} cout{cout}: {int(far.sum())} of {far.numel()}; cancelling elements {int(C.cancelling(model, one).sum())}")
            if c == 64:
                assert not bool(far.any())
                continue
            assert bool(C.cancelling(model, one)[far].all())
            assert bool(((cpu.double() - C.round_to(model, BF16).double()).abs() <= one + 2 * C.half_ulp_bf16(model.abs()))[far].all())
            assert int(far.sum()) <= math.ceil(C.NON_ADJACENT_SHARE * far.numel())


def test_chain_references_agree_with_torch_and_the_oracle():
    """Without rounding points the pipelines ARE the layers' definitions in float64: LayerNorm + Linear (+ GELU + Linear + x), the oracle's GDN, Linear over a concatenation."""
    Fn = torch.nn.functional
    x, g, b, eps, w1, b1, w2, b2 = C.sharp_inputs_ln_mlp(64)
    d = lambda t: t.double()
    n = Fn.layer_norm(d(x), (64,), d(g), d(b), eps)
    want = d(x) + Fn.linear(Fn.gelu(Fn.linear(n, d(w1), d(b1))), d(w2), d(b2))
    # e_weight carries bf16-valued weights unrounded, so the only difference is float64 rounding
    assert (C.ln_mlp64(x, g, b, eps, w1, b1, w2, b2)[0] - want).abs().max().item() <= 1e-12
    x, g, b, eps, w, bias = C.sharp_inputs_ln_linear(32, 96)
    assert (C.ln_linear64(x, g, b, eps, w, bias)[0] - Fn.linear(Fn.layer_norm(d(x), (32,), d(g), d(b), eps), d(w), d(bias))).abs().max().item() <= 1e-12
    for c in (64, 128):
        x, idn, gam, beta = C.sharp_inputs_gdn(c)
        zero = torch.zeros(1, dtype=F64)
        sd = {"g.beta": d(beta).sqrt(), "g.beta_reparam.lower_bound.bound": zero, "g.beta_reparam.pedestal": zero,
              "g.gamma": d(gam).sqrt(), "g.gamma_reparam.lower_bound.bound": zero, "g.gamma_reparam.pedestal": zero}
        for inverse in (False, True):
            want = TO.gdn(sd, "g", d(x).t().reshape(1, c, -1, 1), inverse).reshape(c, -1).t()
            got = C.gdn64(x, idn, gam, beta, inverse)[0] - d(idn)
            assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (c, inverse)
        a, a2, bb, res, w, bias = C.sharp_inputs_cat_linear(c)
        want = Fn.linear(torch.cat([d(a) + d(a2), d(bb)], -1), d(w), d(bias)) + d(res)
        assert (C.cat_linear64(a, a2, bb, res, w, bias)[0] - want).abs().max().item() <= 1e-12
    for c in (64, 128):
        for inverse in (False, True):
            xi, ii, gi, bi, y = C.gdn_int_case(c, 65, 7600 + c + 65, inverse)
            assert torch.equal(C.gdn64(xi, ii, gi, bi, inverse, model=True)[0], (y + ii.double()).to(BF16).double()), (c, inverse)
            assert torch.equal((y + ii.double()).to(BF16).double(), y + ii.double())


# ---- likelihood and symbol kernels ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CHANNELS)
def test_entropy_references_agree_with_the_oracle(c):
    """ref64_entropy_bottleneck on the packed fp32 parameters against oracle/tcm_oracle.entropy_bottleneck on the state_dict (fp32, as the oracle runs): to the oracle's
    own error, 2e-6 of a likelihood <= 1 (some thirty fp32 operations on values of order 1; found: 1.2e-7); the quantised output against the oracle's, exactly."""
    sd = C.eb_random_sd(c, 7800 + c)
    P, med = C.eb_pack(sd, "eb"), sd["eb.quantiles"][:, 0, 1].contiguous()
    g = torch.Generator().manual_seed(c)
    z = med[None, :] + torch.randint(-28, 29, (131, c), generator=g).float() / 4
    out, lik = TO.entropy_bottleneck(sd, "eb", z.t().reshape(1, c, 131, 1), bound=0.0)
    l64, unit = C.ref64_entropy_bottleneck(z, P, med)
    err = (l64 - lik.reshape(c, 131).t().double()).abs().max().item()
    print(f"[entropy_bottleneck C{c}] max |ref64 - oracle| {err:.3e}")
    assert err <= 2e-6 and bool((unit > 0).all())
    assert torch.equal(C.restate32_ste(z, med[None, :].expand_as(z)), out.reshape(c, 131).t())


def test_gaussian_reference_and_symbols_agree_with_the_oracle():
    for dtype in (F32, BF16):
        y, mu = C.tie_values(dtype, 7900, 4096)
        sc = C.scale_cases(E.get_scale_table(), dtype)
        scale = sc[torch.arange(4096) % sc.numel()]
        out, lik = TO.gaussian_conditional(y.double(), scale.double(), mu.double(), bound=0.0)
        l64, unit = C.ref64_gaussian_conditional(y.float(), scale.float(), mu.float())
        assert (l64 - lik).abs().max().item() <= 1e-8                    # the oracle clamps at the double 0.11, the kernel at the float
        assert torch.equal(C.restate32_ste(y, mu).double(), out.to(dtype).double())
        sym, hat = C.restate32_symbols(y, mu)
        assert torch.equal(sym, E.quantize_symbols(y, mu)) and torch.equal(hat, C.round_to(sym.double() + mu.double(), dtype))
        t = (y.float() - mu.float())
        ties = (t - t.floor()) == 0.5
        assert int(ties.sum()) > 40 and bool((sym[ties] % 2 == 0).all())                       # round half to even
        assert bool((t.abs() >= 2.0 ** 23).any()) and bool((t == 0).any()) and bool(((t.abs() < 0.5) & (t != 0)).any())
    table = E.get_scale_table()
    for dtype in (F32, BF16):
        lv = C.neighbours(table, dtype).float()
        assert bool((lv[0] < lv[1]).all()) and bool((lv[1] < lv[2]).all())
        if dtype == F32:
            assert torch.equal(lv[1], table)
            idx = E.gc_build_indexes(lv, table)
            # a scale equal to a level belongs to that level; the next value above it to the next level
            assert torch.equal(idx[1], torch.arange(64, dtype=torch.int32)) and torch.equal(idx[2][:-1], torch.arange(1, 64, dtype=torch.int32))
    assert int(E.gc_build_indexes(torch.tensor([0.05, 0.0, -1.0, 0.11]), table).abs().sum()) == 0


def test_big_tables_are_well_formed():
    t = E.gc_update(E.get_scale_table())
    for rows, entries in ((40, 1000), (961, 8)):
        bt = C.big_tables(t, rows, entries)
        cdf, sizes = bt["_quantized_cdf"], bt["_cdf_length"]
        assert cdf.shape[0] == 64 + rows and int(sizes.max()) <= cdf.shape[1]
        for r in (0, 63, 64, 64 + rows - 1):
            row = cdf[r, :int(sizes[r])]
            assert row[0] == 0 and row[-1] == 65536 and bool((row[1:] > row[:-1]).all())
    assert int(C.big_tables(t, 40, 1000)["_cdf_length"].sum()) > 32 * 1024 >= int(t["_cdf_length"].sum())


# ---- argument checks (no GPU: every call must be refused before a launch) ---------------------------------------------------------------------------------------------
P_, Q_ = 4096, 4100          # dummy device pointers: 16-byte aligned / not


def _bad_calls():
    f, h, x16 = RC_F32, RC_BF16, RC_F16
    A, B = P_, Q_
    t = []
    mk = lambda name, tag, **base: (lambda **k: (name, tag, tuple({**base, **k}.values())))
    wa = mk("rc_window_attention", "rc_window_attention", q=A, rel=A, out=A, dt=h, b=1, H=8, W=8, C=64, hd=8, ws=8, sh=0, st=None)
    t += [wa(q=None), wa(rel=None), wa(out=None), wa(dt=x16), wa(ws=6), wa(hd=12), wa(b=0), wa(H=12), wa(W=4), wa(C=60), wa(C=4), wa(sh=2), wa(ws=4, sh=4), wa(sh=-4)]
    wp = mk("rc_window_attention_planar8", "rc_window_attention", q=A, rel=A, out=A, dt=h, b=1, H=8, W=8, C=64, hd=8, ws=8, sh=0, st=None)
    t += [wp(q=None), wp(dt=f), wp(ws=4, H=4, W=4), wp(H=12), wp(hd=12), wp(b=4, H=4096, W=4096)]
    lm = mk("rc_ln_mlp", "rc_ln_mlp", x=A, out=A, tok=4, c=64, w1=A, b1=None, w2=A, b2=None, g=A, bt=A, eps=1e-5, st=None)
    t += [lm(x=None), lm(out=None), lm(w1=None), lm(w2=None), lm(g=None), lm(bt=None), lm(tok=0), lm(c=48), lm(c=128), lm(x=B), lm(out=B)]
    ll = mk("rc_ln_linear", "rc_ln_linear", x=A, out=A, tok=4, c=64, co=192, w=A, b=None, g=A, bt=A, eps=1e-5, st=None)
    t += [ll(x=None), ll(w=None), ll(g=None), ll(tok=0), ll(c=16), ll(co=0), ll(co=48), ll(co=544), ll(x=B), ll(out=B)]
    lp = mk("rc_ln_linear_planar8", "rc_ln_linear", x=A, out=A, tok=4, c=64, co=192, w=A, b=None, g=A, bt=A, eps=1e-5, st=None)
    t += [lp(x=None), lp(tok=0), lp(c=80), lp(co=40), lp(out=B)]
    gd = mk("rc_gdn_chain", "rc_gdn_chain", x=A, idn=None, out=A, tok=4, c=64, w=A, b=A, inv=0, st=None)
    t += [gd(x=None), gd(out=None), gd(w=None), gd(tok=0), gd(c=32), gd(c=192), gd(x=B), gd(out=B), gd(idn=B)]
    cl = mk("rc_cat_linear", "rc_cat_linear", a=A, a2=None, b=A, res=None, out=A, tok=4, c=64, w=A, bias=None, st=None)
    t += [cl(a=None), cl(b=None), cl(out=None), cl(w=None), cl(tok=0), cl(c=32), cl(c=96), cl(a=B), cl(a2=B), cl(b=B), cl(res=B), cl(out=B)]
    eb = mk("rc_entropy_bottleneck", "rc_entropy_bottleneck", z=A, p=A, m=A, zh=A, lik=A, dt=f, n=4, c=3, bound=1e-9, st=None)
    t += [eb(z=None), eb(p=None), eb(m=None), eb(zh=None), eb(lik=None), eb(dt=x16), eb(n=0), eb(c=0)]
    gc = mk("rc_gaussian_conditional", "rc_gaussian_conditional", y=A, s=A, m=A, yh=A, lik=A, dt=f, n=4, sb=0.11, bound=1e-9, st=None)
    t += [gc(y=None), gc(s=None), gc(m=None), gc(yh=None), gc(lik=None), gc(dt=x16), gc(n=0), gc(sb=0.0), gc(sb=-1.0)]
    th = mk("rc_tanh_half_add", "rc_tanh_half_add", a=A, l=A, out=A, dt=f, n=4, st=None)
    t += [th(a=None), th(l=None), th(out=None), th(dt=x16), th(n=0)]
    gs = mk("rc_gc_symbols", "rc_gc_symbols", y=A, mu=A, s=A, dt=f, b=1, hw=4, c=3, tb=A, nl=64, sb=0.11, sym=A, idx=A, yh=A, st=None)
    t += [gs(s=None), gs(tb=None), gs(idx=None), gs(nl=0), gs(dt=x16), gs(b=0), gs(hw=0), gs(c=0), gs(mu=None), gs(sym=None), gs(yh=None)]
    gq = mk("rc_gc_dequantize", "rc_gc_dequantize", sym=A, mu=A, dt=f, b=1, hw=4, c=3, yh=A, st=None)
    t += [gq(sym=None), gq(mu=None), gq(yh=None), gq(dt=x16), gq(b=0), gq(hw=0), gq(c=0)]
    es = mk("rc_eb_symbols", "rc_eb_symbols", z=A, m=A, dt=f, b=1, hw=4, c=3, enc=1, sym=A, idx=A, zh=A, st=None)
    t += [es(z=None), es(m=None), es(sym=None), es(idx=None), es(zh=None), es(dt=x16), es(b=0), es(hw=0), es(c=0)]
    dc = mk("rc_rans_decode_chunks", "rc_rans_decode_chunks", s=A, nb=64, off=A, idx=A, n=4, ch=2048, cdf=A, stride=8, nc=64, sz=A, co=A, sym=A, err=A, st=None)
    t += [dc(s=None), dc(off=None), dc(idx=None), dc(cdf=None), dc(sz=None), dc(co=None), dc(sym=None), dc(err=None), dc(n=0), dc(ch=0), dc(nb=4), dc(nb=1 << 31), dc(stride=1),
          dc(nc=0)]
    return t


def test_bad_arguments_of_the_codec_entry_points_are_refused_before_any_launch():
    lib = _lib.load()
    calls = _bad_calls()
    assert len({n for n, _, _ in calls}) == 14
    for name, tag, args in calls:
        lib.rc_bayer_unshuffle(None, 0, None, 0, 1, 4, 4, 4, 4, None)       # leaves another entry point's message behind
        code = getattr(lib, name)(*args)
        msg = lib.rc_last_error().decode()
        want = -3 if (name == "rc_window_attention_planar8" and "segment-planar" in msg) else -1
        assert code == want and tag in msg, (name, args, code, msg)         # from the entry point's own check, not a failed launch
    ok = lib.rc_window_attention_planar8_ok
    assert ok(RC_BF16, 1, 8, 8, 64, 8) == 1 and ok(RC_F32, 1, 8, 8, 64, 8) == 0 and ok(RC_BF16, 1, 8, 8, 64, 4) == 0 and ok(RC_BF16, 0, 8, 8, 64, 8) == 0
    assert ok(RC_BF16, 1, 12, 8, 64, 8) == 0 and ok(RC_BF16, 1, 8, 4, 64, 8) == 0 and ok(RC_BF16, 4, 4096, 4096, 64, 8) == 0
    assert lib.rc_debug_set(b"wmsa_mfma", 0) == 0
    try:                                                                    # the pair stays consistent: no planar form while the matrix-core kernel is switched off
        assert ok(RC_BF16, 1, 8, 8, 64, 8) == 0
        assert lib.rc_window_attention_planar8(P_, P_, P_, RC_BF16, 1, 8, 8, 64, 8, 8, 0, None) == -3
    finally:
        assert lib.rc_debug_set(b"wmsa_mfma", 1) == 0
    assert ok(RC_BF16, 1, 8, 8, 64, 8) == 1 and lib.rc_debug_set(b"wmsa_mfmb", 1) == -1


# ---- the coverage table of the GPU file -----------------------------------------------------------------------------------------------------------------------------
CODEC_ENTRY_POINTS = {"rc_window_attention", "rc_window_attention_planar8", "rc_window_attention_planar8_ok", "rc_ln_mlp", "rc_ln_linear", "rc_ln_linear_planar8", "rc_gdn_chain",
                      "rc_cat_linear", "rc_entropy_bottleneck", "rc_gaussian_conditional", "rc_tanh_half_add", "rc_gc_symbols", "rc_gc_dequantize", "rc_eb_symbols",
                      "rc_rans_decode_chunks"}


def test_every_codec_entry_point_is_in_the_gpu_files_coverage_table():
    """Every entry point of the group is declared in the header, has a row in the docstring of test_codec_gpu.py, the test that row names exists, and that test's body
    reaches the entry point: by its raw op, by the library handle, or (the chunk decoder) through bitstream.Decoder."""
    header = open(os.path.join(ROOT, "include", "realcam_hip.h")).read()
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert CODEC_ENTRY_POINTS <= declared, sorted(CODEC_ENTRY_POINTS - declared)
    gpu = open(os.path.join(ROOT, "tests", "test_codec_gpu.py")).read()
    doc = gpu.split('"""')[1]
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", gpu, flags=re.M))
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(rc_[a-z0-9_]+)\s+\S+\s+(test_[a-z0-9_]+)", doc, flags=re.M)}
    assert set(rows) == CODEC_ENTRY_POINTS, (sorted(CODEC_ENTRY_POINTS - set(rows)), sorted(set(rows) - CODEC_ENTRY_POINTS))
    assert all(t in tests for t in rows.values()), sorted(t for t in rows.values() if t not in tests)
    body = gpu.split('"""', 2)[2]
    called = set(re.findall(r"\bhip\.(rc_[a-z0-9_]+)\(", body)) | {"rc_" + n for n in re.findall(r"\b_R\.([a-z0-9_]+)\b", body)}
    if "bitstream.Decoder(" in body:
        called.add("rc_rans_decode_chunks")
    assert CODEC_ENTRY_POINTS <= called, sorted(CODEC_ENTRY_POINTS - called)
