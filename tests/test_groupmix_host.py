"""No GPU: the yardsticks of tests/groupmix_ref.py against each other, against torch's functionals and against the oracle; the CPU side of the sharpness
condition; argument checks of every GroupMix entry point; the coverage table of test_groupmix_gpu.py against the header."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import groupmix_oracle as GO
import groupmix_ref as G
from conftest import golden_names, load_golden
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16


def inside(val, ref, slack, dtype):
    return bool(G.within_rounding(val, ref, slack, dtype).all())


# ---- the models compose into the block upstream defines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", [f for f in golden_names("gma_block_") if "_80_" in f])
def test_models_composed_into_a_block_agree_with_the_oracle(fixture):
    """block64 chains dwconv2d -> qkv_aggregate -> crpe -> kv_mfma -> tail.  Without rounding points it IS upstream's block in float64: it must agree with the fp32
    oracle to the oracle's own error (2e-5 of the largest value, the bar test_gma.py holds the oracle to against the reference; found: 1.6e-7).

    With every kernel's rounding points the block is held to a bf16-rounding distance from the oracle, two ways:
      * max |model - oracle| <= BLOCK_ROUNDING_POINTS * 2^-9 * max |y| = 6 bf16 ulps of the largest value.  Derivation: 12 rounding points stand in series between
        the block's input and its output (groupmix_ref.BLOCK_ROUNDING_POINTS names them), each moves its own value by at most 2^-9 |v|, and each such error reaches
        the output at nominal gain 1: every stage behind it is a LayerNorm-normalised or residual stage with nn.Linear-scale weights, whose outputs are of the size
        of its inputs, so one rounding point contributes at most 2^-9 max |y| and the
        twelve add.  (The weights' own bf16 packing is no term: the fixtures' weights are bf16 values.)
      * PSNR(model, oracle) >= 60 dB re max |y|: the floor test_gma.py::test_gma_block_vs_reference_golden holds the bf16 kernels to on the same fixtures -- a model of
        those kernels that missed it would not describe them.
    Both figures are printed before they are asserted.  The worst-case bound composed from every stage's slack64 (groupmix_ref.block64) is kept as a sanity check
    only: two LayerNorms, a softmax and four dense layers carried by |W| stand behind the first rounding point, and it comes out near 900 on values up to 6.4."""
    g = load_golden(fixture)
    hw = tuple(int(v) for v in g["hw"])
    with torch.no_grad():
        want = GO.gma_block(g["sd"], g["x"], hw, 8).double()
    exact, bound = G.block64(g["sd"], g["x"], hw, False)
    assert (exact.reshape(want.shape) - want).abs().max().item() <= 2e-5 * want.abs().max().item()
    model, _ = G.block64(g["sd"], g["x"], hw, True)
    ymax = want.abs().max().item()
    d = (model.reshape(want.shape) - want).abs()
    psnr = 10 * math.log10(ymax ** 2 / (d * d).mean().item())
    print(f"[block] {fixture}: max |model - oracle| {d.max().item():.4f} = {d.max().item() / (2.0 ** -8 * ymax):.2f} bf16 ulps of max |y| = {ymax:.3f}, median {d.median().item():.5f}, PSNR {psnr:.1f} dB")
    assert d.max().item() <= G.BLOCK_ROUNDING_POINTS * 2.0 ** -9 * ymax
    assert psnr >= 60.0
    assert d.median().item() >= 2.0 ** -14 * ymax                      # the rounding points are there: the last one alone moves a value by 2^-10 |v| on average (and |y| > 2^-4 max |y| for most values); without them: 2^-23
    de = (model - exact).abs()
    assert bool(torch.isfinite(bound).all()) and bool((de <= bound).all())


# ---- ref64 against torch's functionals ---------------------------------------------------------------------------------------------------------------------------------
def test_references_agree_with_the_functionals():
    x = G.randn((2, 9, 11, 16), 1)
    for K in (3, 5, 7):
        w, b = G.randn((16, 1, K, K), 2 + K), G.randn((16,), 3)
        want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=K // 2, groups=16).permute(0, 2, 3, 1)
        assert torch.allclose(G.ref64_dwconv2d(x, G.dw_taps(w), K, b), want, rtol=1e-13, atol=1e-13)
        assert torch.allclose(G.ref64_dwconv2d(x, G.dw_taps(w), K, b, True), want + x.double(), rtol=1e-13, atol=1e-13)
    t = G.randn((50, 80), 4)
    gm, bt = G.randn((80,), 5), G.randn((80,), 6)
    want = F.layer_norm(t.double(), (80,), gm.double(), bt.double(), 1e-5)
    assert torch.allclose(G.e_layernorm(t.double(), None, gm.double(), bt.double(), 1e-5, 80)[0], want, rtol=1e-12, atol=1e-12)
    assert torch.equal(G.ref64_layernorm(t, gm, bt, 1e-5), want)
    h = torch.linspace(-8, 8, 4001)
    assert torch.allclose(G.restate32_hswish(h).double(), F.hardswish(h.double()), rtol=1e-6, atol=1e-7)
    assert torch.equal(torch.signbit(G.restate32_hswish(torch.tensor([-3.0, -8.0, 0.0]))), torch.tensor([True, True, False]))       # x <= -3: exactly -0.0
    k, v = G.randn((2, 300, 64), 7, 2.0), G.randn((2, 300, 64), 8)
    ks = k.double().reshape(2, 300, 8, 8).permute(0, 2, 1, 3).softmax(dim=2)
    want = 0.3 * torch.einsum("bhnk,bhnv->bhkv", ks, v.double().reshape(2, 300, 8, 8).permute(0, 2, 1, 3))           # as oracle/groupmix_oracle.efficient_att
    assert torch.allclose(G.ref64_kv(k, v, 8, 8, 0.3), want, rtol=1e-12, atol=1e-14)
    kb, vb = k.to(BF16), v.to(BF16)
    assert bool(((G.model64_kv_mfma(kb, vb, 0.3) - G.ref64_kv(kb, vb, 8, 8, 0.3)).abs() <= G.slack64_kv(kb, vb, 8, 8, 0.3, G.rel_p_mfma(kb))).all())


def test_pointwise_reference_is_the_aggregators_tail():
    """ref64_pointwise against BatchNorm(eval) / 1x1 convolution / LayerNorm / Hardswish functionals (groupmix.py:92-100)."""
    seg, b, H, W = 8, 2, 3, 5
    qkv, dwc = G.randn((b, H, W, 15 * seg), 11), G.randn((b, H, W, 3, 4 * seg), 12)
    pw, pwl = G.randn((3, seg, seg), 13), G.randn((seg, 3 * seg), 14)
    wgt, bias, mean, var = G.randn((4, seg), 15), G.randn((4, seg), 16), G.randn((4, seg), 17), G.randn((4, seg), 18).abs() + 0.5
    sc = wgt.double() / torch.sqrt(var.double() + 1e-5)
    sh = bias.double() - mean.double() * sc
    lg, lb = G.randn((seg,), 19), G.randn((seg,), 20)
    (rq, _), (rl, _) = G.ref64_pointwise(qkv, dwc, pw, sc, sh, pwl, lg, lb)
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    for w in range(3):
        for g in range(4):
            x = nchw(qkv[..., w * 5 * seg:w * 5 * seg + seg]) if g == 0 else F.conv2d(nchw(dwc[..., w, (g - 1) * seg:g * seg]), pw[g - 1].double()[:, :, None, None])
            y = F.hardswish(F.batch_norm(x, mean[g].double(), var[g].double(), wgt[g].double(), bias[g].double(), False, 0.0, 1e-5)).permute(0, 2, 3, 1)
            assert torch.allclose(rq[..., w, g * seg:(g + 1) * seg], y, rtol=1e-11, atol=1e-12), (w, g)
    t = F.conv2d(nchw(torch.cat([dwc[..., w, 3 * seg:] for w in range(3)], -1)), pwl.double()[:, :, None, None]).permute(0, 2, 3, 1)
    assert torch.allclose(rl, F.hardswish(F.layer_norm(t, (seg,), lg.double(), lb.double(), 1e-5)), rtol=1e-11, atol=1e-12)


# ---- restate32 inside slack64 of ref64, on the kinds of data the GPU file uses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_restatements_lie_inside_the_windows(dtype):
    for K in (3, 5, 7):
        for identity in (False, True):
            x = G.bits12((2, 17, 33, 16), 30 + K) if dtype == F32 else G.real_map((2, 17, 33, 16), 30 + K)
            taps = G.bits12((K * K, 16), 31, 1.0 / K) if dtype == F32 else (G.randn((K * K, 16), 31) / K).to(BF16).float()
            bias = G.randn((16,), 32)
            assert inside(G.restate32_dwconv2d(x, taps, K, bias, identity), G.ref64_dwconv2d(x, taps, K, bias, identity), G.slack64_dwconv2d(x, taps, K, bias, identity), dtype)
            # the products are exact, as the restatement needs
            p = taps.double()[:, None] * x.double().reshape(1, -1, 16)
            assert torch.equal(p.float().double(), p)
    for c in G.LN_C[dtype][:3]:
        x = G.real_map((17, c), 40 + c, dtype, outlier=False) * 2 + 0.5
        g, b = 1 + 0.2 * G.randn((c,), 41), 0.2 * G.randn((c,), 42)
        assert inside(G.restate32_layernorm(x, g, b, 1e-5), G.ref64_layernorm(x, g, b, 1e-5), G.slack64_layernorm(x, g, b, 1e-5), dtype)
    seg = 16
    args = (G.real_map((3, 5, 5, 15 * seg), 50, dtype), G.real_map((3, 5, 5, 3, 4 * seg), 51, dtype), G.randn((3, seg, seg), 52) / 4, 1 + 0.3 * G.randn((4, seg), 53),
            0.3 * G.randn((4, seg), 54), G.randn((seg, 3 * seg), 55) / 7, 1 + 0.2 * G.randn((seg,), 56), 0.2 * G.randn((seg,), 57))
    (rq, eq), (rl, el) = G.ref64_pointwise(*args)
    wq, wl = G.restate32_pointwise(*args)
    assert inside(wq, rq, eq, dtype) and inside(wl, rl, el, dtype)
    mk = (lambda s, sd: G.bits12(s, sd)) if dtype == F32 else (lambda s, sd: G.real_map(s, sd, outlier=False))
    a = (mk((3, 65, 1, 3, 64), 60), mk((3, 65, 1, 64), 61), mk((3, 65, 1, 16), 62), G.bits12((3, 8, 8, 8), 63, 0.3) if dtype == F32 else G.randn((3, 8, 8, 8), 63, 0.3).to(BF16).float())
    assert inside(G.restate32_apply(*a, 8, 8), G.ref64_apply(*a, 8, 8), G.slack64_apply(*a, 8, 8), dtype)


def test_crpe_and_integer_restatements_lie_inside_the_windows():
    qkvp = G.real_map((12, 2, 17, 33, 16), 70)
    taps = [(G.randn((k * k, 16), 71 + s) / k).to(BF16).float() for s, k in enumerate(G.CRPE_K)]
    bias = G.randn((64,), 79)
    assert inside(G.restate32_crpe(qkvp, taps, bias), G.ref64_crpe(qkvp, taps, bias), G.slack64_crpe(qkvp, taps, bias), BF16)
    P = G.agg_params(80, ints=True)
    qkv = G.small_ints((15, 3, 5, 7, 16), 81, 2, BF16)
    wq, wl = G.restate32_aggregate_ints(qkv, P)
    (rq, eq), (rl, el) = G.aggregate64(qkv, P, False)
    assert inside(wq, rq, eq, BF16) and inside(wl, rl, el, BF16)
    (mq, _), (ml, _) = G.aggregate64(qkv, P, True)
    assert G.flip_share(wq, mq)[0] == 0 and G.flip_share(wl, ml)[0] <= 0.01          # LayerNorm(16) in fp32 steps against float64: a rounding boundary now and then
    for kind in ("const", "gate"):
        gen = torch.Generator().manual_seed(90)
        v = torch.randint(-8, 9, (2, 300, 64), generator=gen).float()
        k = (torch.randn(2, 1, 64, generator=gen) * 3).to(BF16).float().expand(2, 300, 64) if kind == "const" else torch.where(torch.rand(2, 300, 64, generator=gen) < 0.5, 0.0, -200.0)
        if kind == "gate":
            k[:, 0] = 0.0
        got = G.exact32_kv(k, v, 8, 8, 0.35)
        assert inside(got, G.ref64_kv(k, v, 8, 8, 0.35), G.slack64_kv(k, v, 8, 8, 0.35, torch.zeros_like(k, dtype=torch.float64)), F32)


def test_the_models_lie_inside_the_windows_of_their_references():
    """round_to(model64) must pass the window test the kernels have to pass: a rounding point missing from a bound (or a bound too narrow for it) shows here."""
    qkv, P = G.sharp_inputs_aggregate()
    (rq, eq), (rl, el) = G.aggregate64(qkv, P, False)
    (mq, _), (ml, _) = G.aggregate64(qkv, P, True)
    assert inside(mq.to(BF16), rq, eq, BF16) and inside(ml.to(BF16), rl, el, BF16)
    x, g1, b1, wq, bq, P = G.sharp_inputs_qkv_aggregate()
    (rq, eq), (rl, el) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, False)
    (mq, _), (ml, _) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, True)
    assert inside(mq.to(BF16), rq, eq, BF16) and inside(ml.to(BF16), rl, el, BF16)
    x, g1, b1, wq, bq = G.sharp_inputs_ln_qkv()
    assert inside(G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, True)[0].to(BF16), *G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, False), BF16)
    for cout in (0, 192):
        a = G.sharp_inputs_tail(cout=cout)
        m, r = G.tail64(*a, True), G.tail64(*a, False)
        assert all(inside(m[k][0].to(BF16), *r[k], BF16) for k in r)
    a = G.sharp_inputs_in_cpe()
    assert inside(G.in_cpe64(*a, True)[0].to(BF16), *G.in_cpe64(*a, False), BF16)


# ---- sharpness: the CPU side ---------------------------------------------------------------------------------------------------------------------------------------------
def _cpu_share(v32, m64):
    return G.flip_share(G.round_to(v32, BF16), m64)[0]


def test_a_cpu_fp32_restatement_stays_under_a_tenth_of_a_percent_on_every_sharpness_input():
    """For every input set test_groupmix_gpu.py holds to the 0.5 % cap: the same pipeline with fp32 tensors (torch's fp32 matmuls and convolutions: another
    summation order than the kernels') differs from round_to(model64) on at most 0.1 % of the stored bf16 values.  If a set exceeds it, change the set."""
    shares = {}
    qkv, P = G.sharp_inputs_aggregate()
    (m, _), (ml, _) = G.aggregate64(qkv, P, True)
    (a, _), (al, _) = G.aggregate64(qkv, P, True, F32)
    shares["aggregate qkvp"], shares["aggregate loc"] = _cpu_share(a, m), _cpu_share(al, ml)
    x, g1, b1, wq, bq, P = G.sharp_inputs_qkv_aggregate()
    (m, _), (ml, _) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, True)
    (a, _), (al, _) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, True, F32)
    shares["qkv_aggregate qkvp"], shares["qkv_aggregate loc"] = _cpu_share(a, m), _cpu_share(al, ml)
    x, g1, b1, wq, bq = G.sharp_inputs_ln_qkv()
    shares["ln_qkv"] = _cpu_share(G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, True, F32)[0], G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, True)[0])
    for cout in (0, 192):
        a = G.sharp_inputs_tail(cout=cout)
        m, f = G.tail64(*a, True), G.tail64(*a, True, F32)
        for k in m:
            shares[f"tail cout{cout} {k}"] = _cpu_share(f[k][0], m[k][0])
    a = G.sharp_inputs_in_cpe()
    shares["in_cpe"] = _cpu_share(G.in_cpe64(*a, True, F32)[0], G.in_cpe64(*a, True)[0])
    print({k: f"{100 * v:.4f} %" for k, v in shares.items()})
    assert all(v <= 1e-3 for v in shares.values()), shares


# ---- argument checks (no GPU: every call must be refused before a launch) -------------------------------------------------------------------------------------------
P_, Q_ = 4096, 4100          # dummy device pointers: 16-byte aligned / not


def _bad_calls():
    """(entry point, the part of the message that names it, arguments); every line one fault."""
    f, h, x16 = RC_F32, RC_BF16, RC_F16
    A, B = P_, Q_
    t = []
    dw = lambda **k: ("rc_dwconv2d", "rc_dwconv2d", tuple({**dict(x=A, xs=16, x0=0, y=A, ys=16, y0=0, dt=h, b=1, H=4, W=4, n=16, K=3, w=A, nw=16, bias=None, rep=1, xr=0, yr=0, wr=0, idn=0, kv=None,
                                                                  st=None), **k}.values()))
    t += [dw(x=None), dw(dt=x16), dw(dt=7), dw(K=4), dw(K=9), dw(n=12), dw(n=4), dw(x0=4), dw(x0=8), dw(ys=8), dw(b=0), dw(H=0), dw(rep=0), dw(x=B), dw(y=B),
          dw(rep=2, xr=8, yr=8, wr=8), dw(n=8, xs=8, ys=8, nw=10, dt=h), dw(dt=f, n=6)]
    ln = lambda **k: ("rc_layernorm", "rc_layernorm", tuple({**dict(x=A, y=A, dt=h, tok=4, c=80, g=A, b=A, eps=1e-5, st=None), **k}.values()))
    t += [ln(x=None), ln(g=None), ln(dt=x16), ln(tok=0), ln(c=4), ln(c=84), ln(c=520), ln(dt=f, c=260), ln(dt=f, c=6), ln(x=B), ln(y=B)]
    pw = lambda **k: ("rc_gma_pointwise", "rc_gma_pointwise", tuple({**dict(q=A, dw=A, dwl=A, a=192, b=64, c=192, d=64, qp=A, loc=A, dt=h, tok=4, C=80, pw=A, sc=A, sh=A, pwl=A, lg=A, lb=A, st=None),
                                                                       **k}.values()))
    t += [pw(q=None), pw(lb=None), pw(dt=x16), pw(tok=0), pw(C=60), pw(C=82), pw(C=5), pw(a=128), pw(b=40), pw(c=40), pw(d=8), pw(a=196), pw(q=B), pw(dw=B), pw(dwl=B), pw(qp=B), pw(loc=B)]
    kv = lambda **k: ("rc_gma_kv", "rc_gma_kv", tuple({**dict(q=A, dt=h, b=1, n=4, hd=8, ch=8, s=1.0, scr=A, out=A, st=None), **k}.values()))
    t += [kv(q=None), kv(scr=None), kv(dt=x16), kv(b=0), kv(b=70000), kv(n=0), kv(hd=0), kv(ch=33), kv(hd=3, ch=3), kv(hd=40, ch=8), kv(dt=f, hd=1, ch=2), kv(q=B)]
    kp = lambda **k: ("rc_gma_kv_planar", "rc_gma_kv", tuple({**dict(q=A, b=1, n=4, hd=8, ch=8, s=1.0, scr=A, out=A, st=None), **k}.values()))
    t += [kp(q=None), kp(hd=3, ch=8), kp(n=0), kp(q=B)]
    ap = lambda **k: ("rc_gma_apply", "rc_gma_apply", tuple({**dict(q=A, cv=A, loc=A, ktv=A, out=A, dt=h, b=1, n=4, hd=8, ch=8, seg=16, st=None), **k}.values()))
    t += [ap(q=None), ap(out=None), ap(dt=x16), ap(b=0), ap(b=70000), ap(n=0), ap(hd=0), ap(ch=33), ap(seg=0), ap(hd=64, ch=32)]
    lq = lambda **k: ("rc_gma_ln_qkv", "rc_gma_ln_qkv", tuple({**dict(x=A, q=A, tok=4, w=A, b=A, g=A, bt=A, eps=1e-5, st=None), **k}.values()))
    t += [lq(x=None), lq(w=None), lq(g=None), lq(tok=0), lq(x=B), lq(q=B), lq(w=B)]
    tl = lambda **k: ("rc_gma_tail", "rc_gma_tail", tuple({**dict(q=A, cv=A, loc=A, x=A, ktv=A, fr=A, b=1, n=4, wp=A, bp=A, g=A, bt=A, eps=1e-5, w1=A, b1=A, w2=A, b2=A, res=None, wo=None, bo=None,
                                                                    co=0, out=A, st=None), **k}.values()))
    t += [tl(q=None), tl(fr=None), tl(b2=None), tl(out=None), tl(b=0), tl(n=0), tl(co=64), tl(co=80), tl(co=192), tl(co=192, res=A, wo=A), tl(q=B), tl(cv=B), tl(loc=B), tl(x=B), tl(out=B),
          tl(co=192, res=B, wo=A, bo=A)]
    ag = lambda **k: ("rc_gma_aggregate", "rc_gma_aggregate", tuple({**dict(q=A, qp=A, loc=A, b=1, H=4, W=4, d3=A, d5=A, d7=A, dl=A, pw=A, pwl=A, sc=A, sh=A, lg=A, lb=A, km=None, st=None),
                                                                       **k}.values()))
    t += [ag(q=None), ag(lb=None), ag(d5=None), ag(b=0), ag(H=0), ag(W=0), ag(q=B), ag(qp=B), ag(loc=B)]
    qa = lambda **k: ("rc_gma_qkv_aggregate", "rc_gma_qkv_aggregate", tuple({**dict(x=A, wq=A, bq=None, g=A, bt=A, eps=1e-5, qp=A, loc=A, b=1, H=4, W=4, tp=A, pw=A, pwl=A, sc=A, sh=A, lg=A, lb=A,
                                                                               km=None, st=None), **k}.values()))
    t += [qa(x=None), qa(tp=None), qa(lb=None), qa(b=0), qa(H=0), qa(W=0), qa(b=70000, H=1024, W=1024), qa(x=B), qa(qp=B), qa(loc=B), qa(tp=B)]
    ic = lambda **k: ("rc_gma_in_cpe", "rc_gma_in_cpe", tuple({**dict(d1=A, w=A, bi=None, tp=A, bc=None, x=A, b=1, H=4, W=4, st=None), **k}.values()))
    t += [ic(d1=None), ic(tp=None), ic(x=None), ic(b=0), ic(H=0), ic(W=0), ic(H=65536, W=65536), ic(d1=B), ic(x=B)]
    cr = lambda **k: ("rc_gma_crpe", "rc_gma_crpe", tuple({**dict(q=A, cv=A, b=1, H=4, W=4, t0=A, t1=A, t2=A, t3=A, bias=A, st=None), **k}.values()))
    t += [cr(q=None), cr(t2=None), cr(bias=None), cr(b=0), cr(H=0), cr(W=0), cr(q=B), cr(cv=B)]
    km = lambda **k: ("rc_gma_kv_mfma", "rc_gma_kv_mfma", tuple({**dict(q=A, b=1, n=4, s=1.0, km=A, scr=A, out=A, st=None), **k}.values()))
    t += [km(q=None), km(km=None), km(b=0), km(b=70000), km(n=0), km(q=B)]
    return t


def test_bad_arguments_of_the_groupmix_entry_points_are_refused_before_any_launch():
    lib = _lib.load()
    calls = _bad_calls()
    assert len({n for n, _, _ in calls}) == 13
    for name, tag, args in calls:
        lib.rc_bayer_unshuffle(None, 0, None, 0, 1, 4, 4, 4, 4, None)       # leaves another entry point's message behind
        code = getattr(lib, name)(*args)
        msg = lib.rc_last_error().decode()
        assert code == -1 and tag in msg, (name, args, code, msg)           # RC_ERR_INVALID from the entry point's own check, not a failed launch


# ---- the coverage table of the GPU file -----------------------------------------------------------------------------------------------------------------------------
def test_every_groupmix_entry_point_is_in_the_gpu_files_coverage_table():
    """Every rc_gma_* / rc_dwconv2d / rc_layernorm symbol of the header, the host packers aside (test_chain_pack.py has those), has a row in the docstring of
    test_groupmix_gpu.py, the test that row names exists, and the file calls the entry point."""
    header = open(os.path.join(ROOT, "include", "realcam_hip.h")).read()
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    mine = {n for n in declared if n.startswith("rc_gma_") or n in ("rc_dwconv2d", "rc_layernorm")} - {"rc_gma_toeplitz_pack"}
    assert len(mine) == 18, sorted(mine)
    gpu = open(os.path.join(ROOT, "tests", "test_groupmix_gpu.py")).read()
    doc = gpu.split('"""')[1]
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", gpu, flags=re.M))
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(rc_[a-z0-9_]+)\s+\S+\s+(test_[a-z0-9_]+)", doc, flags=re.M)}
    assert set(rows) == mine, (sorted(mine - set(rows)), sorted(set(rows) - mine))
    assert all(t in tests for t in rows.values()), sorted(t for t in rows.values() if t not in tests)
    body = gpu.split('"""', 2)[2]
    called = set(re.findall(r"\b(rc_[a-z0-9_]+)\b", body)) | {"rc_" + n for n in re.findall(r"\b(?:_R|ops)\.([a-z0-9_]+)\(", body)}
    # realcam::gma_kv takes rc_gma_kv_planar for a segment-planar tensor: the test its row names must build one and pass it to that op
    planar = re.search(r"^def %s\(.*?(?=^def |\Z)" % rows["rc_gma_kv_planar"], gpu, flags=re.M | re.S).group(0)
    assert "_planar64(" in planar and "_R.gma_kv(" in planar
    assert mine - {"rc_gma_kv_planar"} <= called, sorted(mine - called)


def test_require_acts_refuses_other_dtypes_and_strided_views():
    from realcamnet_amd import torch_ops
    t = torch.zeros(4, 6, dtype=BF16)
    torch_ops.require_acts("op", BF16, t, None, t[1:])
    with pytest.raises(TypeError, match="realcam::op"):
        torch_ops.require_acts("op", BF16, t, t.float())
    with pytest.raises(ValueError, match="realcam::op"):
        torch_ops.require_acts("op", BF16, t, t[:, ::2])
    src = open(os.path.join(ROOT, "realcamnet_amd", "torch_ops.py")).read()
    for op in ("dwconv2d", "layernorm", "gma_pointwise", "gma_kv", "gma_apply", "gma_ln_qkv", "gma_tail", "gma_aggregate", "gma_in_cpe", "gma_qkv_aggregate", "gma_kv_mfma", "gma_crpe"):
        m = re.search(r'define\("%s\(.*?\n\n' % op, src, flags=re.S)
        assert m and "acts=" in m.group(0), op                           # every GroupMix op is registered with its activation check
