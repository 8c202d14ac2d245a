"""CPU yardstick for the convolution launcher rc_conv2d (csrc/conv.hip, conv_kernel.hpp, conv_inst_*.hip).  Plain torch, no dependence on the library or the
oracle; the conventions and helpers are those of streaming_ref.py.

  ref64_conv    the operation in float64 from operands already rounded to the storage dtype: the weights through the round-to-nearest-even cast that
                rc_conv_pack_weights applies, bias and per-image vectors in fp32.
                Input.  Either x, or the gated input x * gate[b, c] + skip.  What commit_tile (vector staging) and stage_tile_scalar (scalar staging) compute for
                the gated input is `f0 * g + f1` in fp32 -- the library is built with -ffp-contract=off, so that is TWO fp32 roundings (product, sum) -- followed by
                ONE round-to-nearest-even cast to the storage dtype (Vec16<T>::pack / from_f32<T>).  The packed value is both what goes to LDS for the MFMA and
                what in_store receives, on both staging paths.  So "rounded once to the storage dtype" holds for the cast, but the value that is cast is the fp32
                evaluation, not the real-valued one: gated_input() restates it in fp32 op by op, which reproduces in_store bit for bit on any data.
                Convolution.  F.conv2d in float64 with zero padding k // 2; ksize 2 is the window at pixel offsets {-1, 0}^2; a ksize-2 launch with src_h / src_w
                is the stride-2 3 x 3 convolution of its own input (ref64_conv_stride2).
                Epilogue, in the order epilogue_generic states it, from the bias as the accumulator's initial value: FiLM v * fs + ft + v, activation,
                x (mul_plus1 + 1), x out_scale, + residual, the ReLU of RC_ACT_RELU_POST, the store (NHWC, PixelShuffle(2), planar with crop, planar
                PixelShuffle(2) with crop).
                Channel sums.  Every kernel (epilogue_generic, epilogue_fast_impl and the carried-sums forms built on it) adds the fp32 value `v` it is about to
                store, i.e. the epilogue's result BEFORE the rounding to the storage dtype, over the valid pixels of the image; "sums" is that total per (b, c).
  slack64_conv  the running-error bound gamma_k * S: k = cin * ksize^2 terms of the dot product + 1 for the bias + the fp32 roundings the epilogue adds on the
                element's path; S = the sum of absolute terms carried through the epilogue (|bias| + sum |x||w|, times |fs| + 1 plus |ft|, times max(1, |slope|),
                times |m + 1|, times |scale|, plus |residual|).  GELU adds groupmix_ref's allowance for gelu_erf_f32.
  plan          make_plan()'s choice of (ck, nt, n_chunks, n_ct, cout_packed, steps) restated (conv32 knob at its default 0), checked against the library's
                packed sizes on the CPU (test_conv_host.py), so that test_conv_gpu.py can say which launch_conv<ConvCfg<T, CK, NT, KS>> a case reaches.

How the matrix cores round inside one MFMA is not documented; every real-valued case of test_conv_gpu.py lies inside gamma_k with k as above on an MI355X (the bound
is linear in k where random data errs like sqrt(k)), so no measured accumulation constant is recorded here and none is needed."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from groupmix_ref import e_gelu
from streaming_ref import DTYPES, TINY, U32, gamma, round_to, same_bits, small_ints, values, within_rounding  # noqa: F401  (re-exported to the tests)

NHWC, PS2, NCHW, PS2_NCHW = 0, 1, 2, 3            # rc_out_mode
OUT_MODES = (NHWC, PS2, NCHW, PS2_NCHW)
TH, TW, WSM_TH = 8, 32, 16                         # kTH, kTW, kWsmTH of conv_kernel.hpp: the 8 x 32 tile, the 16-row strips of kernels 4 / 4b / 6
ELEM = {"f32": "float", "bf16": "bf16_t", "f16": "f16_t"}


# ---- make_plan ---------------------------------------------------------------------------------------------------------------------------------------------
def _rules(cin, cout, ksize, dtype, out_mode, cout_tile):
    """make_plan (csrc/conv.hip), its rules in its order, on integer numpy arrays cin and cout that broadcast against each other (conv32 knob at its default 0):
    a dict of arrays, `ok` False where the library refuses the shape."""
    cin, cout = np.broadcast_arrays(np.asarray(cin, dtype=np.int64), np.asarray(cout, dtype=np.int64))
    ok = (cin >= 1) & (cout >= 1) & (ksize in (1, 2, 3, 5) and dtype in ELEM)
    h16 = dtype != "f32"
    if ksize == 5:
        ok &= (cout <= 16) & (out_mode != PS2) & (((cin % 48 == 0) | (cin % 32 == 0)) if h16 else (cin % 16 == 0))
    if out_mode == PS2_NCHW:
        ok &= cout % 4 == 0
    if ksize == 2:
        ok &= (cin % 16 == 0) & ~((cin % 48 == 0) & (cin % 64 != 0)) & (dtype == "bf16" and out_mode == NHWC)
    unit = 4 if dtype == "f32" else 8
    if ksize == 5:
        ck = np.where(cin % 48 == 0, 48, 32) if h16 else 16 + 0 * cin
    elif h16:
        ck = np.select([cin <= 8, (cin % 80 == 0) & (cin % 64 != 0) & (ksize == 1), (cin % 64 == 0) & (cin > 64) & (ksize >= 2), cin % 64 == 0, cin % 48 == 0,
                        (cin == 32) & (ksize == 3), (cin % 32 == 0) & (cin > 64) & (ksize == 3)], [8, 80, 32, 64, 48, 32, 32], 16)
    else:
        ck = np.where(cin <= 4, 4, 16)
    if out_mode == PS2:
        cps = cout // 4
        nt = np.select([(cps % 64 == 0) & ~((cps % 48 == 0) & (cin == 48) & h16), cps % 48 == 0, cps % 16 == 0], [4, 3, 1], 0)
        ok &= (cout % 4 == 0) & (nt != 0)
    else:
        k3h = h16 and ksize == 3
        nt = np.select([(cout % 48 == 0) & (cin == 48) & h16, (cin == 32) & (cout == 32) & k3h, (cout % 80 == 0) & (ksize == 1), cout % 64 == 0, cout % 48 == 0,
                        (ck == 32) & (cout % 32 == 0) & k3h], [3, 2, 5, 4, 3, 2], 1)
    if cout_tile != 0:
        ok &= not (cout_tile < 16 or cout_tile > 80 or cout_tile % 16 != 0 or ksize in (2, 5) or out_mode in (PS2, PS2_NCHW))
        nt = cout_tile // 16 + 0 * nt
    nt = np.maximum(nt, 1)
    upt, taps = ck // unit, ksize * ksize
    steps = np.where(upt == 6, taps + (taps + 1) // 2, (taps * upt + 3) // 4)           # unit_map_steps
    n_chunks, n_ct = -(-cin // ck), -(-cout // (16 * nt))
    return dict(ok=ok, ck=ck, nt=nt, unit=unit + 0 * ck, steps=steps, n_chunks=n_chunks, n_ct=n_ct, cout_packed=n_ct * 16 * nt, packed_bytes=n_ct * n_chunks * steps * nt * 1024)


@functools.lru_cache(maxsize=None)
def plan(cin, cout, ksize, dtype, out_mode, cout_tile=0):
    """The plan of one shape for dtype "f32" / "bf16" / "f16": a dict (ck, nt, unit, steps, n_chunks, n_ct, cout_packed, packed_bytes; do not modify it), or None
    where the library refuses the shape."""
    r = _rules(cin, cout, ksize, dtype, out_mode, cout_tile)
    return {k: int(v) for k, v in r.items() if k != "ok"} if bool(r["ok"]) else None


def plan_grid(ksize, dtype, out_mode, cout_tile=0, n=640):
    """The same rules over every cin (rows) and cout (columns) in 1 .. n at once: (valid, cout_packed, packed_bytes, ck, nt) as (n, n) arrays (sizes 0 where refused)."""
    r = _rules(np.arange(1, n + 1)[:, None], np.arange(1, n + 1)[None, :], ksize, dtype, out_mode, cout_tile)
    return r["ok"], np.where(r["ok"], r["cout_packed"], 0), np.where(r["ok"], r["packed_bytes"], 0), r["ck"], r["nt"]


def packed_to_cout(p, cout, out_mode, j):
    """packed cout index j -> conv output channel, -1 for the padding rows (packed_to_cout of csrc/conv.hip)."""
    if out_mode == PS2:
        tile = 16 * p["nt"]
        ct, within = divmod(j, tile)
        return 4 * ((ct >> 2) * tile + within) + (ct & 3)
    return j if j < cout else -1


def instantiation(p, ksize, dtype):
    return f"ConvCfg<{ELEM[dtype]}, {p['ck']}, {p['nt']}, {ksize}>"


# ---- cases and their data ----------------------------------------------------------------------------------------------------------------------------------
class Case(dict):
    """One launch: cin, cout, k, shape (B, H, W), act, slope, the optional operands as flags, the store, the knobs.  `name` is the pytest id."""
    DEFAULTS = dict(k=3, shape=(1, 9, 33), act=None, slope=0.0, bias=True, film=False, mul=False, res=False, scale=False, sums=False, gated=False, store=False,
                    out_mode=NHWC, crop=None, out_dtype=None, cout_tile=0, offset=0, film_offset=0, knobs=(), dtypes=("bf16", "f16", "f32"), poison=False)

    def __init__(self, name, cin, cout, **kw):
        bad = set(kw) - set(self.DEFAULTS)
        assert not bad, bad
        super().__init__(self.DEFAULTS, name=name, cin=cin, cout=cout, **kw)

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)

    def out_hw(self):
        _, H, W = self.shape
        full = (2 * H, 2 * W) if self.out_mode in (PS2, PS2_NCHW) else (H, W)
        return self.crop if (self.crop is not None and self.out_mode in (NCHW, PS2_NCHW)) else full


def carries_fractions(c):
    """Does the exact regime give this case the fractional bias?  Every case with a bias, except the channel-sum cases on maps so large that the per-lane sums a
    persistent block carries over many tiles would leave fp32's 24 bits."""
    B, H, W = c.shape
    return bool(c.bias) and (not c.sums or B * H * W <= 8192)


def _choice(g, shape, options, weights=None):
    w = torch.tensor(weights if weights is not None else [1.0] * len(options), dtype=torch.float64)
    idx = torch.multinomial(w, int(math.prod(shape)), replacement=True, generator=g)
    return torch.tensor(options, dtype=torch.float32)[idx].reshape(shape)


def exact_data(c, dtype, seed=0):
    """Operands whose every product, partial sum and epilogue intermediate is a dyadic number of fewer than 24 significant bits (test_conv_host.py checks the
    head-room per case): x in halves |x| <= 2, integer weights |w| <= 2, a bias of magnitude 64 + 4 sqrt(terms) or a little more + an odd number of 64ths (so that the result needs a rounding
    in bf16 and fp16; all but channels 7, 23, ... positive under a ReLU, so that most outputs stay non-zero), gate / FiLM / out_scale / mul_plus1 in {0, 1, 2}, slopes 0.5 or 0.25.
    With channel sums on a large map (carries_fractions) the bias is a small integer: the per-lane sums carried over many tiles then stay exact too; on the small maps
    a slot holds at most one tile's 64 pixels a wave, which leaves the fractions room."""
    T = DTYPES[dtype]
    g = torch.Generator().manual_seed(1000 + seed)
    B, H, W = c.shape
    d = {}
    d["x"] = (torch.randint(-4, 5, (B, H, W, c.cin), generator=g).float() / 2).to(T)
    d["w"] = torch.randint(-2, 3, (c.cout, c.cin, c.k, c.k), generator=g).float()
    if c.bias:
        if not carries_fractions(c):
            d["bias"] = torch.randint(-6, 10, (c.cout,), generator=g).float()
        else:
            base = 64 + int(4 * math.sqrt(c.cin * c.k * c.k))                          # clear of the dot product's spread (about 1.8 sqrt(terms))
            mag = torch.randint(base, base + 64, (c.cout,), generator=g).float() + (2 * torch.randint(0, 32, (c.cout,), generator=g).float() + 1) / 64
            pos = c.act in ("relu", "relu_post")
            d["bias"] = mag * (torch.where(torch.arange(c.cout) % 16 == 7, -1.0, 1.0) if pos else _choice(g, (c.cout,), [1.0, -1.0]))
    if c.gated:
        d["gate"] = _choice(g, (B, c.cin), [0.0, 1.0, 2.0], [1, 3, 3])
        d["skip"] = (torch.randint(-4, 5, (B, H, W, c.cin), generator=g).float() / 2).to(T)
    if c.film:
        d["fs"] = _choice(g, (B, c.cout), [0.0, 1.0, 2.0])
        d["ft"] = torch.randint(-8, 9, (B, c.cout), generator=g).float()
    if c.mul:
        d["mul"] = _choice(g, (B, H, W, c.cout), [0.0, 1.0, 2.0]).to(T)
    if c.scale:
        d["scale"] = _choice(g, (B, c.cout), [0.0, 1.0, 2.0], [1, 4, 3])
    if c.res:
        d["res"] = (torch.randint(-16, 17, (B, H, W, c.cout), generator=g).float() / 2).to(T)
    return d


def real_data(c, dtype, seed=0):
    """values(): normals over a few binades with zeros and 16-bit subnormals mixed in.  |x| < 8, |w| < 1, so a dot product of the largest case (2 880 terms) stays
    below 23 040 and nothing overflows fp16."""
    T = DTYPES[dtype]
    s = 2000 + 16 * seed
    B, H, W = c.shape
    d = {}
    d["x"] = values((B, H, W, c.cin), T, s, span=2)
    d["w"] = values((c.cout, c.cin, c.k, c.k), torch.float32, s + 1, span=2, specials=False) / 8
    if c.bias:
        d["bias"] = values((c.cout,), torch.float32, s + 2, span=2, specials=False)
    if c.gated:
        d["gate"] = values((B, c.cin), torch.float32, s + 3, span=1, specials=False).abs()
        d["skip"] = values((B, H, W, c.cin), T, s + 4, span=2)
    if c.film:
        d["fs"] = values((B, c.cout), torch.float32, s + 5, span=1, specials=False)
        d["ft"] = values((B, c.cout), torch.float32, s + 6, span=2, specials=False)
    if c.mul:
        d["mul"] = values((B, H, W, c.cout), T, s + 7, span=1)
    if c.scale:
        d["scale"] = values((B, c.cout), torch.float32, s + 8, span=1, specials=False).abs()
    if c.res:
        d["res"] = values((B, H, W, c.cout), T, s + 9, span=3)
    return d


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------------------
def gated_input(d, dtype):
    """What both staging paths put into LDS and in_store: fp32 product, fp32 sum, one round-to-nearest-even cast (see the module docstring)."""
    T = DTYPES[dtype]
    if "gate" not in d:
        return d["x"]
    return (d["x"].float() * d["gate"][:, None, None, :] + d["skip"].float()).to(T)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv64(x_nhwc, w, k, absolute=False, prec=torch.float64):
    x, w = _nchw(x_nhwc.to(prec)), w.to(prec)
    if absolute:
        x, w = x.abs(), w.abs()
    if k == 2:
        return F.conv2d(F.pad(x, (1, 0, 1, 0)), w)
    return F.conv2d(x, w, padding=k // 2)


def _store(c, y):
    """(B, cout, H, W) -> the launch's output layout."""
    if c.out_mode == NHWC:
        return y.permute(0, 2, 3, 1).contiguous()
    if c.out_mode == PS2:
        return F.pixel_shuffle(y, 2).permute(0, 2, 3, 1).contiguous()
    oh, ow = c.out_hw()
    y = F.pixel_shuffle(y, 2) if c.out_mode == PS2_NCHW else y
    return y[:, :, :oh, :ow].contiguous()


def _epilogue(c, d, v, S, k_round):
    """The epilogue on the float64 value v (B, cout, H, W); S the sum of absolute terms, k_round the count of fp32 roundings so far, extra an additive allowance.
    (Evaluated in v's own precision: test_conv_host.py runs it in fp32 as well to prove that the exact regime's data is exact.)"""
    prec = v.dtype
    per_image = lambda t: t.to(prec)[:, :, None, None]          # noqa: E731
    extra = torch.zeros_like(v)
    if c.film:
        fs, ft = per_image(d["fs"]), per_image(d["ft"])
        v, S, k_round = v * fs + ft + v, S * (fs.abs() + 1) + ft.abs(), k_round + 3
    if c.act == "relu":
        v = v.clamp_min(0)
    elif c.act == "leaky":
        sl = float(torch.tensor(c.slope, dtype=torch.float32))
        v, S, k_round = torch.where(v > 0, v, v * sl), S * max(1.0, abs(sl)), k_round + 1
    elif c.act == "gelu":
        e = gamma(k_round) * S
        v, bound = e_gelu(v, e)                                   # groupmix_ref: the bound after gelu_erf_f32 of a value that carries the error e
        extra = bound - e                                         # S stays (|gelu(v)| <= |v| <= S), so gamma(k) * S + extra is that bound
    if c.mul:
        m1 = _nchw(d["mul"].to(prec)) + 1.0
        v, S, extra, k_round = v * m1, S * m1.abs(), extra * m1.abs(), k_round + 2
    if c.scale:
        s = per_image(d["scale"])
        v, S, extra, k_round = v * s, S * s.abs(), extra * s.abs(), k_round + 1
    if c.res:
        r = _nchw(d["res"].to(prec))
        v, S, k_round = v + r, S + r.abs(), k_round + 1
    if c.act == "relu_post":
        v = v.clamp_min(0)
    return v, S, k_round, extra


def ref64_conv(c, d, dtype, prec=torch.float64):
    """-> {"out": float64 in the store's layout, "slack": float64 alike, "stored": the materialised gated input (storage dtype) or None,
           "sums": (B, cout) float64 totals or None, "sums_slack": alike}."""
    T = DTYPES[dtype]
    xin = gated_input(d, dtype)
    w = d["w"].to(T)
    n = c.cin * c.k * c.k
    v = _conv64(xin, w, c.k, prec=prec)
    S = _conv64(xin, w, c.k, absolute=True, prec=prec)
    if c.bias:
        b = d["bias"].to(prec)[None, :, None, None]
        v, S = v + b, S + b.abs()
    v, S, k_round, extra = _epilogue(c, d, v, S, n + 1)
    slack = gamma(k_round) * S + extra + TINY
    out = {"out": _store(c, v), "slack": _store(c, slack), "stored": xin if (c.gated and c.store) else None, "sums": None, "sums_slack": None}
    if c.sums:
        px = v.shape[2] * v.shape[3]
        out["sums"] = v.sum(dim=(2, 3))
        out["sums_slack"] = slack.sum(dim=(2, 3)) + gamma(px) * v.abs().sum(dim=(2, 3))
    return out


def slack64_conv(c, d, dtype):
    """The bound alone, in the store's layout (ref64_conv computes it alongside the value: both need the same two convolutions)."""
    return ref64_conv(c, d, dtype)["slack"]


def ref64_conv_stride2(x, w, bias, dtype, act=None, slope=0.0):
    """The 3 x 3 stride-2 convolution that a ksize-2 launch with src_h / src_w computes from its own input (the window gathers the space-to-depth channels while
    staging): F.conv2d(stride=2, padding=1) in float64 on NHWC x, the activation, -> (out NHWC, slack) with k = 9 cin terms + the bias (+ 1 for a LeakyReLU)."""
    T = DTYPES[dtype]
    xd, wd = _nchw(x.double()), w.to(T).double()
    v = F.conv2d(xd, wd, bias.double(), stride=2, padding=1)
    S = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), stride=2, padding=1)
    k_round = 9 * x.shape[-1] + 1
    if act == "relu":
        v = v.clamp_min(0)
    elif act == "leaky":
        sl = float(torch.tensor(slope, dtype=torch.float32))
        v, S, k_round = torch.where(v > 0, v, v * sl), S * max(1.0, abs(sl)), k_round + 1
    return v.permute(0, 2, 3, 1).contiguous(), (gamma(k_round) * S + TINY).permute(0, 2, 3, 1).contiguous()


def exact_headroom(c, d, dtype):
    """Largest sum of absolute terms any element can reach in any summation order, in units of the data's finest bit: below 2^24 every intermediate is exact in fp32."""
    T = DTYPES[dtype]
    xin = gated_input(d, dtype)
    S = _conv64(xin, d["w"].to(T), c.k, absolute=True)
    if c.bias:
        S = S + d["bias"].double().abs()[None, :, None, None]
    _, S, _, _ = _epilogue(c, d, S, S, 0)
    frac = 1 + (6 if carries_fractions(c) else 0) + (2 if c.act == "leaky" else 0)          # halves x 64ths x the slope's quarter
    return float(S.max()) * 2.0 ** frac


def shares(ref_out, dtype):
    """(share of non-zero outputs, share whose float64 value is not representable in the storage dtype)."""
    r = round_to(ref_out, DTYPES[dtype]).double()
    return float((ref_out != 0).double().mean()), float((r != ref_out).double().mean())
