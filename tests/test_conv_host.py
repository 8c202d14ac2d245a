"""CPU: the convolution yardstick (conv_ref.py) against itself and torch's functionals, its restatement of make_plan against the library, the packers on every case of
test_conv_gpu.py, the coverage of csrc/conv_inst_*.hip by those cases, and the refusals of conv_build_args that need no GPU."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import test_conv_gpu as G
from conv_ref import NCHW, NHWC, PS2, PS2_NCHW, Case
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC = {"f32": RC_F32, "bf16": RC_BF16, "f16": RC_F16}

# Instantiations of csrc/conv_inst_*.hip that no (cin, cout, ksize, dtype, out_mode, cout_tile) reaches through make_plan, one line each on why.
# (dtype, ksize, ck, nt): reason.  Empty: every instantiation is reachable -- the sweep below proves it, and nothing is retired here.
UNREACHABLE = {}


def _host_cases():
    """The GPU file's cases, the several-tiles shapes cut down to a few rows (the generators and the packers do not depend on the map's height)."""
    out = []
    for c in G.all_cases():
        if c.name.startswith("tiles-"):
            c = Case(c.name, c.cin, c.cout, **{k: v for k, v in c.items() if k not in ("name", "cin", "cout", "shape")}, shape=(c.shape[0], 24, c.shape[2]))
        out.append(c)
    return out


# ---- the yardstick against itself --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_ref64_conv_is_the_composition_of_torch_functionals(dtype):
    T = R.DTYPES[dtype]

    def nchw(t):
        return t.double().permute(0, 3, 1, 2)
    for c in (Case("a", 12, 20, shape=(2, 9, 11), act="leaky", slope=0.3, film=True, res=True, scale=True, mul=True, sums=True),
              Case("b", 16, 16, k=1, shape=(2, 5, 7), act="gelu"),
              Case("c", 16, 12, k=5, shape=(1, 6, 9), act="relu", out_mode=PS2_NCHW, crop=(11, 15)),
              Case("d", 8, 16, shape=(2, 4, 6), act="relu_post", res=True, out_mode=NHWC, gated=True, store=True),
              Case("e", 16, 64, shape=(1, 4, 6), out_mode=PS2, bias=False),
              Case("f", 16, 8, k=2, shape=(1, 7, 6), dtypes=("bf16",)),
              Case("g", 6, 5, shape=(2, 7, 9), out_mode=NCHW, crop=(3, 8), act="leaky", slope=-0.5)):
        d = R.real_data(c, dtype, seed=3)
        got = R.ref64_conv(c, d, dtype)
        x = d["x"]
        if c.gated:
            x = (d["x"].float() * d["gate"][:, None, None, :] + d["skip"].float()).to(T)
            assert R.same_bits(got["stored"], x)
        w = d["w"].to(T).double()
        b = d["bias"].double() if c.bias else None
        y = F.conv2d(F.pad(nchw(x), (1, 0, 1, 0)), w, b) if c.k == 2 else F.conv2d(nchw(x), w, b, padding=c.k // 2)
        if c.film:
            y = y * d["fs"].double()[:, :, None, None] + d["ft"].double()[:, :, None, None] + y
        y = {None: lambda t: t, "relu": F.relu, "gelu": F.gelu, "relu_post": lambda t: t, "leaky": lambda t: F.leaky_relu(t, float(torch.tensor(c.slope, dtype=torch.float32)))}[c.act](y)
        if c.mul:
            y = y * (nchw(d["mul"]) + 1)
        if c.scale:
            y = y * d["scale"].double()[:, :, None, None]
        if c.res:
            y = y + nchw(d["res"])
        if c.act == "relu_post":
            y = F.relu(y)
        if c.sums:
            assert torch.allclose(got["sums"], y.sum((2, 3)), rtol=1e-12, atol=1e-12)
        if c.out_mode in (PS2, PS2_NCHW):
            y = F.pixel_shuffle(y, 2)
        y = y.permute(0, 2, 3, 1) if c.out_mode in (NHWC, PS2) else y[:, :, :c.crop[0], :c.crop[1]]
        assert got["out"].shape == y.shape and torch.allclose(got["out"], y, rtol=1e-12, atol=1e-12), c.name
        assert bool((got["slack"] > 0).all()) and bool((got["slack"] < 1e-3 * (1 + got["out"].abs().max())).all())


def test_exact_regime_data_is_exact_and_most_results_need_a_rounding():
    """Per case and dtype: the fp32 and the float64 evaluations of the reference agree bit for bit, the sum of absolute terms leaves head-room below 2^24 units of the
    finest bit, and -- where the form has the fractional bias that makes it possible (conv_ref.carries_fractions: not the no-bias "plain" cases nor the channel-sum cases on
    the several-tiles maps) -- at least half of the outputs are non-zero and at least half are not representable in a 16-bit storage dtype without a rounding."""
    seen = set()
    for c in _host_cases():
        for dtype in c.dtypes:
            key = (c.cin, c.cout, c.k, c.shape, c.act, c.slope, c.bias, c.film, c.mul, c.res, c.scale, c.sums, c.gated, c.out_mode, c.crop, c.out_dtype, dtype)
            if c.act == "gelu" or key in seen:
                continue
            seen.add(key)
            d = R.exact_data(c, dtype)
            r64, r32 = R.ref64_conv(c, d, dtype), R.ref64_conv(c, d, dtype, prec=torch.float32)
            assert r32["out"].dtype == torch.float32 and torch.equal(r32["out"].double(), r64["out"]), (c.name, dtype)
            frac = 2.0 ** (1 + (6 if R.carries_fractions(c) else 0) + (2 if c.act == "leaky" else 0))
            if c.sums and not R.carries_fractions(c):
                assert torch.equal(r32["sums"].double(), r64["sums"]), (c.name, dtype)              # large maps, integer data: even the whole total is exact in fp32
            elif c.sums:
                B, H, W = c.shape                                                                     # small maps: per-tile slots (rc_conv_sum_tiles is the smaller layout
                assert B * -(-H // 8) * -(-W // 32) <= 64                                            # below 64 tiles), 64 pixels a wave: each slot's partial sum is exact
                assert 64 * float(r64["out"].abs().max()) * frac < 2.0 ** 24, (c.name, dtype)
            assert R.exact_headroom(c, d, dtype) < 2.0 ** 24, (c.name, dtype, R.exact_headroom(c, d, dtype))
            nz, rnd = R.shares(r64["out"], G.out_dtype_of(c, dtype))
            if R.carries_fractions(c):
                assert nz >= 0.5, (c.name, dtype, nz)
                if G.out_dtype_of(c, dtype) != "f32":
                    assert rnd >= 0.5, (c.name, dtype, rnd)


def test_a_truncated_store_fails_both_regimes_checks():
    """The exact regime pins round-to-nearest-even: a truncated (round-toward-zero) bf16 store of the same reference has other bits, and within_rounding refuses it."""
    c = Case("t", 48, 48)
    d = R.exact_data(c, "bf16")
    ref = R.ref64_conv(c, d, "bf16")["out"]
    rne = R.round_to(ref, torch.bfloat16)
    trunc = (ref.float().view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()
    assert float((rne != trunc).double().mean()) > 0.2 and not R.same_bits(rne, trunc)
    assert bool(R.within_rounding(rne, ref, torch.zeros_like(ref), torch.bfloat16).all())
    assert float((~R.within_rounding(trunc, ref, R.gamma(433) * ref.abs(), torch.bfloat16)).double().mean()) > 0.2


# ---- make_plan ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_of_the_layers_the_sources_name():
    """Anchors of the one rule table (conv_ref._rules) that plan() and plan_grid() both evaluate: the choices the comments of make_plan spell out."""
    want = {(48, 48, 3, "bf16", NHWC): (48, 3, 1, 1), (32, 32, 3, "f16", NHWC): (32, 2, 1, 1), (160, 224, 3, "bf16", NHWC): (32, 2, 5, 7), (80, 80, 1, "bf16", NHWC): (80, 5, 1, 1),
            (240, 64, 1, "bf16", NHWC): (80, 4, 3, 1), (128, 128, 3, "bf16", NHWC): (32, 4, 4, 2), (64, 64, 3, "bf16", NHWC): (64, 4, 1, 1), (4, 128, 3, "f32", NHWC): (4, 4, 1, 2),
            (48, 192, 3, "bf16", PS2): (48, 3, 1, 4), (48, 12, 5, "f16", PS2_NCHW): (48, 1, 1, 1), (256, 64, 2, "bf16", NHWC): (32, 4, 8, 1), (128, 128, 3, "f32", NCHW): (16, 4, 8, 2)}
    for (ci, co, ks, dt, om), (ck, nt, n_chunks, n_ct) in want.items():
        p = R.plan(ci, co, ks, dt, om)
        assert (p["ck"], p["nt"], p["n_chunks"], p["n_ct"]) == (ck, nt, n_chunks, n_ct), (ci, co, ks, dt, om, p)
        ok, cp, pb, gck, gnt = R.plan_grid(ks, dt, om)
        assert ok[ci - 1, co - 1] and (cp[ci - 1, co - 1], pb[ci - 1, co - 1], gck[ci - 1, co - 1], gnt[ci - 1, co - 1]) == (p["cout_packed"], p["packed_bytes"], ck, nt)
    assert R.plan(128, 128, 3, "f32", NHWC, 16)["n_ct"] == 8 and R.plan(48, 48, 7, "bf16", NHWC) is None and R.plan(16, 32, 5, "f32", NHWC) is None


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("ksize", [1, 2, 3, 5])
def test_plan_restatement_against_the_library_for_every_cin_and_cout_up_to_640(ksize, dtype):
    """rc_conv_packed_cout_ct, rc_conv_packed_bytes_ct and their zero / error returns at every cin and cout in 1 .. 640, for every out_mode and cout_tile in
    {0, 16, 32, 48, 64, 80}."""
    lib = _lib.load()
    fb, fc = lib.rc_conv_packed_bytes_ct, lib.rc_conv_packed_cout_ct
    n = 640
    pts = [(ci, co) for ci in range(1, n + 1) for co in range(1, n + 1)]
    idx = np.array(pts) - 1
    for om in R.OUT_MODES:
        for ct in (0, 16, 32, 48, 64, 80):
            ok, cp, pb, _, _ = R.plan_grid(ksize, dtype, om, ct, n)
            dt = RC[dtype]
            got_b = np.fromiter((fb(ci, co, ksize, dt, om, ct) for ci, co in pts), dtype=np.int64, count=len(pts))
            got_c = np.fromiter((fc(ci, co, ksize, dt, om, ct) for ci, co in pts), dtype=np.int64, count=len(pts))
            exp_b, exp_c, exp_ok = pb[idx[:, 0], idx[:, 1]], cp[idx[:, 0], idx[:, 1]], ok[idx[:, 0], idx[:, 1]]
            bad = np.nonzero((got_b != exp_b) | (np.where(exp_ok, got_c, 0) != exp_c) | (~exp_ok & (got_c >= 0)))[0]
            assert bad.size == 0, (ksize, dtype, om, ct, [pts[i] for i in bad[:5]], got_b[bad[:5]], exp_b[bad[:5]], got_c[bad[:5]], exp_c[bad[:5]])
    for bad_ct in (8, 24, 96, -16):
        assert fb(64, 64, 3 if ksize in (2, 5) else ksize, RC[dtype], NHWC, bad_ct) == 0 and b"bad shape" in lib.rc_last_error()


# ---- packing -----------------------------------------------------------------------------------------------------------------------------------------------
def _bits(a, dtype):
    return a.view(np.float32) if dtype == "f32" else a.view(np.uint16)


def test_packers_on_every_case_of_the_gpu_table():
    """rc_conv_pack_weights_ct: the advertised size, exactly the multiset of storage-dtype-rounded weights plus zeros, and every lane's values from the output channel
    that packed_to_cout gives its MFMA row (the PixelShuffle order: conv channel 4c + sub).  rc_conv_pack_bias_ct likewise."""
    lib = _lib.load()
    seen = set()
    for c in _host_cases():
        for dtype in c.dtypes:
            key = (c.cin, c.cout, c.k, dtype, c.out_mode, c.cout_tile)
            if key in seen:
                continue
            seen.add(key)
            T, dt = R.DTYPES[dtype], RC[dtype]
            p = R.plan(c.cin, c.cout, c.k, dtype, c.out_mode, c.cout_tile)
            assert p is not None, key
            nbytes = lib.rc_conv_packed_bytes_ct(c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile)
            assert nbytes == p["packed_bytes"] and lib.rc_conv_packed_cout_ct(c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile) == p["cout_packed"], key
            # (a) the multiset, on real-valued weights
            w = R.values((c.cout, c.cin, c.k, c.k), torch.float32, 77, span=6, specials=False)
            wn = np.ascontiguousarray(w.numpy())
            guard = 64
            dst = np.full(nbytes + 2 * guard, 0xA5, np.uint8)
            assert lib.rc_conv_pack_weights_ct(wn.ctypes.data, c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile, dst[guard:].ctypes.data) == 0, key
            assert (dst[:guard] == 0xA5).all() and (dst[guard + nbytes:] == 0xA5).all(), key
            packed = _bits(dst[guard:guard + nbytes].copy(), dtype)
            want = w.to(T).contiguous()
            want = want.numpy() if dtype == "f32" else want.view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(np.sort(packed[packed != 0]), np.sort(want[want != 0].ravel())), key
            # (b) the row order, on weights that name their output channel
            w2 = (torch.arange(c.cout, dtype=torch.float32) + 1)[:, None, None, None].expand(c.cout, c.cin, c.k, c.k).contiguous()
            dst2 = np.zeros(nbytes, np.uint8)
            assert lib.rc_conv_pack_weights_ct(np.ascontiguousarray(w2.numpy()).ctypes.data, c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile, dst2.ctypes.data) == 0
            if dtype == "f32":
                v = torch.from_numpy(dst2.view(np.float32).copy())
            else:
                v = torch.from_numpy(dst2.view(np.int16).copy()).view(T).float()
            nt = p["nt"]
            v = v.reshape(p["n_ct"], p["n_chunks"], p["steps"], nt, 64, p["unit"])
            lane = torch.arange(64)
            m = lane & 15
            for ct in range(p["n_ct"]):
                for t in range(nt):
                    j = ct * 16 * nt + (m >> 2) * (4 * nt) + t * 4 + (m & 3)
                    ch = torch.tensor([R.packed_to_cout(p, c.cout, c.out_mode, int(x)) for x in j])
                    name = torch.where((ch >= 0) & (ch < c.cout), ch + 1, torch.zeros_like(ch)).float()
                    blk = v[ct, :, :, t]                                       # (chunks, steps, 64, unit)
                    assert bool(((blk == 0) | (blk == name[None, None, :, None])).all()), (key, ct, t)
                    live = blk.abs().amax(dim=(0, 1, 3)).reshape(4, 16).amax(0)      # over the four K groups of lanes (some hold no live unit on narrow chunks)
                    assert torch.equal(live, name[:16]), (key, ct, t)         # every named row does occur
            bias = np.arange(1, c.cout + 1, dtype=np.float32)
            pbias = np.full(p["cout_packed"] + 2, -7.0, np.float32)
            assert lib.rc_conv_pack_bias_ct(bias.ctypes.data, c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile, pbias[1:].ctypes.data) == 0
            exp = [R.packed_to_cout(p, c.cout, c.out_mode, j) for j in range(p["cout_packed"])]
            assert pbias[0] == -7.0 and pbias[-1] == -7.0 and np.array_equal(pbias[1:-1], np.array([e + 1 if 0 <= e < c.cout else 0 for e in exp], np.float32)), key


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------------------
def _parsed_instantiations():
    elem = {v: k for k, v in R.ELEM.items()}
    out = set()
    for f in glob.glob(os.path.join(ROOT, "realcamnet_amd", "csrc", "conv_inst_*.hip")):
        for t, ck, nt, ks in re.findall(r"launch_conv<ConvCfg<(\w+), (\d+), (\d+), (\d+)>>", open(f).read()):
            out.add((elem[t], int(ks), int(ck), int(nt)))
    return out


def test_every_reachable_instantiation_is_reached_by_a_gpu_case():
    parsed = _parsed_instantiations()
    assert len(parsed) == 92 and parsed == set(G.instantiations())
    reachable = set()
    for ks in (1, 2, 3, 5):
        for dt in ("f32", "bf16", "f16"):
            for om in R.OUT_MODES:
                for ct in (0, 16, 32, 48, 64, 80):
                    ok, _, _, ck, nt = R.plan_grid(ks, dt, om, ct)
                    reachable |= {(dt, ks, int(a), int(b)) for a, b in np.unique(np.stack([ck[ok], nt[ok]], 1), axis=0)}
    assert parsed - reachable == set(UNREACHABLE), sorted(parsed - reachable)
    reached = set()
    for c in G.all_cases():
        for dt in c.dtypes:
            p = R.plan(c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile)
            assert p is not None and (dt, c.k, p["ck"], p["nt"]) in parsed, (c.name, dt, p)       # a case must not ask for a kernel that does not exist
            reached.add((dt, c.k, p["ck"], p["nt"]))
    assert reached >= (parsed & reachable), sorted((parsed & reachable) - reached)


def test_coverage_table_of_the_gpu_file():
    """Every row names a test that exists; every epilogue key, generic form, staging path, store mode and persistent kernel has its row; every test of the file is named."""
    src = open(os.path.join(ROOT, "tests", "test_conv_gpu.py")).read()
    doc = src.split('"""')[1]
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", src, flags=re.M))
    rows = {m.group(1).strip(): m.group(2) for m in re.finditer(r"^  (\S.*?)\s{2,}(?:bf16|f16|f32).*?\s(test_[a-z0-9_]+)$", doc, flags=re.M)}
    assert len(rows) >= 40 and all(t in tests for t in rows.values()), sorted(t for t in rows.values() if t not in tests)
    assert set(rows.values()) == tests, sorted(tests - set(rows.values()))
    need = [f"key {k}" for k in G.FAST_KEYS] + ["generic gelu", "generic relu_post", "generic film", "generic film misaligned", "generic leaky slope", "generic res+relu",
                                                 "generic mul+res", "generic scale", "ragged cout", "scalar staging offset", "scalar staging cin", "scalar staging gated", "cin 4",
                                                 "ragged chunk", "planar NCHW", "planar PixelShuffle NCHW", "PixelShuffle NHWC", "ksize 2", "instantiation plain",
                                                 "instantiation relu+bias", "routes resident weights", "routes fp32"] + [f"several tiles kernel {k}" for k in (2, "2 resident", 3, 4, "4b", 6, 7)]
    assert not [r for r in need if r not in rows], [r for r in need if r not in rows]
    assert sorted(G.FAST_KEYS) == [0, 1, 2, 6, 8, 16, 32, 33, 34, 80]             # the switch in conv_build_args
    assert re.search(r"case 0: case 1: case 2: case 16: case 32: case 8: case 6: case 33: case 34: case 80: break;", open(os.path.join(ROOT, "realcamnet_amd", "csrc", "conv.hip")).read())
    assert {k for _, c, _ in G.multi_tile_cases() for k in [c.name.split("-")[1]]} == {"k2", "k2r", "k3", "k4", "k4b", "k6", "k7"}
    assert (R.TH, R.TW, R.WSM_TH) == tuple(int(re.search(rf"\b{n} = (\d+)", open(os.path.join(ROOT, "realcamnet_amd", "csrc", "conv_kernel.hpp")).read()).group(1))
                                           for n in ("kTH", "kTW", "kWsmTH"))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = _lib.ConvDesc()
    d.batch, d.height, d.width, d.cin, d.cout, d.ksize, d.dtype, d.out_dtype = 1, 16, 32, 48, 48, 3, RC_BF16, RC_BF16
    d.in0 = d.wpacked = d.out = 4096
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSALS = [
    (dict(act=4, residual=4096, film_scale=4096, film_shift=4096), b"RC_ACT_RELU_POST is relu(conv + residual)"),
    (dict(act=4, residual=4096, mul_plus1=4096), b"RC_ACT_RELU_POST is relu(conv + residual)"),
    (dict(act=4, residual=4096, chan_sums=4096), b"RC_ACT_RELU_POST is relu(conv + residual)"),
    (dict(act=4), b"needs residual"),
    (dict(cout=22, residual=4096), b"mul_plus1/residual need cout % 4 == 0"),
    (dict(cout=22, mul_plus1=4096), b"mul_plus1/residual need cout % 4 == 0"),
    (dict(residual=4096, out_mode=NCHW, out_h=16, out_w=32), b"mul_plus1/residual need cout % 4 == 0 and RC_OUT_NHWC"),
    (dict(mul_plus1=4096, out_mode=PS2, cout=192), b"mul_plus1/residual need cout % 4 == 0 and RC_OUT_NHWC"),
    (dict(out_scale=4098), b"out_scale must be 4-byte aligned"),
    (dict(out_scale=4096, out_mode=PS2, cout=192), b"out_scale needs RC_OUT_NHWC"),
    (dict(residual=4104), b"residual must be 16-byte aligned"),
    (dict(mul_plus1=4100), b"mul_plus1 must be 16-byte aligned"),
    (dict(out_mode=NCHW, out_h=0, out_w=32), b"bad NCHW crop"),
    (dict(out_mode=NCHW, out_h=17, out_w=32), b"bad NCHW crop"),
    (dict(out_mode=NCHW, out_h=16, out_w=33), b"bad NCHW crop"),
    (dict(out_mode=PS2_NCHW, out_h=33, out_w=64), b"bad pixel-shuffle NCHW crop"),
    (dict(out_mode=PS2_NCHW, out_h=32, out_w=0), b"bad pixel-shuffle NCHW crop"),
    (dict(out_mode=PS2_NCHW, out_h=32, out_w=64, chan_sums=4096), b"chan_sums needs RC_OUT_NHWC"),
    (dict(out_mode=NCHW, out_h=16, out_w=32, out_dtype=RC_F16), b"bad out_dtype"),
    (dict(out_mode=NCHW, out_h=16, out_w=32, dtype=RC_F16, out_dtype=RC_BF16), b"bad out_dtype"),
    (dict(out_dtype=RC_F32), b"out_dtype must equal dtype for RC_OUT_NHWC"),
    (dict(out=4104), b"out must be 16-byte aligned"),
    (dict(cin=64, cout=64, ksize=2, cout_tile=16), b"unsupported cin/cout/ksize/dtype/cout_tile"),
    (dict(cin=48, cout=16, ksize=5, cout_tile=16), b"unsupported cin/cout/ksize/dtype/cout_tile"),
    (dict(cout=192, out_mode=PS2, cout_tile=48), b"unsupported cin/cout/ksize/dtype/cout_tile"),
    (dict(cout=192, out_mode=PS2_NCHW, out_h=32, out_w=64, cout_tile=48), b"unsupported cin/cout/ksize/dtype/cout_tile"),
    (dict(cout_tile=24), b"unsupported cin/cout/ksize/dtype/cout_tile"),
    (dict(src_h=32, src_w=64), b"src_h/src_w need ksize 2"),
    (dict(cin=64, cout=64, ksize=2, src_h=32, src_w=64), b"src_h/src_w need ksize 2 and cin / 4 a whole number of Cin chunks"),
    (dict(cin=256, cout=64, ksize=2, src_h=33, src_w=64), b"height/width must be ceil(src_h / 2)"),
    (dict(cin=256, cout=64, ksize=2, src_h=32, src_w=0), b"height/width must be ceil(src_h / 2)"),
    (dict(cin=256, cout=64, ksize=2, src_h=32, src_w=64, in_gate=4096, in1=4096), b"src_h/src_w exclude the gated input"),
    (dict(cin=256, cout=64, ksize=2, src_h=32, src_w=64, in0=4098), b"src_h/src_w need a 16-byte aligned in0"),
    (dict(in_gate=4096), b"in_gate needs in1"),
    (dict(film_scale=4096), b"film_scale/film_shift must come together"),
    (dict(act=7), b"bad act"),
    (dict(batch=65536), b"batch > 65535"),
]


@pytest.mark.parametrize("kw,fragment", REFUSALS, ids=[f"{i}-{m[:28].decode().replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_conv_build_args_refusals(kw, fragment):
    """Asked through rc_conv_sum_slots: the same conv_build_args as rc_conv2d, and a description that were accepted by mistake is still never launched."""
    lib = _lib.load()
    assert lib.rc_conv_sum_slots(C.byref(_desc())) > 0                                     # the base description itself is fine
    assert lib.rc_conv_sum_slots(C.byref(_desc(**kw))) == -1, kw
    assert fragment in lib.rc_last_error(), (kw, lib.rc_last_error())
