"""No GPU: the yardsticks of tests/fused_ref.py against plain float64 compositions of torch's functionals and against each other; the CPU side of the sharpness
condition; the head-room of every exact-regime case test_fused_gpu.py launches; rc_lsc_pack's blob against the state-dict tensors; the argument checks of
rc_lsc_chain, rc_lsc_pack, rc_pointwise_chain48 and rc_conv_pair; the coverage table of test_fused_gpu.py against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_ref as R
import test_fused_gpu as G
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_ACT_LEAKY, RC_ACT_NONE, RC_ACT_RELU, RC_BF16, RC_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _bf(w):
    return w.float().to(BF16).double()


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


# ---- ref64 against the functionals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.LSC_WIDTHS)
def test_chain_references_are_the_float64_composition_of_conv2d_and_leaky_relu(c):
    for cin0, n_mid, raw_c, slope in ((2, 3, 4, 0.2), (3, 1, 1, 0.0), (1, 4, 3, 1.0), (4, 2, 0, 0.5)):
        raw_c = 0 if c == 128 else raw_c
        d = R.real_chain(c, cin0, n_mid, (2, 5, 9), slope, raw_c, 3)
        s = float(torch.tensor(slope, dtype=F32))
        v = F.leaky_relu(F.conv2d(_nchw(d["x"]), _bf(d["w0"]).reshape(c, cin0, 1, 1), d["b0"].double()), s)
        for l, (w, b) in enumerate(zip(d["wmid"], d["bmid"])):
            v = F.conv2d(v, _bf(w).reshape(c, c, 1, 1), b.double())
            v = F.leaky_relu(v, s) if l + 1 < n_mid else v
        if raw_c:
            h = F.conv2d(_nchw(d["raw"]), _bf(d["whead"]), d["bhead"].double(), padding=1)
            v = h * (v + 1)
        want = v.permute(0, 2, 3, 1)
        ref, slack, model = R.chain_yardsticks(d)
        tol = 1e-12 * (1 + want.abs().max())
        assert (ref - want).abs().max() <= tol
        if not raw_c and c == 48:
            a = (d["x"], d["w0"], d["b0"], d["wmid"], d["bmid"], slope)
            assert torch.equal(R.ref64_chain48(*a), ref) and torch.equal(R.slack64_chain48(*a), slack) and torch.equal(R.model64_chain48(*a), model)
        a = (d["x"], d["w0"], d["b0"], d["wmid"], d["bmid"], slope, d.get("whead"), d.get("bhead"), d.get("raw"))
        assert torch.equal(R.ref64_lsc_chain(*a), ref) and torch.equal(R.slack64_lsc_chain(*a), slack) and torch.equal(R.model64_lsc_chain(*a), model)


@pytest.mark.parametrize("mode", R.PAIR_MODES)
def test_pair_reference_is_two_float64_convolutions_with_a_zero_padded_mid(mode):
    f = R.pair_flags(mode)
    d = R.real_pair(mode, (2, 9, 11), 3)
    x = d["x"].float()
    if f["gated"]:
        x = (x * d["gate"][:, None, None, :] + d["skip"].float()).to(BF16).float()      # two fp32 roundings, one cast: what in_store holds
    v = F.conv2d(_nchw(x), _bf(d["w1"]), d["b1"].double(), padding=1)
    if f["film"]:
        fs, ft = d["fs"].double()[:, :, None, None], d["ft"].double()[:, :, None, None]
        v = F.leaky_relu(v * fs + ft + v, float(torch.tensor(d["slope"], dtype=F32)))
    else:
        v = F.relu(v)
    out = F.conv2d(v, _bf(d["w2"]), d["b2"].double(), padding=1)                         # padding=1 twice: mid is zero-padded by the second convolution
    if f["res"]:
        out = out + _nchw(d["res"])
    want = out.permute(0, 2, 3, 1)
    y = R.pair_yardsticks(d)
    assert (y["ref"] - want).abs().max() <= 1e-12 * (1 + want.abs().max())
    assert bool(R.within_rounding(R.round_to(y["model"], BF16), y["ref"], y["slack"], BF16).all())
    assert (y["stored"] is not None) == f["store"] and (y["sums"] is not None) == f["sums"]
    if f["store"]:
        assert R.same_bits(y["stored"], x.to(BF16))
    if f["sums"]:
        assert (y["sums"] - want.sum(dim=(1, 2))).abs().max() <= 1e-9 and tuple(y["sums"].shape) == (2, 48)
    assert torch.equal(R.ref64_conv_pair(d), y["ref"]) and torch.equal(R.slack64_conv_pair(d), y["slack"]) and torch.equal(R.model64_conv_pair(d), y["model"])


# ---- the fp32 restatement: inside the window, and under 0.1 % against the model ----------------------------------------------------------------------------------
def _share(val32, model64):
    return R.flip_share(R.round_to(val32, BF16), model64)[0]


def test_a_cpu_fp32_restatement_lies_inside_the_windows_and_under_a_tenth_of_a_percent():
    """For every input set test_fused_gpu.py holds to the 0.5 % cap: the same pipeline with fp32 tensors (torch's own summation order) lies inside slack64 of ref64
    everywhere and differs from round_to(model64) on at most 0.1 % of the bf16 values.  If a set exceeds it, change the set."""
    shares = {}
    for what, d in G.lsc_sharp_sets() + [G.chain48_sharp_set()]:
        ref, slack, model = R.chain_yardsticks(d)
        val = R.chain_restated32(d)
        assert bool(R.within_rounding(R.round_to(val, BF16), ref, slack, BF16).all()), what
        shares[what] = _share(val, model)
    for what, d in G.pair_sharp_sets():
        y = R.pair_yardsticks(d)
        val = R.model64_conv_pair(d, F32)
        assert bool(R.within_rounding(R.round_to(val, BF16), y["ref"], y["slack"], BF16).all()), what
        shares[what] = _share(val, y["model"])
    print({k: f"{100 * v:.4f} %" for k, v in shares.items()})
    assert all(v <= 1e-3 for v in shares.values()), shares


def test_restatements_of_every_real_valued_case_of_the_gpu_file_lie_inside_their_windows():
    inside = lambda val, ref, slack: bool(R.within_rounding(R.round_to(val, BF16), ref, slack, BF16).all())
    for k in G.lsc_parameter_cases() + G.lsc_shape_cases():
        for slope in (G.REAL_SLOPES if k in G.lsc_parameter_cases() else (0.2,)):
            d = G.lsc_data(k, slope, False)
            ref, slack, _ = R.chain_yardsticks(d)
            assert inside(R.chain_restated32(d), ref, slack), (k, slope)
    for k in G.chain48_cases():
        for slope in G.REAL_SLOPES:
            d = G.chain48_data(k, slope, False)
            ref, slack, _ = R.chain_yardsticks(d)
            assert inside(R.chain_restated32(d), ref, slack), (k, slope)
    for mode in R.PAIR_MODES:
        for i, shape in enumerate(G.PAIR_SHAPES):
            d = R.real_pair(mode, shape, i)
            y = R.pair_yardsticks(d)
            assert inside(R.model64_conv_pair(d, F32), y["ref"], y["slack"]), (mode, shape)


# ---- the exact regime ------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_exact_case_of_the_gpu_file_has_its_head_room():
    """Every exact-regime launch of test_fused_gpu.py (every width, n_mid, cin0, raw_c, slope, mode and shape it uses): each value at a rounding point is a bf16
    number, each accumulation stays below 2^24 units of the finest bit, so the fp32 pipeline reproduces the float64 one and a kernel may sum in any order.  And
    the data is worth the comparison: at least 15 % of the outputs are non-zero (a slope of 0 without biases zeroes the most; with biases it is over half)."""
    n = 0
    for name, d, kind in G.all_exact_sets():
        if kind == "chain":
            inexact, room = R.exact_headroom_chain(d)
            ref = R.chain_yardsticks(d)[0]
            assert torch.equal(R.chain_restated32(d).double(), ref), name
        else:
            inexact, room, slot = R.exact_headroom_pair(d)
            assert slot < 2.0 ** 24, (name, slot)
            ref = R.ref64_conv_pair(d)
            assert torch.equal(R.model64_conv_pair(d, F32).double(), ref), name
        assert inexact == 0 and room < 2.0 ** 24, (name, inexact, room)
        assert float((ref != 0).double().mean()) > 0.15, (name, "mostly zeros")
        n += 1
    assert n > 500


def test_exact_chain_rows_differ_per_tile_and_lane_group():
    """Every row of an exact mid-layer matrix is another row; the 16-channel tiles of layer 0, of the head and of the biases differ pairwise, the head's
    4-row lane groups likewise: a swapped tile, row group, tap or bias row changes the result."""
    blocks = lambda w, n: {tuple(b.flatten().tolist()) for b in w.reshape(w.shape[0] // n, n, -1)}
    for c in R.LSC_WIDTHS:
        for slope, n_mid in ((0.5, 2), (0.5, 4)):
            d = R.exact_chain(c, 2, n_mid, (1, 1, 4), slope, 0 if c == 128 else 4, 0)
            for w in d["wmid"]:
                assert len(blocks(w, 1)) == c, c
            assert len(blocks(d["w0"], 16)) == c // 16, c                        # (two columns and three values: too few patterns for every group of 4 rows)
            if c != 128:
                w = d["whead"].reshape(c, -1)
                assert len(blocks(w, 16)) == c // 16 and len(blocks(w, 4)) == c // 4, (c, len(blocks(w, 4)))
            for b in [d["b0"]] + d["bmid"] + ([d["bhead"]] if c != 128 else []):
                assert len(blocks(b[:, None], 16)) == c // 16, c
    d = R.exact_pair("plain", (1, 8, 32), 0)
    assert int((d["b1"] > 0).sum()) >= 8                                          # relu(b1) != 0 on several channels: conv1 on the padding ring would show


# ---- rc_lsc_pack ----------------------------------------------------------------------------------------------------------------------------------------------------
def _pack(lib, w0, b0, wmid, bmid, whead, bhead, c):
    arr = lambda t: None if t is None else np.ascontiguousarray(t.float().numpy())
    ptr = lambda a: None if a is None else a.ctypes.data
    keep = [arr(w0), arr(b0), [arr(w) for w in wmid], [arr(b) for b in bmid], arr(whead), arr(bhead)]
    n = len(wmid)
    wp = (C.c_void_p * n)(*[ptr(a) for a in keep[2]])
    bp = (C.c_void_p * n)(*[ptr(a) for a in keep[3]])
    size = lib.rc_lsc_packed_bytes(c, n, int(whead is not None))
    dst = np.full(size + 64, 0xAB, dtype=np.uint8)
    code = lib.rc_lsc_pack(ptr(keep[0]), ptr(keep[1]), w0.shape[1], wp, bp, n, ptr(keep[4]), ptr(keep[5]), 0 if whead is None else whead.shape[1], c, dst.ctypes.data)
    assert code == 0, lib.rc_last_error().decode()
    assert bool((dst[size:] == 0xAB).all()), "rc_lsc_pack wrote past rc_lsc_packed_bytes"
    return dst[:size].copy()


@pytest.mark.parametrize("c", R.LSC_WIDTHS)
def test_lsc_pack_blob_unpacks_to_the_state_dict_tensors_rounded_to_bf16(c):
    lib = _lib.load()
    i = 0
    for cin0 in (1, 2, 3, 4):
        for n_mid in (1, 2, 3, 4):
            for raw_c in (0, 1, 2, 3, 4):
                i += 1
                null_bias = i % 3 == 0
                d = R.real_chain(c, cin0, n_mid, (1, 1, 1), 0.2, raw_c, i)
                b0 = None if null_bias else d["b0"]
                bmid = [None if (null_bias and l % 2 == 0) else b for l, b in enumerate(d["bmid"])]
                bhead = None if (null_bias or not raw_c) else d["bhead"]
                blob = _pack(lib, d["w0"], b0, d["wmid"], bmid, d.get("whead"), bhead, c)
                assert blob.size == R.lsc_packed_bytes(c, n_mid, raw_c > 0)
                u = R.unpack_lsc_blob(blob, c, cin0, n_mid, raw_c)
                tag = (c, cin0, n_mid, raw_c, null_bias)
                assert u["padding_zero"], tag
                rb = lambda w: w.float().to(BF16).float()
                assert torch.equal(u["w0"], rb(d["w0"])), tag
                assert all(torch.equal(a, rb(w)) for a, w in zip(u["wmid"], d["wmid"])), tag
                assert (u["whead"] is None) == (raw_c == 0) and (raw_c == 0 or torch.equal(u["whead"], rb(d["whead"]))), tag
                want = [b0] + bmid + ([bhead] if raw_c else [])
                assert len(u["biases"]) == len(want)
                assert all(torch.equal(a, torch.zeros(c) if b is None else b) for a, b in zip(u["biases"], want)), tag


def test_lsc_packed_bytes_is_the_documented_sum():
    lib = _lib.load()
    for c in R.LSC_WIDTHS:
        for n_mid in (1, 2, 3, 4):
            for head in (0, 1):
                assert lib.rc_lsc_packed_bytes(c, n_mid, head) == R.lsc_packed_bytes(c, n_mid, bool(head)), (c, n_mid, head)
    assert R.lsc_packed_bytes(48, 3, True) == 3 * 512 + 3 * 3 * 1536 + 3 * 1536 + 5 * 48 * 4
    assert all(lib.rc_lsc_packed_bytes(c, 3, 0) == 0 for c in (0, 16, 40, 96, 256)) and lib.rc_lsc_packed_bytes(48, 0, 0) == 0


# ---- argument checks (no GPU: every call must be refused by the entry point's own check, before a launch) ----------------------------------------------------------
P_, Q_ = 4096, 4100          # dummy device pointers: 16-byte aligned / not


def _bad_calls(lib):
    A, B = P_, Q_
    t = []
    lc = lambda **k: ("rc_lsc_chain", tuple({**dict(x=A, cin0=2, blob=A, c=48, n_mid=3, slope=0.2, raw=None, raw_c=0, out=A, b=1, H=4, W=4, st=None), **k}.values()))
    t += [lc(c=w) for w in (0, 16, 40, 96, 256)] + [lc(c=128, raw=A, raw_c=4), lc(slope=-0.01), lc(slope=1.5), lc(slope=float("nan")), lc(out=B), lc(blob=B),
                                                     lc(cin0=0), lc(cin0=5), lc(raw=A, raw_c=0), lc(raw=A, raw_c=5), lc(n_mid=0), lc(n_mid=5), lc(x=None), lc(blob=None),
                                                     lc(out=None), lc(b=0), lc(H=0), lc(W=0), lc(b=64, H=2048, W=2048), lc(b=1, H=16384, W=16384)]
    z = np.zeros(128 * 128, dtype=np.float32)
    zp = z.ctypes.data
    one = (C.c_void_p * 4)(zp, zp, zp, zp)
    hole = (C.c_void_p * 4)(zp, None, zp, zp)
    nob = (C.c_void_p * 4)(None, None, None, None)
    dst = np.zeros(1 << 20, dtype=np.uint8)
    lp = lambda **k: ("rc_lsc_pack", tuple({**dict(w0=zp, b0=None, cin0=2, wmid=one, bmid=nob, n_mid=3, wh=None, bh=None, raw_c=0, c=48, dst=dst.ctypes.data), **k}.values()))
    t += [lp(c=w) for w in (0, 16, 40, 96, 256)] + [lp(cin0=0), lp(cin0=5), lp(n_mid=0), lp(n_mid=5), lp(wh=zp, raw_c=0), lp(wh=zp, raw_c=5), lp(w0=None), lp(wmid=None),
                                                     lp(bmid=None), lp(dst=None), lp(wmid=hole)]
    dw = (C.c_void_p * 4)(A, A, A, A)
    dwh = (C.c_void_p * 4)(A, A, None, A)
    db = (C.c_void_p * 4)(None, None, None, None)
    pc = lambda **k: ("rc_pointwise_chain48", tuple({**dict(x=A, cin0=2, w0=A, b0=None, w=dw, b=db, n_mid=3, slope=0.2, out=A, dt=RC_BF16, px=64, st=None), **k}.values()))
    t += [pc(x=None), pc(w0=None), pc(out=None), pc(w=None), pc(b=None), pc(dt=RC_F32), pc(cin0=0), pc(cin0=9), pc(n_mid=0), pc(n_mid=5), pc(px=0), pc(slope=-0.01),
          pc(slope=1.01), pc(out=B), pc(w=dwh)]
    keep = []

    def cp(impl=0, **k):
        d = _lib.ConvPairDesc()
        base = dict(batch=1, height=8, width=32, channels=48, dtype=RC_BF16, in0=A, w1=A, w2=A, out=A, act1=RC_ACT_RELU, act1_slope=0.0)
        for key, v in {**base, **k}.items():
            setattr(d, key, v)
        keep.append(d)
        return ("rc_conv_pair", (C.byref(d), None), impl)
    film = dict(act1=RC_ACT_LEAKY, film_scale=A, film_shift=A, act1_slope=0.5)
    t += [("rc_conv_pair", (None, None)), cp(channels=32), cp(channels=64), cp(dtype=RC_F32), cp(batch=0), cp(height=0), cp(width=0), cp(in0=None), cp(w1=None), cp(w2=None),
          cp(out=None), cp(act1=RC_ACT_NONE), cp(act1=3), cp(act1=RC_ACT_LEAKY), cp(act1=RC_ACT_LEAKY, film_scale=A), cp(**{**film, "act1_slope": -0.5}),
          cp(**{**film, "act1_slope": 1.5}), cp(**film, in_gate=A, in1=A), cp(**film, chan_sums=A), cp(film_scale=A, film_shift=A), cp(film_shift=A), cp(residual=A),
          cp(in_gate=A), cp(in0=B), cp(in_gate=A, in1=B), cp(in_gate=A, in1=A, in_store=B), cp(out=B), cp(**film, residual=B), cp(**{**film, "film_scale": B}),
          cp(**{**film, "film_shift": B}), cp(height=4096, width=4096), cp(batch=70000, height=64, width=1024), cp(impl=2, batch=49, in_gate=A, in1=A)]
    return t, (z, dst, one, hole, nob, dw, dwh, db, keep)


def test_bad_arguments_of_the_fused_entry_points_are_refused_before_any_launch():
    lib = _lib.load()
    calls, keep = _bad_calls(lib)
    assert {c[0] for c in calls} == {"rc_lsc_chain", "rc_lsc_pack", "rc_pointwise_chain48", "rc_conv_pair"}
    try:
        for name, args, *impl in calls:
            assert lib.rc_debug_set(b"pair_impl", impl[0] if impl else 0) == 0
            lib.rc_bayer_unshuffle(None, 0, None, 0, 1, 4, 4, 4, 4, None)       # leaves another entry point's message behind
            code = getattr(lib, name)(*args)
            msg = lib.rc_last_error().decode()
            assert code == -1 and name in msg, (name, args, code, msg)           # RC_ERR_INVALID from the entry point's own check, not a failed launch
    finally:
        lib.rc_debug_set(b"pair_impl", 0)


# ---- the coverage table of the GPU file ----------------------------------------------------------------------------------------------------------------------------
def test_every_fused_entry_point_is_in_the_gpu_files_coverage_table():
    """Every rc_lsc_* / rc_pointwise_chain48 / rc_conv_pair* symbol of the header has a row in the docstring of test_fused_gpu.py, the tests the rows name exist
    and the file calls the entry point; every kernel form, loader, pair_impl and mode the issue names is reached by a case of the tables."""
    header = open(os.path.join(ROOT, "include", "realcam_hip.h")).read()
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    mine = {n for n in declared if n.startswith("rc_lsc_") or n.startswith("rc_conv_pair") or n == "rc_pointwise_chain48"}
    assert len(mine) == 7, sorted(mine)
    gpu = open(os.path.join(ROOT, "tests", "test_fused_gpu.py")).read()
    doc = gpu.split('"""')[1]
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", gpu, flags=re.M))
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\s*(rc_[a-z0-9_]+)\s.*?\s(test_[a-z0-9_]+)$", doc, flags=re.M)}
    assert set(rows) == mine, (sorted(mine - set(rows)), sorted(set(rows) - mine))
    named = set(re.findall(r"\b(test_[a-z0-9_]+)$", doc, flags=re.M))
    assert named <= tests, sorted(named - tests)
    body = gpu.split('"""', 2)[2]
    called = set(re.findall(r"\b(rc_[a-z0-9_]+)\b", body)) | {"rc_" + n for n in re.findall(r"\b_R\.([a-z0-9_]+)\(", body)}
    called |= {"rc_pointwise_chain48"} if "torch_ops._chain_launch(" in body else set()
    called |= {"rc_conv_pair"} if "torch_ops._pair_launch(" in body else set()
    assert mine <= called, sorted(mine - called)
    ks = G.lsc_shape_cases() + G.lsc_parameter_cases()
    assert {(k["c"], k["raw_c"] > 0) for k in ks} == set(G.LSC_FORMS)
    fast = lambda k: k["cin0"] == 2 and k["raw_c"] in (0, 4) and k["shape"][2] >= 64                # lsc_chain_kernel's `fast`
    for c, head in G.LSC_FORMS:
        assert {fast(k) for k in ks if (k["c"], k["raw_c"] > 0) == (c, head)} == {True, False}, (c, head)
    for c in (48, 64):
        sel = [k for k in ks if k["c"] == c]
        assert {k["cin0"] for k in sel} == {1, 2, 3, 4} and {k["n_mid"] for k in sel} == {1, 2, 3, 4} and {k["raw_c"] for k in sel} == {0, 1, 3, 4}
        assert any(not k["bias"] for k in sel)
    c48 = G.chain48_cases()
    assert {k["pixels"] for k in c48} == {1, 63, 64, 65, 257} and {k["cin0"] for k in c48} == {1, 2, 4, 8} and {k["n_mid"] for k in c48} == {1, 2, 3, 4}
    assert any(not k["bias"] for k in c48)
    assert set(G.PAIR_SHAPES) == {(1, 1, 1), (1, 8, 32), (1, 9, 33), (2, 7, 31), (3, 5, 7), (1, 17, 65)}
    forms = {(f["gated"], f["film"], "sums" if f["sums"] else "res" if f["res"] else "plain") for f in map(R.pair_flags, R.PAIR_MODES)}
    assert forms == {(False, False, "plain"), (False, False, "sums"), (True, False, "plain"), (True, False, "sums"), (False, True, "plain"), (False, True, "res")}
    assert {R.pair_flags(m)["store"] for m in R.PAIR_MODES if R.pair_flags(m)["gated"]} == {True, False}
