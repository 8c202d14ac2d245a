"""Defective-pixel correction (Defects / DefectMap / rc_raw_defects), CPU side: the elementwise torch restatement of the header's arithmetic
(the GPU tests import it), a frame computed by hand, the selectivity condition, validation, the bitmap layout, the C entry's bad-argument
table, FakeTensorMode traces and the kernels' resources."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd import raw2bit as RB
from realcamnet_amd.defects import DefectMap, Defects

RING = ((0, -2), (0, 2), (-2, 0), (2, 0), (-2, -2), (-2, 2), (2, -2), (2, 2))      # (dy, dx) of W, E, N, S, NW, NE, SW, SE
PAIRS = ((0, 1), (2, 3), (4, 7), (5, 6))                                           # H, V, D1, D2 as ring indices


def restated_defects(mosaic, blacks, map_mask, hot, cold):
    """include/realcam_hip.h, rc_raw_defects, step for step in elementwise fp32 torch.  mosaic (B,H,W): counts (any integer dtype) or a float
    dtype; blacks: four levels in CFA-position order; map_mask (H,W) bool or None; hot / cold: None or (t_abs, t_rel).
    Returns (corrected, counts): uint16 for counts and the source dtype for float; counts (B,3) int64: mapped, hot, cold."""
    is_float = mosaic.dtype.is_floating_point
    v = mosaic.to(torch.float32) if is_float else mosaic.to(torch.int64).to(torch.float32)
    b, h, w = v.shape
    dev = v.device
    mapped = torch.zeros(h, w, dtype=torch.bool, device=dev) if map_mask is None else map_mask.to(dev).bool()
    vp = F.pad(v, (2, 2, 2, 2))
    gp = F.pad(~mapped, (2, 2, 2, 2), value=False)                                 # good: inside the frame and not in the map
    ring = [vp[:, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w] for dy, dx in RING]
    good = [gp[2 + dy:2 + dy + h, 2 + dx:2 + dx + w].unsqueeze(0).expand(b, h, w) for dy, dx in RING]
    ys, xs = torch.arange(h, device=dev), torch.arange(w, device=dev)
    black = torch.tensor(blacks, dtype=torch.float32, device=dev)[(2 * (ys & 1))[:, None] + (xs & 1)[None, :]].unsqueeze(0)
    mapped = mapped.unsqueeze(0).expand(b, h, w)

    # 1. mapped samples: the whole pair that differs least (first on a tie), else the first good neighbour, else unchanged
    have = torch.zeros(b, h, w, dtype=torch.bool, device=dev)
    best = torch.zeros_like(v)
    fixed = v.clone()
    for ia, ib in PAIRS:
        d = (ring[ia] - ring[ib]).abs()
        take = good[ia] & good[ib] & (~have | (d < best))
        best = torch.where(take, d, best)
        fixed = torch.where(take, (ring[ia] + ring[ib]) * 0.5, fixed)
        have = have | take
    single = torch.zeros(b, h, w, dtype=torch.bool, device=dev)
    for i in range(7, -1, -1):
        t = good[i] & ~have
        fixed = torch.where(t, ring[i], fixed)
        single = single | t
    replaced = mapped & (have | single)

    # 2. the others: hot against the good ring's maximum, otherwise cold against its minimum
    some = good[0]
    for g in good[1:]:
        some = some | g
    inf = torch.full_like(v, float("inf"))
    hi, lo = -inf, inf
    for r, g in zip(ring, good):
        hi = torch.maximum(hi, torch.where(g, r, -inf))
        lo = torch.minimum(lo, torch.where(g, r, inf))
    live = some & ~mapped
    is_hot = torch.zeros_like(live)
    is_cold = torch.zeros_like(live)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)               # noqa: E731
    if hot is not None:
        t = f32(hot[0]) + f32(hot[1]) * (hi - black).clamp_min(0.0)
        is_hot = live & ((v - hi) > t)
    if cold is not None:
        t = f32(cold[0]) + f32(cold[1]) * (lo - black).clamp_min(0.0)
        is_cold = live & ~is_hot & ((lo - v) > t)
    out = torch.where(replaced, fixed, v)
    out = torch.where(is_hot, hi, out)
    out = torch.where(is_cold, lo, out)

    # 3. the store
    out = out.to(mosaic.dtype) if is_float else out.round().to(torch.int32).to(torch.uint16)
    counts = torch.stack([replaced.sum((1, 2)), is_hot.sum((1, 2)), is_cold.sum((1, 2))], dim=1).to(torch.int64)
    return out, counts


# ---- 1. a frame computed by hand ----------------------------------------------------------------------------------------------------------
# The four colour classes of the mosaic never meet, so each hosts its own cases.  blacks (16, 32, 48, 64); hot = cold = (64, 0.5): every
# sample that is not planted lies within 53 of its ring and t >= 64, so nothing else is touched.
#   (even y, even x)  (2,2) mapped: H |390 - 430| = 40, V |404 - 408| = 4, D1 |360 - 400| = 40, D2 |400 - 450| = 50: V wins, (404 + 408) / 2 = 406.
#   (odd y, odd x)    (3,3) mapped: H |410 - 420| = 10 ties with V |395 - 405| = 10 (D1 20, D2 30): H wins, 415 (V would give 400).
#                     (7,7) mapped, a corner: no pair is whole; W (7,5) is mapped, E is outside, N (5,7) = 388 is the first good one.
#                     (7,5) mapped: E (7,7) is mapped, S / SE / SW are outside: W (7,3) = 377.
#   (odd y, even x)   (5,2) mapped with all eight ring neighbours mapped: unchanged (4095), not counted; of those eight, (5,0), (7,0) and
#                     (7,2) have no good neighbour either and stay; (3,0) -> N (1,0) = 411; (3,2) -> N (1,2) = 401; (5,4) -> E (5,6) = 404;
#                     (7,4) -> E (7,6) = 407; (3,4): D1 is its only whole pair, (401 + 404) / 2 = 402.5 -> 402, half to even.
#   (even y, odd x)   black 32.  (2,3) = 1000: hi = 420, t = 64 + 0.5 (420 - 32) = 258, 580 > 258: hot -> 420.
#                     (6,1) = 100: lo = 400, t = 64 + 0.5 (400 - 32) = 248, 300 > 248: cold -> 400.
#                     (0,7) = 678: hi = 420, t = 258, v - hi = 258 == t: not replaced.
HAND_IN = [[360, 400, 404, 400, 400, 400, 400, 678],
           [411, 400, 401, 395, 400, 400, 400, 400],
           [390, 400, 4095, 1000, 430, 420, 400, 400],
           [4095, 410, 0, 0, 4095, 420, 400, 400],
           [450, 400, 408, 400, 400, 400, 400, 400],
           [0, 430, 4095, 405, 0, 420, 404, 388],
           [400, 100, 400, 400, 400, 400, 400, 400],
           [4095, 400, 0, 377, 4095, 4095, 407, 4095]]
HAND_OUT = [[360, 400, 404, 400, 400, 400, 400, 678],
            [411, 400, 401, 395, 400, 400, 400, 400],
            [390, 400, 406, 420, 430, 420, 400, 400],
            [411, 410, 401, 415, 402, 420, 400, 400],
            [450, 400, 408, 400, 400, 400, 400, 400],
            [0, 430, 4095, 405, 404, 420, 404, 388],
            [400, 400, 400, 400, 400, 400, 400, 400],
            [4095, 400, 0, 377, 407, 377, 407, 388]]
HAND_MAP = [(2, 2), (3, 3), (7, 5), (7, 7), (3, 0), (3, 2), (3, 4), (5, 0), (5, 2), (5, 4), (7, 0), (7, 2), (7, 4)]
HAND_BLACKS = (16.0, 32.0, 48.0, 64.0)
HAND_COUNTS = [9, 1, 1]


def test_restatement_matches_the_frame_computed_by_hand():
    src = torch.tensor(HAND_IN, dtype=torch.int32).unsqueeze(0)
    dmap = DefectMap.from_coords((8, 8), HAND_MAP)
    out, counts = restated_defects(src, HAND_BLACKS, dmap.mask(), (64.0, 0.5), (64.0, 0.5))
    assert out.dtype == torch.uint16 and out.to(torch.int32)[0].tolist() == HAND_OUT
    assert counts.tolist() == [HAND_COUNTS]
    # the same frame as floats in [0, 1) scale (x / 4096 is exact in fp32, thresholds scaled alike): the .5 is kept, nothing rounds
    f = src.to(torch.float32) / 4096.0
    outf, cf = restated_defects(f, tuple(v / 4096.0 for v in HAND_BLACKS), dmap.mask(), (64.0 / 4096.0, 0.5), (64.0 / 4096.0, 0.5))
    want = torch.tensor(HAND_OUT, dtype=torch.float32)
    want[3, 4] = 402.5
    assert torch.equal(outf[0] * 4096.0, want) and cf.tolist() == [HAND_COUNTS]
    # each stage alone
    only_map, c = restated_defects(src, HAND_BLACKS, dmap.mask(), None, None)
    assert c.tolist() == [[9, 0, 0]] and only_map[0, 2, 3] == 1000 and only_map[0, 6, 1] == 100 and only_map[0, 3, 4] == 402
    only_hot, c = restated_defects(src, HAND_BLACKS, None, (64.0, 0.5), None)
    assert only_hot[0, 2, 3] == 420 and only_hot[0, 6, 1] == 100 and c[0, 0] == 0 and c[0, 2] == 0 and c[0, 1] >= 1


# ---- 2. selectivity: a condition on the inputs ----------------------------------------------------------------------------------------------
def planted_ramp(h=48, w=60, g=3, n=2, t_abs=20.0, t_rel=0.125, seed=5):
    """A ramp of gradient g per step plus noise within +-n, with hot / cold samples planted on a lattice of step 6 (no two inside one ring).
    A ring neighbour is at most 2 steps away on each axis: it differs by at most 4 g + 2 n = 16 < t_abs, so no unplanted sample can be
    replaced; t <= t_abs + t_rel range with range < 4096, and the offset 600 exceeds t_abs + 512 + 16 = 548."""
    assert 4 * g + 2 * n < t_abs
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    base = 1000 + g * (ys + xs) + torch.randint(-n, n + 1, (h, w), generator=gen)
    offset = 600
    assert offset > t_abs + t_rel * 4096 + 4 * g + 2 * n and int(base.max()) + offset < 4096 and int(base.min()) - offset >= 0
    frame = base.clone()
    hot, cold = [], []
    for i, y in enumerate(range(1, h, 6)):
        for j, x in enumerate(range(2, w, 6)):
            if (i + j) % 2:
                frame[y, x] += offset
                hot.append((y, x))
            else:
                frame[y, x] -= offset
                cold.append((y, x))
    return base, frame, hot, cold, (t_abs, t_rel)


def test_exactly_the_planted_samples_are_replaced():
    base, frame, hot, cold, thr = planted_ramp()
    out, counts = restated_defects(frame.unsqueeze(0).to(torch.int32), (64.0, 64.0, 64.0, 64.0), None, thr, thr)
    out = out[0].to(torch.int64)
    changed = {(int(y), int(x)) for y, x in (out != frame).nonzero().tolist()}
    assert changed == set(hot) | set(cold) and counts.tolist() == [[0, len(hot), len(cold)]] and len(hot) > 20 and len(cold) > 20
    for y, x in hot + cold:                                     # ... by a value of the neighbourhood: within 4 g + 2 n of what was there
        assert abs(int(out[y, x]) - int(base[y, x])) <= 16


# ---- 3. validation ------------------------------------------------------------------------------------------------------------------------
def test_defects_validation():
    m = DefectMap.from_coords((8, 12), [(0, 0), (7, 11), (0, 0)])
    assert m.count == 2 and m.size == (8, 12) and m == DefectMap.from_coords((8, 12), [(7, 11), (0, 0)]) and hash(m) == hash(DefectMap.from_coords((8, 12), [(7, 11), (0, 0)]))
    assert Defects(map=m).flags == 0 and Defects(hot=(1, 0)).flags == _lib.RC_DEFECT_HOT and Defects(cold=(0, 0.5)).flags == _lib.RC_DEFECT_COLD
    assert Defects(map=m, hot=(1, 2), cold=(3, 4), counts=True).thresholds() == (1.0, 2.0, 3.0, 4.0)
    with pytest.raises(ValueError):
        Defects()
    with pytest.raises(ValueError):
        Defects(counts=True)
    for bad in ((-1.0, 0.0), (0.0, -0.5), (float("inf"), 0.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            Defects(hot=bad)
        with pytest.raises(ValueError):
            Defects(cold=bad)
    for bad in (1.0, (1.0,), (1.0, 2.0, 3.0), ("a", 1.0), (True, 1.0)):
        with pytest.raises(TypeError):
            Defects(hot=bad)
    with pytest.raises(TypeError):
        Defects(map=torch.zeros(8, 8, dtype=torch.bool))
    with pytest.raises(TypeError):
        Defects(hot=(1.0, 0.0), counts=1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        Defects(hot=(1.0, 0.0)).hot = None
    with pytest.raises(AttributeError):
        m.size = (2, 2)
    for size in ((7, 8), (8, 0), (8, 9), (0, 8)):
        with pytest.raises(ValueError):
            DefectMap.from_coords(size, [])
    with pytest.raises(TypeError):
        DefectMap.from_coords((8.0, 8), [])
    for c in ((8, 0), (0, 12), (-1, 0)):
        with pytest.raises(ValueError):
            DefectMap.from_coords((8, 12), [c])
    for c in ((0,), (0.5, 1), "ab"):
        with pytest.raises(TypeError):
            DefectMap.from_coords((8, 12), [c])
    with pytest.raises(TypeError):
        DefectMap.from_mask(torch.zeros(8, 8))
    with pytest.raises(ValueError):
        DefectMap.from_mask(torch.zeros(2, 8, 8, dtype=torch.bool))
    with pytest.raises(ValueError):
        DefectMap((8, 12), np.full((8, 1), 1 << 12, dtype=np.uint32))      # a bit past the last column
    # RawFormat carries it; the size is checked against the mosaic
    fmt = M.RawFormat(storage="u16", white_level=1023.0, defects=Defects(map=m, hot=(8, 0.1)))
    assert fmt.validate((2, 8, 12)) == (8, 12)
    with pytest.raises(ValueError, match="map"):
        fmt.validate((2, 8, 16))
    with pytest.raises(TypeError):
        M.RawFormat(defects="all").validate((2, 8, 12))
    assert M.RawFormat().defects is None and "DefectMap" in M.__all__ and "Defects" in M.__all__ and "raw_defects" in M.torch_ops.SCHEMAS


def test_map_bitmap_layout_is_the_headers():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(10, 70, generator=g) < 0.2
    m = DefectMap.from_mask(mask)
    assert m.words.dtype == np.uint32 and m.words.shape == (10, 3) and m.pitch_bytes == 12 and not m.words.flags.writeable
    for y in range(10):
        for x in range(70):
            assert bool((int(m.words[y, x >> 5]) >> (x & 31)) & 1) == bool(mask[y, x])       # bit x & 31 of dword x >> 5 of row y
    assert not (m.words[:, 2] >> np.uint32(70 - 64)).any()                                   # nothing past the last column
    assert torch.equal(m.mask(), mask) and m.count == int(mask.sum())
    assert m == DefectMap.from_coords((10, 70), [tuple(c) for c in mask.nonzero().tolist()]) == DefectMap.from_mask(mask.numpy())


def test_forward_mosaic_refuses_a_map_of_the_wrong_size():
    with FakeTensorMode():
        with torch.device("cuda"):
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(2, 1, 64, 80, dtype=torch.uint8), torch.empty(2, 2, 32, 32)
            fmt = M.RawFormat(storage="mipi10", width=64, white_level=1023.0, defects=Defects(map=DefectMap.from_coords((64, 68), [(1, 1)])))
            with pytest.raises(ValueError, match="map"):
                net.forward_mosaic(mosaic, None, coord, raw_format=fmt)
            with pytest.raises(ValueError, match="raw_defects"):        # the ingest alone does not correct: it refuses rather than ignore the request
                M.ops.raw_ingest(mosaic, dtype=torch.float32, raw_format=dataclasses.replace(fmt, defects=Defects(hot=(1.0, 0.0))))
            with pytest.raises(TypeError):
                M.ops.raw_defects(mosaic, M.RawFormat(storage="mipi10", width=64, white_level=1023.0))     # nothing asked for
            with pytest.raises(TypeError):
                M.ops.raw_defects(mosaic.to(torch.int32), dataclasses.replace(fmt, defects=None), Defects(hot=(1.0, 0.0)))


# ---- 4. traces ----------------------------------------------------------------------------------------------------------------------------
def test_fake_trace_of_forward_mosaic_with_defects():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                dm = DefectMap.from_coords((144, 208), [(0, 0), (143, 207), (70, 100)])
                spec = Defects(map=dm, hot=(24.0, 0.1), cold=(24.0, 0.1), counts=True)
                fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=1023.0, defects=spec)
                mosaic, coord = torch.empty(2, 1, 144, 272, dtype=torch.uint8), torch.empty(2, 2, 72, 104)
                net = M.LiteISPNet_GFM_LSC().eval()
                with torch.no_grad():
                    y = net.forward_mosaic(mosaic, None, coord, raw_format=fmt)
                assert y.shape == (2, 3, 144, 208) and y.dtype == torch.bfloat16
                assert net.defect_counts.shape == (2, 3) and net.defect_counts.dtype == torch.int64 and net.defect_counts.device.type == "cuda"
                fixed, counts = M.ops.raw_defects(mosaic, fmt)
                assert fixed.shape == (2, 144, 208) and fixed.dtype == torch.uint16 and counts.shape == (2, 3)
                fl = M.ops.raw_defects(torch.empty(2, 144, 208), M.RawFormat(), Defects(cold=(0.1, 0.0)))
                assert fl.shape == (2, 144, 208) and fl.dtype == torch.bfloat16
                codec = RB.raw_compression_tcm_final(N=64).eval()
                dm2 = DefectMap.from_coords((512, 512), [(5, 5)])
                fmt2 = M.RawFormat(storage="mipi12", width=512, white_level=4095.0, defects=Defects(map=dm2, hot=(64.0, 0.1)))
                with torch.no_grad():
                    out = codec.forward_mosaic(torch.empty(2, 512, 768, dtype=torch.uint8), None, torch.empty(2, 2, 256, 256), raw_format=fmt2)
                assert isinstance(out, dict) and out["x_hat"].shape[0] == 2 and out["x_hat"].shape[-2:] == (512, 512)
                assert "defect_counts" not in codec.__dict__                       # counts were not asked for
        assert "_rc_cache" not in dm.__dict__                                     # a trace uploads and keeps nothing
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before anything is enqueued
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("width", dict(width=12), b"width"), ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("map pitch % 4", dict(map_pitch=6), b"map pitch"), ("map pitch short", dict(w=20, width=40, map_pitch=4), b"map pitch"), ("map pitch 0", dict(map_pitch=0), b"map pitch"),
    ("map misaligned", dict(map=FAKE + 2), b"4-byte"),
    ("dst pitch short", dict(dst_pitch=30), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=33), b"dst pitch"), ("dst misaligned", dict(dst=FAKE + 1), b"dst misaligned"),
    ("f32 dst misaligned", dict(storage=_lib.RC_RAW_F32, dst=FAKE + 2), b"dst misaligned"), ("counts misaligned", dict(counts=FAKE + 4), b"8-byte"),
    ("hot_abs < 0", dict(thr=(-1.0, 0, 0, 0)), b"thresholds"), ("hot_rel nan", dict(thr=(0, NAN, 0, 0)), b"thresholds"), ("cold_abs inf", dict(thr=(0, 0, INF, 0)), b"thresholds"),
    ("cold_rel < 0", dict(thr=(0, 0, 0, -0.5)), b"thresholds"),
    ("reserved", dict(reserved=(0, 1, 0)), b"reserved"), ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("flags", dict(flags=4), b"flags"),
    ("nothing enabled", dict(flags=0, map=None), b"nothing enabled"),
    ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
])
def test_raw_defects_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, map=FAKE, map_pitch=4, dst=FAKE, dst_pitch=0, counts=FAKE, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0, line_bytes=0,
              width=0, flags=3, thr=(1.0, 0.0, 1.0, 0.0), reserved=(0, 0, 0), fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], white=1.0, reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    t = kw["thr"]
    d = _lib.DefectDesc(flags=kw["flags"], hot_abs=t[0], hot_rel=t[1], cold_abs=t[2], cold_rel=t[3], reserved=(C.c_int32 * 3)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_defects(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["map"], kw["map_pitch"], kw["dst"], kw["dst_pitch"],
                              kw["counts"], kw["b"], kw["h"], kw["w"], None) == -1, case                        # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_raw_defects_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_defects", "rc_defect_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_defect_desc_size() == C.sizeof(_lib.DefectDesc) == 32
    header = _lib.HEADER.read_text()
    for name in ("RC_DEFECT_HOT", "RC_DEFECT_COLD"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert M.defects.WAVE_SPAN == 248 and M.defects.BLOCK_SPAN == 496 and M.defects.BLOCK_ROWS == 64 and M.defects.LANE_PX == 4
    src = (_lib.PKG / "csrc" / "defects.hip").read_text()                          # the constants the GPU tests place their seams on
    assert "kDfPx = 4" in src and "kDfSpan = 62 * kDfPx" in src and "kDfRows = 64" in src and "kDfStrips = kDfWaves / 2" in src


def test_raw_defects_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "defects.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "raw_defects_kernel" in k}
    assert len(mine) == 7, sorted(mine)                    # fp32, bf16, fp16, u16, u8, RAW10, RAW12
    assert all(v["tu"] == "defects.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 128 and v["sgprs"] <= 102 for v in mine.values())    # 4 waves per SIMD at least
    assert all(v["lds"] <= 64 for v in mine.values())                             # three counters: no LDS tile
    assert not [k for k, v in res.items() if v["tu"] == "defects.hip" and k not in mine]


# (vgprs, sgprs, agprs, scratch, lds, occupancy, vgpr_spill, sgpr_spill) of every ingest kernel, from a build of the commit before this stage
INGEST_KERNELS = {
    '_ZN2rc17raw_ingest_kernelIDF16_DF16_EEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIDF16_fEEvPKT_PT0_S5_iiiiiiiffff': (38, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIDF16bDF16_EEvPKT_PT0_S5_iiiiiiiffff': (37, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIDF16bDF16bEEvPKT_PT0_S5_iiiiiiiffff': (37, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIDF16bfEEvPKT_PT0_S5_iiiiiiiffff': (36, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIfDF16_EEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIfDF16bEEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelIffEEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelItDF16_EEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelItDF16bEEvPKT_PT0_S5_iiiiiiiffff': (39, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc17raw_ingest_kernelItfEEvPKT_PT0_S5_iiiiiiiffff': (38, 69, 0, 0, 0, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16_DF16_EEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16_DF16bEEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16_fEEvNS_10IngestArgsEPT1_S3_': (48, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16bDF16_EEvNS_10IngestArgsEPT1_S3_': (49, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16bDF16bEEvNS_10IngestArgsEPT1_S3_': (49, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EDF16bfEEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EfDF16_EEvNS_10IngestArgsEPT1_S3_': (48, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EfDF16bEEvNS_10IngestArgsEPT1_S3_': (48, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EffEEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EhDF16_EEvNS_10IngestArgsEPT1_S3_': (46, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EhDF16bEEvNS_10IngestArgsEPT1_S3_': (46, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EhfEEvNS_10IngestArgsEPT1_S3_': (48, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EtDF16_EEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EtDF16bEEvNS_10IngestArgsEPT1_S3_': (47, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi0EtfEEvNS_10IngestArgsEPT1_S3_': (48, 89, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi1EhDF16_EEvNS_10IngestArgsEPT1_S3_': (67, 87, 0, 0, 8192, 7, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi1EhDF16bEEvNS_10IngestArgsEPT1_S3_': (67, 87, 0, 0, 8192, 7, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi1EhfEEvNS_10IngestArgsEPT1_S3_': (68, 87, 0, 0, 8192, 7, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi2EhDF16_EEvNS_10IngestArgsEPT1_S3_': (61, 95, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi2EhDF16bEEvNS_10IngestArgsEPT1_S3_': (61, 95, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc21raw_ingest_fmt_kernelILi2EhfEEvNS_10IngestArgsEPT1_S3_': (61, 95, 0, 0, 8192, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIDF16_DF16_EEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIDF16_fEEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIDF16bDF16_EEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIDF16bDF16bEEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIDF16bfEEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIfDF16_EEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIfDF16bEEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
    '_ZN2rc22bayer_unshuffle_kernelIffEEvPKT_PT0_iiiii': (21, 43, 0, 0, 0, 8, 0, 0),
}


def test_ingest_kernels_are_unchanged():
    """The correction runs in front of the ingest and edits none of its kernels: their resource entries are the previous commit's."""
    from realcamnet_amd import build
    res = build.kernel_resources()
    now = {k: tuple(v.get(f, 0) for f in ("vgprs", "sgprs", "agprs", "scratch", "lds", "occupancy", "vgpr_spill", "sgpr_spill"))
           for k, v in res.items() if "raw_ingest" in k or "bayer_unshuffle_kernel" in k}
    assert now == INGEST_KERNELS
