"""RAW noise measurement (rc_raw_noise, ops.raw_noise, RawFormat.noise): what runs without a GPU.

The yardstick is tests/raw_noise_ref.py, a NumPy restatement of the arithmetic fixed in include/realcam_hip.h; here it is checked against a
plain Python loop over tiles and samples, the torch helpers of RawNoiseStats against their float64 NumPy restatement, and the estimator
itself against synthetic scenes of known noise (the figures and how the bounds were set: DESIGN.md 4.h).
"""
import ctypes as C
import dataclasses
import itertools
import math

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.raw_format import CFAS, SLOT_POS
from realcamnet_amd.raw_noise import chi2_quantile, ebin, ebin_range
import raw_noise_ref as R

NAN, INF = float("nan"), float("inf")


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------------------
def looped_raw_noise(values, cfa, blacks, top, spec):
    """Steps 1 to 6 of the header, one tile and one sample at a time, in Python integers."""
    v = np.asarray(values).astype(np.float32)
    B, H, W = v.shape
    S = (1 << spec.bits) - 1
    cy0, cx0, rh, rw = spec.check(H // 2, W // 2)
    T, L = spec.tile, spec.levels
    hist = np.zeros((B, 4, L, 320), dtype=np.int32)
    level = np.zeros((B, 4, L), dtype=np.int64)

    def code(b, y, x):
        pos = 2 * (y & 1) + (x & 1)
        p = np.float32(0) if np.isnan(v[b, y, x]) else v[b, y, x]
        black = np.float32(blacks[pos])
        k = np.float32(float(S) / (float(np.float32(top)) - float(black)))
        with np.errstate(over="ignore", invalid="ignore"):
            n = np.float32(np.float32(p - black) * k)
        return int(min(max(np.rint(n), -S), S))

    for b, c, ty, tx in itertools.product(range(B), range(4), range(rh // T), range(rw // T)):
        pos = SLOT_POS[cfa][c]
        q = [[code(b, 2 * (cy0 + T * ty + y) + pos // 2, 2 * (cx0 + T * tx + x) + pos % 2) for x in range(T)] for y in range(T)]
        flat = [x for row in q for x in row]
        if max(flat) >= spec.sat_code or min(flat) <= spec.floor_code:
            continue
        s1 = sum(flat)
        e = sum((row[2 * j] - row[2 * j + 1]) ** 2 for row in q for j in range(T // 2))
        l = max(s1, 0) >> (2 * int(math.log2(T)) + spec.bits - spec.level_bits)
        hist[b, c, l, ebin(e)] += 1
        level[b, c, l] += s1
    return hist, level


def small_frame(shape, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-40.0, 1100.0, (shape[0], shape[1] // 8, shape[2] // 8)).astype(np.float32).repeat(8, 1).repeat(8, 2)
         + rng.normal(0.0, 6.0, shape).astype(np.float32))
    flat = v.reshape(-1)
    for i, x in enumerate((NAN, INF, -INF, 64.5, 65.5, 1023.0, 5000.0, -5000.0)):         # halves (ties to even), the top, beyond both clamps
        flat[(i * 997 + 3) % flat.size] = x
    return v


@pytest.mark.parametrize("cfa", sorted(CFAS))
def test_restatement_equals_a_plain_loop(cfa):
    v = small_frame((2, 24, 40), 5)
    blacks = (64.0, 60.0, 66.5, 70.0)
    for tile, bits, lb, roi, sat, floor in ((4, 10, 5, None, None, None), (8, 8, 3, (1, 2, 10, 17), 250, -20), (4, 16, 6, (3, 0, 9, 20), 65536, -65536),
                                            (4, 12, 4, None, 4000, 0)):
        spec = M.RawNoise(tile=tile, bits=bits, level_bits=lb, roi=roi, sat=sat, floor=floor)
        want = looped_raw_noise(v, cfa, blacks, 1023.0, spec)
        got = R.restated_raw_noise(v, cfa, blacks, 1023.0, spec)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and want[0].sum() > 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (tile, bits)


def test_ebin_is_monotone_continuous_and_bounded():
    assert [ebin(e) for e in range(18)] == list(range(16)) + [16, 16] and ebin(15) + 1 == ebin(16)       # continuous at 16
    es = sorted(set(list(range(4096)) + [(1 << k) + d for k in range(4, 41) for d in (-1, 0, 1)] + [(m << k) + d for k in range(1, 38) for m in range(8, 16) for d in (-1, 0)]))
    bins = [ebin(e) for e in es]
    assert all(b1 - b0 in (0, 1) for b0, b1 in zip(bins, bins[1:]))                          # monotone, no bin skipped
    for T, bits in ((16, 16), (4, 16), (8, 10)):
        S = (1 << bits) - 1
        assert 2 * T * T * S * S < 1 << 41 and ebin(2 * T * T * S * S) <= 311 < _lib.RC_RAW_NOISE_EBINS
    assert ebin(2 * 16 * 16 * 65535 ** 2) == 311                                             # the largest e of all lands in the last bin used
    for b in range(312):
        lo, hi = ebin_range(b)
        assert ebin(lo) == ebin(hi) == b and (b == 0 or ebin(lo - 1) == b - 1)
        assert R.bin_centres()[b] == (lo + hi) / 2.0
    assert np.array_equal(R.ebin_of(np.array(es[:5000] + es[-300:])), np.array([ebin(e) for e in es[:5000] + es[-300:]]))


def test_invariants_of_the_restatement():
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 1024, (2, 40, 72))
    spec = M.RawNoise(tile=4, bits=10, level_bits=5, roi=(1, 2, 17, 30))
    hist, level = R.restated_raw_noise(codes, "RGGB", (0.0,) * 4, 1023.0, spec)
    assert hist.shape == (2, 4, 32, 320) and level.shape == (2, 4, 32)
    full = R.restated_raw_noise(codes, "RGGB", (0.0,) * 4, 1023.0, dataclasses.replace(spec, sat=1024))
    assert (R.tiles_of(full[0]).sum(-1) == 4 * 7).all() and (R.tiles_of(hist) <= R.tiles_of(full[0])).all() and R.tiles_of(hist).sum() < 2 * 4 * 28
    # the left-over cells are not measured: the same tables from the frame cut to the whole tiles
    cut = R.restated_raw_noise(codes[:, 2:34, 4:60], "RGGB", (0.0,) * 4, 1023.0, dataclasses.replace(spec, roi=None))
    assert np.array_equal(cut[0], hist) and np.array_equal(cut[1], level)
    # a frame flat per colour: every tile in energy bin 0, the level sums are the codes
    flat = np.zeros((1, 16, 16), dtype=np.int64)
    for p, lv in enumerate((100, 400, 402, 900)):
        flat[:, p // 2::2, p % 2::2] = lv
    h, l = R.restated_raw_noise(flat, "RGGB", (0.0,) * 4, 1023.0, M.RawNoise(tile=4, level_bits=3))
    assert h[..., 0].sum() == 16 and h[..., 1:].sum() == 0 and l.sum(-1).tolist() == [[100 * 64, 400 * 64, 402 * 64, 900 * 64]]
    # codes below black are kept signed: the level sum of a frame at black - 3 is negative, and its tiles sit in level bin 0
    h, l = R.restated_raw_noise(np.full((1, 8, 8), 61), "RGGB", (64.0,) * 4, 1087.0, M.RawNoise(tile=4, level_bits=3))
    assert l[0, :, 0].tolist() == [-48] * 4 and h[0, :, 0, 0].tolist() == [1] * 4
    assert R.restated_raw_noise(np.full((1, 8, 8), 61), "RGGB", (64.0,) * 4, 1087.0, M.RawNoise(tile=4, level_bits=3, floor=-3))[0].sum() == 0
    # permuting cfa together with the data leaves the colours unchanged
    cells = np.stack([codes[:, p // 2::2, p % 2::2] for p in range(4)], 1)
    for cfa in sorted(CFAS):
        moved = np.zeros_like(codes)
        for c, pos in enumerate(SLOT_POS[cfa]):
            moved[:, pos // 2::2, pos % 2::2] = cells[:, c]
        h2, l2 = R.restated_raw_noise(moved, cfa, (0.0,) * 4, 1023.0, spec)
        assert np.array_equal(h2, hist) and np.array_equal(l2, level), cfa


# ---- 2. the helpers ----------------------------------------------------------------------------------------------------------------------------------
def scene_tables(seed, gain, offset, tile, **kw):
    v, _ = R.patch_scene(seed, gain, offset, **kw)
    spec = M.RawNoise(tile=tile, bits=10, level_bits=4, top=1087.0)
    hist, level = R.restated_raw_noise(v, "RGGB", (64.0,) * 4, 1087.0, spec)
    return spec, hist, level, R.unit_of("RGGB", (64.0,) * 4, 1087.0, 10)


def test_helpers_equal_their_numpy_restatement():
    spec, hist, level, unit = scene_tables(3, 0.5, 4.0, 8, H=256, W=384, dark=0.2)
    hist, level = np.concatenate([hist, hist[:, ::-1]]), np.concatenate([level, level[:, ::-1]])       # two frames, the second with the colours swapped
    ns = M.RawNoiseStats(torch.from_numpy(hist), torch.from_numpy(level), spec, (0, 0, 128, 192), unit)
    assert ns.tiles().dtype == torch.int64 and np.array_equal(ns.tiles().numpy(), R.tiles_of(hist))
    for q, mt in ((0.1, 16), (0.25, 4)):
        var = ns.variance(q, mt)
        assert var.dtype == torch.float64 and var.shape == (2, 4, 16)
        np.testing.assert_allclose(var.numpy(), R.variance_of(hist, spec, unit, q, mt), rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(ns.profile(q, mt).numpy(), R.profile_of(hist, level, spec, unit, q, mt), rtol=1e-9)
        np.testing.assert_allclose(ns.temporal_noise(q, mt).numpy(), R.temporal_noise_of(hist, level, spec, unit, q, mt), rtol=1e-9)
    np.testing.assert_allclose(ns.levels().numpy(), R.levels_of(hist, level, spec, unit), rtol=1e-12, equal_nan=True)
    assert torch.isnan(ns.variance()).any() and torch.isnan(ns.levels()).any() and ns.profile().shape == (4, 2) and ns.temporal_noise().shape == (2,)
    assert "RawNoiseStats" in repr(ns) and ns.unit == tuple(unit)
    M.Temporal(tuple(ns.temporal_noise().tolist()))                                          # what the filter takes, as it comes
    # by hand: one bin of 20 tiles, all in the energy bin of e = 640 (bin 64 = [640, 703]), tile 8
    h = torch.zeros(1, 4, 8, 320, dtype=torch.int32)
    h[0, 0, 2, ebin(640)] = 20
    lv = torch.zeros(1, 4, 8, dtype=torch.int64)
    lv[0, 0, 2] = 20 * 64 * 300
    one = M.RawNoiseStats(h, lv, M.RawNoise(tile=8, level_bits=3), (0, 0, 64, 64), (2.0, 1.0, 1.0, 1.0))
    assert one.levels()[0, 0, 2].item() == 600.0 and one.tiles()[0, 0].tolist() == [0, 0, 20, 0, 0, 0, 0, 0]
    assert one.variance()[0, 0, 2].item() == pytest.approx(671.5 / (2 * chi2_quantile(0.1, 32)) * 4.0, rel=1e-12) and torch.isnan(one.variance(min_tiles=21)).all()
    assert chi2_quantile(0.1, 32) == pytest.approx(22.271, rel=2e-3) and chi2_quantile(0.5, 8) == pytest.approx(7.344, rel=2e-3)      # against chi-squared tables
    with pytest.raises(ValueError, match="quantile"):
        one.variance(quantile=1.0)
    # no measured bin at all: NaN, and the floors hold where the line falls or vanishes
    none = M.RawNoiseStats(torch.zeros_like(h), torch.zeros_like(lv), M.RawNoise(tile=8, level_bits=3), (0, 0, 64, 64), (1.0,) * 4)
    assert torch.isnan(none.profile()).all() and torch.isnan(none.temporal_noise()).all()
    tn = one.temporal_noise()                                                                # one point: no slope
    assert tn[1].item() == 0.0 and tn[0].item() == pytest.approx(math.sqrt(one.variance()[0, 0, 2].item()), rel=1e-12)


# The statistical test.  Scene: tests/raw_noise_ref.patch_scene -- 512 x 768 samples, 32 x 32-sample flat patches at 1 .. 90 % of a 10-bit scale over
# a black level of 64, 30 % of them textured, noise variance O + g level, rounded to integers (hence the + 1/12).  quantile 0.1, level_bits 4,
# min_tiles 16.  MEASURED is what the committed restatement gives on the committed generator (seed 7): the worst |median(variance / truth) - 1|
# over the three noise models and the worst |gain / g - 1| over models and colours; the bound is that plus half as much again.
MODELS = ((0.5, 4.0), (0.1, 1.0), (2.0, 16.0))
MEASURED = {4: (0.157, 0.213), 8: (0.047, 0.095), 16: (0.045, 0.101)}


@pytest.mark.parametrize("tile", (4, 8, 16))
def test_the_estimator_recovers_a_known_noise_model(tile):
    worst_var = worst_gain = 0.0
    for g, O in MODELS:
        spec, hist, level, unit = scene_tables(7, g, O, tile)
        ns = M.RawNoiseStats(torch.from_numpy(hist), torch.from_numpy(level), spec, (0, 0, 256, 384), unit)
        var, lev = ns.variance(0.1, 16).numpy(), ns.levels().numpy()
        ok = np.isfinite(var)
        assert ok.sum() >= 48                                                                # at least 12 of the 16 level bins per colour
        ratio = float(np.median(var[ok] / (O + g * lev[ok] + 1.0 / 12.0)))
        gains = ns.profile(0.1, 16)[:, 0].numpy() / g
        print(f"tile {tile} g {g} O {O}: bins {ok.sum()} median variance / truth {ratio:.3f}  gain / g {np.round(gains, 3).tolist()}")
        worst_var, worst_gain = max(worst_var, abs(ratio - 1.0)), max(worst_gain, float(np.abs(gains - 1.0).max()))
    assert worst_var <= 1.5 * MEASURED[tile][0] and worst_gain <= 1.5 * MEASURED[tile][1], (worst_var, worst_gain)


# The intercept cannot be had from a scene without dark areas (a line through bins at 1 .. 90 % extrapolates it: -1.0 .. 4.4 came out for O = 4
# at tile 8).  The second scene (seed 8) has a quarter of its patches at level 0 and the others from 10 % up, so that the darkest level bin
# holds dark tiles only: a bin's variance comes from its low-energy end and its level from its mean, and dark tiles mixed with brighter ones
# in one bin pull the intercept down (1.7 .. 2.1 for O = 4 with patches from 1 %).  MEASURED_DARK: worst |offset / (O + 1/12) - 1| over
# models and colours; the bound is that plus half as much again.
MEASURED_DARK = {4: 0.075, 8: 0.081, 16: 0.084}


@pytest.mark.parametrize("tile", (4, 8, 16))
def test_the_intercept_needs_and_gets_dark_patches(tile):
    worst = 0.0
    for g, O in MODELS:
        spec, hist, level, unit = scene_tables(8, g, O, tile, lo=0.10, dark=0.25)
        ns = M.RawNoiseStats(torch.from_numpy(hist), torch.from_numpy(level), spec, (0, 0, 256, 384), unit)
        off = ns.profile(0.1, 16)[:, 1].numpy() / (O + 1.0 / 12.0)
        tn = ns.temporal_noise(0.1, 16).tolist()
        print(f"tile {tile} g {g} O {O}: offset / truth {np.round(off, 3).tolist()}  temporal_noise {tn}")
        worst = max(worst, float(np.abs(off - 1.0).max()))
        assert 0.5 * math.sqrt(O) < tn[0] < 1.5 * math.sqrt(O + 0.15 * 1023 * g) and tn[1] > 0          # a line from sigma(0) upwards: sanity, not a figure
    assert worst <= 1.5 * MEASURED_DARK[tile], worst


# ---- 3. RawNoise, RawFormat ------------------------------------------------------------------------------------------------------------------
def test_raw_noise_validation_equality_and_immutability():
    s = M.RawNoise()
    assert (s.tile, s.bits, s.level_bits, s.roi, s.top, s.sat, s.floor) == (8, 10, 5, None, None, None, None)
    assert s.codes == 1024 and s.levels == 32 and s.pairs == 32 and s.sat_code == 1023 and s.floor_code == -1024
    assert M.RawNoise(bits=16, sat=65536, floor=65534).sat_code == 65536 and M.RawNoise(tile=16, level_bits=6).pairs == 128
    assert M.RawNoise(roi=[0, 2, 16, 16]) == M.RawNoise(roi=(0, 2, 16, 16)) and hash(M.RawNoise(roi=[0, 2, 16, 16])) == hash(M.RawNoise(roi=(0, 2, 16, 16)))
    assert M.RawNoise(top=1023).top == 1023.0 and isinstance(M.RawNoise(top=1023).top, float)
    with pytest.raises(Exception):
        s.bits = 12                                                                          # frozen
    for bad in (dict(tile=2), dict(tile=12), dict(tile=32), dict(bits=7), dict(bits=17), dict(level_bits=2), dict(level_bits=7), dict(roi=(0, 1, 8, 8)),
                dict(roi=(0, 0, 7, 8)), dict(roi=(0, 0, 8, 7)), dict(roi=(-1, 0, 8, 8)), dict(roi=(0, 0, 0, 8)), dict(tile=16, roi=(0, 0, 16, 15)), dict(top=INF), dict(top=NAN),
                dict(sat=0), dict(sat=1025), dict(floor=-1025), dict(floor=1023), dict(bits=8, sat=257)):
        with pytest.raises(ValueError):
            M.RawNoise(**bad)
    for bad in (dict(tile=8.0), dict(bits=True), dict(level_bits="5"), dict(roi=(0, 0, 8)), dict(roi=(0, 0, 8, 8.5)), dict(top="white"), dict(top=True), dict(sat=1.5),
                dict(floor=2.0)):
        with pytest.raises(TypeError):
            M.RawNoise(**bad)
    assert M.RawNoise(roi=(3, 2, 8, 9)).check(11, 12) == (3, 2, 8, 9) and M.RawNoise().check(8, 100) == (0, 0, 8, 100)
    for spec, hw in ((M.RawNoise(roi=(3, 2, 8, 9)), (10, 12)), (M.RawNoise(roi=(3, 2, 8, 9)), (11, 10)), (M.RawNoise(), (7, 100)), (M.RawNoise(), (100, 7)),
                     (M.RawNoise(tile=4), (0, 4)), (M.RawNoise(), (1 << 15, 1 << 14))):
        with pytest.raises(ValueError):
            spec.check(*hw)
    assert s.top_value(1023.0, (64.0,) * 4) == 1023.0 and M.RawNoise(top=4095).top_value(1023.0, (64.0,) * 4) == 4095.0
    with pytest.raises(ValueError, match="top"):
        M.RawNoise(top=64.0).top_value(1023.0, (64.0, 64.0, 64.0, 60.0))


def test_raw_format_carries_the_field():
    names = [f.name for f in dataclasses.fields(M.RawFormat)]
    assert names.index("noise") == names.index("quad") + 1 == names.index("temporal") - 1 and names[-3:] == ["exposures", "defects", "calibration"]
    assert M.RawFormat().noise is None and "noise" in M.RawFormat.__doc__
    fmt = M.RawFormat(storage="u16", black_level=64.0, white_level=1023.0, noise=M.RawNoise(tile=4))
    assert fmt.validate((2, 16, 24)) == (16, 24)
    with pytest.raises(ValueError, match="tile"):
        fmt.validate((2, 6, 24))                                                             # 3 cell rows
    with pytest.raises(ValueError, match="roi"):
        dataclasses.replace(fmt, noise=M.RawNoise(tile=4, roi=(0, 0, 8, 13))).validate((2, 16, 24))       # 12 cell columns
    with pytest.raises(ValueError, match="top"):
        dataclasses.replace(fmt, noise=M.RawNoise(tile=4, top=64.0)).validate((2, 16, 24))
    with pytest.raises(TypeError, match="RawNoise"):
        dataclasses.replace(fmt, noise=M.RawStats()).validate((2, 16, 24))
    quad = M.RawFormat(storage="u16", white_level=1023.0, quad=M.QuadBayer("bin"), noise=M.RawNoise(tile=8))      # a binned 32 x 32 frame has 8 x 8 cells
    assert quad.validate((1, 32, 32)) == (16, 16)
    with pytest.raises(ValueError, match="tile"):
        dataclasses.replace(quad, noise=M.RawNoise(tile=16)).validate((1, 32, 32))


# ---- 4. refusals before any launch, fake traces ----------------------------------------------------------------------------------------------------
def test_ops_refuse_before_any_launch(monkeypatch):
    spec = M.RawNoise(tile=4)
    u16 = dict(storage="u16", black_level=64.0, white_level=1023.0)
    with pytest.raises(RuntimeError, match="no CPU|CUDA|cuda"):
        ops.raw_noise(torch.zeros(1, 16, 16, dtype=torch.uint16), M.RawFormat(**u16), spec)   # a CPU tensor: there is no CPU path
    called = []
    monkeypatch.setattr(_lib, "load", lambda: called.append("load") or (_ for _ in ()).throw(AssertionError("the library was reached")))
    with FakeTensorMode():
        with torch.device("cuda"):
            frame = torch.empty(2, 32, 48, dtype=torch.uint16)
            with pytest.raises(TypeError, match="RawFormat"):
                ops.raw_noise(frame, "u16", spec)
            with pytest.raises(TypeError, match="RawNoise"):
                ops.raw_noise(frame, M.RawFormat(**u16))                                     # nothing asked for
            with pytest.raises(TypeError, match="RawNoise"):
                ops.raw_noise(frame, M.RawFormat(**u16), M.RawStats())
            for stage, kw in (("raw_quad", dict(quad=M.QuadBayer())), ("raw_defects", dict(defects=M.Defects(hot=(24.0, 0.1)))),
                              ("merge", dict(exposures=M.Exposures((1.0, 4.0), knee=(700.0, 900.0))))):
                with pytest.raises(ValueError, match=stage):                                 # the existing refusals: run that stage first
                    ops.raw_noise(frame if stage != "merge" else torch.empty(2, 2, 32, 48, dtype=torch.uint16), M.RawFormat(noise=spec, **u16, **kw))
            with pytest.raises(TypeError, match="uint16"):
                ops.raw_noise(frame.to(torch.int16), M.RawFormat(**u16), spec)
            with pytest.raises(ValueError, match="tile"):
                ops.raw_noise(torch.empty(2, 30, 48, dtype=torch.uint16), M.RawFormat(**u16), M.RawNoise(tile=16))      # 15 cell rows
            with pytest.raises(ValueError, match="roi"):
                ops.raw_noise(frame, M.RawFormat(**u16), M.RawNoise(tile=4, roi=(0, 20, 8, 8)))
            with pytest.raises(ValueError, match="top"):
                ops.raw_noise(frame, M.RawFormat(**u16), M.RawNoise(tile=4, top=60.0))
            with pytest.raises(ValueError, match="width"):
                ops.raw_noise(torch.empty(2, 32, 60, dtype=torch.uint8), M.RawFormat(storage="mipi10", white_level=1023.0), spec)
            # the calibration and the filter are seen and not looked at; every other op ignores the field; the shapes, dtypes and device of a trace
            fmt = M.RawFormat(storage="mipi12", cfa="GBRG", width=48, black_level=(64.0, 65.0, 66.0, 67.0), white_level=4095.0, temporal=M.Temporal((4, 0.25)),
                              calibration=M.Calibration(gains=(2.0, 1.0, 1.0, 1.5)), noise=M.RawNoise(tile=4, bits=12, level_bits=6, roi=(1, 2, 14, 20)))
            ns = ops.raw_noise(torch.empty(2, 1, 32, 80, dtype=torch.uint8), fmt)
            assert isinstance(ns, M.RawNoiseStats) and ns.hist.shape == (2, 4, 64, 320) and ns.level.shape == (2, 4, 64) and ns.roi == (1, 2, 14, 20)
            assert ns.hist.dtype == torch.int32 and ns.level.dtype == torch.int64 and ns.hist.device.type == ns.level.device.type == "cuda" and ns.spec is fmt.noise
            assert ns.unit == ((4095.0 - 66.0) / 4095, (4095.0 - 67.0) / 4095, (4095.0 - 64.0) / 4095, (4095.0 - 65.0) / 4095)      # GBRG: R is position 2
            assert ns.tiles().shape == ns.levels().shape == ns.variance().shape == (2, 4, 64) and ns.profile().shape == (4, 2) and ns.temporal_noise().shape == (2,)
            stats = ops.raw_stats(torch.empty(2, 1, 32, 80, dtype=torch.uint8), dataclasses.replace(fmt, temporal=None), M.RawStats(grid=(2, 2)))
            assert stats.hist.shape == (2, 4, 256)
            a, b = torch.ops.realcam.raw_noise(torch.empty(3, 16, 24), _lib.RC_RAW_F32, 0, 24, [0.0] * 4, [0, 0, 8, 12], 4, 10, 3, 1.0, 1023, -1024)
            assert a.shape == (3, 4, 8, 320) and b.shape == (3, 4, 8) and a.dtype == torch.int32 and b.dtype == torch.int64
    assert not called


def test_forward_mosaic_taps_in_front_of_temporal(monkeypatch):
    """The shared front end with the stages' ops wrapped: the order of the calls, the format the tap is handed, net.raw_noise."""
    from realcamnet_amd.temporal import Temporal, TemporalState
    order = []
    real = {name: getattr(ops, name) for name in ("raw_defects", "raw_noise", "raw_temporal", "raw_stats", "raw_calibrate", "raw_ingest")}

    def wrap(name):
        def call(mosaic, *args, **kw):
            order.append((name, kw["raw_format"] if "raw_format" in kw else args[0], mosaic.dtype, tuple(mosaic.shape)))
            out = real[name](mosaic, *args, **kw)
            if name == "raw_noise":
                order.append(("result", out, None, None))
            return out
        return call

    for name in real:
        monkeypatch.setattr(ops, name, wrap(name))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                spec = M.RawNoise(tile=8, roi=(2, 2, 60, 90))
                base = dict(storage="mipi10", cfa="GRBG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=1023.0)
                cal = M.Calibration(gains=torch.empty(2, 4, dtype=torch.float32), clip=(0.0, 1.0))
                mosaic, coord = torch.empty(2, 1, 144, 272, dtype=torch.uint8), torch.empty(2, 2, 72, 104)
                net = M.LiteISPNet_GFM_LSC().eval()
                with torch.no_grad():
                    y0 = net.forward_mosaic(mosaic, None, coord, raw_format=M.RawFormat(defects=M.Defects(hot=(24.0, 0.1)), calibration=cal, **base))
                assert [o[0] for o in order] == ["raw_defects", "raw_calibrate", "raw_ingest"] and "raw_noise" not in net.__dict__      # without the field nothing changes
                del order[:]
                full = M.RawFormat(defects=M.Defects(hot=(24.0, 0.1)), temporal=Temporal((4, 0.25), state=TemporalState()), calibration=cal, noise=spec,
                                   stats=M.RawStats(grid=(4, 4)), **base)
                with torch.no_grad():
                    y = net.forward_mosaic(mosaic, None, coord, raw_format=full)
                assert [o[0] for o in order] == ["raw_defects", "raw_noise", "result", "raw_temporal", "raw_stats", "raw_calibrate", "raw_ingest"]
                _, fmt, dt, shape = order[1]                                                # what the repair left: uint16, unpacked, the same cfa and levels
                assert (fmt.storage, fmt.width, fmt.cfa, fmt.blacks(), fmt.white_level) == ("u16", None, "GRBG", (64.0, 65.0, 66.0, 67.0), 1023.0)
                assert dt == torch.uint16 and shape == (2, 144, 208) and fmt.noise is spec and fmt.calibration is cal and fmt.temporal is full.temporal
                assert fmt.defects is None and fmt.quad is None and fmt.exposures is None
                assert net.raw_noise is order[2][1] and isinstance(net.raw_noise, M.RawNoiseStats) and net.raw_noise.roi == (2, 2, 60, 90)
                assert net.raw_noise.hist.shape == (2, 4, 32, 320) and net.raw_noise.level.shape == (2, 4, 32)
                assert all(o[1].noise is None for o in order[3:]) and y.shape == y0.shape == (2, 3, 144, 208)
                del order[:]
                with torch.no_grad():                                                       # with no other stage: the frame as delivered
                    net.forward_mosaic(mosaic, None, coord, raw_format=M.RawFormat(noise=spec, **base))
                assert [(o[0], o[2], o[3]) for o in order if o[0] != "result"] == [("raw_noise", torch.uint8, (2, 1, 144, 272)), ("raw_ingest", torch.uint8, (2, 1, 144, 272))]
                assert order[0][1].storage == "mipi10" and order[0][1].width == 208
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch
U16, F32, MIPI10, MIPI12 = _lib.RC_RAW_U16, _lib.RC_RAW_F32, _lib.RC_RAW_MIPI10, _lib.RC_RAW_MIPI12


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=None), b"null"), ("null desc", dict(desc=None), b"null"), ("null hist", dict(hist=None), b"null"),
    ("null level", dict(level=None), b"null"),
    # everything rc_raw_stats refuses
    ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("2^31 samples", dict(h=1 << 15, w=1 << 14), b"2^31"),
    ("storage 7", dict(storage=7), b"storage"), ("storage -1", dict(storage=-1), b"storage"), ("cfa 4", dict(cfa=4), b"cfa"), ("cfa -1", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("line_bytes short (u16)", dict(line_bytes=30), b"line_bytes"), ("line_bytes short (RAW10)", dict(storage=MIPI10, line_bytes=19), b"line_bytes"),
    ("line_bytes short (RAW12)", dict(storage=MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("RAW10 2w % 4", dict(storage=MIPI10, w=7, width=14), b"RAW10"),
    ("mipi base misaligned", dict(storage=MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=F32, src=FAKE + 2), b"misaligned"),
    ("black nan", dict(black=(64.0, NAN, 64.0, 64.0)), b"black"), ("black inf", dict(black=(64.0, 64.0, 64.0, -INF)), b"black"),
    ("desc reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"),
    ("top nan", dict(top=NAN), b"top"), ("top inf", dict(top=INF), b"top"), ("top at a black", dict(top=64.0), b"top"), ("top below one black", dict(black=(64.0, 64.0, 2000.0, 64.0)), b"top"),
    ("top one ulp above black 0", dict(black=(0.0,) * 4, top=1e-45), b"top"),
    # the request
    ("tile 0", dict(tile=0), b"tile"), ("tile 2", dict(tile=2), b"tile"), ("tile 12", dict(tile=12), b"tile"), ("tile 32", dict(tile=32), b"tile"),
    ("bits 7", dict(bits=7), b"bits"), ("bits 17", dict(bits=17), b"bits"), ("level_bits 2", dict(level_bits=2), b"level_bits"), ("level_bits 7", dict(level_bits=7), b"level_bits"),
    ("sat 0", dict(sat=0), b"sat"), ("sat 1025", dict(sat=1025), b"sat"), ("sat 257 at 8 bits", dict(bits=8, sat=257), b"sat"),
    ("floor -1025", dict(floor=-1025), b"floor"), ("floor 1023", dict(floor=1023), b"floor"),
    ("cx0 odd", dict(roi=(0, 1, 4, 4)), b"even"),
    ("roi beyond rows", dict(roi=(6, 0, 5, 8)), b"roi"), ("roi beyond columns", dict(roi=(0, 2, 4, 8)), b"roi"), ("roi negative", dict(roi=(-1, 0, 4, 4)), b"roi"),
    ("roi one zero side", dict(roi=(0, 0, 0, 8)), b"roi"), ("roi other zero side", dict(roi=(0, 0, 4, 0)), b"roi"), ("whole frame moved", dict(roi=(1, 0, 0, 0)), b"roi"),
    ("roi overflow", dict(roi=(2147483647, 0, 4, 4)), b"roi"), ("roi size overflow", dict(roi=(1, 2, 2147483647, 2147483647)), b"roi"),
    ("too few rows", dict(roi=(0, 0, 3, 8)), b"tile"), ("too few columns", dict(roi=(0, 0, 8, 3)), b"tile"), ("frame below a tile", dict(tile=16), b"tile"),
    ("hist misaligned", dict(hist=FAKE + 2), b"4-byte"), ("level misaligned", dict(level=FAKE + 4), b"8-byte"),
])
def test_raw_noise_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, hist=FAKE, level=FAKE, b=1, h=10, w=8, storage=U16, cfa=0, line_bytes=0, width=0, black=(64.0,) * 4, fmt_reserved=(0, 0, 0, 0),
              roi=(0, 0, 0, 0), tile=4, bits=10, level_bits=5, top=1023.0, sat=1024, floor=-1024, reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=0.0,
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.RawNoiseDesc(roi=(C.c_int32 * 4)(*kw["roi"]), tile=kw["tile"], bits=kw["bits"], level_bits=kw["level_bits"], top=kw["top"], sat=kw["sat"], floor=kw["floor"],
                          reserved=(C.c_int32 * 4)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_noise(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["hist"], kw["level"], kw["b"], kw["h"], kw["w"],
                            None) == -1, case                                                # RC_ERR_INVALID
    err = lib.rc_last_error()
    assert err.startswith(b"rc_raw_noise:") and msg in err, (case, err)


def test_raw_noise_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_noise", "rc_raw_noise_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                              # additive: the version stays
    assert lib.rc_raw_noise_desc_size() == C.sizeof(_lib.RawNoiseDesc) == 56
    header = _lib.HEADER.read_text()
    for name in ("RC_RAW_NOISE_EBINS", "RC_RAW_NOISE_MAX_LEVEL_BITS"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert header.index("int rc_raw_stats(") < header.index("RC_RAW_NOISE_EBINS") < header.index("int rc_raw_noise(") < header.index("rc_nchw_to_nhwc")
    assert M.raw_noise.EBINS == 320 and M.raw_noise.MAX_LEVEL_BITS == 6 and M.raw_noise.TILES == (4, 8, 16)
    assert "raw_noise" in M.torch_ops.SCHEMAS and "RawNoise" in M.__all__ and "RawNoiseStats" in M.__all__


def test_raw_noise_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "raw_noise.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "raw_noise_kernel" in k}
    assert len(mine) == 12, sorted(mine)                   # the five element storages with and without vector loads, RAW10, RAW12
    assert all(v["tu"] == "raw_noise.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 64 for v in mine.values())               # 8 waves per SIMD: the row loads' latency is hidden by waves, too
    assert all(v["lds"] == 4 * 64 * 8 + 4 * 4 * 320 * 4 for v in mine.values())      # the block's level sums and its histogram window: 7 blocks per CU
    zero = [k for k, v in res.items() if v["tu"] == "raw_noise.hip" and k not in mine]      # the launch that zeroes the outputs, and nothing else
    assert len(zero) == 1 and "raw_noise_zero_kernel" in zero[0] and not res[zero[0]].get("scratch", 0) and res[zero[0]]["lds"] == 0
