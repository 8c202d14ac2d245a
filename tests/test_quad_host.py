"""Quad-Bayer sensors, the CPU side: the elementwise restatement of rc_raw_quad (written from the header's text, index gathers over the whole
frame, no lane map), frames computed by hand, the properties the header promises, the quality ordering, validation, the C ABI."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd.defects import DefectMap, Defects
from realcamnet_amd.exposures import Exposures
from realcamnet_amd.quad import QuadBayer

CFA_NAMES = ("RGGB", "BGGR", "GRBG", "GBRG")
RECIPES = ("keep", "G:H", "G:V", "G:tie", "H", "V", "diag")


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------------
def _reflect(i, n):
    i = np.where(i < 0, 1 - i, i)
    return np.where(i >= n, 2 * n - 3 - i, i)


def quad_colours(cfa, h, w):
    """The sensor's colour at every site of an (h, w) quad frame, as characters."""
    y, x = np.mgrid[0:h, 0:w]
    return np.array(list(cfa))[2 * ((y >> 1) & 1) + ((x >> 1) & 1)]


def bayer_colours(cfa, h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.array(list(cfa))[2 * (y & 1) + (x & 1)]


def restated_quad(frame, cfa, mode, out_dtype=None, nearest=False, recipes=False):
    """rc_raw_quad in numpy fp32, step for step the header's: frame (B,H,W) or (H,W), integer counts or floats.  out_dtype: torch.uint16 (the
    count storages: rint, half to even), a float dtype (round to nearest even), default fp32; "bin" is always fp32.  nearest: the baseline
    that takes `near` in place of every axis estimate (case 5: the diagonal neighbour).  recipes: also return the (H,W) array of RECIPES names
    (the frame must then hold one image)."""
    t = torch.as_tensor(frame)
    lead = t.dim() == 2
    v = (t[None] if lead else t).to(torch.float32).numpy()
    _, h, w = v.shape
    if mode == "bin":
        out = ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * np.float32(0.25)
        res = torch.from_numpy(out)
        return res[0] if lead else res
    assert mode == "remosaic"
    y, x = np.mgrid[0:h, 0:w]
    sensor, want = quad_colours(cfa, h, w), bayer_colours(cfa, h, w)
    sy, sx = np.where(y & 1, 1, -1), np.where(x & 1, 1, -1)
    at = lambda yy, xx: v[:, _reflect(yy, h), _reflect(xx, w)]
    col = lambda yy, xx: sensor[_reflect(yy, h), _reflect(xx, w)]
    three = np.float32(3.0)
    axis = (lambda near, far: near) if nearest else (lambda near, far: near + (far - near) / three)
    on_h, on_v = col(y, x + sx) == want, col(y + sy, x) == want
    assert (col(y, x - 2 * sx) == want)[on_h].all() and (col(y - 2 * sy, x) == want)[on_v].all()        # near and far at distances 1 and 2
    hn, hf, vn, vf = at(y, x + sx), at(y, x - 2 * sx), at(y + sy, x), at(y - 2 * sy, x)
    e_h, d_h, e_v, d_v = axis(hn, hf), np.abs(hf - hn), axis(vn, vf), np.abs(vf - vn)
    both = np.where(d_h < d_v, e_h, np.where(d_v < d_h, e_v, (e_h + e_v) * np.float32(0.5)))
    diag = ~(sensor == want) & ~on_h & ~on_v
    for yy, xx in ((y + sy, x + sx), (y + sy, x - 2 * sx), (y - 2 * sy, x + sx), (y - 2 * sy, x - 2 * sx)):
        assert (col(yy, xx) == want)[diag].all()                                                        # the diagonal neighbour and its square
    r_near = axis(at(y + sy, x + sx), at(y + sy, x - 2 * sx))
    r_far = axis(at(y - 2 * sy, x + sx), at(y - 2 * sy, x - 2 * sx))
    out = np.where(sensor == want, v, np.where(on_h & on_v, both, np.where(on_h, e_h, np.where(on_v, e_v, axis(r_near, r_far)))))
    assert out.dtype == np.float32
    if out_dtype == torch.uint16:
        res = torch.from_numpy(np.rint(out).astype(np.uint16))
    else:
        res = torch.from_numpy(out).to(out_dtype or torch.float32)
    res = res[0] if lead else res
    if not recipes:
        return res
    assert v.shape[0] == 1
    names = np.where(sensor == want, "keep", np.where(on_h & on_v, np.where(d_h[0] < d_v[0], "G:H", np.where(d_v[0] < d_h[0], "G:V", "G:tie")),
                                                      np.where(on_h, "H", np.where(on_v, "V", "diag"))))
    return res, names


def test_site_classes_of_a_tile():
    """6 of the 16 sites keep their sample; the other ten are 4 G-at-R/B, 4 single-axis and 2 diagonal sites -- for every phase."""
    for cfa in CFA_NAMES:
        _, names = restated_quad(torch.arange(64.0).reshape(8, 8) ** 2 % 97, cfa, "remosaic", recipes=True)
        tile = names[0:4, 0:4]
        kinds = [n.split(":")[0] for n in tile.ravel()]
        assert kinds.count("keep") == 6 and kinds.count("G") == 4 and kinds.count("H") == 2 and kinds.count("V") == 2 and kinds.count("diag") == 2, (cfa, tile)
        for j in range(0, 8, 4):
            for i in range(0, 8, 4):
                assert [n.split(":")[0] for n in names[j:j + 4, i:i + 4].ravel()] == kinds                # the classes repeat with the tile


# ---- 2. frames computed by hand ---------------------------------------------------------------------------------------------------------------
# Every sample is a multiple of 9, so every (far - near) / 3 and every nested one is an integer, and a tie's mean ends in .0 or .5: the
# values below were worked out with exact fractions, site by site, from the header's text.  In the 4 x 4 tile every neighbour is a reflection:
# near and far are then the same sample on each axis (d = 0), so every G site is a tie and every estimate is a plain copy.
T4 = [[9, 90, 180, 27], [45, 18, 99, 360], [270, 36, 450, 81], [54, 720, 63, 900]]
T4_OUT = {
    "RGGB": [[9.0, 108.0, 90.0, 27.0], [184.5, 450.0, 99.0, 81.0], [45.0, 36.0, 18.0, 198.0], [54.0, 63.0, 409.5, 900.0]],
    "GRBG": [[9.0, 180.0, 270.0, 27.0], [270.0, 18.0, 36.0, 49.5], [247.5, 99.0, 450.0, 360.0], [54.0, 40.5, 720.0, 900.0]],
}
T4_RECIPE = {
    "RGGB": [['keep', 'G:tie', 'H', 'keep'], ['G:tie', 'diag', 'keep', 'V'], ['V', 'keep', 'diag', 'G:tie'], ['keep', 'H', 'G:tie', 'keep']],
    "GRBG": [['keep', 'H', 'G:tie', 'keep'], ['V', 'keep', 'diag', 'G:tie'], ['G:tie', 'diag', 'keep', 'V'], ['keep', 'G:tie', 'H', 'keep']],
}
T8 = [[1485, 693, 1818, 2997, 216, 333, 2466, 432], [1683, 2682, 261, 2331, 981, 171, 396, 1998], [1926, 315, 1107, 414, 2538, 1953, 270, 2601],
      [567, 1026, 2898, 2889, 2682, 279, 2655, 2691], [1827, 225, 1017, 207, 2565, 612, 1332, 1926], [657, 2484, 540, 2628, 1413, 2574, 3141, 828],
      [468, 2673, 2628, 2943, 864, 1710, 441, 2520], [3276, 288, 2592, 270, 2844, 945, 2286, 3132]]
T8_OUT = {
    "RGGB": [[1485.0, 1066.5, 534.0, 2997.0, 216.0, 1953.0, 333.0, 432.0], [1093.5, 1107.0, 261.0, 414.0, 2538.0, 318.0, 396.0, 2601.0],
             [1731.0, 315.0, 1745.0, 1623.0, 1509.0, 1953.0, 318.0, 1953.0], [567.0, 2898.0, 765.0, 2889.0, 2682.0, 2733.0, 279.0, 2691.0],
             [1827.0, 1017.0, 1005.0, 207.0, 2565.0, 957.0, 612.0, 1926.0], [540.0, 2718.0, 540.0, 2925.0, 2799.0, 1761.0, 3141.0, 2577.0],
             [657.0, 2673.0, 2127.0, 2628.0, 1413.0, 1710.0, 2574.0, 1269.0], [3276.0, 2592.0, 540.0, 270.0, 2844.0, 1614.0, 2043.0, 3132.0]],
    "GRBG": [[1485.0, 1818.0, 1107.0, 2997.0, 216.0, 2643.0, 301.5, 432.0], [1926.0, 2682.0, 1056.0, 414.0, 2538.0, 171.0, 1953.0, 1386.0],
             [1107.0, 513.0, 1107.0, 1623.0, 366.0, 1013.0, 270.0, 1974.0], [567.0, 2898.0, 1578.0, 2889.0, 2682.0, 2733.0, 279.0, 2691.0],
             [1827.0, 1017.0, 2808.0, 207.0, 2565.0, 957.0, 612.0, 1926.0], [501.0, 2484.0, 1906.0, 2925.0, 1470.0, 2574.0, 1233.0, 2574.0],
             [1642.5, 540.0, 2628.0, 2628.0, 1413.0, 2970.0, 441.0, 828.0], [3276.0, 2538.0, 1140.0, 270.0, 2844.0, 2574.0, 945.0, 3132.0]],
}
T8_RECIPE = {
    "RGGB": [['keep', 'G:tie', 'H', 'keep', 'keep', 'G:V', 'H', 'keep'], ['G:tie', 'diag', 'keep', 'V', 'G:V', 'diag', 'keep', 'V'],
             ['V', 'keep', 'diag', 'G:V', 'V', 'keep', 'diag', 'G:H'], ['keep', 'H', 'G:V', 'keep', 'keep', 'H', 'G:H', 'keep'],
             ['keep', 'G:H', 'H', 'keep', 'keep', 'G:H', 'H', 'keep'], ['G:H', 'diag', 'keep', 'V', 'G:H', 'diag', 'keep', 'V'],
             ['V', 'keep', 'diag', 'G:V', 'V', 'keep', 'diag', 'G:tie'], ['keep', 'H', 'G:V', 'keep', 'keep', 'H', 'G:tie', 'keep']],
    "GRBG": [['keep', 'H', 'G:V', 'keep', 'keep', 'H', 'G:tie', 'keep'], ['V', 'keep', 'diag', 'G:V', 'V', 'keep', 'diag', 'G:tie'],
             ['G:H', 'diag', 'keep', 'V', 'G:H', 'diag', 'keep', 'V'], ['keep', 'G:H', 'H', 'keep', 'keep', 'G:H', 'H', 'keep'],
             ['keep', 'H', 'G:V', 'keep', 'keep', 'H', 'G:H', 'keep'], ['V', 'keep', 'diag', 'G:V', 'V', 'keep', 'diag', 'G:H'],
             ['G:tie', 'diag', 'keep', 'V', 'G:V', 'diag', 'keep', 'V'], ['keep', 'G:tie', 'H', 'keep', 'keep', 'G:V', 'H', 'keep']],
}
HAND = (("4x4", T4, T4_OUT, T4_RECIPE), ("8x8", T8, T8_OUT, T8_RECIPE))


def hand_counts(out):
    """A hand result as the count storages store it: rint, half to even (184.5 -> 184, 409.5 -> 410)."""
    return np.rint(np.array(out, dtype=np.float64)).astype(np.int64).tolist()


@pytest.mark.parametrize("cfa", ("RGGB", "GRBG"))
def test_restatement_matches_the_frames_computed_by_hand(cfa):
    for name, src, outs, recipe in HAND:
        got, names = restated_quad(torch.tensor(src, dtype=torch.float32), cfa, "remosaic", recipes=True)
        assert got.tolist() == outs[cfa], (name, cfa)
        assert names.tolist() == recipe[cfa], (name, cfa)
        assert set(names.ravel().tolist()) <= set(RECIPES)
        counts = restated_quad(torch.tensor(src, dtype=torch.int32), cfa, "remosaic", torch.uint16)
        assert counts.dtype == torch.uint16 and counts.to(torch.int64).tolist() == hand_counts(outs[cfa])
    assert {n for r in T8_RECIPE[cfa] for n in r} == set(RECIPES)                     # the 8 x 8 frame takes every recipe and every arm
    # bin: the hand value of the first block of the 4 x 4 tile, (9 + 90) + (45 + 18) over 4
    assert restated_quad(torch.tensor(T4, dtype=torch.int32), cfa, "bin").tolist() == [[40.5, 166.5], [270.0, 373.5]]


# ---- 3. what the header promises ----------------------------------------------------------------------------------------------------------------
def colour_planes_to(colours, planes):
    """Sample per-colour images {"R": (h,w), "G": .., "B": ..} at the sites of a (h,w) colour map."""
    out = np.zeros(colours.shape, dtype=np.float32)
    for c, p in planes.items():
        out[colours == c] = np.broadcast_to(np.asarray(p, dtype=np.float32), colours.shape)[colours == c]
    return out


@pytest.mark.parametrize("cfa", CFA_NAMES)
def test_flat_fields_and_integer_ramps_are_exact(cfa):
    h, w = 16, 24
    flat = {"R": np.float32(100.3), "G": np.float32(200.7), "B": np.float32(50.1)}                      # not integers: /3 of a zero difference is exact
    got = restated_quad(colour_planes_to(quad_colours(cfa, h, w), flat), cfa, "remosaic").numpy()
    assert np.array_equal(got, colour_planes_to(bayer_colours(cfa, h, w), flat))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    for ay, ax in ((0, 5), (7, 0), (7, 5), (-7, 5)):
        planes = {"R": 1000 + ay * y + ax * x, "G": 2000 + ax * y + ay * x, "B": 500 + ay * y - ax * x}
        got = restated_quad(colour_planes_to(quad_colours(cfa, h, w), planes), cfa, "remosaic").numpy()
        want = colour_planes_to(bayer_colours(cfa, h, w), planes)
        assert np.array_equal(got[2:-2, 2:-2], want[2:-2, 2:-2]), (cfa, ay, ax)


@pytest.mark.parametrize("cfa", CFA_NAMES)
def test_kept_sites_are_the_input_and_bin_returns_constant_blocks(cfa):
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        src = torch.rand(2, 12, 16, generator=g).to(dtype)
        got = restated_quad(src, cfa, "remosaic", dtype)
        kept = torch.from_numpy(quad_colours(cfa, 12, 16) == bayer_colours(cfa, 12, 16))
        assert kept.sum() == 12 * 16 * 6 // 16
        assert torch.equal(got[:, kept].view(torch.int16 if dtype != torch.float32 else torch.int32),
                           src[:, kept].view(torch.int16 if dtype != torch.float32 else torch.int32))
    counts = torch.randint(0, 1 << 14, (2, 12, 16), generator=g, dtype=torch.int32)
    got = restated_quad(counts, cfa, "remosaic", torch.uint16)
    assert torch.equal(got[:, kept].to(torch.int32), counts[:, kept])
    blocks = torch.rand(2, 6, 8, generator=g) * 1000
    out = restated_quad(blocks.repeat_interleave(2, 1).repeat_interleave(2, 2), cfa, "bin")
    assert out.dtype == torch.float32 and torch.equal(out, blocks)
    assert torch.equal(restated_quad(counts, cfa, "bin"), counts.to(torch.float64).view(2, 6, 2, 8, 2).sum((2, 4)).div(4).to(torch.float32))


# ---- 4. quality -------------------------------------------------------------------------------------------------------------------------------
def scene(h=48, w=64):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.25 * np.sin(x / 9) * np.cos(y / 7)
    edge = 0.2 * (((x - w / 2) * 0.8 + (y - h / 2) * 0.6) > 0)
    disk = 0.15 * (((x - w / 3) ** 2 + (y - h / 3) ** 2) < (h / 5) ** 2)
    return {"R": np.rint((0.9 * base + edge) * 4095), "G": np.rint((base + disk) * 4095), "B": np.rint((0.7 * base + 0.5 * edge + disk) * 4095)}


def psnr(a, b, peak=4095.0):
    return 10 * np.log10(peak ** 2 / np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))


@pytest.mark.parametrize("cfa", CFA_NAMES)
def test_remosaic_beats_the_nearest_sample_on_a_scene(cfa):
    """Measured here: remosaic 37.5 .. 38.2 dB, nearest same-colour sample 33.1 .. 34.7 dB, the quad frame read as Bayer about 19.8 dB."""
    planes = scene()
    h, w = planes["R"].shape
    quad, bayer = colour_planes_to(quad_colours(cfa, h, w), planes), colour_planes_to(bayer_colours(cfa, h, w), planes)
    ours = psnr(restated_quad(quad, cfa, "remosaic").numpy(), bayer)
    near = psnr(restated_quad(quad, cfa, "remosaic", nearest=True).numpy(), bayer)
    asis = psnr(quad, bayer)
    print(f"quad quality {cfa}: remosaic {ours:.2f} dB, nearest {near:.2f} dB, read as Bayer {asis:.2f} dB")
    assert ours > near + 1.0, (cfa, ours, near)
    assert near > asis + 1.0, (cfa, near, asis)


# ---- 5. validation: pure Python, no GPU, no library -----------------------------------------------------------------------------------------------
def test_quad_validation():
    assert QuadBayer().mode == "remosaic" and M.QuadBayer is QuadBayer
    for bad in ("Bin", "nona", None, 1):
        with pytest.raises(ValueError, match="mode"):
            QuadBayer(mode=bad)
    re, bn = M.RawFormat(quad=QuadBayer()), M.RawFormat(quad=QuadBayer("bin"))
    assert re.validate((2, 1, 40, 56)) == (40, 56) and bn.validate((2, 40, 56)) == (20, 28)          # the size of what leaves the stage
    assert M.RawFormat(storage="mipi10", width=56, white_level=1023.0, quad=QuadBayer("bin")).validate((2, 40, 72)) == (20, 28)
    assert re.validate((1, 4, 4)) == (4, 4) and bn.validate((1, 4, 4)) == (2, 2)
    for shape in ((1, 42, 56), (1, 40, 54), (1, 2, 8), (1, 8, 2), (1, 6, 6)):
        for fmt in (re, bn):
            with pytest.raises(ValueError, match="multiples of 4"):
                fmt.validate(shape)
    with pytest.raises(ValueError, match="multiples of 4"):
        M.RawFormat(storage="mipi12", width=42, white_level=4095.0, quad=QuadBayer()).validate((1, 40, 64))
    for notquad in ("remosaic", True, object()):
        with pytest.raises(ValueError, match="QuadBayer"):
            M.RawFormat(quad=notquad).validate((1, 8, 8))
    # exposures: whole frames are fine (E = 2: (B,E,H,X)), interleaved lines are refused
    ex = Exposures(times=(1.0, 4.0), knee=(3000.0, 3500.0))
    assert M.RawFormat(storage="u16", white_level=4095.0, exposures=ex, quad=QuadBayer("bin")).validate((2, 2, 40, 56)) == (20, 28)
    with pytest.raises(ValueError, match="de-interleave"):
        M.RawFormat(storage="u16", white_level=4095.0, exposures=dataclasses.replace(ex, layout="lines"), quad=QuadBayer()).validate((2, 80, 56))
    # defects: a factory map is refused, the dynamic tests are not
    dm = DefectMap.from_coords((40, 56), [(1, 1)])
    for q in (QuadBayer(), QuadBayer("bin")):
        with pytest.raises(ValueError, match="Defects.map"):
            M.RawFormat(quad=q, defects=Defects(map=dm, hot=(0.1, 0.0))).validate((1, 40, 56))
        assert M.RawFormat(quad=q, defects=Defects(hot=(0.1, 0.0), cold=(0.1, 0.0))).validate((1, 40, 56)) == q.out_size(40, 56)
    # the later stages are checked against the size that leaves the stage
    from realcamnet_amd.calibration import Calibration, GainMap
    gm = GainMap(torch.ones(4, 3, 3), cell=8)                                            # nodes for a 20 x 28 mosaic's 10 x 14 planes: ceil(10/8)+1, ceil(14/8)+1
    assert M.RawFormat(quad=QuadBayer("bin"), calibration=Calibration(shading=gm)).validate((1, 40, 56)) == (20, 28)
    with pytest.raises(ValueError):
        M.RawFormat(quad=QuadBayer(), calibration=Calibration(shading=gm)).validate((1, 40, 56))


def test_forward_mosaic_and_ops_refuse_before_any_launch():
    with FakeTensorMode():
        with torch.device("cuda"):
            net = M.LiteISPNet().eval()
            u16 = dict(storage="u16", white_level=4095.0)
            with pytest.raises(ValueError, match="multiples of 4"):
                net.forward_mosaic(torch.empty(1, 1, 34, 32, dtype=torch.uint16), raw_format=M.RawFormat(quad=QuadBayer(), **u16))
            with pytest.raises(ValueError, match="de-interleave"):
                net.forward_mosaic(torch.empty(1, 64, 32, dtype=torch.uint16),
                                   raw_format=M.RawFormat(quad=QuadBayer(), exposures=Exposures(times=(1.0, 4.0), knee=(3000.0, 3500.0), layout="lines"), **u16))
            with pytest.raises(ValueError, match="Defects.map"):
                net.forward_mosaic(torch.empty(1, 32, 32, dtype=torch.uint16),
                                   raw_format=M.RawFormat(quad=QuadBayer("bin"), defects=Defects(map=DefectMap.from_coords((32, 32), [(0, 0)])), **u16))
            with pytest.raises(ValueError, match="QuadBayer"):
                net.forward_mosaic(torch.empty(1, 32, 32, dtype=torch.uint16), raw_format=M.RawFormat(quad="bin", **u16))
            frame = torch.empty(2, 32, 48, dtype=torch.uint16)
            with pytest.raises(ValueError, match="QuadBayer"):
                M.ops.raw_quad(frame, M.RawFormat(**u16))                                 # nothing asked for
            with pytest.raises(ValueError, match="raw_quad"):                             # the other stages read a Bayer mosaic: they refuse rather than misread
                M.ops.raw_defects(frame, M.RawFormat(quad=QuadBayer(), defects=Defects(hot=(1.0, 0.0)), **u16))
            with pytest.raises(ValueError, match="raw_quad"):
                M.ops.raw_ingest(frame, dtype=torch.float32, raw_format=M.RawFormat(quad=QuadBayer(), **u16))
            with pytest.raises(ValueError, match="one exposure"):
                M.ops.raw_quad(torch.empty(2, 2, 32, 48, dtype=torch.uint16), M.RawFormat(quad=QuadBayer(), exposures=Exposures(times=(1.0, 4.0), knee=(3000.0, 3500.0)), **u16))


def test_fake_trace_of_forward_mosaic_with_quad():
    with FakeTensorMode():
        with torch.device("cuda"):
            frame = torch.empty(2, 1, 64, 96, dtype=torch.uint16)
            u16 = dict(storage="u16", cfa="GRBG", white_level=4095.0)
            out = M.ops.raw_quad(frame, M.RawFormat(quad=QuadBayer(), **u16))
            assert out.shape == (2, 64, 96) and out.dtype == torch.uint16
            out = M.ops.raw_quad(frame, M.RawFormat(**u16), QuadBayer("bin"))
            assert out.shape == (2, 32, 48) and out.dtype == torch.float32
            packed = torch.empty(2, 64, 128, dtype=torch.uint8)
            assert M.ops.raw_quad(packed, M.RawFormat(storage="mipi10", width=96, white_level=1023.0, quad=QuadBayer())).shape == (2, 64, 96)
            fl = M.ops.raw_quad(torch.empty(2, 64, 96, dtype=torch.bfloat16), M.RawFormat(quad=QuadBayer()))
            assert fl.shape == (2, 64, 96) and fl.dtype == torch.bfloat16
            assert torch.ops.realcam.raw_quad(frame[:, 0], _lib.RC_RAW_U16, 0, 96, _lib.RC_QUAD_BIN).shape == (2, 32, 48)
            net = M.LiteISPNet().eval()
            with torch.no_grad():
                y = net.forward_mosaic(frame, raw_format=M.RawFormat(quad=QuadBayer(), **u16))
                assert y.shape == (2, 3, 64, 96)
                y = net.forward_mosaic(frame, raw_format=M.RawFormat(quad=QuadBayer("bin"), defects=Defects(hot=(64.0, 0.1)), **u16), out_format="rgb8")
                assert y.shape == (2, 32, 48, 3) and y.dtype == torch.uint8                # every later stage, the crop and the encoder see the binned size
                ex = Exposures(times=(1.0, 4.0), knee=(3000.0, 3500.0))
                y = net.forward_mosaic(torch.empty(2, 2, 64, 96, dtype=torch.uint16), raw_format=M.RawFormat(quad=QuadBayer("bin"), exposures=ex, **u16))
                assert y.shape == (2, 3, 32, 48)
                strided = M.ISPUNet_GFM_LSC().eval()
                y = strided.forward_mosaic(frame, None, torch.empty(2, 2, 16, 24), raw_format=M.RawFormat(quad=QuadBayer("bin"), **u16))
                assert y.shape == (2, 3, 32, 48)
                with pytest.raises(ValueError, match="coord"):                            # coord at the SENSOR's packed size is the wrong size
                    strided.forward_mosaic(frame, None, torch.empty(2, 2, 32, 48), raw_format=M.RawFormat(quad=QuadBayer("bin"), **u16))


# ---- 6. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before anything is enqueued


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("width", dict(width=12), b"width"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("dst pitch short", dict(dst_pitch=30), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=33), b"dst pitch"), ("dst misaligned", dict(dst=FAKE + 1), b"dst misaligned"),
    ("f32 dst misaligned", dict(storage=_lib.RC_RAW_F32, dst=FAKE + 2), b"dst misaligned"),
    ("bin dst pitch short", dict(mode=1, dst_pitch=28), b"dst pitch"), ("bin dst misaligned", dict(mode=1, dst=FAKE + 2), b"dst misaligned"),
    ("H % 4", dict(H=10), b"multiples of 4"), ("W % 4", dict(W=18, width=18), b"multiples of 4"), ("H < 4", dict(H=2), b"bad shape"), ("W < 4", dict(W=0), b"bad shape"),
    ("mode", dict(mode=2), b"mode"), ("mode < 0", dict(mode=-1), b"mode"),
    ("reserved", dict(reserved=(0, 1, 0)), b"reserved"), ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"),
    ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
])
def test_raw_quad_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, dst=FAKE, dst_pitch=0, b=1, H=8, W=16, storage=_lib.RC_RAW_U16, cfa=0, line_bytes=0, width=0, mode=0,
              reserved=(0, 0, 0), fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], white=1.0, reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.QuadDesc(mode=kw["mode"], reserved=(C.c_int32 * 3)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_quad(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["dst"], kw["dst_pitch"],
                           kw["b"], kw["H"], kw["W"], None) == -1, case                                       # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_raw_quad_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_quad", "rc_quad_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_quad_desc_size() == C.sizeof(_lib.QuadDesc) == 16
    assert lib.rc_raw_format_size() == C.sizeof(_lib.RawFormatDesc)                                            # the descriptor travels beside it
    header = _lib.HEADER.read_text()
    for name in ("RC_QUAD_REMOSAIC", "RC_QUAD_BIN"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert QuadBayer("remosaic").code == _lib.RC_QUAD_REMOSAIC and QuadBayer("bin").code == _lib.RC_QUAD_BIN
    Q = M.quad
    assert (Q.LANE_PX, Q.WAVE_SPAN, Q.BLOCK_SPAN, Q.WAVE_ROWS, Q.BLOCK_ROWS) == (4, 248, 496, 16, 32)
    src = (_lib.PKG / "csrc" / "quad.hip").read_text()                              # the constants the GPU tests place their seams on
    assert "kQdPx = 4" in src and "kQdSpan = 62 * kQdPx" in src and "kQdStrips = 2" in src and "kQdWaveRows = 16" in src and "kQdRows = 2 * kQdWaveRows" in src
    assert "raw_quad" in M.torch_ops.SCHEMAS


def test_raw_quad_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "quad.hip" in build.SOURCES
    res = build.kernel_resources()
    remosaic = {k: v for k, v in res.items() if "raw_quad_remosaic_kernel" in k}
    binned = {k: v for k, v in res.items() if "raw_quad_bin_kernel" in k}
    assert len(remosaic) == 14 and len(binned) == 7, (sorted(remosaic), sorted(binned))   # fp32, bf16, fp16, u16, u8, RAW10, RAW12 (x the two G layouts)
    mine = {**remosaic, **binned}
    assert all(v["tu"] == "quad.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 128 and v["sgprs"] <= 102 for v in mine.values())            # 4 waves per SIMD at least
    assert all(v["lds"] == 0 for v in mine.values())
    assert not [k for k, v in res.items() if v["tu"] == "quad.hip" and k not in mine]
