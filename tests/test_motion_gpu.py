"""Motion estimation on an MI355X: rc_motion_pyramid, rc_motion_search and ops.motion_estimate equal the NumPy restatement
(tests/motion_ref.py) bit for bit; the stabiliser closes the loop through ops.warp; forward_mosaic carries a Motion; graph replay."""
import ctypes as C

import numpy as np
import pytest
import torch

import liteisp_oracle as O
import motion_ref as R
import realcamnet_amd as M
from realcamnet_amd import _lib, ops

DEV = "cuda"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MATRICES = ("bt601", "bt709", "bt2020")


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def eq(t, a):
    a = torch.as_tensor(np.ascontiguousarray(a))
    return t.shape == a.shape and t.dtype == a.dtype and torch.equal(t.cpu(), a)


def source(shape, dt, seed):
    """A planar frame with values below 0 and above 1, NaNs, exact 0 / 1 and values that land on rounding ties, as `dt` stores it."""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g) * 1.4 - 0.2
    flat = y.view(-1)
    n = flat.numel()
    flat[torch.randperm(n, generator=g)[:max(1, n // 50)]] = float("nan")
    flat[torch.randperm(n, generator=g)[:max(1, n // 50)]] = 0.5 / 255.0 * 3                   # 1.5 / 255: a tie where the luma keeps it
    flat[torch.randperm(n, generator=g)[:max(1, n // 100)]] = 1.0
    flat[torch.randperm(n, generator=g)[:max(1, n // 100)]] = -0.0
    return y.to(dt)


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------------------------
PYR_CASES = (((2, 3, 40, 64), (37, 53), (1, 2, 3)), ((1, 3, 64, 255), None, (4,)), ((2, 3, 64, 257), None, (4,)), ((1, 3, 9, 8), None, (4,)),
             ((1, 3, 20, 520), (19, 518), (3, 4)))


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_pyramid_equals_restatement(hip, dt, matrix):
    for n, (shape, crop, levels) in enumerate(PYR_CASES):
        y = source(shape, dt, n)
        h, w = crop or shape[2:]
        want = R.pyramid(y.float().numpy()[:, :, :h, :w], max(levels), matrix)
        yd = y.to(DEV)
        for lv in levels:
            got = ops.motion_pyramid(yd, lv, matrix, crop_hw=crop)
            assert len(got) == lv
            for k in range(lv):
                assert eq(got[k], want[k]), (shape, crop, lv, k, int((got[k].cpu() != torch.as_tensor(want[k])).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_level_0_is_the_full_range_nv12_luma(hip, dt):
    y = source((2, 3, 40, 72), dt, 11).to(DEV)
    crop = (36, 70)
    for m in MATRICES:
        nv12 = ops.yuv_encode(y, M.OutFormat("nv12", matrix=m, range="full"), crop_hw=crop)
        assert torch.equal(ops.motion_pyramid(y, 1, m, crop_hw=crop)[0], nv12.planes[0].contiguous()), m
        st = ops.frame_stats(y, M.Stats(grid=(1, 1), matrix=m), crop_hw=crop)
        lv0 = ops.motion_pyramid(y, 1, m, crop_hw=crop)[0]
        counts = torch.stack([torch.bincount(f.flatten().long(), minlength=256) for f in lv0])
        assert torch.equal(st.hist[:, 3], counts), m


# ---- 2. the search ----------------------------------------------------------------------------------------------------------------------------
def planes(hs, ws, shifts, noise=0, seed=0):
    """cur, ref (B,hs,ws) uint8: ref a crop of a blurred noise scene, cur[b] the crop moved by shifts[b]; `noise` > 0 adds +-noise to cur."""
    sc = np.rint(R.scene(hs, ws, seed) * 255).astype(np.int64)
    m = R.MARGIN
    ref = np.stack([sc[m:m + hs, m:m + ws]] * len(shifts))
    cur = np.stack([sc[m + dy:m + dy + hs, m + dx:m + dx + ws] for dx, dy in shifts])
    if noise:
        cur = cur + np.random.default_rng(seed + 1).integers(-noise, noise + 1, cur.shape)
    return np.clip(cur, 0, 255).astype(np.uint8), np.clip(ref, 0, 255).astype(np.uint8)


def check_search(cur, ref, block, rng, pred=None, shift=0):
    want = R.search(cur, ref, block, rng, pred, shift)
    got = ops.motion_search(dev(cur), dev(ref), block, rng, pred=None if pred is None else dev(pred), pred_shift=shift)
    assert eq(got, want), (cur.shape, block, rng, shift, (got.cpu().numpy() != want).reshape(-1, 4).sum(0).tolist())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("rng", (0, 1, 4, 8))
@pytest.mark.parametrize("block", (8, 16, 32))
def test_search_equals_restatement(hip, block, rng):
    shifts = [(3, -2), (-7, 5), (0, 1)]                                                       # B = 3, a shift per frame
    cur, ref = planes(70, 53, shifts)                                                          # ws is no multiple of 4; block 32: one column of blocks
    want = check_search(cur, ref, block, rng)
    if rng == 8 and block >= 16:
        inner = want[:, 1:-1, 1:-1] if block == 16 else want[:, :0]
        for b, (dx, dy) in enumerate(shifts):
            assert (inner[b, ..., 0] == dx).all() and (inner[b, ..., 1] == dy).all()
    noisy, _ = planes(70, 53, shifts, noise=6, seed=4)
    want = check_search(noisy, ref, block, rng)
    assert (want[..., 2] > 0).all()                                                            # a pair where no cost is 0
    by, bx = 70 // block, 53 // block
    g = np.random.default_rng(block + rng)
    same = np.zeros((3, by, bx, 4), np.int32)
    same[..., :2] = g.integers(-6, 7, (3, by, bx, 2))
    same[..., 2:] = g.integers(0, 1 << 30, (3, by, bx, 2))                                     # slots 2 and 3 of a predictor are not read
    check_search(cur, ref, block, rng, same, 0)
    coarse = np.zeros((3, max(1, by // 2), max(1, (bx + 1) // 2), 4), np.int32)
    coarse[..., :2] = g.integers(-3, 4, coarse.shape[:3] + (2,))
    check_search(noisy, ref, block, rng, coarse, 1)
    one = np.zeros((3, 1, 1, 4), np.int32)                                                     # a grid smaller than by / 2: the min() clamp
    one[:, 0, 0, :2] = [(1, -1), (-2, 2), (4, 0)]
    check_search(cur, ref, block, rng, one, 1)
    check_search(cur, ref, block, rng, one, 0)


@pytest.mark.gpu
def test_search_with_wild_predictors(hip):
    """Predictors far outside the plane, beyond the +-32768 bound, and the extreme ints: every index is clamped, nothing else is read."""
    cur, ref = planes(40, 52, [(2, 1), (-1, 0)], noise=3, seed=2)
    for block, rng in ((8, 2), (16, 1), (32, 8)):
        by, bx = 40 // block, 52 // block
        pred = np.zeros((2, by, bx, 4), np.int32)
        vals = [(1000, -1000), (-1000, 1000), (40000, -40000), (-40000, 40000), (2147483647, -2147483648), (-32768, 32767), (32767, -32768), (7, -45), (-60, 3), (51, 39)]
        for n in range(by * bx):
            pred[0].reshape(-1, 4)[n, :2] = vals[n % len(vals)]
            pred[1].reshape(-1, 4)[n, :2] = vals[(n + 3) % len(vals)][::-1]
        for shift in (0, 1):
            want = check_search(cur, ref, block, rng, pred, shift)
            assert np.abs(want[..., :2]).max() <= (32768 << shift) + rng


@pytest.mark.gpu
def test_search_flat_periodic_and_single_block(hip):
    flat = np.full((2, 64, 48), 131, np.uint8)
    pred = np.zeros((2, 2, 1, 4), np.int32)
    pred[0, ..., :2], pred[1, ..., :2] = (5, -3), (-1000, 20)
    for block, rng in ((16, 4), (32, 8), (8, 0)):
        for shift in (0, 1):
            want = check_search(flat, flat, block, rng, pred, shift)
            assert (want[..., 2:] == 0).all()                                                  # cost 0 and texture 0 ...
            assert (want[0, ..., 0] == 5 << shift).all() and (want[1, ..., 1] == 20 << shift).all()            # ... at the predictor itself
    x = np.arange(96)
    for period, rng in ((4, 8), (2, 4), (4, 4)):                                               # the period divides R: ties along x, and every oy ties
        per = np.broadcast_to(((x % period) * 40 + 9).astype(np.uint8)[None, None, :], (1, 48, 96)).copy()
        for block in (8, 16, 32):
            want = check_search(per, per, block, rng)
            assert (want[0, :, 1:-1, :3] == 0).all()                                            # (0, 0) wins among the zero-cost offsets
            moved = np.roll(per, 1, axis=2)
            check_search(per, moved, block, rng)
    for block, (hs, ws) in ((8, (9, 8)), (16, (16, 31)), (32, (33, 63))):                       # by bx = 1
        cur, ref = planes(hs, ws, [(1, -1)], seed=5)
        assert check_search(cur, ref, block, 8).shape == (1, 1, 1, 4)
        assert check_search(cur, ref, block, 1).shape == (1, 1, 1, 4)


# ---- 3. the whole estimate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", R.SCENES, ids=lambda c: "x".join(map(str, c[0])))
def test_motion_estimate_equals_restatement(hip, case):
    (h, w), (dx, dy), levels, block, search, refine = case
    cur, ref = R.scene_pair(case)
    want = R.estimate(R.pyramid(cur, levels), R.pyramid(ref, levels), block, search, refine)
    m = M.Motion(levels=levels, block=block, search=search, refine=refine)
    pc, pr = ops.motion_pyramid(dev(cur), levels), ops.motion_pyramid(dev(ref), levels)
    f = ops.motion_estimate(pc, pr, m)
    assert isinstance(f, M.MotionField) and f.frame == (h, w) and f.spec is m and len(f.levels) == levels and f.levels[0] is f.vectors
    for k in range(levels):
        assert eq(f.levels[k], want[k]), k
    assert f.global_shift().tolist() == [[dx, dy]] and f.global_shift().is_cuda
    assert f.mesh()[0, 0, 0].tolist() == [dx, dy]


@pytest.mark.gpu
def test_stabilisation_closes_the_loop(hip):
    """Three frames cut from one scene at integer offsets; pyramid, estimate against the previous frame, Stabilizer(alpha=0), ops.warp with
    bilinear taps: every frame comes back as frame 0 on the interior, exactly (taps at integer positions are exact in rc_warp)."""
    h, w = 128, 160
    offsets = [(0, 0), (5, -3), (-4, 6)]
    sc = R.scene(h, w, seed=9)
    frames = [dev(R.crop(sc, h, w, o)) for o in offsets]
    m = M.Motion(levels=2, block=16, search=4, refine=1)
    stab = M.Stabilizer(alpha=0.0)
    prev = None
    far = max(max(abs(v) for v in o) for o in offsets)
    for k, y in enumerate(frames):
        cur = ops.motion_pyramid(y, m.levels, m.matrix)
        field = ops.motion_estimate(cur, cur if prev is None else prev, m)
        want = (0, 0) if k == 0 else (offsets[k][0] - offsets[k - 1][0], offsets[k][1] - offsets[k - 1][1])
        assert field.global_shift().tolist() == [list(want)], k
        mesh = stab.update(field)
        assert mesh.is_cuda and mesh.shape == (1, h // 16 + 1, w // 16 + 1, 2)
        out = ops.warp(y, mesh, size=(h, w), cell=16, interp="bilinear")
        assert torch.equal(out[..., far:h - far, far:w - far], frames[0][..., far:h - far, far:w - far]), k
        prev = cur
    assert stab.c.tolist() == [[4.0, -6.0]]


# ---- 4. forward_mosaic ------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def net_on_gpu(name, dt):
    key = (name, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        _NETS[key] = getattr(M, name)().to(device=DEV, dtype=dt).eval()
    return _NETS[key]


def tsame(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


@pytest.mark.gpu
def test_forward_mosaic_with_motion(hip):
    dt = torch.bfloat16
    net = net_on_gpu("LiteISPNet_GFM_LSC", dt)
    g = torch.Generator().manual_seed(7)
    m1 = (torch.rand(2, 1, 144, 208, generator=g) * 1.4 - 0.2).to(DEV, dt)
    m2 = (torch.rand(2, 1, 144, 208, generator=g) * 1.4 - 0.2).to(DEV, dt)
    coord = O.make_coord(2, 72, 104).to(DEV, dt)
    nv12 = M.OutFormat("nv12")
    st = M.MotionState()
    mo = M.Motion(levels=2, block=16, search=3, state=st)
    with torch.no_grad():
        y1, y2 = net.forward_mosaic(m1, None, coord), net.forward_mosaic(m2, None, coord)
        plain = net.forward_mosaic(m2, None, coord, outputs=[M.Output("rgb8"), M.Output(nv12, M.Resize((72, 104)))])
        f1 = net.forward_mosaic(m1, None, coord, out_format=mo)
        q8, f2, small = net.forward_mosaic(m2, None, coord, outputs=[M.Output("rgb8"), M.Output(mo), M.Output(nv12, M.Resize((72, 104)))])
    p1, p2 = ops.motion_pyramid(y1, 2), ops.motion_pyramid(y2, 2)
    own = ops.motion_estimate(p1, p1, mo)
    assert isinstance(f1, M.MotionField) and f1.vectors.shape == (2, 9, 13, 4) and f1.frame == (144, 208)
    assert (f1.vectors[..., :3] == 0).all() and tsame(f1.vectors, own.vectors) and (f1.vectors[..., 3] > 0).any()      # the first call: zero vectors, the real texture
    want = ops.motion_estimate(p2, p1, mo)
    assert all(tsame(a, b) for a, b in zip(f2.levels, want.levels)) and (f2.vectors[..., 2] > 0).any()
    assert all(tsame(a, b) for a, b in zip(st.levels, p2))                                                                # the state is the last frame's pyramid
    assert tsame(q8, plain[0]) and tsame(small.buffer, plain[1].buffer)                                                   # the other rungs do not notice
    st.reset()
    with torch.no_grad():
        f3 = net.forward_mosaic(m2, None, coord, out_format=mo)
        f4 = net.forward_mosaic(m1, None, coord, out_format=mo)
        none = net.forward_mosaic(m1, None, coord, out_format=M.Motion(levels=2, block=16, search=3))
    assert (f3.vectors[..., :3] == 0).all() and tsame(f3.vectors, ops.motion_estimate(p2, p2, mo).vectors)               # reset(): like a first call
    assert tsame(f4.vectors, ops.motion_estimate(p1, p2, mo).vectors)
    assert tsame(none.vectors, own.vectors)                                                                                # no state: against itself
    kept = [t.clone() for t in st.levels]
    mark = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"cannot be captured.*ops\.motion_pyramid.*ops\.motion_estimate"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                mark.add_(1.0)                                                                                             # the graph is not empty when the capture ends
                net.forward_mosaic(m2, None, coord, out_format=mo)
    torch.cuda.synchronize()
    assert all(tsame(a, b) for a, b in zip(st.levels, kept))                                                              # refused before the state was touched


# ---- 5. graph replay, reproducibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_ops_equal_eager(hip):
    m = M.Motion(levels=3, block=8, search=5, refine=2)
    ya, yb, yc = (source((2, 3, 72, 100), torch.bfloat16, s).to(DEV) for s in (21, 22, 23))

    def fn(y, r):
        cur, ref = ops.motion_pyramid(y, 3, crop_hw=(70, 99)), ops.motion_pyramid(r, 3, crop_hw=(70, 99))
        return cur + list(ops.motion_estimate(cur, ref, m).levels)
    flat = lambda outs: [t.clone() for t in outs]
    e1, e2 = flat(fn(ya, yb)), flat(fn(yc, ya))
    call = M.GraphedCall(fn)
    g1, g2, g3 = flat(call(ya, yb)), flat(call(yc, ya)), flat(call(yc, ya))
    assert all(tsame(a, b) for a, b in zip(g1, e1)) and all(tsame(a, b) for a, b in zip(g2, e2)) and all(tsame(a, b) for a, b in zip(g3, e2))
    assert not tsame(g1[0], g2[0]) and not tsame(g1[3], g2[3])


@pytest.mark.gpu
def test_same_call_twice_and_prefilled_outputs(hip):
    y = source((2, 3, 40, 64), torch.float16, 31)
    crop = (37, 53)
    want = R.pyramid(y.float().numpy()[:, :, :37, :53], 3, "bt2020")
    yd = y.to(DEV)
    mine = [torch.empty(s, dtype=torch.uint8, device=DEV).fill_(0xA5) for s in ((2, 37, 53), (2, 18, 26), (2, 9, 13))]
    got = ops.motion_pyramid(yd, 3, "bt2020", crop_hw=crop, out=mine)
    again = ops.motion_pyramid(yd, 3, "bt2020", crop_hw=crop)
    assert all(a is b for a, b in zip(got, mine)) and all(eq(a, b) for a, b in zip(mine, want)) and all(eq(a, b) for a, b in zip(again, want))
    cur, ref = planes(70, 53, [(2, 2), (-3, 1)], noise=4, seed=6)
    want = R.search(cur, ref, 8, 3)
    cd, rd = dev(cur), dev(ref)
    out = torch.empty(2, 8, 6, 4, dtype=torch.int32, device=DEV)
    out.view(torch.uint8).fill_(0x7F)
    assert ops.motion_search(cd, rd, 8, 3, out=out) is out and eq(out, want) and eq(ops.motion_search(cd, rd, 8, 3), want)
    out.view(torch.uint8).fill_(0x7F)
    d = _lib.MotionDesc(block=8, range=3, pred_shift=0)
    rc = hip.rc_motion_search(cd.data_ptr(), rd.data_ptr(), C.byref(d), None, 0, 0, out.data_ptr(), 2, 70, 53, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.rc_last_error()
    assert eq(out, want)                                                                        # every element written
