"""Motion estimation, host side (no GPU): validation of Motion / Stabilizer and of the C entries, the ABI, fake-tensor traces, MotionField and
Stabilizer on CPU tensors, and the NumPy reference (tests/motion_ref.py) recovering known shifts.

What the reference gives on the three scenes of motion_ref.SCENES (grey noise, 5 x 5 box mean, crops of one scene):
    192 x 192, (13, -6), 3 / 16 / 4 / 1:   144 blocks, all exact
    200 x 264, (5, 3),   2 /  8 / 4 / 1:   825 blocks, all exact
    192 x 256, (-21, 10), 3 / 16 / 7 / 1:  192 blocks, every block off the outer ring exact, 93.75 % of all, global_shift exact
Costs are not 0 on the ring: a block whose match lies partly outside the reference frame is compared with clamped pixels.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F32

import motion_ref as R


# ---- 1. the request -----------------------------------------------------------------------------------------------------------------------
def test_motion_validation_identity_and_immutability():
    m = M.Motion()
    assert (m.levels, m.block, m.search, m.refine, m.matrix, m.state) == (3, 16, 4, 1, "bt709", None)
    for kw in (dict(levels=0), dict(levels=5), dict(block=4), dict(block=24), dict(block=64), dict(search=0), dict(search=9), dict(refine=-1), dict(refine=3),
               dict(matrix="bt470"), dict(matrix=None)):
        with pytest.raises(ValueError):
            M.Motion(**kw)
    for kw in (dict(levels=2.0), dict(levels=True), dict(block="16"), dict(search=1.5), dict(refine=None), dict(state="state"), dict(state=M.TemporalState())):
        with pytest.raises(TypeError):
            M.Motion(**kw)
    with pytest.raises(Exception):
        m.levels = 2                                                            # frozen
    assert M.Motion() != M.Motion() and m == m and len({m, M.Motion()}) == 2    # eq=False: compared by identity, as Temporal is
    st = M.MotionState()
    assert M.Motion(state=st).state is st and st.levels is None
    assert m.check(2160, 3840) == (135, 240) and M.Motion(levels=1, block=8).check(9, 8) == (1, 1)
    assert M.Motion(levels=4, block=8).check(64, 64) == (8, 8)
    for hw in ((63, 64), (64, 63), (0, 64)):
        with pytest.raises(ValueError):
            M.Motion(levels=3, block=16).check(*hw)
    with pytest.raises(ValueError, match="2\\^29"):
        m.check(1 << 15, 1 << 14)
    assert m.level_shapes(2, 37, 53) == [(2, 37, 53), (2, 18, 26), (2, 9, 13)]


def test_stabilizer_validation():
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(max_shift=-1), dict(max_shift=float("inf"))):
        with pytest.raises(ValueError):
            M.Stabilizer(**kw)
    for kw in (dict(alpha="0.1"), dict(alpha=True), dict(max_shift=None)):
        with pytest.raises(TypeError):
            M.Stabilizer(**kw)
    with pytest.raises(TypeError):
        M.Stabilizer().update("field")


def test_output_carries_a_motion():
    m = M.Motion(levels=2, block=8)
    o = M.Output(m, M.Resize((72, 104)))
    assert o.format is m and o.plan(144, 208) == (72, 104)
    with pytest.raises(ValueError):
        M.Output(M.Motion(levels=4, block=32)).plan(144, 208)                   # level 3 is 18 x 26: no block of 32
    with pytest.raises(TypeError, match="a Motion"):
        M.Output(3.5)
    with pytest.raises(ValueError, match="a Motion"):
        M.Output("rgb12")


# ---- 2. MotionField and Stabilizer on CPU tensors -----------------------------------------------------------------------------------------------
def _field(vectors, frame=(64, 64), spec=None):
    v = torch.as_tensor(np.asarray(vectors), dtype=torch.int32)
    return M.MotionField(v, spec or M.Motion(), frame, [v])


def test_global_shift_is_the_lower_median_of_the_valid_blocks():
    rng = np.random.default_rng(3)
    v = np.zeros((3, 4, 5, 4), np.int32)
    v[..., 0] = rng.integers(-9, 10, (3, 4, 5))
    v[..., 1] = rng.integers(-9, 10, (3, 4, 5))
    v[..., 2] = rng.integers(0, 500, (3, 4, 5))
    v[..., 3] = rng.integers(0, 100, (3, 4, 5))
    v[2, ..., 3] = 0                                                            # frame 2: nothing passes min_texture
    f = _field(v)
    for mt, ms in ((0, None), (40, None), (40, 300), (0, 100)):
        ok = (v[..., 3] >= mt) & ((v[..., 2] <= ms) if ms is not None else True)
        assert torch.equal(f.valid(mt, ms), torch.as_tensor(ok))
        want = [[R.lower_median(v[b, ..., k][ok[b]]) for k in (0, 1)] for b in range(3)]
        got = f.global_shift(min_texture=mt, max_sad=ms)
        assert got.dtype == torch.int64 and got.tolist() == want, (mt, ms)
    assert f.global_shift(min_texture=1)[2].tolist() == [0, 0]                  # all blocks invalid -> 0
    assert _field(v[:1] * 0 + np.array([4, -2, 0, 0], np.int32)).global_shift(min_texture=1).tolist() == [[0, 0]]
    even = np.zeros((1, 1, 4, 4), np.int32)
    even[0, 0, :, 0] = [7, 1, 5, 3]
    assert _field(even).global_shift().tolist() == [[3, 0]]                     # four values: the lower of the two middle ones


def test_mesh_nodes_and_shapes():
    v = np.zeros((2, 2, 2, 4), np.int32)
    v[0, ..., 0], v[0, ..., 1], v[1, ..., 0], v[1, ..., 1] = 3, -2, -5, 7
    f = _field(v, frame=(40, 70))
    m = f.mesh()
    assert m.shape == (2, 4, 6, 2) and m.dtype == torch.float32                 # ceil(40 / 16) + 1, ceil(70 / 16) + 1
    for b, (sx, sy) in enumerate(((3, -2), (-5, 7))):
        for j in range(4):
            for i in range(6):
                assert m[b, j, i].tolist() == [16 * i + sx, 16 * j + sy]
    m = f.mesh((33, 17), cell=8, shift=torch.tensor([[0.5, -1.25]]))
    assert m.shape == (1, 6, 4, 2) and m[0, 5, 3].tolist() == [24.5, 38.75]
    with pytest.raises(ValueError):
        f.mesh(shift=torch.zeros(3, 2))
    with pytest.raises(ValueError):
        f.mesh((0, 8))


def _shift_field(dx, dy):
    v = np.zeros((1, 3, 3, 4), np.int32)
    v[..., 0], v[..., 1], v[..., 3] = dx, dy, 10
    return _field(v, frame=(48, 48))


def test_stabilizer_paths():
    shifts = [(0, 0), (3, -1), (-2, 4), (5, 5)]
    ident = _shift_field(0, 0).mesh(shift=torch.zeros(1, 2))
    s = M.Stabilizer(alpha=1.0)
    for d in shifts:
        assert torch.equal(s.update(_shift_field(*d)), ident)                   # alpha = 1: the identity mesh
    s = M.Stabilizer(alpha=0.0)
    cx = cy = 0
    for d in shifts:
        mesh = s.update(_shift_field(*d))
        cx, cy = cx - d[0], cy - d[1]
        assert mesh[0, 0, 0].tolist() == [cx, cy] and mesh[0, 2, 1].tolist() == [16 + cx, 32 + cy]      # alpha = 0: e is the accumulated shift
    assert s.c.tolist() == [[-6.0, -8.0]] and s.s.tolist() == [[0.0, 0.0]]
    s.reset()
    assert s.c is None and s.update(_shift_field(1, 1))[0, 0, 0].tolist() == [-1.0, -1.0]
    s = M.Stabilizer(alpha=0.0, max_shift=4)
    for d, want in (((3, -1), [-3, 1]), ((3, -9), [-4, 4]), ((-1, 1), [-4, 4]), ((-3, 7), [-2, 2])):
        assert s.update(_shift_field(*d))[0, 0, 0].tolist() == want                                      # the clamp; the state itself is not clamped
    s = M.Stabilizer(alpha=0.5)
    s.update(_shift_field(0, 0))
    assert s.update(_shift_field(-8, 4))[0, 0, 0].tolist() == [4.0, -2.0]       # c = (8, -4), s = (4, -2), e = c - s


# ---- 3. the reference recovers a known shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SCENES, ids=lambda c: "x".join(map(str, c[0])))
def test_reference_recovers_the_shift(case):
    (h, w), (dx, dy), levels, block, search, refine = case
    cur, ref = R.scene_pair(case)
    assert np.array_equal(cur[0, 0, max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)],
                          ref[0, 0, max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)])                     # cur[y][x] = ref[y + dy][x + dx]
    res = R.estimate(R.pyramid(cur, levels), R.pyramid(ref, levels), block, search, refine)
    v = res[0]
    assert v.shape == (1, h // block, w // block, 4)
    exact = (v[0, ..., 0] == dx) & (v[0, ..., 1] == dy)
    print(f"{case}: {exact.size} blocks, {100.0 * exact.mean():.2f} % exact, ring {100.0 * (exact.sum() - exact[1:-1, 1:-1].sum()) / (exact.size - exact[1:-1, 1:-1].size):.2f} %")
    assert exact[1:-1, 1:-1].all()                                              # every block off the outer ring
    f = M.MotionField(torch.as_tensor(v), M.Motion(levels=levels, block=block, search=search, refine=refine), (h, w), [torch.as_tensor(r) for r in res])
    assert f.global_shift().tolist() == [[dx, dy]]
    assert f.mesh()[0, 0, 0].tolist() == [dx, dy]


def test_reference_tie_rule_and_flat_frames():
    flat = np.full((1, 32, 32), 77, np.uint8)
    pred = np.zeros((1, 1, 1, 4), np.int32)
    pred[..., 0], pred[..., 1] = 5, -3
    out = R.search(flat, flat, 16, 4, pred, 1)
    assert (out[..., 0] == 10).all() and (out[..., 1] == -6).all() and (out[..., 2:] == 0).all()             # a flat frame returns its predictor
    x = np.arange(64)
    per = np.broadcast_to(((x % 4) * 60).astype(np.uint8)[None, None, :], (1, 32, 64)).copy()                 # period 4 along x, constant along y
    out = R.search(per, per, 8, 4)
    assert (out[0, 1:-1, 1:-1, :3] == 0).all()                                                                  # cost 0 at ox = -4, 0, 4 and every oy: (0, 0) wins


# ---- 4. refusals before any launch, fake traces ---------------------------------------------------------------------------------------------------
def test_ops_refuse_before_any_launch_and_fake_traces():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.motion_pyramid(torch.zeros(1, 3, 16, 16), 2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.motion_search(torch.zeros(1, 16, 16, dtype=torch.uint8), torch.zeros(1, 16, 16, dtype=torch.uint8), 8, 1)
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 40, 64, dtype=torch.bfloat16)
            for bad in (0, 5, 2.0, True):
                with pytest.raises(ValueError, match="levels"):
                    ops.motion_pyramid(y, bad)
            with pytest.raises(ValueError, match="matrix"):
                ops.motion_pyramid(y, 2, matrix="bt470")
            for crop in ((41, 64), (40, 65), (0, 8)):
                with pytest.raises(ValueError):
                    ops.motion_pyramid(y, 1, crop_hw=crop)
            with pytest.raises(ValueError, match="empty"):
                ops.motion_pyramid(y, 4, crop_hw=(7, 64))
            with pytest.raises(ValueError):
                ops.motion_pyramid(torch.empty(2, 4, 40, 64), 2)
            with pytest.raises(TypeError):
                ops.motion_pyramid(y.to(torch.float64), 2)
            with pytest.raises(ValueError, match="out"):
                ops.motion_pyramid(y, 2, out=[torch.empty(2, 40, 64, dtype=torch.uint8)])
            with pytest.raises(ValueError, match="out"):
                ops.motion_pyramid(y, 1, out=[torch.empty(2, 40, 64, dtype=torch.int8)])
            lv = ops.motion_pyramid(y, 3, "bt601", crop_hw=(37, 53))
            assert [tuple(t.shape) for t in lv] == [(2, 37, 53), (2, 18, 26), (2, 9, 13)] and all(t.dtype == torch.uint8 and t.device.type == "cuda" for t in lv)
            mine = [torch.empty(2, 40, 64, dtype=torch.uint8), torch.empty(2, 20, 32, dtype=torch.uint8)]
            got = ops.motion_pyramid(y, 2, out=mine)
            assert all(a is b for a, b in zip(got, mine))

            cur = torch.empty(2, 40, 53, dtype=torch.uint8)
            for kw in (dict(block=12), dict(range=9), dict(range=-1), dict(range=1.0), dict(pred_shift=2)):
                args = dict(block=8, range=2)
                args.update(kw)
                with pytest.raises(ValueError):
                    ops.motion_search(cur, cur, **args)
            with pytest.raises(ValueError, match="no block"):
                ops.motion_search(torch.empty(2, 24, 53, dtype=torch.uint8), torch.empty(2, 24, 53, dtype=torch.uint8), 32, 1)
            with pytest.raises(ValueError):
                ops.motion_search(cur, torch.empty(2, 40, 52, dtype=torch.uint8), 8, 1)
            with pytest.raises(ValueError):
                ops.motion_search(cur.to(torch.int32), cur.to(torch.int32), 8, 1)
            with pytest.raises(ValueError, match="pred"):
                ops.motion_search(cur, cur, 8, 1, pred=torch.empty(2, 2, 3, 4, dtype=torch.int64))
            with pytest.raises(ValueError, match="pred"):
                ops.motion_search(cur, cur, 8, 1, pred=torch.empty(1, 2, 3, 4, dtype=torch.int32))
            with pytest.raises(ValueError, match="out"):
                ops.motion_search(cur, cur, 8, 1, out=torch.empty(2, 5, 6, 3, dtype=torch.int32))
            with pytest.raises(ValueError, match="2\\^29"):
                ops.motion_search(torch.empty(1, 1 << 15, 1 << 14, dtype=torch.uint8), torch.empty(1, 1 << 15, 1 << 14, dtype=torch.uint8), 8, 1)
            out = ops.motion_search(cur, cur, 8, 3, pred=torch.empty(2, 2, 3, 4, dtype=torch.int32), pred_shift=1)
            assert out.shape == (2, 5, 6, 4) and out.dtype == torch.int32 and out.device.type == "cuda"
            e = torch.ops.realcam.motion_search(cur, cur, None, out, 8, 3, 0)
            assert e.numel() == 0
            e = torch.ops.realcam.motion_pyramid(y, mine, 1, 40, 64)
            assert e.numel() == 0

            m = M.Motion(levels=2, block=8, search=3)
            with pytest.raises(TypeError):
                ops.motion_estimate(lv, lv, "motion")
            with pytest.raises(ValueError, match="levels"):
                ops.motion_estimate(lv, lv, m)
            with pytest.raises(ValueError):
                ops.motion_estimate(lv[:2], [lv[0], lv[0]], m)
            f = ops.motion_estimate(lv[:2], lv[:2], m)
            assert isinstance(f, M.MotionField) and f.vectors.shape == (2, 4, 6, 4) and f.frame == (37, 53) and f.spec is m
            assert [tuple(t.shape) for t in f.levels] == [(2, 4, 6, 4), (2, 2, 3, 4)] and f.levels[0] is f.vectors
            assert f.valid(1).shape == (2, 4, 6) and f.global_shift().shape == (2, 2) and f.mesh().shape == (2, 4, 5, 2)

            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=m, outputs=[M.Output(m)])
                for bad in ([M.Output(M.Motion(levels=3, block=16))], [M.Output(None), M.Output(M.Motion(levels=1, block=16), M.Resize((8, 8)))]):
                    with pytest.raises(ValueError, match="smaller than one block"):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                with pytest.raises(ValueError, match="smaller than one block"):
                    net.forward_mosaic(mosaic, None, coord, out_format=M.Motion(levels=4, block=8))
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, out_format=M.Motion)
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(m)])


def test_fake_trace_of_forward_mosaic_with_motion():
    """forward_mosaic(out_format=Motion(...)) and a ladder with a Motion under FakeTensorMode, with and without a state."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    st = M.MotionState()
                    m = M.Motion(levels=3, block=16, state=st)
                    with torch.no_grad():
                        one = net.forward_mosaic(mosaic, None, coord, out_format=m)
                        first = st.levels
                        two = net.forward_mosaic(mosaic, None, coord, out_format=m)
                        a, b, c = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output("rgb8"), M.Output(M.Motion(levels=2, block=8), M.Resize((72, 104))), M.Output(None)])
                    for f in (one, two):
                        assert isinstance(f, M.MotionField) and f.vectors.shape == (2, 9, 13, 4) and f.vectors.dtype == torch.int32 and f.frame == (144, 208)
                        assert [tuple(t.shape) for t in f.levels] == [(2, 9, 13, 4), (2, 4, 6, 4), (2, 2, 3, 4)] and f.vectors.device.type == "cuda"
                    assert [tuple(t.shape) for t in st.levels] == [(2, 144, 208), (2, 72, 104), (2, 36, 52)]
                    assert st._spare is first and st.levels is not first                                   # the two sets swapped
                    st.reset()
                    assert st.levels is None
                    assert a.shape == (2, 144, 208, 3) and isinstance(b, M.MotionField) and b.vectors.shape == (2, 9, 13, 4) and b.frame == (72, 104)
                    assert c.shape == (2, 3, 144, 208)
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null levels", dict(ptrs=None), b"null"), ("null level", dict(ptrs=(FAKE, 0)), b"null level"),
    ("bad dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("unknown dtype", dict(sdt=7), b"dtype"),
    ("matrix", dict(matrix=3), b"matrix"), ("matrix < 0", dict(matrix=-1), b"matrix"),
    ("levels 0", dict(levels=0), b"levels"), ("levels 5", dict(levels=5, ptrs=(FAKE,) * 5), b"levels"),
    ("coarsest empty rows", dict(levels=4, ptrs=(FAKE,) * 4, h=7), b"coarsest"), ("coarsest empty columns", dict(levels=3, ptrs=(FAKE,) * 3, w=3), b"coarsest"),
    ("h > H", dict(h=17), b"bad shape"), ("w > W", dict(w=17), b"bad shape"), ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"),
    ("too many frames", dict(b=65536), b"65535"), ("plane too large", dict(H=1 << 15, W=1 << 14), b"2^29"),
    ("src misaligned", dict(src=FAKE + 2), b"misaligned"), ("bf16 src misaligned", dict(sdt=RC_BF16, src=FAKE + 1), b"misaligned"),
])
def test_motion_pyramid_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, matrix=1, levels=2, ptrs=(FAKE, FAKE), b=1, H=16, W=16, h=8, w=8)
    kw.update(kwargs)
    ptrs = None if kw["ptrs"] is None else (C.c_void_p * len(kw["ptrs"]))(*kw["ptrs"])
    lib = _lib.load()
    assert lib.rc_motion_pyramid(kw["src"], kw["sdt"], kw["matrix"], kw["levels"], ptrs, kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None) == -1, case
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null cur", dict(cur=None), b"null"), ("null ref", dict(ref=None), b"null"), ("null desc", dict(desc=False), b"null"), ("null out", dict(out=None), b"null"),
    ("out misaligned", dict(out=FAKE + 8), b"16-byte"), ("pred misaligned", dict(pred=FAKE + 4), b"16-byte"),
    ("block 0", dict(block=0), b"block"), ("block 12", dict(block=12), b"block"), ("block 64", dict(block=64), b"block"),
    ("range -1", dict(range=-1), b"range"), ("range 9", dict(range=9), b"range"),
    ("shift 2", dict(shift=2), b"pred_shift"), ("shift -1", dict(shift=-1), b"pred_shift"),
    ("reserved", dict(reserved=(0, 0, 0, 0, 1)), b"reserved"), ("reserved first", dict(reserved=(7, 0, 0, 0, 0)), b"reserved"),
    ("no rows of blocks", dict(hs=15), b"smaller than one block"), ("no columns of blocks", dict(ws=15), b"smaller than one block"),
    ("empty", dict(hs=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"65535"),
    ("pred_by 0", dict(pred=FAKE, pby=0), b"pred_by"), ("pred_bx 0", dict(pred=FAKE, pbx=0), b"pred_by"),
    ("plane too large", dict(hs=1 << 15, ws=1 << 14), b"2^29"),
])
def test_motion_search_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(cur=FAKE, ref=FAKE, desc=True, pred=None, pby=1, pbx=1, out=FAKE, b=1, hs=32, ws=32, block=16, range=2, shift=0, reserved=(0,) * 5)
    kw.update(kwargs)
    d = _lib.MotionDesc(block=kw["block"], range=kw["range"], pred_shift=kw["shift"], reserved=(C.c_int32 * 5)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_motion_search(kw["cur"], kw["ref"], C.byref(d) if kw["desc"] else None, kw["pred"], kw["pby"], kw["pbx"], kw["out"], kw["b"], kw["hs"], kw["ws"],
                                None) == -1, case
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_motion_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_motion_pyramid", "rc_motion_search", "rc_motion_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_motion_desc_size() == C.sizeof(_lib.MotionDesc) == 32
    header = _lib.HEADER.read_text()
    for name in ("RC_MOTION_MAX_LEVELS", "RC_MOTION_MAX_RANGE"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert M.motion.MAX_LEVELS == 4 and M.motion.MAX_RANGE == 8 and M.motion.BLOCKS == (8, 16, 32)
    for name in ("motion_pyramid", "motion_search"):
        assert name in M.torch_ops.SCHEMAS
    for name in ("Motion", "MotionField", "MotionState", "Stabilizer"):
        assert name in M.__all__


def test_motion_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "motion.hip" in build.SOURCES
    res = build.kernel_resources()
    pyr = {k: v for k, v in res.items() if "motion_pyramid_kernel" in k}
    srch = {k: v for k, v in res.items() if "motion_search_kernel" in k}
    assert len(pyr) == 3 and len(srch) == 3, (sorted(pyr), sorted(srch))       # one per source dtype; one per block size
    mine = {**pyr, **srch}
    assert all(v["tu"] == "motion.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 64 for v in mine.values())                         # 8 waves per SIMD
    assert all(v["lds"] == 0 for v in pyr.values()) and all(0 < v["lds"] <= 20 * 1024 for v in srch.values())
    assert not [k for k, v in res.items() if v["tu"] == "motion.hip" and k not in mine]
