"""Motion-compensated temporal noise reduction without a GPU: the validation of TemporalMotion, Temporal(motion=) and the new ops
arguments, every refusal of rc_raw_motion_pyramid and rc_raw_temporal_mc through the C ABI, the integer square root of the proxy over its
whole domain, the fake trace of the ops and of forward_mosaic, the kernels' resources, and -- on the reference alone
(tests/temporal_mc_ref.py) -- what the feature is for: on a moving scene every block finds the true vector, the compensated filter removes
the noise and the uncompensated one does not."""
import ctypes as C
import dataclasses
import math
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import motion_ref
import realcamnet_amd as M
import temporal_mc_ref as R
from realcamnet_amd import _lib
from realcamnet_amd.temporal import Temporal, TemporalMotion, TemporalState
from temporal_ref import F32, blacks_of, restated_temporal

NAN, INF = float("nan"), float("inf")


# ---- 1. the request ---------------------------------------------------------------------------------------------------------------------------
def test_temporal_motion_defaults_and_validation():
    tm = TemporalMotion()
    assert (tm.levels, tm.block, tm.search, tm.refine, tm.min_texture, tm.max_sad) == (3, 16, 4, 1, 0, None)
    spec = tm.spec()
    assert isinstance(spec, M.Motion) and (spec.levels, spec.block, spec.search, spec.refine, spec.state) == (3, 16, 4, 1, None)
    assert TemporalMotion(levels=4, block=32, search=8, refine=2, min_texture=100, max_sad=0).max_sad == 0
    for kw in (dict(levels=0), dict(levels=5), dict(block=12), dict(block=64), dict(search=0), dict(search=9), dict(refine=-1), dict(refine=3),
               dict(min_texture=-1), dict(max_sad=-1)):
        with pytest.raises(ValueError, match=f"TemporalMotion.{next(iter(kw))}"):
            TemporalMotion(**kw)
    for kw in (dict(levels=2.0), dict(block="16"), dict(search=True), dict(refine=None), dict(min_texture=1.5), dict(min_texture=None), dict(max_sad=2.5),
               dict(max_sad=False)):
        with pytest.raises(TypeError, match=f"TemporalMotion.{next(iter(kw))}"):
            TemporalMotion(**kw)


def test_temporal_motion_check_refuses_a_frame_without_a_whole_block_at_the_coarsest_level():
    tm = TemporalMotion()                                                          # level 2 of (h, w) cells needs 16 x 16: 64 x 64 cells
    assert tm.check(64, 64) == (4, 4) and tm.check(96, 160) == (6, 10) and tm.check(67, 130) == (4, 8)
    for h, w in ((63, 64), (64, 63), (16, 400)):
        with pytest.raises(ValueError, match="TemporalMotion: level 2 .* cells"):
            tm.check(h, w)
    assert TemporalMotion(levels=1, block=8).check(8, 9) == (1, 1)


def test_temporal_takes_a_motion_and_keeps_every_earlier_construction():
    t = Temporal((8.0, 0.03))
    assert t.motion is None and Temporal((8.0, 0.03), 0.25, 4.0, None, None).motion is None                # the new field is last and defaults
    tm = TemporalMotion(block=8)
    t = Temporal((8.0, 0.03), motion=tm, state=TemporalState())
    assert t.motion is tm and t.params() == (8.0, float(np.float32(0.03)), 0.125, 3.0)
    for bad in (M.Motion(), "block", 16, (3, 16, 4, 1)):
        with pytest.raises(TypeError, match="Temporal.motion"):
            Temporal((8.0, 0.03), motion=bad)
    t.check(2 * 32, 2 * 40)                                                        # block 8 at level 2: 32 x 32 cells
    with pytest.raises(ValueError, match="TemporalMotion"):
        t.check(2 * 31, 2 * 40)
    fmt = M.RawFormat(storage="u16", white_level=1023.0, temporal=t)
    assert fmt.validate((1, 64, 80)) == (64, 80)
    with pytest.raises(ValueError, match="TemporalMotion"):                        # every refusal before any launch
        fmt.validate((1, 62, 80))


def test_temporal_state_carries_the_field():
    st = TemporalState()
    assert st.frame is None and st.field is None
    st.frame, st.field = torch.zeros(1, 4, 4), torch.zeros(1, 1, 1, 4, dtype=torch.int32)
    st.reset()
    assert st.frame is None and st.field is None
    shapes = [(2, 8, 12), (2, 4, 6)]
    a = st.pyramids(shapes, torch.zeros(1))
    assert len(a) == 2 and a[0] is not a[1] and all([tuple(t.shape) for t in p] == shapes and all(t.dtype == torch.uint8 for t in p) for p in a)
    assert st.pyramids(shapes, torch.zeros(1)) is a                                # kept while they fit
    assert st.pyramids(shapes[:1], torch.zeros(1)) is not a and st.pyramids([(2, 8, 10)], torch.zeros(1))[0][0].shape == (2, 8, 10)
    st._pyramids = tuple([t.to(torch.int8) for t in p] for p in st._pyramids)      # another dtype does not fit
    assert all(t.dtype == torch.uint8 for p in st.pyramids([(2, 8, 10)], torch.zeros(1)) for t in p)


# ---- 2. the ops' arguments ----------------------------------------------------------------------------------------------------------------------
def test_ops_refuse_bad_arguments_before_anything_runs():
    fmt = M.RawFormat(storage="u16", black_level=64.0, white_level=1023.0, temporal=Temporal((8.0, 0.03)))
    x = torch.zeros(1, 64, 64, dtype=torch.uint16)
    for levels in (0, 5, 2.0, True, None):
        with pytest.raises(ValueError, match="levels must be an int in 1 .. 4"):
            M.ops.raw_motion_pyramid(x, fmt, levels)
    with pytest.raises(TypeError, match="RawFormat"):
        M.ops.raw_motion_pyramid(x, None, 3)
    with pytest.raises(ValueError, match="raw_defects"):                           # the proxy alone does not repair
        M.ops.raw_motion_pyramid(x, dataclasses.replace(fmt, defects=M.Defects(hot=(1.0, 0.0))), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ops.raw_motion_pyramid(x, fmt, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ops.raw_temporal(x, fmt, prev=torch.zeros(1, 64, 64), vectors=torch.zeros(1, 2, 2, 4, dtype=torch.int32))
    with FakeTensorMode():
        with torch.device("cuda"):
            x = torch.empty(2, 64, 80, dtype=torch.uint16)
            lv = M.ops.raw_motion_pyramid(x, fmt, 4)
            assert [tuple(t.shape) for t in lv] == [(2, 32, 40), (2, 16, 20), (2, 8, 10), (2, 4, 5)] and all(t.dtype == torch.uint8 for t in lv)
            assert M.ops.raw_motion_pyramid(x, fmt, 4, gain=1.5, out=lv)[0] is lv[0]
            M.ops.raw_motion_pyramid(x, fmt, 2, gain=torch.empty(2, 1))
            M.ops.raw_motion_pyramid(torch.empty(2, 64, 100, dtype=torch.uint8), M.RawFormat(storage="mipi10", width=80, white_level=1023.0), 1)
            with pytest.raises(ValueError, match="is empty"):
                M.ops.raw_motion_pyramid(torch.empty(1, 8, 80, dtype=torch.uint16), fmt, 4)
            for gain, err in ((0.0, ValueError), (-1.0, ValueError), (NAN, ValueError), (INF, ValueError), ("1", TypeError), (True, TypeError),
                              (torch.empty(3, 1), ValueError), (torch.empty(2), ValueError), (torch.empty(2, 1, dtype=torch.float64), ValueError)):
                with pytest.raises(err, match="gain"):
                    M.ops.raw_motion_pyramid(x, fmt, 2, gain=gain)
            for out in (lv[:3], [lv[0], lv[1], lv[2], lv[3].to(torch.int8)], [lv[1], lv[1], lv[2], lv[3]], [t[:, :, ::1].transpose(1, 2) for t in lv]):
                with pytest.raises(ValueError, match="out must be 4 contiguous uint8"):
                    M.ops.raw_motion_pyramid(x, fmt, 4, out=out)
            # the filter's new keywords
            prev, vec = torch.empty(2, 64, 80), torch.empty(2, 2, 2, 4, dtype=torch.int32)
            out = M.ops.raw_temporal(x, fmt, prev=prev, vectors=vec)
            assert out.shape == (2, 64, 80) and out.dtype == torch.float32
            assert M.ops.raw_temporal(x, fmt, prev=prev, out=out, vectors=torch.empty(2, 9, 1, 4, dtype=torch.int32), block=8) is out
            with pytest.raises(ValueError, match="give prev"):
                M.ops.raw_temporal(x, fmt, vectors=vec)
            for block in (4, 12, 64, 16.0, True, None):
                with pytest.raises(ValueError, match="block must be one of"):
                    M.ops.raw_temporal(x, fmt, prev=prev, vectors=vec, block=block)
            with pytest.raises(TypeError, match="vectors must be a tensor"):
                M.ops.raw_temporal(x, fmt, prev=prev, vectors=[[0, 0, 0, 0]])
            for bad in (torch.empty(2, 2, 2, 4, dtype=torch.int64), torch.empty(1, 2, 2, 4, dtype=torch.int32), torch.empty(2, 2, 2, 2, dtype=torch.int32),
                        torch.empty(2, 2, 4, dtype=torch.int32), torch.empty(2, 0, 2, 4, dtype=torch.int32), torch.empty(2, 2, 2, 8, dtype=torch.int32)[..., ::2]):
                with pytest.raises(ValueError, match="vectors must be a contiguous"):
                    M.ops.raw_temporal(x, fmt, prev=prev, vectors=bad)


def test_fake_trace_of_forward_mosaic_with_motion():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                st = TemporalState()
                t = Temporal((8.0, 0.03), gain=torch.empty(2, 1, dtype=torch.float32), state=st, motion=TemporalMotion(levels=2, block=16, min_texture=64, max_sad=4000))
                fmt = M.RawFormat(storage="mipi12", cfa="GRBG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=4095.0, temporal=t)
                frames = torch.empty(2, 144, 313, dtype=torch.uint8)
                net = M.LiteISPNet_GFM_LSC().eval()
                coord = torch.empty(2, 2, 72, 104)
                fields = []
                for _ in range(3):
                    with torch.no_grad():
                        y = net.forward_mosaic(frames, None, coord, raw_format=fmt)
                    assert y.shape == (2, 3, 144, 208) and st.frame.shape == (2, 144, 208)
                    fields.append(st.field)
                assert fields[0] is None                                                           # the first call is a reset
                assert all(f.shape == (2, 72 // 16, 104 // 16, 4) and f.dtype == torch.int32 for f in fields[1:])
                st.reset()
                with torch.no_grad():
                    net.forward_mosaic(frames, None, coord, raw_format=fmt)
                assert st.field is None and st.frame is not None
                with pytest.raises(ValueError, match="TemporalMotion"):                            # 2 x 20 cells: no block of 16 at level 1
                    net.forward_mosaic(torch.empty(2, 4, 40, dtype=torch.uint16), None, torch.empty(2, 2, 2, 20),
                                       raw_format=dataclasses.replace(fmt, storage="u16", width=None))
    finally:
        torch.set_default_dtype(old)


# ---- 3. the proxy's square root -----------------------------------------------------------------------------------------------------------------
def test_isqrt_is_exact_for_every_q():
    q = np.arange(65026)
    r = R.isqrt(q)
    assert r.min() == 0 and r.max() == 255 and ((r * r <= q) & ((r + 1) * (r + 1) > q)).all()
    assert [int(v) for v in r] == [math.isqrt(int(v)) for v in q]
    # the correction rule repairs a square root that is off by one either way
    for off in (-1, 1):
        r0 = np.clip(r + off, 0, None)
        fixed = np.where(r0 * r0 > q, r0 - 1, np.where((r0 + 1) * (r0 + 1) <= q, r0 + 1, r0))
        assert (fixed == r).all()


def test_the_proxy_on_hand_values():
    blacks, white = (64.0, 60.0, 68.0, 64.0), 1023.0                               # mean black 64: inv = 1 / 959
    cell = lambda v: np.array([[[blacks[0] + v, blacks[1] + v], [blacks[2] + v, blacks[3] + v]]], dtype=np.float32)
    assert R.proxy(cell(0.0), blacks, white).tolist() == [[[0]]]
    assert R.proxy(cell(959.0), blacks, white).tolist() == [[[255]]]
    assert R.proxy(cell(2000.0), blacks, white).tolist() == [[[255]]]              # above white: clamped
    assert R.proxy(cell(-30.0), blacks, white).tolist() == [[[0]]]                 # below black
    assert R.proxy(cell(NAN), blacks, white).tolist() == [[[0]]]
    assert R.proxy(cell(959.0 / 4), blacks, white).tolist() == [[[127]]]           # q = rint(16256.25) = 16256, floor(sqrt) = 127
    assert R.proxy(cell(959.0 / 4), blacks, white, gain=4.0).tolist() == [[[255]]]
    assert R.proxy(np.concatenate([cell(959.0 / 4)] * 2), blacks, white, gain=np.array([[1.0], [4.0]])).tolist() == [[[127]], [[255]]]
    lv = R.pyramid(np.tile(cell(959.0), (1, 5, 7)), blacks, white, 3)
    assert [p.shape for p in lv] == [(1, 5, 7), (1, 2, 3), (1, 1, 1)] and all((p == 255).all() for p in lv)


def test_step_0_is_an_index_gather_in_whole_cells():
    s = torch.arange(2 * 8 * 12, dtype=F32).reshape(2, 8, 12)                      # 4 x 6 cells
    zero = np.zeros((2, 1, 1, 4), np.int32)
    assert torch.equal(R.displaced(s, zero, 8), s)
    vec = zero.copy()
    vec[0, 0, 0, :2] = (1, -1)                                                     # frame 0: the cell right of and above
    vec[1, 0, 0, :2] = (2 ** 31 - 1, -2 ** 31)                                     # frame 1: clamped to the last column and the first row of cells
    d = R.displaced(s, vec, 8)
    assert d[0, 2, 2] == s[0, 0, 4] and d[0, 3, 3] == s[0, 1, 5] and d[0, 0, 0] == s[0, 0, 2] and d[0, 7, 11] == s[0, 5, 11] and d[0, 6, 10] == s[0, 4, 10]
    assert torch.equal(d[1], s[1][[0, 1] * 4][:, [10, 11] * 6])
    rows, cols = R.gather_index(8, 12, vec, 8)
    assert ((rows & 1) == (np.arange(8) & 1)[None, :, None]).all() and ((cols & 1) == (np.arange(12) & 1)[None, None, :]).all()      # its own CFA position


# ---- 4. what the feature is for: the reference chain on a moving scene ------------------------------------------------------------------------
SCENE_CELLS = (96, 160)                                                            # a 192 x 320 mosaic


@pytest.fixture(scope="module")
def moving_scene():
    h, w = SCENE_CELLS
    sc = motion_ref.scene(h, w)
    blacks = (R.BLACK,) * 4
    state_clean = R.clean_mosaic(sc, h, w)
    ref = R.pyramid(state_clean.astype(np.float32), blacks, R.WHITE, R.LEVELS)
    return sc, blacks, state_clean, ref


@pytest.mark.parametrize("sigma", (4.0, 12.0))
@pytest.mark.parametrize("shift", R.SHIFTS)
def test_on_a_moving_scene_the_vectors_are_true_and_only_the_compensated_filter_denoises(moving_scene, sigma, shift):
    h, w = SCENE_CELLS
    sc, blacks, state_clean, ref = moving_scene
    clean = R.clean_mosaic(sc, h, w, shift)
    codes = R.noisy_codes(clean, sigma, 7)
    field = motion_ref.estimate(R.pyramid(codes, blacks, R.WHITE, R.LEVELS), ref, R.BLOCK, R.SEARCH, R.REFINE)[0]
    assert field.shape == (1, 6, 10, 4)
    assert (field[..., 0] == shift[0]).all() and (field[..., 1] == shift[1]).all(), field[..., :2].reshape(-1, 2).tolist()      # 60 of 60
    assert field[..., 3].min() > 1000
    c, state, plane = torch.from_numpy(codes).to(F32), torch.from_numpy(state_clean).to(F32), blacks_of(blacks, 2 * h, 2 * w)
    params = (sigma, 0.0) + R.NOISE_ALPHA_RAMP
    inner = (slice(None), slice(32, -32), slice(32, -32))                          # away from the clamped border: 16 cells

    def rms(x):
        return float(np.sqrt(np.mean((np.asarray(x, dtype=np.float64) - clean)[inner] ** 2)))

    noise = rms(codes)
    with_mc = rms(R.restated_temporal_mc(c, state, plane, params, field, R.BLOCK).numpy()) / noise
    without = rms(restated_temporal(c, state, plane, params).numpy()) / noise
    print(f"sigma {sigma} shift {shift}: residual noise {with_mc:.3f} x compensated, {without:.3f} x uncompensated")
    assert abs(noise / sigma - 1.0) < 0.05
    assert with_mc <= 0.25                                                         # alpha 0.125 and the ramp's share
    if shift != (0, 0):
        assert without >= 0.9


# ---- 5. the C ABI -------------------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # non-null, aligned addresses that are never dereferenced: every case below fails before anything is enqueued
PREV, DST, VEC = FAKE + (1 << 16), FAKE + (1 << 17), FAKE + (1 << 18)


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null levels", dict(levels_ptr=False), b"null"),
    ("null level pointer", dict(null_level=1), b"null level"),
    ("empty", dict(h=0), b"bad shape"), ("no columns", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("black nan", dict(black=(64.0, NAN, 64.0, 64.0)), b"black"), ("black inf", dict(black=(64.0, 64.0, 64.0, INF)), b"black"),
    ("white nan", dict(white=NAN), b"white"), ("white inf", dict(white=INF), b"white"), ("white at the mean black", dict(black=(60.0, 64.0, 64.0, 68.0), white=64.0), b"white"),
    ("white below black", dict(white=10.0), b"white"),
    ("rows too far apart", dict(h=1 << 19, line_bytes=4096), b"2 GiB"),
    ("gain batch 2 of 3", dict(b=3, gain_ptr=FAKE, gain_batch=2), b"gain_batch"), ("gain batch 0", dict(gain_ptr=FAKE, gain_batch=0), b"gain_batch"),
    ("gain batch without tensor", dict(gain_batch=1), b"gain_batch"), ("gain misaligned", dict(gain_ptr=FAKE + 2, gain_batch=1), b"4-byte"),
    ("gain both ways", dict(gain=2.0, gain_ptr=FAKE, gain_batch=1), b"both ways"),
    ("gain zero", dict(gain=0.0), b"gain must be finite"), ("gain negative", dict(gain=-1.0), b"gain must be finite"),
    ("gain nan", dict(gain=NAN), b"gain must be finite"), ("gain inf", dict(gain=INF), b"gain must be finite"),
    ("no levels", dict(levels=0), b"levels"), ("five levels", dict(levels=5), b"levels"), ("levels < 0", dict(levels=-1), b"levels"),
    ("coarsest level empty in h", dict(levels=4), b"coarsest"), ("coarsest level empty in w", dict(levels=3, h=8, w=3), b"coarsest"),
])
def test_raw_motion_pyramid_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, levels_ptr=True, null_level=None, gain=1.0, gain_ptr=None, gain_batch=0, levels=2, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0,
              line_bytes=0, width=0, black=(64.0,) * 4, white=1023.0, fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=kw["white"],
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    ptrs = (C.c_void_p * 4)(*(None if k == kw["null_level"] else DST + 4096 * k for k in range(4)))
    lib = _lib.load()
    assert lib.rc_raw_motion_pyramid(kw["src"], C.byref(f) if kw["fmt"] else None, kw["gain"], kw["gain_ptr"], kw["gain_batch"], kw["levels"],
                                     ptrs if kw["levels_ptr"] else None, kw["b"], kw["h"], kw["w"], None) == -1, case               # RC_ERR_INVALID
    assert b"rc_raw_motion_pyramid" in lib.rc_last_error() and msg in lib.rc_last_error(), (case, lib.rc_last_error())


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("empty", dict(h=0), b"bad shape"), ("no columns", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("black nan", dict(black=(64.0, NAN, 64.0, 64.0)), b"black"), ("black inf", dict(black=(64.0, 64.0, 64.0, INF)), b"black"),
    ("reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"), ("flags", dict(flags=4), b"flags"), ("flags < 0", dict(flags=-1), b"flags"),
    ("no state", dict(prev=None), b"no state"), ("no state, host gain", dict(prev=None, flags=_lib.RC_TNR_GAIN, gain=2.0), b"no state"),
    ("dst is prev", dict(dst=PREV), b"overlaps"), ("dst inside prev", dict(dst=PREV + 256), b"overlaps"), ("dst ends in prev", dict(dst=PREV - 256), b"overlaps"),
    ("dst's last row in prev", dict(dst=PREV - 448 - 60), b"overlaps"), ("prev's last row in dst", dict(dst=PREV + 448 + 60), b"overlaps"),
    ("padded dst over prev", dict(dst=PREV - 900, dst_pitch=128), b"overlaps"), ("padded prev over dst", dict(dst=PREV + 1024, prev_pitch=160), b"overlaps"),
    ("batch of prev over dst", dict(b=3, dst=PREV + 1024), b"overlaps"),
    ("dst pitch short", dict(dst_pitch=60), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=66), b"dst pitch"), ("dst misaligned", dict(dst=DST + 2), b"dst misaligned"),
    ("prev pitch short", dict(prev_pitch=60), b"prev pitch"), ("prev pitch odd", dict(prev_pitch=70), b"prev pitch"), ("prev misaligned", dict(prev=PREV + 2), b"prev misaligned"),
    ("rows too far apart", dict(h=1 << 19, line_bytes=4096, dst=1 << 40), b"2 GiB"), ("dst frame too large", dict(h=1 << 19, dst_pitch=4096, dst=1 << 40), b"2 GiB"),
    ("prev frame too large", dict(h=1 << 19, prev_pitch=4096, dst=1 << 40), b"2 GiB"),
    ("gain batch 2 of 3", dict(b=3, dst=DST, gain_ptr=FAKE, gain_batch=2), b"gain_batch"), ("gain batch 0", dict(gain_ptr=FAKE, gain_batch=0), b"gain_batch"),
    ("gain batch without tensor", dict(gain_batch=1), b"gain_batch"), ("gain misaligned", dict(gain_ptr=FAKE + 2, gain_batch=1), b"4-byte"),
    ("gain both ways", dict(flags=_lib.RC_TNR_GAIN, gain=2.0, gain_ptr=FAKE, gain_batch=1), b"both ways"),
    ("gain zero", dict(flags=_lib.RC_TNR_GAIN, gain=0.0), b"gain must be finite"), ("gain negative", dict(flags=_lib.RC_TNR_GAIN, gain=-1.0), b"gain must be finite"),
    ("gain nan", dict(flags=_lib.RC_TNR_GAIN, gain=NAN), b"gain must be finite"), ("gain inf", dict(flags=_lib.RC_TNR_GAIN, gain=INF), b"gain must be finite"),
    ("noise_abs zero", dict(noise=(0.0, 0.0)), b"noise_abs"), ("noise_abs negative", dict(noise=(-1.0, 0.0)), b"noise_abs"), ("noise_abs nan", dict(noise=(NAN, 0.0)), b"noise_abs"),
    ("noise_abs inf", dict(noise=(INF, 0.0)), b"noise_abs"), ("noise_rel negative", dict(noise=(1.0, -0.5)), b"noise_rel"), ("noise_rel nan", dict(noise=(1.0, NAN)), b"noise_rel"),
    ("noise_rel inf", dict(noise=(1.0, INF)), b"noise_rel"),
    ("parameters are checked on a reset too", dict(flags=_lib.RC_TNR_RESET, prev=None, vec=None, noise=(0.0, 0.0)), b"noise_abs"),
    ("alpha zero", dict(alpha=0.0), b"alpha"), ("alpha negative", dict(alpha=-0.5), b"alpha"), ("alpha above one", dict(alpha=1.5), b"alpha"), ("alpha nan", dict(alpha=NAN), b"alpha"),
    ("ramp one", dict(ramp=1.0), b"ramp"), ("ramp below one", dict(ramp=0.5), b"ramp"), ("ramp nan", dict(ramp=NAN), b"ramp"), ("ramp inf", dict(ramp=INF), b"ramp"),
    # the field
    ("no vectors", dict(vec=None), b"no vectors"), ("vectors 8-byte aligned", dict(vec=VEC + 8), b"16-byte"), ("vectors 4-byte aligned", dict(vec=VEC + 4), b"16-byte"),
    ("block 4", dict(block=4), b"block"), ("block 12", dict(block=12), b"block"), ("block 64", dict(block=64), b"block"), ("block 0", dict(block=0), b"block"),
    ("block < 0", dict(block=-16), b"block"), ("the block is checked on a reset too", dict(flags=_lib.RC_TNR_RESET, prev=None, vec=None, block=5), b"block"),
    ("by 0", dict(by=0), b"by, bx"), ("bx 0", dict(bx=0), b"by, bx"), ("by < 0", dict(by=-1), b"by, bx"),
])
def test_raw_temporal_mc_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, prev=PREV, prev_pitch=0, gain_ptr=None, gain_batch=0, dst=DST, dst_pitch=0, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0,
              line_bytes=0, width=0, black=(64.0,) * 4, flags=0, noise=(4.0, 0.03125), alpha=0.125, ramp=3.0, gain=0.0, reserved=(0, 0, 0, 0), fmt_reserved=(0, 0, 0, 0),
              vec=VEC, by=1, bx=1, block=16)
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=0.0,
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.TemporalDesc(flags=kw["flags"], noise_abs=kw["noise"][0], noise_rel=kw["noise"][1], alpha=kw["alpha"], ramp=kw["ramp"], gain=kw["gain"],
                          reserved=(C.c_int32 * 4)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_temporal_mc(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["prev"], kw["prev_pitch"], kw["gain_ptr"],
                                  kw["gain_batch"], kw["dst"], kw["dst_pitch"], kw["b"], kw["h"], kw["w"], kw["vec"], kw["by"], kw["bx"], kw["block"], None) == -1, case
    assert b"rc_raw_temporal_mc" in lib.rc_last_error() and msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_the_entries_are_declared_bound_and_exported_and_the_lane_map_is_temporal_hips():
    lib = _lib.load()
    for name in ("rc_raw_motion_pyramid", "rc_raw_temporal_mc"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    for op in ("raw_motion_pyramid", "raw_temporal_mc"):
        assert op in M.torch_ops.SCHEMAS and hasattr(torch.ops.realcam, op)
    src = (_lib.PKG / "csrc" / "temporal_mc.hip").read_text()                      # the lane map is temporal.hip's: the GPU tests share its seams
    shared = (_lib.PKG / "csrc" / "temporal_kernel.hpp").read_text()               # ... as the one set of constants both kernels are built from
    assert ("kTnrPx = 4" in shared and "kTnrSpan = 64 * kTnrPx" in shared and "kTnrOut = kTnrSpan - 2 * kTnrPx" in shared and "kTnrRows = 32" in shared
            and "kTnrStrips = kTnrWaves / 2" in shared and "kTnrWaves = 4" in shared)
    for name in ("temporal.hip", "temporal_mc.hip"):                               # neither file defines a lane-map constant of its own
        assert not re.search(r"\bk(Tnr|Tmc)\w* *=[^=]", (_lib.PKG / "csrc" / name).read_text()), name
    tail = (_lib.PKG / "csrc" / "pyramid_tail.hpp").read_text()
    assert not re.search(r"\bk(Pyr|Rp)\w* *=[^=]", src + (_lib.PKG / "csrc" / "motion.hip").read_text()) and "kPyrTile = 4" in tail      # and one pyramid map
    for text in (src, shared, tail):
        assert "__shared__" not in text and "atomic" not in text.replace("no atomics", "")


def test_the_kernels_exist_for_every_storage_and_use_no_scratch():
    from realcamnet_amd import build
    assert "temporal_mc.hip" in build.SOURCES
    res = build.kernel_resources()
    for name in ("raw_pyramid_kernel", "temporal_mc_kernel"):
        mine = {k: v for k, v in res.items() if name in k}
        assert len(mine) == 7, sorted(mine)                # fp32, bf16, fp16, u16, u8, RAW10, RAW12 sources
        assert all(v["tu"] == "temporal_mc.hip" for v in mine.values())
        assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
        assert all(v["lds"] == 0 for v in mine.values())
