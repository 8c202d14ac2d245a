"""GPU: the output stages behind the network on both of their access paths and on every step of their tile walks.  Every expected value
is a CPU restatement that the host tests export (never a kernel's output); every comparison is on bit patterns: there is no tolerance.

A  the source path matrix through the Python ops: the frame is a contiguous view `o` elements into a larger allocation, so a row of a
   multiple of 4 elements meets a base that is not on a vector boundary ("source by elements, destination by vectors"), at rows of
   264 .. 267 elements and crops whose last strip holds 1, 2 or 3 pixels.  Every cell is compared with the restatement and with the
   o = 0 cell of the same geometry: a difference between the two is a path, not arithmetic.
B  a destination of the caller's through the C entries: a window, element-aligned but not vector-aligned, into a buffer of sentinels
   with a guard band on both sides, against a source on and off a vector boundary.
C  tile walks of more than one step: lut3d_lds_kernel at more tiles than compute units, frame_stats_kernel at more tiles than blocks on
   frames that tell tiles apart.

Coverage (entry point, the (source, destination) path pairs it has -- v: vector, e: element, -: the side has one path only -- and the test
that runs each of them; test_output_paths_host.py checks this table against the header and the sources):

    rc_lut3d          vv,ve,ev,ee     test_lut3d_source_paths
    rc_lut3d          vv,ve,ev,ee     test_planar_destination_of_the_callers
    rc_lut3d          walk            test_lut3d_lds_walk_takes_more_than_one_step
    rc_warp           -v,-e           test_warp_source_paths
    rc_warp           -v,-e           test_planar_destination_of_the_callers
    rc_resize         --              test_resize_source_paths
    rc_resize         --              test_planar_destination_of_the_callers
    rc_sharpen        vv,ve,ev,ee     test_planar_destination_of_the_callers
    rc_sharpen        e-              test_sharpen_gpu.py::test_misaligned_base_takes_the_element_path
    rc_tone_hist      v-,e-           test_tone_gpu.py::test_misaligned_base_takes_the_element_path
    rc_tone_apply     vv,ve,ev,ee     test_planar_destination_of_the_callers
    rc_tone_apply     e-              test_tone_gpu.py::test_misaligned_base_takes_the_element_path
    rc_frame_stats    v-,e-           test_frame_stats_source_paths
    rc_frame_stats    walk            test_frame_stats_walk_on_frames_that_tell_tiles_apart
    rc_yuv_encode     vv,ve,ev,ee     test_yuv_encode_source_paths
    rc_yuv_encode     guard,refusal   test_encoder_destinations_guarded_and_refused_off_16_bytes
    rc_rgb_encode     v-,e-           test_rgb_encode_source_paths
    rc_rgb_encode     guard,refusal   test_encoder_destinations_guarded_and_refused_off_16_bytes
"""
import ctypes as C
import math

import pytest
import torch

import realcamnet_amd as M
import yuv_surface_ref as R
from realcamnet_amd import _lib, ops
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32
from realcamnet_amd.out_format import LAYOUTS, MATRICES, RANGES, SITINGS
from realcamnet_amd.warp import BORDERS, INTERPS
from sharpen_ref import restated_sharpen, sharpen_source
from test_lut3d_host import lut_random, lut_source, restated_lut3d
from test_resize_host import CASES as RESIZE_CASES
from test_resize_host import restated_resize
from test_stats_host import restated_stats, stats_source
from test_warp_host import FILL, restated_warp, warp_mesh, warp_source
from test_yuv_host import restated_frames
from tone_ref import restated_apply, restated_gains, restated_hist, tone_source

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
RC = {F32: RC_F32, BF16: RC_BF16, F16: RC_F16}
DT = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
ROWS, BATCH = 7, 2               # source rows: one more than the tallest crop, so a NaN row lies under every crop; two frames for the frame stride
# (source row W, crop w): more than one 64-lane x 4-pixel tile and less than two; rows that are and are not a multiple of 4; a vector-eligible
# row whose last strip holds 1, 2 or 3 pixels
GEOMS = ((264, 264), (265, 265), (266, 266), (267, 267), (264, 261), (264, 262), (264, 263))
EVEN_GEOMS = tuple(dict.fromkeys((W, w & ~1) for W, w in GEOMS))             # the same rows for the layouts that need an even width
SENTINEL, GUARD = 7.0, 64        # no result is 7: looks lie in [-0.5, 1.5], fills and frames in [-0.5, 1.5], the other stages clamp to [0, 1]


def out_types(dt):
    return (F32,) if dt == F32 else (F32, dt)


def offsets(dt):
    """Element offsets of the base: every residue of a 4-element vector; for a 2-byte type also 4, which is on 8 bytes and off 16."""
    return (0, 1, 2, 3) if dt == F32 else (0, 1, 2, 3, 4)


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    """The tensor on the CPU as integers of its element's width: a -0.0 for a 0.0 shows, a NaN compares."""
    t = t.detach().cpu().contiguous()
    if t.dtype == F32:
        return t.view(torch.int32)
    if t.dtype in (BF16, F16, torch.uint16):
        return t.view(torch.int16)
    return t


def check(got, want, *where):
    """Equal bit patterns, or the count of mismatches and the first mismatching coordinate."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (*where, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    bad = (bits(got) != bits(want)).nonzero()
    assert len(bad) == 0, (*where, f"{len(bad)} mismatches, the first at {tuple(bad[0].tolist())}")


def placed(y, o):
    """The frames as a contiguous view `o` elements into a larger allocation on the device."""
    buf = torch.empty(y.numel() + 4, dtype=y.dtype, device=DEV)
    view = buf[o:o + y.numel()].view(y.shape)
    view.copy_(y)
    assert view.is_contiguous()
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (o * y.element_size()) % 16
    return view


def vector_side(ptr, es, row):
    """rgb_strip.hpp's rule for a side: the base on a 4-element boundary and rows of a multiple of 4."""
    return ptr % (4 * es) == 0 and row % 4 == 0


def listed(x):
    return list(x) if isinstance(x, (tuple, list)) else [x]


def path_matrix(entry, dt, groups, geoms=GEOMS):
    """groups(W, w) -> [(frames on the host, [(label, call(view) -> tensor(s), wanted tensor(s))])].  Every call runs at every offset of
    the base; each result is compared with the restatement and with the o = 0 result of the same cell."""
    for W, w in geoms:
        for y, cells in groups(W, w):
            first = {}
            for o in offsets(dt):
                view = placed(y, o)
                for label, call, want in cells:
                    where = (entry, str(dt), label, f"o = {o}", f"W = {W}", f"w = {w}")
                    got = listed(call(view))
                    for g, x in zip(got, listed(want)):
                        assert not (x.is_floating_point() and torch.isnan(x).any()), where
                        check(g, x, *where, "against the restatement")
                    for g, g0 in zip(got, first.setdefault(label, [g.cpu() for g in got])):
                        check(g, g0, *where, "against the o = 0 cell: the path, not the arithmetic")


def unit_source(shape, crop, dt):
    """(B,3,H,W) in [0, 1] with 0, -0.0 and 1 planted; NaN outside the crop.  For the scaler, whose sums keep a NaN."""
    h, w = crop
    v = torch.rand(shape[0], 3, h, w, generator=torch.Generator().manual_seed(6000 + shape[3]))
    v.view(-1)[::13] = 0.0
    v.view(-1)[5::17] = 1.0
    v.view(-1)[7::19] = -0.0
    y = torch.full(tuple(shape), float("nan"))
    y[:, :, :h, :w] = v
    return y.to(dt)


# ---- A. the source path matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
def test_lut3d_source_paths(hip, dt):
    """n = 17 is the LDS kernel, n = 18 the gather kernel; an fp32 vector goes through lut_load's own branch."""
    def groups(W, w):
        out = []
        for n in (17, 18):
            crop, lut = (5, w), lut_random(n)
            y = lut_source((BATCH, 3, ROWS, W), crop, n, dt)
            want = restated_lut3d(y, lut, crop)
            out.append((y, [(f"n = {n} -> {od}", lambda v, lut=lut, crop=crop, od=od: ops.lut3d(v, lut, crop_hw=crop, out_dtype=od), want.to(od)) for od in out_types(dt)]))
        return out
    path_matrix("rc_lut3d", dt, groups)


WARP_FORMS = (("bilinear", "clamp"), ("bicubic", "constant"))


def warp_size(w):
    """Taller than the frame and 8 columns narrower: destination strips and source rows are unrelated, and ow % 4 = w % 4."""
    return (7, w - 8)


@pytest.mark.parametrize("dt", DT)
def test_warp_source_paths(hip, dt):
    def groups(W, w):
        frame, size = (5, w), warp_size(w)
        y = warp_source((BATCH, 3, ROWS, W), frame, dt)
        mesh = warp_mesh(frame, size, 8)
        md = mesh.to(DEV)
        cells = []
        for interp, border in WARP_FORMS:
            want = restated_warp(y, mesh, size, 8, interp, border, FILL, crop=frame)
            for od in out_types(dt):
                cells.append((f"{interp} {border} -> {od}", lambda v, i=interp, b=border, od=od: ops.warp(v, md, size=size, cell=8, interp=i, border=b, fill=FILL, crop_hw=frame,
                                                                                                          out_dtype=od), want.to(od)))
        return [(y, cells)]
    path_matrix("rc_warp", dt, groups)


(_, _, _RS_H, _RS_W), _, _RS_KW = RESIZE_CASES[5]                            # 80 x 160 -> 48 x 130: 1.67 : 1 down, 1.23 : 1 across
assert _RS_H % _RS_KW["size"][0] and _RS_W % _RS_KW["size"][1]               # no integer ratio


def resize_of(h, w, filt):
    return M.Resize((h * _RS_KW["size"][0] // _RS_H, w * _RS_KW["size"][1] // _RS_W), filter=filt)


@pytest.mark.parametrize("dt", DT)
def test_resize_source_paths(hip, dt):
    """rc_resize reads and writes by elements whatever the base: the matrix fixes that a base off a vector boundary stays invisible."""
    def groups(W, w):
        crop = (5, w)
        y = unit_source((BATCH, 3, ROWS, W), crop, dt)
        cells = []
        for filt in ("area", "bilinear"):
            rs = resize_of(*crop, filt)
            want = restated_resize(y, rs, crop)
            cells += [(f"{filt} -> {od}", lambda v, rs=rs, od=od: ops.resize(v, rs, crop_hw=crop, out_dtype=od), want.to(od)) for od in out_types(dt)]
        return [(y, cells)]
    path_matrix("rc_resize", dt, groups)


@pytest.mark.parametrize("dt", DT)
def test_frame_stats_source_paths(hip, dt):
    """No ROI, a ROI at x0 = 4 (vector loads on an aligned base, a partial last strip) and one at x0 = 3 (element loads)."""
    def groups(W, w):
        h = 6
        out = []
        for roi in (None, (1, 4, h - 1, 257), (1, 3, h - 1, 257)):
            y = stats_source((BATCH, 3, ROWS, W), (h, w), roi, dt)
            cells = []
            for nbits in (8, 10):
                for grid in ((1, 1), (5, 7)):
                    spec = M.Stats(grid=grid, bits=nbits, roi=roi, dark=4 << (nbits - 8), clip=250 << (nbits - 8))
                    want = restated_stats(y, spec, (h, w))

                    def call(v, spec=spec):
                        got = ops.frame_stats(v, spec, crop_hw=(h, w))
                        return got.hist, got.zones
                    cells.append((f"bits {nbits} grid {grid} roi {roi}", call, want))
            out.append((y, cells))
        return out
    path_matrix("rc_frame_stats", dt, groups)


def yuv_bytes(y, fmt, crop):
    """The bytes (B, frame_bytes) uint8 of whole frames, padding included: test_yuv_host's restatement for the layouts of yuv_encode.hip,
    yuv_surface_ref's for the others."""
    h, w = crop
    if fmt.layout in ("nv12", "p010", "i420"):
        return restated_frames(y, fmt, crop).contiguous().view(torch.uint8)
    return torch.from_numpy(R.pack(fmt.layout, *R.format_codes(y[:, :, :h, :w].float().numpy(), fmt), fmt.plane_layout(h, w)))


def yuv_format(layout, siting="left"):
    return M.OutFormat(layout, chroma_siting=siting, pitch_align=64, height_align=4)        # padded rows and columns: the padding is compared too


# per translation unit and per strip width: 16 and 8 pixels (yuv_encode.hip), 16 pixels planar, packed and 4:4:4, 24 pixels of v210 (yuv_surface.hip)
YUV_EVEN = (("nv12", "left"), ("nv12", "center"), ("p010", "left"), ("i420", "left"), ("i422", "left"), ("yuy2", "left"), ("v210", "left"))
YUV_ANY = (("i444", "left"),)


@pytest.mark.parametrize("dt", DT)
def test_yuv_encode_source_paths(hip, dt):
    """rc_yuv_encode's own rule in both translation units: base % 16 and row bytes % 16, so o = 4 of a 2-byte type is off it too."""
    def groups_of(formats):
        def groups(W, w):
            crop = (6, w)
            y = stats_source((BATCH, 3, ROWS, W), crop, None, dt)
            cells = []
            for layout, siting in formats:
                fmt = yuv_format(layout, siting)
                cells.append((f"{layout} {siting}", lambda v, fmt=fmt: ops.yuv_encode(v, fmt, crop_hw=crop).buffer.contiguous().view(torch.uint8), yuv_bytes(y, fmt, crop)))
            return [(y, cells)]
        return groups
    path_matrix("rc_yuv_encode", dt, groups_of(YUV_EVEN), EVEN_GEOMS)
    path_matrix("rc_yuv_encode", dt, groups_of(YUV_ANY), GEOMS)


def restated_rgb(y, nbits, crop):
    """ops.rgb_encode's docstring in torch: clamp(rint(float(y) * S), 0, S) with S = 2**bits - 1, half to even, NaN -> 0, interleaved."""
    h, w = crop
    S = float(2 ** nbits - 1)
    q = torch.round(y[:, :, :h, :w].float() * S)                              # one fp32 product, then half to even
    q = torch.where(q > 0, torch.where(q < S, q, torch.full_like(q, S)), torch.zeros_like(q))      # NaN compares false: 0
    q = q.permute(0, 2, 3, 1).contiguous().to(torch.int32)
    return q.to(torch.uint8) if nbits == 8 else q.to(torch.uint16)


@pytest.mark.parametrize("dt", DT)
def test_rgb_encode_source_paths(hip, dt):
    """rgb_encode_kernel decides per item: with a base off 16 bytes, the items whose own address falls on 16 bytes still load vectors."""
    def groups(W, w):
        crop = (5, w)
        y = stats_source((BATCH, 3, ROWS, W), crop, None, dt)
        return [(y, [(f"bits {nbits}", lambda v, nbits=nbits: ops.rgb_encode(v, nbits, crop_hw=crop), restated_rgb(y, nbits, crop)) for nbits in (8, 16)])]
    path_matrix("rc_rgb_encode", dt, groups)


# ---- B. a destination of the caller's ---------------------------------------------------------------------------------------------------------
def guarded(numel, dtype, o):
    """(buffer of sentinels, window of `numel` elements `o` elements past a vector boundary, with GUARD sentinels or more on both sides)."""
    buf = torch.full((GUARD + 4 + numel + GUARD,), 7, dtype=dtype, device=DEV)
    win = buf[GUARD + o:GUARD + o + numel]
    assert buf.data_ptr() % 16 == 0 and win.data_ptr() % 16 == (o * buf.element_size()) % 16
    return buf, win


def guards_intact(buf, win, *where):
    lo = (win.data_ptr() - buf.data_ptr()) // buf.element_size()
    guard = torch.cat([buf[:lo], buf[lo + win.numel():]]).cpu()
    assert len(guard) >= 2 * GUARD
    bad = (bits(guard) != bits(torch.full_like(guard, 7))).nonzero()
    assert len(bad) == 0, (*where, f"{len(bad)} guard elements written, the first at {int(bad[0])} of {len(guard)} (the window starts at {lo})")


def planar_entries(hip, dt, W, w):
    """Per entry that writes planar RGB: (label, frames on the host, output shape, destination row, call(src, sdt, dst, ddt) -> code, wanted fp32)."""
    shape, crop = (BATCH, 3, ROWS, W), (5, w)
    h = crop[0]
    out = []
    for n in (17, 18):
        lut = lut_random(n)
        y = lut_source(shape, crop, n, dt)
        table = ops.lut3d_table(lut, torch.device(DEV, torch.cuda.current_device()))
        out.append((f"rc_lut3d n = {n}", y, (BATCH, 3, h, w), w,
                    lambda s, sd, d, dd, table=table, n=n: hip.rc_lut3d(s, sd, d, dd, table.data_ptr(), n, BATCH, ROWS, W, h, w, stream()), restated_lut3d(y, lut, crop)))
    y = warp_source(shape, crop, dt)
    oh, ow = size = warp_size(w)
    mesh = warp_mesh(crop, size, 8)
    md = mesh.to(DEV)
    for interp, border in WARP_FORMS:
        out.append((f"rc_warp {interp} {border}", y, (BATCH, 3, oh, ow), ow,
                    lambda s, sd, d, dd, i=INTERPS[interp], b=BORDERS[border]: hip.rc_warp(s, sd, d, dd, md.data_ptr(), 1, 3, i, b, *FILL, BATCH, ROWS, W, h, w, oh, ow, stream()),
                    restated_warp(y, mesh, size, 8, interp, border, FILL, crop=crop)))
    y = unit_source(shape, crop, dt)
    for filt in ("area", "bilinear"):
        rs = resize_of(*crop, filt)
        rh, rw = rs.size
        fy, wy, fx, wx = ops.resize_tables(rs, h, w, torch.device(DEV, torch.cuda.current_device()))
        out.append((f"rc_resize {filt}", y, (BATCH, 3, rh, rw), rw,
                    lambda s, sd, d, dd, t=(fy, wy, fx, wx), rh=rh, rw=rw: hip.rc_resize(s, sd, d, dd, BATCH, ROWS, W, rh, rw, t[0].data_ptr(), t[1].data_ptr(), t[1].shape[1],
                                                                                         t[2].data_ptr(), t[3].data_ptr(), t[3].shape[1], stream()),
                    restated_resize(y, rs, crop)))
    y = sharpen_source(shape, crop, dt)
    sp = M.Sharpen(1.5, 2, 1 / 64, 1 / 32)
    sdesc = _lib.SharpenDesc(radius=sp.radius, matrix=sp.matrix_code, amount=sp.amount, core=sp.core, overshoot=sp.overshoot)
    out.append(("rc_sharpen", y, (BATCH, 3, h, w), w, lambda s, sd, d, dd: hip.rc_sharpen(s, sd, d, dd, C.byref(sdesc), BATCH, ROWS, W, h, w, stream()), restated_sharpen(y, sp, crop)))
    y = tone_source(shape, crop, dt)
    tm = M.ToneMap(grid=(2, 3), clip=1.5)
    gains = restated_gains(restated_hist(y, tm, crop), tm)
    gd = gains.to(DEV)
    (iy, uy), (ix, ux) = ops.tone_axis_tables(h, tm.grid[0], torch.device(DEV)), ops.tone_axis_tables(w, tm.grid[1], torch.device(DEV))
    tdesc = _lib.ToneDesc(grid=(C.c_int32 * 2)(*tm.grid), matrix=tm.matrix_code, clip_q8=tm.clip_q8, strength=tm.strength, max_gain=tm.max_gain)
    assert gd.data_ptr() % 16 == 0
    out.append(("rc_tone_apply", y, (BATCH, 3, h, w), w,
                lambda s, sd, d, dd: hip.rc_tone_apply(s, sd, d, dd, C.byref(tdesc), gd.data_ptr(), BATCH, iy.data_ptr(), uy.data_ptr(), ix.data_ptr(), ux.data_ptr(),
                                                       BATCH, ROWS, W, h, w, stream()), restated_apply(y, gains, tm, crop)))
    return out


@pytest.mark.parametrize("dt", DT)
def test_planar_destination_of_the_callers(hip, dt):
    """rc_lut3d, rc_warp, rc_resize, rc_sharpen and rc_tone_apply write a window that starts 0 .. 3 elements past a vector boundary, from a
    source on one and one element off it, at a row that is and one that is not a multiple of 4: the window holds the restatement, every
    guard element its sentinel, and every (source, destination) pair of vector and element access occurs for every entry that has both."""
    pairs = {}
    for W in (264, 266):
        for label, y, oshape, drow, call, want in planar_entries(hip, dt, W, W):
            assert not torch.isnan(want).any(), label
            for o_src in (0, 1):
                src = placed(y, o_src)
                for od in out_types(dt):
                    wanted = want.to(od)
                    for o_dst in (0, 1, 2, 3):
                        buf, win = guarded(math.prod(oshape), od, o_dst)
                        where = (label, str(dt), f"-> {od}", f"source o = {o_src}", f"destination o = {o_dst}", f"W = w = {W}")
                        _lib.check(call(src.data_ptr(), RC[dt], win.data_ptr(), RC[od]), label)
                        torch.cuda.synchronize()
                        check(win.view(oshape), wanted, *where)
                        guards_intact(buf, win, *where)
                        pairs.setdefault(label, set()).add((vector_side(src.data_ptr(), src.element_size(), W), vector_side(win.data_ptr(), win.element_size(), drow)))
    # rc_resize has one path per side, and its output row is not the source's: each side meets both alignments, not every pair of them
    assert len(pairs) == 8 and all(len(p) == 4 for label, p in pairs.items() if "rc_resize" not in label), pairs
    assert all({s for s, _ in p} == {d for _, d in p} == {False, True} for p in pairs.values()), pairs


def test_encoder_destinations_guarded_and_refused_off_16_bytes(hip):
    """rc_yuv_encode (a layout of each translation unit) and rc_rgb_encode demand a 16-byte destination.  On one, inside a guard band: the
    frames are the restatement and the band keeps its sentinels.  4 bytes off it: an error return with the documented message, checked on
    the host before any launch (yuv_encode.hip and yuv_surface.hip: "dst must be 16-byte aligned" in front of the first launch;
    raw_format.hip the same), and an untouched buffer."""
    dt, W, crop = BF16, 264, (6, 264)
    y = stats_source((BATCH, 3, ROWS, W), crop, None, dt)
    src = placed(y, 0)
    cases = []
    for layout in ("nv12", "yuy2"):
        fmt = yuv_format(layout)
        pl = fmt.plane_layout(*crop)
        d = _lib.OutFormatDesc(layout=LAYOUTS[layout], matrix=MATRICES[fmt.matrix], range=RANGES[fmt.range], siting=SITINGS[fmt.chroma_siting], pitch=pl.pitch,
                               rows=pl.planes[0].alloc_rows)
        cases.append((f"rc_yuv_encode {layout}", b"rc_yuv_encode: dst must be 16-byte aligned", yuv_bytes(y, fmt, crop),
                      lambda dst, d=d: hip.rc_yuv_encode(src.data_ptr(), RC[dt], C.byref(d), dst, BATCH, ROWS, W, *crop, stream())))
    for nbits in (8, 16):
        cases.append((f"rc_rgb_encode {nbits}", b"rc_rgb_encode: dst must be 16-byte aligned", restated_rgb(y, nbits, crop).contiguous().view(torch.uint8),
                      lambda dst, nbits=nbits: hip.rc_rgb_encode(src.data_ptr(), RC[dt], dst, nbits, BATCH, ROWS, W, *crop, stream())))
    for label, message, want, call in cases:
        buf, win = guarded(want.numel(), torch.uint8, 0)
        _lib.check(call(win.data_ptr()), label)
        torch.cuda.synchronize()
        check(win.view(want.shape), want, label, "aligned, inside a guard band")
        guards_intact(buf, win, label)
        buf, win = guarded(want.numel(), torch.uint8, 4)
        assert win.data_ptr() % 16 == 4
        code = call(win.data_ptr())
        assert code != 0 and message in hip.rc_last_error(), (label, code, hip.rc_last_error())
        torch.cuda.synchronize()
        assert bool((buf == 7).all()), (label, "a refused call wrote")


# ---- C. tile walks that take more than one step -----------------------------------------------------------------------------------------------
LDS_TILE_W, LDS_TILE_H = 1024, 4              # lut3d.hip: kLutLdsStrips * kLutPx columns, kLutRows rows


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def lds_walk(hip, dt, W, w, h, steps):
    """rc_lut3d with n = 17 on (3,3,h+1,W) cropped to (h,w), into sentinels; `steps`: the tiles the busiest block may walk (lo, hi)."""
    cus, b, n = cu_count(), 3, 17
    ctiles, rtiles = -(-w // LDS_TILE_W), -(-h // LDS_TILE_H)
    total = ctiles * rtiles * b
    # the kernel launches min(total, CUs) blocks and block i walks tiles i, i + blocks, ...
    assert total > cus, (total, cus)                                           # a second step is taken
    assert steps[0] <= -(-total // cus) <= steps[1], (total, cus)
    assert total % cus != 0 and h % LDS_TILE_H != 0, (total, cus, h)           # the last step is not taken by every block; the last row tile is partial
    lut = lut_random(n)
    y = lut_source((b, 3, h + 1, W), (h, w), n, dt)
    want = restated_lut3d(y, lut, (h, w))
    assert not torch.isnan(want).any()
    src = placed(y, 0)
    table = ops.lut3d_table(lut, torch.device(DEV, torch.cuda.current_device()))
    for od in out_types(dt):
        buf, win = guarded(want.numel(), od, 0)
        _lib.check(hip.rc_lut3d(src.data_ptr(), RC[dt], win.data_ptr(), RC[od], table.data_ptr(), n, b, h + 1, W, h, w, stream()), "rc_lut3d")
        torch.cuda.synchronize()
        where = ("lut3d_lds_kernel", str(dt), f"-> {od}", f"{total} tiles on {cus} blocks")
        got = win.view(want.shape)
        unwritten = int((bits(got) == bits(torch.full_like(got.cpu(), 7))).sum())
        assert unwritten == 0, (*where, f"{unwritten} samples still hold the sentinel: a tile nobody wrote")
        check(got, want.to(od), *where)
        guards_intact(buf, win, *where)
    return total


@pytest.mark.parametrize("dt", [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")])
def test_lut3d_lds_walk_takes_more_than_one_step(hip, dt):
    """The persistent blocks of the LDS form at more tiles than compute units: the stride t += gridDim.x and the (frame, row tile, column
    tile) decomposition of t >= gridDim.x, which every 4K frame runs and no smaller case reaches."""
    cus = cu_count()
    # one column tile: 3 ceil(h / 4) tiles, between 2 and 3 per block, no multiple of the block count
    lds_walk(hip, dt, 72, 70, 4 * -(-(2 * cus + 37) // 3) + 1, (2, 3))
    # two column tiles: 6 ceil(h / 4) tiles, about 1.5 per block
    h = 4 * -(-cus // 4) - 1
    total = lds_walk(hip, dt, 1032, 1030, h, (2, 2))
    assert total == 2 * -(-h // 4) * 3 and min(total % cus, cus - total % cus) > 8, (total, cus)    # neither a multiple of the block count nor within 8 of one


def test_frame_stats_walk_on_frames_that_tell_tiles_apart(hip):
    """frame_stats_kernel at more tiles than blocks per frame, on random frames: a tile read at the wrong place changes the sums (an
    all-ones frame, the only such case before, gives the same sums wherever a tile is read)."""
    cus = cu_count()
    batch = cus // 2
    cap = max(1, 4 * cus // batch)                                             # frame_stats.hip: blocks per frame are at most 4 CUs / frames ...
    h, w, tile_h, tile_w = 129, 513, 64, 256
    ntiles = -(-h // tile_h) * -(-w // tile_w)
    assert cap == 8 and ntiles == 9 > cap, (cus, batch, cap, ntiles)
    blocks = max(1, min(cap, ntiles // 3))                                     # ... and at most a third of the tiles
    assert blocks < ntiles
    spec = M.Stats(grid=(3, 5), bits=10, dark=16, clip=1000)
    from realcamnet_amd.stats import zone_bounds
    assert all(v % tile_h for v in zone_bounds(h, 3)[1:-1]) and all(v % tile_w for v in zone_bounds(w, 5)[1:-1])      # zone boundaries fall inside tiles
    four = stats_source((4, 3, h, w), None, None, BF16, seed=9)
    assert not any(torch.equal(bits(four[i]), bits(four[j])) for i in range(4) for j in range(i))
    hist4, zones4 = restated_stats(four, spec)
    assert zones4[..., 5].sum() > 0 and zones4[..., 6].sum() > 0 and not any(torch.equal(zones4[i], zones4[j]) for i in range(4) for j in range(i))
    which = torch.arange(batch) % 4
    got = ops.frame_stats(four.to(DEV)[which.to(DEV)].contiguous(), spec)
    check(got.hist, hist4[which], "frame_stats_kernel", "hist", f"{ntiles} tiles on {blocks} blocks, {batch} frames")
    check(got.zones, zones4[which], "frame_stats_kernel", "zones", f"{ntiles} tiles on {blocks} blocks, {batch} frames")
