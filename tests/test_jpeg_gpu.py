"""GPU: the JPEG output of forward_mosaic (rc_jpeg_encode).  The yardstick is tests/jpeg_ref.py, the NumPy restatement of the header's
arithmetic (never the kernel's own output): every file is compared byte for byte and every length with the reference's; Pillow, which the
package itself never uses, opens every stream."""
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as R
import liteisp_oracle as O
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from test_jpeg_host import FIDELITY_SHORTFALL_DB, pillow_psnr, rgb8_of

DEV = "cuda"
_REF = {}


def case(name):
    """(Jpeg with a capacity that holds every frame, the source tensor on the host in its dtype, (h, w), the reference files), computed once."""
    if name not in _REF:
        sub, quality, restart, dtype, src, (h, w) = R.case_source(name)
        y = torch.from_numpy(src).to(getattr(torch, dtype))
        files = [R.encode(f[:, :h, :w], quality, sub, restart) for f in y.float().numpy()]
        cap = max(R.plan(sub, restart, h, w)[3], max(len(f) for f in files))
        _REF[name] = (M.Jpeg(quality, sub, restart, capacity=cap), y, (h, w), files)
    return _REF[name]


def check(frames, files, what=""):
    assert frames.buffer.dtype == torch.uint8 and frames.lengths.dtype == torch.int64 and frames.lengths.shape == (len(files),)
    assert frames.lengths.cpu().tolist() == [len(f) for f in files], what
    got = frames.files()
    for b, (g, f) in enumerate(zip(got, files)):
        assert g == f, (what, b, next(i for i in range(len(f)) if g[i] != f[i]))
        assert frames.tobytes(b) == f


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_jpeg_encode_equals_reference(hip, name):
    """Every case of jpeg_ref.CASES -- one MCU, padding on both axes, intervals that cross MCU rows, a short last interval, noise with NaN at
    quality 10 / 90 / 100, flat frames, full-swing checkerboards, the three source types, a crop, a batch of two different frames: the files
    and the lengths equal the reference's, and Pillow opens each at the crop's size."""
    fmt, y, (h, w), files = case(name)
    frames = ops.jpeg_encode(y.to(DEV), fmt, crop_hw=(h, w))
    assert frames.fmt == fmt and frames.size == (h, w) and frames.buffer.shape == (y.shape[0], fmt.capacity)
    check(frames, files, name)
    for f in frames.files():
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (w, h) and im.mode == "RGB"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("420_crop", "444_crop", "420_rows_wrap"))
def test_base_pointer_off_by_one_element(hip, name):
    """The same frames from a base pointer misaligned by one element: the element load path gives the same bytes."""
    fmt, y, (h, w), files = case(name)
    flat = torch.empty(y.numel() + 1, dtype=y.dtype, device=DEV)
    view = flat[1:].view(y.shape)
    view.copy_(y)
    assert view.data_ptr() % (2 * y.element_size()) != 0
    check(ops.jpeg_encode(view, fmt, crop_hw=(h, w)), files, name)


@pytest.mark.gpu
def test_samples_are_the_i420_full_range_surface(hip):
    """The sample step: for even sizes the reference's codes -- which the byte-equal streams carry -- are the planes rc_yuv_encode writes for
    I420 / BT.601 / full range / centre siting, from the device."""
    surface = M.OutFormat("i420", "bt601", "full", "center")
    for name in ("420_rows_wrap", "420_batch", "420_checker"):
        fmt, y, (h, w), _ = case(name)
        assert h % 2 == 0 and w % 2 == 0
        planes = [p.cpu().numpy().astype(np.int64) for p in ops.yuv_encode(y.to(DEV), surface).planes]
        for b, f in enumerate(y.float().numpy()):
            yc, cb, cr = R.samples(f, "420")
            assert np.array_equal(planes[0][b], yc[:h, :w]) and np.array_equal(planes[1][b], cb[:h // 2, :w // 2]) and np.array_equal(planes[2][b], cr[:h // 2, :w // 2])


@pytest.mark.gpu
def test_capacity_too_small_for_one_frame(hip):
    """Frame 0 of 2 does not fit: lengths[0] is still what it needs, frame 1 is intact, tobytes(0) names the capacity that would do -- and,
    through the C ABI with guard bytes around the frames, nothing outside a frame's capacity bytes is written."""
    big = torch.from_numpy(R.noise((1, 3, 48, 64), 11))
    small = torch.from_numpy(R.flat((1, 3, 48, 64)))
    y = torch.cat([big, small])
    for sub in ("420", "444"):
        files = [R.encode(f, 100, sub, 2) for f in y.numpy()]
        cap = len(files[1]) + 40
        assert len(files[0]) > 4 * cap
        fmt = M.Jpeg(100, sub, 2, capacity=cap)
        frames = ops.jpeg_encode(y.to(DEV), fmt)
        assert frames.lengths.cpu().tolist() == [len(f) for f in files]
        assert frames.tobytes(1) == files[1]
        with pytest.raises(ValueError, match=f"capacity={len(files[0])}"):
            frames.tobytes(0)
        with pytest.raises(ValueError, match=f"capacity={len(files[0])}"):
            frames.files()
        # both frames too large, guard bytes in front of and behind them
        for capacity in (1, 100, 700, 2001):
            yd = torch.cat([big, big.flip(3)]).to(DEV)
            guard = 4096
            dst = torch.full((guard + 2 * capacity + guard,), 0xAB, dtype=torch.uint8, device=DEV)
            lengths = torch.zeros(2, dtype=torch.int64, device=DEV)
            header = ops.jpeg_header(fmt, 48, 64, DEV)
            d, p = fmt.desc(), _lib.JpegPlanInfo()
            _lib.check(hip.rc_jpeg_plan(C.byref(d), 48, 64, C.byref(p)))
            scratch = torch.empty(2 * p.scratch_bytes // 4, dtype=torch.int32, device=DEV)
            _lib.check(hip.rc_jpeg_encode(yd.data_ptr(), _lib.RC_F32, C.byref(d), header.data_ptr(), scratch.data_ptr(), dst.data_ptr() + guard, lengths.data_ptr(),
                                          2, 48, 64, 48, 64, capacity, torch.cuda.current_stream().cuda_stream), "rc_jpeg_encode")
            torch.cuda.synchronize()
            want = [len(R.encode(f, 100, sub, 2)) for f in yd.cpu().numpy()]
            assert lengths.cpu().tolist() == want and min(want) > 2001
            host = dst.cpu()
            assert bool((host[:guard] == 0xAB).all()) and bool((host[guard + 2 * capacity:] == 0xAB).all())


@pytest.mark.gpu
def test_frames_beyond_two_gib(hip):
    """Three small frames with a capacity of 2^30 + 5 bytes each: the last frame starts beyond 2^31 bytes into the buffer."""
    y = torch.from_numpy(np.concatenate([R.noise((1, 3, 16, 24), 31), R.smooth((1, 3, 16, 24)), R.noise((1, 3, 16, 24), 32)]))
    fmt = M.Jpeg(90, "420", 1, capacity=(1 << 30) + 5)
    frames = ops.jpeg_encode(y.to(DEV), fmt)
    assert frames.buffer.shape == (3, (1 << 30) + 5)
    files = [R.encode(f, 90, "420", 1) for f in y.numpy()]
    assert frames.lengths.cpu().tolist() == [len(f) for f in files] and [frames.tobytes(b) for b in range(3)] == files


@pytest.mark.gpu
def test_two_runs_are_equal_and_keep_one_header(hip):
    fmt, y, (h, w), files = case("420_rows_wrap")
    yd = y.to(DEV)
    a = ops.jpeg_encode(yd, fmt)
    header = ops.jpeg_header(fmt, h, w, yd.device)
    b = ops.jpeg_encode(yd, fmt)
    assert torch.equal(a.buffer, b.buffer) and torch.equal(a.lengths, b.lengths)
    assert ops.jpeg_header(fmt, h, w, yd.device) is header                  # a warmed-up call copies nothing to the device
    assert bytes(header.cpu().tolist()) == R.header(fmt.quality, fmt.subsampling, fmt.restart, h, w)


@pytest.mark.gpu
def test_graphed_call_replays_on_a_rewritten_input(hip):
    fmt = M.Jpeg(90, "420", 3)
    y1 = torch.from_numpy(R.noise((2, 3, 40, 56), 21))
    y2 = torch.from_numpy(R.smooth((2, 3, 40, 56)))
    call = M.GraphedCall(lambda x: ops.jpeg_encode(x, fmt, crop_hw=(37, 50)))
    for y in (y1, y2, y1):
        frames = call(y.to(DEV))
        check(frames, [R.encode(f[:, :37, :50], 90, "420", 3) for f in y.numpy()])


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ("420", "444"))
def test_fidelity_of_the_device_stream(hip, sub):
    """The device's stream, decoded by Pillow, against the source: within the host test's figure of Pillow's own file at the same settings."""
    y = torch.from_numpy(R.smooth((1, 3, 96, 128)))
    for quality in (50, 90, 100):
        f = ops.jpeg_encode(y.to(DEV), M.Jpeg(quality, sub, 4, capacity=1 << 17)).tobytes(0)
        rgb8 = rgb8_of(y[0].numpy())
        ours = R.psnr(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), rgb8)
        assert ours >= pillow_psnr(rgb8, quality, sub) - FIDELITY_SHORTFALL_DB[(sub, quality)] - 0.1, (quality, ours)


@pytest.mark.gpu
def test_forward_mosaic_emits_a_jpeg_beside_an_encoder_surface(hip):
    """forward_mosaic(outputs=[nv12, Jpeg of a resized rendition]) on the smallest net and frame of the forward_mosaic tests: the JPEG is
    ops.jpeg_encode of the same float rendition, and the nv12 output is what it is without the JPEG beside it."""
    dt = torch.bfloat16
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(device=DEV, dtype=dt).eval()
    g = torch.Generator().manual_seed(5)
    mosaic = torch.rand(2, 1, 80, 112, generator=g).to(DEV, dt)
    coord = O.make_coord(2, 40, 56).to(DEV, dt)
    nv12, rs, jp = M.OutFormat("nv12"), M.Resize((40, 56)), M.Jpeg(75)
    with torch.no_grad():
        y = net.forward_mosaic(mosaic, None, coord)
        alone = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(nv12)])[0]
        surface, stills = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(nv12), M.Output(jp, rs)])
        whole = net.forward_mosaic(mosaic, None, coord, out_format=jp)
    assert torch.equal(surface.buffer, alone.buffer)
    want = ops.jpeg_encode(ops.resize(y, rs), jp)
    assert isinstance(stills, M.JpegFrames) and stills.size == (40, 56) and stills.files() == want.files()
    assert whole.size == (80, 112) and whole.files() == ops.jpeg_encode(y, jp).files()
    rendition = ops.resize(y, rs).float().cpu().numpy()
    for b, f in enumerate(stills.files()):
        assert f == R.encode(rendition[b], 75, "420", 8)
        im = Image.open(io.BytesIO(f))
        assert im.size == (56, 40)
