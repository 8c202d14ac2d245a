"""CPU: the JPEG output's public types, the library's host functions (rc_jpeg_tables / rc_jpeg_plan / rc_jpeg_header) and the reference the
GPU tests compare with (tests/jpeg_ref.py) -- against Pillow / libjpeg, against the float64 DCT, and against a Huffman decoder of its own."""
import ctypes as C
import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image, JpegImagePlugin

import jpeg_ref as R
import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.jpeg import HEADER_BYTES, JpegPlan

PIL_SUB = {"420": 2, "444": 0}
# PSNR (dB) by which the reference stream, decoded by Pillow, falls short of Pillow's own file of the same rgb8 at the same quality and
# subsampling, on jpeg_ref.smooth at 96 x 128 -- measured; where the reference is ahead there is no shortfall.  The two differ in the DCT's
# rounding (and in nothing else that loses information): the tests allow 0.1 dB over these.
FIDELITY_SHORTFALL_DB = {("420", 50): 0.0, ("420", 90): 0.0, ("420", 100): 0.0, ("444", 50): 0.017, ("444", 90): 0.0, ("444", 100): 0.0}


def rgb8_of(x):
    """(3, h, w) float -> (h, w, 3) uint8 as rc_rgb_encode rounds it."""
    with np.errstate(invalid="ignore"):
        x = np.where(x > 0, np.where(x < 1, x, 1), 0).astype(np.float32)
    return np.rint(x * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)


def pillow_file(rgb8, quality, sub):
    b = io.BytesIO()
    Image.fromarray(rgb8).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sub])
    return b.getvalue()


def pillow_psnr(rgb8, quality, sub):
    return R.psnr(np.asarray(Image.open(io.BytesIO(pillow_file(rgb8, quality, sub))).convert("RGB")), rgb8)


def case_frames(name):
    sub, quality, restart, dtype, src, (h, w) = R.case_source(name)
    frames = torch.from_numpy(src).to(getattr(torch, dtype)).float().numpy()[:, :, :h, :w]
    return sub, quality, restart, frames, (h, w)


# ---- the public types ----------------------------------------------------------------------------------------------------------------------------
def test_jpeg_validation_and_plan():
    j = M.Jpeg()
    assert (j.quality, j.subsampling, j.restart, j.capacity) == (90, "420", 8, None)
    assert hash(M.Jpeg(75, "444", 3)) == hash(M.Jpeg(75, "444", 3)) and M.Jpeg(75) != M.Jpeg(76) and {M.Jpeg(): 1}[M.Jpeg()] == 1
    with pytest.raises(Exception):
        j.quality = 5
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling="422"), dict(subsampling=420), dict(restart=0), dict(restart=65536), dict(capacity=0)):
        with pytest.raises(ValueError):
            M.Jpeg(**bad)
    for bad in (dict(quality=90.0), dict(quality=True), dict(restart="8"), dict(capacity=1.5)):
        with pytest.raises(TypeError):
            M.Jpeg(**bad)
    assert j.plan(2160, 3840) == JpegPlan(HEADER_BYTES, 240, 135, 4050, HEADER_BYTES + 3 * 2160 * 3840 // 2 + 2 * 4050 + 2)
    assert M.Jpeg(subsampling="444", restart=4).plan(24, 80) == JpegPlan(HEADER_BYTES, 10, 3, 8, HEADER_BYTES + 3 * 24 * 80 + 16 + 2)
    assert j.plan(17, 23) == JpegPlan(HEADER_BYTES, 2, 2, 1, HEADER_BYTES + 3 * 32 * 32 // 2 + 2 + 2)              # any size: padded to the MCU
    assert j.plan(1, 1).mcu_cols == 1 and M.Jpeg(capacity=1000).plan(64, 64).capacity == 1000
    assert j.plan(65535, 65535).intervals == -(-4096 * 4096 // 8)
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        with pytest.raises(ValueError):
            j.plan(h, w)
    with pytest.raises(TypeError):
        j.plan(8.0, 8)
    assert "Jpeg" in M.__all__ and "JpegFrames" in M.__all__


def test_plan_and_desc_agree_with_the_library():
    L = _lib.load()
    assert L.rc_jpeg_desc_size() == C.sizeof(_lib.JpegDesc) == 32
    for sub in ("420", "444"):
        for restart in (1, 3, 8, 65535):
            for h, w in ((1, 1), (17, 23), (40, 136), (2160, 3840), (65535, 65535)):
                fmt = M.Jpeg(50, sub, restart)
                p, d = _lib.JpegPlanInfo(), fmt.desc()
                _lib.check(L.rc_jpeg_plan(C.byref(d), h, w, C.byref(p)))
                assert fmt.plan(h, w) == JpegPlan(p.header_bytes, p.mcu_cols, p.mcu_rows, p.intervals, p.capacity)
                assert p.scratch_bytes == 4 * p.intervals and R.plan(sub, restart, h, w) == (p.mcu_cols, p.mcu_rows, p.intervals, p.capacity)
    p = _lib.JpegPlanInfo()
    for d, h, w in ((_lib.JpegDesc(0, 0, 8), 8, 8), (_lib.JpegDesc(101, 0, 8), 8, 8), (_lib.JpegDesc(90, 2, 8), 8, 8), (_lib.JpegDesc(90, 0, 0), 8, 8),
                    (_lib.JpegDesc(90, 0, 65536), 8, 8), (_lib.JpegDesc(90, 0, 8), 0, 8), (_lib.JpegDesc(90, 0, 8), 8, 65536)):
        assert L.rc_jpeg_plan(C.byref(d), h, w, C.byref(p)) != 0
    d = _lib.JpegDesc(90, 0, 8)
    d.reserved[2] = 1
    assert L.rc_jpeg_plan(C.byref(d), 8, 8, C.byref(p)) != 0 and b"reserved" in L.rc_last_error()


def test_refusals_without_a_gpu():
    """Output / out_format learn the type; the refusals stay ValueError / TypeError raised before anything touches a device."""
    jp = M.Jpeg(75)
    o = M.Output(jp, M.Resize((37, 51)))                                      # odd sizes: the 4:2:0 evenness rule is the encoder surfaces' alone
    assert o.plan(144, 208) == (37, 51) and hash(o) == hash(M.Output(jp, M.Resize((37, 51))))
    with pytest.raises(ValueError):
        M.Output(M.OutFormat("nv12"), M.Resize((37, 51)))
    with pytest.raises(TypeError, match="a Jpeg"):
        M.Output(3)
    with pytest.raises(ValueError, match="a Jpeg"):
        M.Output("jpeg")
    with pytest.raises(TypeError, match="Jpeg"):
        ops.jpeg_encode(torch.zeros(1, 3, 8, 8), "jpeg")
    with pytest.raises(Exception):
        ops.jpeg_encode(torch.zeros(1, 3, 8, 8), jp)                          # a CPU tensor: refused, no fall-back
    net = M.LiteISPNet().eval()
    mosaic, coord = torch.zeros(1, 1, 32, 32), torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="either out_format or outputs"):
        net.forward_mosaic(mosaic, None, coord, out_format=jp, outputs=[M.Output(jp)])
    with pytest.raises(TypeError, match="a Jpeg"):
        net.forward_mosaic(mosaic, None, coord, out_format=3)


def test_fake_trace_of_a_ladder_with_a_jpeg():
    """forward_mosaic(outputs=[... Jpeg ...]) under FakeTensorMode: the shapes, dtypes and device planned, for a DWT net and a strided net,
    without the library being asked for a header; the codec's forward_mosaic keeps refusing outputs."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                jp = M.Jpeg(80, "444", 5)
                ladder = [M.Output(M.OutFormat("nv12")), M.Output(jp, M.Resize((37, 51))), M.Output(M.Jpeg(capacity=5000))]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                        one = net.forward_mosaic(mosaic, None, coord, out_format=jp)
                    assert isinstance(a, M.YuvFrames) and isinstance(b, M.JpegFrames) and b.fmt == jp and b.size == (37, 51)
                    assert b.buffer.shape == (2, jp.plan(37, 51).capacity) and b.buffer.dtype == torch.uint8 and b.buffer.device.type == "cuda"
                    assert b.lengths.shape == (2,) and b.lengths.dtype == torch.int64
                    assert c.buffer.shape == (2, 5000) and c.size == (144, 208) and one.buffer.shape == (2, jp.plan(144, 208).capacity)
                import realcamnet_amd.raw2bit as RB
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(jp)])
    finally:
        torch.set_default_dtype(old)
    assert not any(k[0] == "jpeg_header" for k in ops._JPEG_HEADERS.__dict__.get("_rc_cache", {}))          # a trace builds and keeps nothing


def test_frames_say_which_capacity_would_do():
    fr = M.JpegFrames(torch.zeros(2, 10, dtype=torch.uint8), torch.tensor([12, 4]), M.Jpeg(capacity=10), (8, 8))
    assert fr.tobytes(1) == bytes(4)
    with pytest.raises(ValueError, match="capacity=12"):
        fr.tobytes(0)
    with pytest.raises(ValueError, match="capacity=12"):
        fr.files()


# ---- the library's host functions against Pillow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", (1, 10, 50, 75, 90, 95, 100))
def test_tables_are_the_ones_pillow_writes(quality):
    ql, qc = M.Jpeg(quality).tables()
    assert np.array_equal(ql.reshape(64), R.tables(quality)[0]) and np.array_equal(qc.reshape(64), R.tables(quality)[1])
    im = Image.open(io.BytesIO(pillow_file(np.zeros((16, 16, 3), np.uint8), quality, "420")))
    theirs = {k: list(v) for k, v in im.quantization.items()}
    ours = [ql.reshape(64).tolist(), qc.reshape(64).tolist()]
    zig = [ql.reshape(64)[R.ZIGZAG].tolist(), qc.reshape(64)[R.ZIGZAG].tolist()]
    assert [theirs[0], theirs[1]] in (ours, zig)                               # whichever order this Pillow reports them in


@pytest.mark.parametrize("sub", ("420", "444"))
def test_header_opens_in_pillow(sub):
    for quality, restart, (h, w) in ((90, 8, (16, 16)), (10, 3, (17, 23)), (100, 65535, (9, 13))):
        fmt = M.Jpeg(quality, sub, restart)
        head = fmt.header(h, w)
        assert len(head) == HEADER_BYTES == fmt.plan(h, w).header_bytes and head == R.header(quality, sub, restart, h, w)
        x = R.noise((1, 3, h, w), 1)[0]
        data = R.encode(x, quality, sub, restart)
        assert data[:HEADER_BYTES] == head                                     # the library's header followed by a reference stream
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h) and im.mode == "RGB" and JpegImagePlugin.get_sampling(im) == PIL_SUB[sub]
        assert im.info.get("jfif") == 257 and im.info.get("jfif_density") == (1, 1)
    # the DHT segment is the one libjpeg writes for its default (Annex K.3.3) tables
    theirs = pillow_file(np.zeros((16, 16, 3), np.uint8), 90, sub)
    assert sorted(_dht_tables(M.Jpeg(90, sub).header(16, 16))) == sorted(_dht_tables(theirs)) and len(_dht_tables(theirs)) == 4
    short, n = C.create_string_buffer(100), C.c_size_t(0)
    d = fmt.desc()
    assert _lib.load().rc_jpeg_header(C.byref(d), 16, 16, C.cast(short, C.c_void_p), 100, C.byref(n)) != 0


def _dht_tables(data):
    """Every Huffman table (class / id byte, BITS, HUFFVAL) of the DHT segments in front of SOS."""
    pos, out = 2, []
    while data[pos + 1] != 0xda:
        length = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg, k = data[pos + 4:pos + 2 + length], 0
        while data[pos + 1] == 0xc4 and k < len(seg):
            n = sum(seg[k + 1:k + 17])
            out.append(bytes(seg[k:k + 17 + n]))
            k += 17 + n
        pos += 2 + length
    return out


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------------
def test_m_is_regenerated_from_its_formula():
    assert np.array_equal(R.make_m(), R.M) and int(np.abs(R.M).max()) == 8035
    src = (Path(_lib.PKG) / "csrc" / "jpeg.hip").read_text()
    table = re.search(r"kJpegM\[64\] = \{([^}]*)\}", src).group(1)
    assert np.array_equal(np.array([int(v) for v in table.replace("\n", " ").split(",")]).reshape(8, 8), R.make_m())
    zig = re.search(r"kZigzag\[64\] = \{([^}]*)\}", src).group(1)
    assert [int(v) for v in zig.replace("\n", " ").split(",")] == R.ZIGZAG.tolist()
    order = sorted(range(64), key=lambda i: ((i // 8 + i % 8), (i // 8 if (i // 8 + i % 8) % 2 else i % 8)))     # the zigzag walk itself
    assert order == R.ZIGZAG.tolist()


def test_dct_accuracy_and_int32_bounds():
    rng = np.random.default_rng(0)
    blocks = rng.integers(0, 256, size=(20000, 8, 8))
    signs = np.sign(R.make_m().astype(np.float64))
    extreme = np.array([[np.where(s * np.outer(signs[v], signs[u]) >= 0, 255, 0) for s in (1, -1)] for v in range(8) for u in range(8)]).reshape(128, 8, 8)
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    cmat = np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    worst = {}
    for name, b in (("random", blocks), ("extreme", extreme)):
        r, f = R.fdct(b)
        exact = cmat @ (b.astype(np.float64) - 128) @ cmat.T
        worst[name] = float(np.abs(f / 2.0 ** 19 - exact).max())
        assert np.abs(r).max() <= 11586 and np.abs(f).max() <= 536941584 < 2 ** 30
        assert np.abs((b - 128) @ R.M.T).max() < 2 ** 31
    print("DCT error (coefficient units):", worst)
    assert max(worst.values()) <= 0.25
    _, f = R.fdct(np.zeros((1, 8, 8), dtype=np.int64))
    assert f[0, 0, 0] == -536941584                                           # the bound is reached: a black block


def test_the_kernels_division_is_exact():
    """q = (((|F| + (Q << 18)) >> 19) * ceil(2^20 / Q)) >> 20 in uint32, as jpeg.hip divides, for every dividend and every Q."""
    t = np.arange(4096, dtype=np.uint64)
    for q in range(1, 256):
        rcp = ((1 << 20) + q - 1) // q
        assert 4095 * rcp < 2 ** 32 and np.array_equal((t * np.uint64(rcp)) >> np.uint64(20), t // np.uint64(q))
    f = np.random.default_rng(1).integers(-536941584, 536941585, size=100000)
    for q in (1, 2, 3, 16, 99, 255):
        assert np.array_equal(np.abs(R.quantise(f, q)), ((np.abs(f) + (q << 18)) >> 19) // q)
    assert ((536941584 + (255 << 18)) >> 19) < 4096


# ---- the reference streams of the GPU cases ----------------------------------------------------------------------------------------------------
def test_reference_streams_decode_to_their_coefficients_and_load_in_pillow():
    """jpeg_ref's own Huffman decoder gives back the reference's quantised coefficients exactly, Pillow loads every stream at the crop's
    size -- and, across the set, the inputs reach every branch of the coder."""
    met = {}
    for name in sorted(R.CASES):
        sub, quality, restart, frames, (h, w) = case_frames(name)
        for f in frames:
            st = {}
            data = R.encode(f, quality, sub, restart, st)
            want = R.coefficients(f, quality, sub)
            got = R.decode_coefficients(data)
            assert len(got) == len(want) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got, want)), name
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.size == (w, h) and JpegImagePlugin.get_sampling(im) == PIL_SUB[sub]
            for k, v in st.items():
                met[k] = max(met.get(k, 0), v)
    assert met["stuffed"] > 0 and met["zrl"] > 0 and met["no_eob"] > 0 and met["all_eob"] > 0, met
    assert met["max_dc_cat"] == 11 and met["max_ac_cat"] == 10, met
    assert met["short_last"] > 0 and met["rst_wrap"] > 0, met


def test_reference_pixels_track_pillows_decoder_input():
    """The reference's samples are JFIF's: Pillow's decode of a flat quality-100 stream (every AC zero, DC exact: Q = 1) gives the source
    colour back within 2 codes -- half a code of Y, half a code of Cb times 1.772 (blue, the worst channel), the decoder's own rounding and
    the rgb8's: 0.5 + 0.886 + 0.5 + 0.5 < 3."""
    x = R.flat((1, 3, 16, 16), (0.2, 0.6, 0.9))[0]
    for sub in ("420", "444"):
        got = np.asarray(Image.open(io.BytesIO(R.encode(x, 100, sub, 8))).convert("RGB")).astype(int)
        assert np.abs(got - rgb8_of(x).astype(int)).max() <= 2


@pytest.mark.parametrize("sub", ("420", "444"))
def test_fidelity_against_pillows_own_file(sub):
    x = R.smooth((1, 3, 96, 128))[0]
    rgb8 = rgb8_of(x)
    for quality in (50, 90, 100):
        ours = R.psnr(np.asarray(Image.open(io.BytesIO(R.encode(x, quality, sub, 4))).convert("RGB")), rgb8)
        theirs = pillow_psnr(rgb8, quality, sub)
        print(f"fidelity {sub} q{quality}: reference {ours:.3f} dB, Pillow {theirs:.3f} dB, shortfall {theirs - ours:+.3f} dB")
        assert ours >= theirs - FIDELITY_SHORTFALL_DB[(sub, quality)] - 0.1
