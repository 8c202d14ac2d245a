"""NumPy restatement of rc_yuv_encode for the professional video surfaces (include/realcam_hip.h, the layouts from RC_YUV_NV16 on): the
arithmetic step by step in fp32 (or, for the error bound, the same chain in float64), one packer per container that writes the bytes of
whole frames, padding included, and the inverse unpackers back to (Y, Cb, Cr) code arrays.  Nothing here imports the library: the plane
numbers come in as a PlaneLayout (OutFormat.plane_layout / out_format.frame_layout), whose values the host tests write out by hand."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}

# name -> (subsampling, bits, container, shift of the code in its sample)
LAYOUTS = {
    "nv12": ("420", 8, "semi", 0), "p010": ("420", 10, "semi", 6), "i420": ("420", 8, "planar", 0),
    "nv16": ("422", 8, "semi", 0), "p210": ("422", 10, "semi", 6), "i422": ("422", 8, "planar", 0), "i210": ("422", 10, "planar", 0),
    "i010": ("420", 10, "planar", 0), "i444": ("444", 8, "planar", 0), "i410": ("444", 10, "planar", 0),
    "yuy2": ("422", 8, "yuyv", 0), "uyvy": ("422", 8, "uyvy", 0), "y210": ("422", 10, "yuyv", 6), "v210": ("422", 10, "v210", 0),
}
NEW = tuple(n for n in LAYOUTS if n not in ("nv12", "p010", "i420"))


def codes(x, sub, bits, matrix="bt709", vrange="limited", siting="left", dtype=np.float32):
    """x (B,3,h,w) float -> int32 codes Y (B,h,w), Cb, Cr (B,h,w) / (B,h,w/2) / (B,h/2,w/2) for sub "444" / "422" / "420".  Every product
    and every sum is one operation of `dtype`, in the order the header writes them; the constants are doubles rounded to `dtype` once."""
    t = dtype
    x = np.asarray(x).astype(t)
    x = np.clip(np.where(np.isnan(x), t(0), x), t(0), t(1))
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    kr, kb = KR_KB[matrix]
    y = ((t(kr) * r) + (t(1.0 - kr - kb) * g)) + (t(kb) * b)
    cb = (b - y) * t(0.5 / (1.0 - kb))
    cr = (r - y) * t(0.5 / (1.0 - kr))

    def row_left(c):                                                  # t of the header: x = 2i, c[x - 1] clamped to column 0
        left = np.concatenate([c[..., :1], c[..., :-1]], -1)
        return ((left[..., 0::2] + c[..., 1::2]) + (c[..., 0::2] + c[..., 0::2])) * t(0.25)

    def sub_chroma(c):
        if sub == "444":
            return c
        if sub == "422":
            return row_left(c) if siting == "left" else (c[..., 0::2] + c[..., 1::2]) * t(0.5)
        if siting == "left":
            tt = row_left(c)
            return (tt[:, 0::2] + tt[:, 1::2]) * t(0.5)
        return ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * t(0.25)

    k, top = float(1 << (bits - 8)), float((1 << bits) - 1)
    if vrange == "limited":
        qy, qc = (219 * k, 16 * k, 16 * k, 235 * k), (224 * k, 128 * k, 16 * k, 240 * k)
    else:
        qy, qc = (top, 0.0, 0.0, top), (top, float(1 << (bits - 1)), 0.0, top)
    q = lambda v, p: np.clip(np.rint((v * t(p[0])) + t(p[1])), p[2], p[3]).astype(np.int32)       # rint: half to even
    return q(y, qy), q(sub_chroma(cb), qc), q(sub_chroma(cr), qc)


def format_codes(x, fmt, dtype=np.float32):
    """codes() for an OutFormat-like object (layout, matrix, range, chroma_siting)."""
    sub, bits, _, _ = LAYOUTS[fmt.layout]
    return codes(x, sub, bits, fmt.matrix, fmt.range, fmt.chroma_siting, dtype)


def _samples(c, es, shift):
    """(B,rows,n) codes -> (B,rows,n*es) little-endian bytes."""
    return np.ascontiguousarray((c.astype(np.uint32) << shift).astype("<u1" if es == 1 else "<u2")).view(np.uint8).reshape(c.shape[0], c.shape[1], -1)


def v210_words(y, cb, cr):
    """(B,h,w), (B,h,w/2) x 2 -> (B,h,ceil(w/6),4) uint32: six pixels in four dwords, the fields of samples that do not exist zero."""
    B, h, w = y.shape
    G = -(-w // 6)
    Y = np.zeros((B, h, 6 * G), np.uint32); Y[..., :w] = y
    U = np.zeros((B, h, 3 * G), np.uint32); U[..., :w // 2] = cb
    V = np.zeros((B, h, 3 * G), np.uint32); V[..., :w // 2] = cr
    Y, U, V = Y.reshape(B, h, G, 6), U.reshape(B, h, G, 3), V.reshape(B, h, G, 3)
    return np.stack([U[..., 0] | Y[..., 0] << 10 | V[..., 0] << 20, Y[..., 1] | U[..., 1] << 10 | Y[..., 2] << 20,
                     V[..., 1] | Y[..., 3] << 10 | U[..., 2] << 20, Y[..., 4] | V[..., 2] << 10 | Y[..., 5] << 20], -1)


def pack(name, yc, cb, cr, pl):
    """The bytes (B, frame_bytes) uint8 of whole frames of layout `name` with the planes of `pl`, every byte that is not a sample zero."""
    _, bits, cont, shift = LAYOUTS[name]
    es = 1 if bits == 8 else 2
    il = lambda *c: np.stack(c, -1).reshape(c[0].shape[0], c[0].shape[1], -1)      # interleave along the row
    parts = {"y": lambda: _samples(yc, es, shift), "cb": lambda: _samples(cb, es, shift), "cr": lambda: _samples(cr, es, shift),
             "cbcr": lambda: _samples(il(cb, cr), es, shift),
             "yuyv": lambda: _samples(il(yc[..., 0::2], cb, yc[..., 1::2], cr), es, shift),
             "uyvy": lambda: _samples(il(cb, yc[..., 0::2], cr, yc[..., 1::2]), es, shift),
             "v210": lambda: np.ascontiguousarray(v210_words(yc, cb, cr).astype("<u4")).view(np.uint8).reshape(yc.shape[0], yc.shape[1], -1)}
    buf = np.zeros((yc.shape[0], pl.frame_bytes), np.uint8)
    for p in pl.planes:
        data = parts[p.name]()
        assert data.shape[1:] == (p.rows, p.valid_bytes), (name, p, data.shape)
        buf[:, p.offset:p.offset + p.pitch * p.alloc_rows].reshape(-1, p.alloc_rows, p.pitch)[:, :p.rows, :p.valid_bytes] = data
    assert cont in ("planar", "semi") or len(pl.planes) == 1
    return buf


def unpack(name, buf, pl, h, w):
    """The inverse: frames' bytes (B, frame_bytes) uint8 -> int32 codes (Y, Cb, Cr)."""
    sub, bits, cont, shift = LAYOUTS[name]
    es = 1 if bits == 8 else 2
    buf = np.ascontiguousarray(buf)
    got = {}
    for p in pl.planes:
        raw = buf[:, p.offset:p.offset + p.pitch * p.alloc_rows].reshape(-1, p.alloc_rows, p.pitch)[:, :p.rows, :p.valid_bytes]
        raw = np.ascontiguousarray(raw)
        if p.name == "v210":
            wd = raw.view("<u4").astype(np.uint32).reshape(raw.shape[0], p.rows, -1, 4)
            f = lambda i, s: (wd[..., i] >> s) & 1023
            Y = np.stack([f(0, 10), f(1, 0), f(1, 20), f(2, 10), f(3, 0), f(3, 20)], -1).reshape(raw.shape[0], p.rows, -1)
            U = np.stack([f(0, 0), f(1, 10), f(2, 20)], -1).reshape(raw.shape[0], p.rows, -1)
            V = np.stack([f(0, 20), f(2, 0), f(3, 10)], -1).reshape(raw.shape[0], p.rows, -1)
            return Y[..., :w].astype(np.int32), U[..., :w // 2].astype(np.int32), V[..., :w // 2].astype(np.int32)
        got[p.name] = (raw.view("<u1" if es == 1 else "<u2").astype(np.int32) >> shift)
    if cont == "planar":
        return got["y"], got["cb"], got["cr"]
    if cont == "semi":
        return got["y"], got["cbcr"][..., 0::2], got["cbcr"][..., 1::2]
    s = got[cont]
    if cont == "yuyv":
        return np.stack([s[..., 0::4], s[..., 2::4]], -1).reshape(s.shape[0], h, w), s[..., 1::4], s[..., 3::4]
    return np.stack([s[..., 1::4], s[..., 3::4]], -1).reshape(s.shape[0], h, w), s[..., 0::4], s[..., 2::4]
