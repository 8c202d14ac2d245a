"""The DNG stage restated in NumPy (include/realcam_hip.h, rc_dng_*), in two halves that share nothing.

The ENCODER half restates the file bit for bit: the tile grid and its padding, the lossless-JPEG stream of a tile, the TIFF header with its
tag table, and the whole file.  Codes and lengths are formed for a whole tile at once and packed with np.packbits.

The READER half is written from TIFF 6.0 and ITU-T T.81 alone: it parses the IFD generically, builds its Huffman decoder from the DHT
segment it finds in the stream, and takes precision, dimensions and the predictor from SOF3 / SOS.  It uses no table or constant of the
encoder half (everything it needs has the prefix `rd_` or is local to it).
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

# ================================================================ the encoder half ================================================================
BITS = (0, 0, 5, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0)
HUFFVAL = (1, 2, 3, 4, 5, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
PRECISION = {"u8": 8, "mipi10": 10, "mipi12": 12, "u16": 16}
XYZ_TO_SRGB = (3.2404542, -1.5371385, -0.4985314, -0.9692660, 1.8760108, 0.0415560, 0.0556434, -0.2040259, 1.0572252)
COLOR = {"R": 0, "G": 1, "B": 2}


def huff_table():
    """SSSS -> (code, length) of the canonical code BITS / HUFFVAL describe (T.81 Annex C)."""
    t, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(BITS[length - 1]):
            t[HUFFVAL[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return t


def tile_header(storage, tw, th, components):
    """SOI, SOF3, DHT, SOS of a tile of tw x th samples."""
    p, nc = PRECISION[storage], components
    o = bytearray(b"\xff\xd8")
    o += b"\xff\xc3" + struct.pack(">HBHHB", 8 + 3 * nc, p, th, tw // nc, nc)
    for c in range(nc):
        o += bytes((c + 1, 0x11, 0))
    o += b"\xff\xc4" + struct.pack(">HB", 2 + 1 + 16 + len(HUFFVAL), 0x00) + bytes(BITS) + bytes(HUFFVAL)
    o += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc)
    for c in range(nc):
        o += bytes((c + 1, 0x00))
    o += bytes((1, 0, 0))
    return bytes(o)


def tile_samples(frame, ty, tx, tw, th):
    """The (th, tw) samples of tile (ty, tx) of a frame (H, W): beyond the frame the last sample of the same colour repeats."""
    H, W = frame.shape
    y = ty * th + np.arange(th)
    x = tx * tw + np.arange(tw)
    y = np.where(y < H, y, H - 2 + (y & 1))
    x = np.where(x < W, x, W - 2 + (x & 1))
    return frame[np.ix_(y, x)]


def entropy_bits(s, precision, components):
    """The tile's (words, lengths): per sample, in coding order, the Huffman code with its extra bits behind it and their bit count."""
    v = s.astype(np.int64)
    nc = components
    pred = np.empty_like(v)
    pred[:, nc:] = v[:, :-nc]
    pred[1:, :nc] = v[:-1, :nc]
    pred[0, :nc] = 1 << (precision - 1)
    d = (v - pred) & 0xffff
    d = np.where(d >= 32768, d - 65536, d)
    a = np.abs(d)
    ssss = np.zeros_like(a)
    for k in range(16):
        ssss += a >= (1 << k)
    nextra = np.where(ssss == 16, 0, ssss)
    extra = np.where(d >= 0, d, d + (1 << ssss) - 1) & ((1 << nextra) - 1)
    tab = huff_table()
    code = np.array([tab[i][0] for i in range(17)], np.int64)[ssss]
    clen = np.array([tab[i][1] for i in range(17)], np.int64)[ssss]
    return ((code << nextra) | extra).ravel(), (clen + nextra).ravel()


def entropy_bytes(words, lengths):
    """(the stuffed bytes, the 1-bits that padded the last byte): MSB first, 0xFF -> 0xFF 0x00."""
    j = np.arange(27)
    bits = (words[:, None] >> np.maximum(lengths[:, None] - 1 - j, 0)) & 1
    bits = bits[j[None, :] < lengths[:, None]].astype(np.uint8)
    pad = -len(bits) % 8
    raw = np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)]))
    ff = np.flatnonzero(raw == 0xff)
    return np.insert(raw, ff + 1, 0).tobytes(), pad


def tile_stream(s, storage, components):
    """The complete stream of a tile: SOI .. EOI."""
    th, tw = s.shape
    data, _ = entropy_bytes(*entropy_bits(s, PRECISION[storage], components))
    return tile_header(storage, tw, th, components) + data + b"\xff\xd9"


def _rational(v, signed=False):
    f = Fraction(int(np.rint(float(v) * (1 << 20))), 1 << 20)
    return struct.pack("<ii" if signed else "<II", f.numerator, f.denominator)


def tiff_header(tags):
    """`tags`: ascending (tag, type, count, value bytes).  II*, one IFD at 8, out-of-line values behind it on even offsets; the header's
    length is even.  Returns (bytes, {tag: offset of its value})."""
    n = len(tags)
    at = 8 + 2 + 12 * n + 4
    ifd, tail, where = bytearray(struct.pack("<H", n)), bytearray(), {}
    for i, (tag, typ, count, value) in enumerate(tags):
        if len(value) <= 4:
            where[tag] = 8 + 2 + 12 * i + 8
            field = value + bytes(4 - len(value))
        else:
            where[tag] = at + len(tail)
            field = struct.pack("<I", at + len(tail))
            tail += value + bytes(len(value) & 1)
        ifd += struct.pack("<HHI", tag, typ, count) + field
    ifd += struct.pack("<I", 0)
    return b"II*\0" + struct.pack("<I", 8) + bytes(ifd) + bytes(tail), where


def cfa_pattern(cfa, quad=False):
    """CFAPattern's bytes in row-major order: 2x2, or for a Quad-Bayer sensor the 4x4 tile whose 2x2 blocks have the colours of `cfa`."""
    c = [COLOR[ch] for ch in cfa]
    if not quad:
        return c
    return [c[2 * ((y >> 1) & 1) + ((x >> 1) & 1)] for y in range(4) for x in range(4)]


def header(h2, w2, storage, tw, th, cfa="RGGB", quad=False, blacks=(0.0,) * 4, white=1023, make="", model="realcam", unique_model=None,
           software="realcamnet_amd", datetime=None, linearization=None, color_matrix=XYZ_TO_SRGB, neutral=(1.0, 1.0, 1.0), noise_profile=None):
    """The TIFF header and IFD 0 of the file, the two tile arrays zero.  Returns (bytes, offsets_at, counts_at)."""
    tiles = -(-w2 // tw) * -(-h2 // th)
    S, L, B, A, R, SR, D = 3, 4, 1, 2, 5, 10, 12
    short = lambda *v: struct.pack(f"<{len(v)}H", *v)
    long_ = lambda *v: struct.pack(f"<{len(v)}I", *v)
    asc = lambda s: s.encode("ascii") + b"\0"
    pat = cfa_pattern(cfa, quad)
    dim = 4 if quad else 2
    unique = f"{make} {model}" if unique_model is None else unique_model
    tags = [(254, L, 1, long_(0)), (256, L, 1, long_(w2)), (257, L, 1, long_(h2)), (258, S, 1, short(8 if storage == "u8" else 16)), (259, S, 1, short(7)),
            (262, S, 1, short(32803)), (271, A, len(make) + 1, asc(make)), (272, A, len(model) + 1, asc(model)), (274, S, 1, short(1)), (277, S, 1, short(1)),
            (284, S, 1, short(1)), (305, A, len(software) + 1, asc(software))]
    if datetime is not None:
        tags.append((306, A, len(datetime) + 1, asc(datetime)))
    tags += [(322, L, 1, long_(tw)), (323, L, 1, long_(th)), (324, L, tiles, bytes(4 * tiles)), (325, L, tiles, bytes(4 * tiles)),
             (33421, S, 2, short(dim, dim)), (33422, B, len(pat), bytes(pat)), (50706, B, 4, bytes((1, 4, 0, 0))), (50707, B, 4, bytes((1, 1, 0, 0))),
             (50708, A, len(unique) + 1, asc(unique)), (50710, B, 3, bytes((0, 1, 2))), (50711, S, 1, short(1))]
    if linearization is not None:
        tags.append((50712, S, len(linearization), short(*linearization)))
    tags += [(50713, S, 2, short(2, 2)), (50714, R, 4, b"".join(_rational(b) for b in blacks)), (50717, L, 1, long_(int(white))),
             (50721, SR, 9, b"".join(_rational(m, True) for m in color_matrix)), (50728, R, 3, b"".join(_rational(v) for v in neutral)),
             (50778, S, 1, short(21))]
    if noise_profile is not None:
        tags.append((51041, D, len(noise_profile), struct.pack(f"<{len(noise_profile)}d", *noise_profile)))
    data, where = tiff_header(tags)
    return data, where[324], where[325]


def encode(frame, storage, tw, th, components, **tags):
    """The complete file of one frame (H, W) of integer codes.  Returns (bytes, the tiles' streams in raster order)."""
    H, W = frame.shape
    hdr, offsets_at, counts_at = header(H, W, storage, tw, th, **tags)
    out = bytearray(hdr)
    streams, offsets, counts = [], [], []
    for ty in range(-(-H // th)):
        for tx in range(-(-W // tw)):
            s = tile_stream(tile_samples(frame, ty, tx, tw, th), storage, components)
            streams.append(s)
            offsets.append(len(out))
            counts.append(len(s))
            out += s + bytes(len(s) & 1)
    out[offsets_at:offsets_at + 4 * len(offsets)] = struct.pack(f"<{len(offsets)}I", *offsets)
    out[counts_at:counts_at + 4 * len(counts)] = struct.pack(f"<{len(counts)}I", *counts)
    return bytes(out), streams


# ---- sensor lines, for the tests' inputs ----------------------------------------------------------------------------------------------------
def pack_lines(frame, storage):
    """A frame (H, W) of codes as the storage's dense lines: (H, W) uint16 / uint8, or (H, line bytes) uint8 of MIPI RAW10 / RAW12."""
    f = frame.astype(np.int64)
    H, W = f.shape
    if storage == "u16":
        return f.astype(np.uint16)
    if storage == "u8":
        return f.astype(np.uint8)
    if storage == "mipi10":
        g = f.reshape(H, W // 4, 4)
        low = (g[..., 0] & 3) | ((g[..., 1] & 3) << 2) | ((g[..., 2] & 3) << 4) | ((g[..., 3] & 3) << 6)
        return np.concatenate([g >> 2, low[..., None]], axis=-1).astype(np.uint8).reshape(H, -1)
    g = f.reshape(H, W // 2, 2)
    low = (g[..., 0] & 15) | ((g[..., 1] & 15) << 4)
    return np.concatenate([g >> 4, low[..., None]], axis=-1).astype(np.uint8).reshape(H, -1)


# ================================================================ the reader half =================================================================
RD_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4), 10: ("ii", 8),
            11: ("f", 4), 12: ("d", 8)}


def rd_ifd(data, at=None):
    """{tag: (type, count, values)} of the IFD at `at` (default: the first) of a TIFF file; rationals as Fractions, ASCII as str."""
    order = {b"II": "<", b"MM": ">"}[data[:2]]
    magic, first = struct.unpack(order + "HI", data[2:8])
    assert magic == 42
    at = first if at is None else at
    (n,) = struct.unpack_from(order + "H", data, at)
    out, last = {}, -1
    for i in range(n):
        tag, typ, count, field = struct.unpack_from(order + "HHI4s", data, at + 2 + 12 * i)[0:4]
        assert tag > last, "IFD entries must ascend"
        last = tag
        fmt, size = RD_TYPES[typ]
        nbytes = size * count
        if nbytes <= 4:
            raw = field[:nbytes]
        else:
            (off,) = struct.unpack(order + "I", field)
            assert off % 2 == 0, "values start on even offsets"
            raw = data[off:off + nbytes]
            assert len(raw) == nbytes
        if typ == 2:
            vals = raw.decode("ascii")
        else:
            flat = struct.unpack(order + fmt * count, raw)
            vals = tuple(Fraction(flat[2 * k], flat[2 * k + 1]) for k in range(count)) if typ in (5, 10) else flat
        out[tag] = (typ, count, vals)
    return out


def rd_huffman(bits, vals):
    """{(length, code): value} of a DHT table (T.81 C.2)."""
    t, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            t[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return t


def rd_tile(stream):
    """A lossless-JPEG stream (T.81 process 14) -> (samples (lines, columns * components) int64, precision, components, the count of
    stuffed bytes, the padding bits of the last byte)."""
    assert stream[:2] == b"\xff\xd8"
    at, tables, frame, scan = 2, {}, None, None
    while scan is None:
        assert stream[at] == 0xff
        marker = stream[at + 1]
        (length,) = struct.unpack_from(">H", stream, at + 2)
        body = stream[at + 4:at + 2 + length]
        if marker == 0xc3:
            p, lines, cols, nf = struct.unpack_from(">BHHB", body)
            comps = [struct.unpack_from("BBB", body, 6 + 3 * c) for c in range(nf)]
            assert all(hv == 0x11 for _, hv, _ in comps)
            frame = (p, lines, cols, [c[0] for c in comps])
        elif marker == 0xc4:
            k = 0
            while k < len(body):
                tc_th, counts = body[k], body[k + 1:k + 17]
                nv = sum(counts)
                assert tc_th >> 4 == 0
                tables[tc_th & 15] = rd_huffman(counts, body[k + 17:k + 17 + nv])
                k += 17 + nv
        elif marker == 0xda:
            ns = body[0]
            sel = {body[1 + 2 * c]: body[2 + 2 * c] >> 4 for c in range(ns)}
            ss, se, ahal = body[1 + 2 * ns:4 + 2 * ns]
            assert se == 0 and ahal == 0, "lossless scans have Se = 0 and no point transform here"
            scan = (sel, ss)
        else:
            raise AssertionError(f"unexpected marker {marker:#x}")
        at += 2 + length
    p, lines, cols, ids = frame
    sel, predictor = scan
    assert sorted(sel) == sorted(ids)
    # the entropy-coded segment: up to the first marker that is not a stuffed 0xFF
    end = at
    while not (stream[end] == 0xff and stream[end + 1] != 0):
        end += 1
    assert stream[end:end + 2] == b"\xff\xd9" and end + 2 == len(stream), "EOI ends the stream"
    seg = stream[at:end]
    stuffed = seg.count(b"\xff\x00")
    raw = seg.replace(b"\xff\x00", b"\xff")
    assert stuffed == raw.count(b"\xff"), "every 0xFF of the data is stuffed"
    nbits = 8 * len(raw)
    acc = int.from_bytes(raw, "big")
    pos = 0

    def take(n):
        nonlocal pos
        assert pos + n <= nbits, "the stream ends early"
        v = (acc >> (nbits - pos - n)) & ((1 << n) - 1)
        pos += n
        return v

    nc = len(ids)
    out = np.zeros((lines, cols, nc), np.int64)
    for y in range(lines):
        for x in range(cols):
            for c, cid in enumerate(ids):
                table = tables[sel[cid]]
                length, code = 0, 0
                while (length, code) not in table:
                    code = (code << 1) | take(1)
                    length += 1
                    assert length <= 16
                ssss = table[(length, code)]
                if ssss == 0:
                    d = 0
                elif ssss == 16:
                    d = 32768
                else:
                    e = take(ssss)
                    d = e if e >> (ssss - 1) else e - (1 << ssss) + 1
                if y == 0 and x == 0:
                    pred = 1 << (p - 1)
                elif y == 0:
                    pred = out[y, x - 1, c]
                elif x == 0:
                    pred = out[y - 1, x, c]
                else:
                    ra, rb, rc = out[y, x - 1, c], out[y - 1, x, c], out[y - 1, x - 1, c]
                    pred = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[predictor]
                out[y, x, c] = (pred + d) & 0xffff
    left = nbits - pos
    assert left < 8 and take(left) == (1 << left) - 1, "the last byte is padded with 1-bits"
    return out.reshape(lines, cols * nc), p, nc, stuffed, left


def rd_file(data):
    """A DNG file -> (the image (ImageLength, ImageWidth) int64, the IFD, the tiles as rd_tile returns them, in raster order)."""
    ifd = rd_ifd(data)
    one = lambda tag: ifd[tag][2][0]
    assert one(259) == 7 and one(262) == 32803 and one(277) == 1
    w, h, tw, th = one(256), one(257), one(322), one(323)
    nx, ny = -(-w // tw), -(-h // th)
    offsets, counts = ifd[324][2], ifd[325][2]
    assert len(offsets) == len(counts) == nx * ny
    img = np.zeros((ny * th, nx * tw), np.int64)
    tiles = []
    for t, (off, cnt) in enumerate(zip(offsets, counts)):
        assert off % 2 == 0 and off + cnt <= len(data)
        tile = rd_tile(data[off:off + cnt])
        assert tile[0].shape == (th, tw)
        tiles.append(tile)
        img[(t // nx) * th:(t // nx + 1) * th, (t % nx) * tw:(t % nx + 1) * tw] = tile[0]
    return img[:h, :w], ifd, tiles
