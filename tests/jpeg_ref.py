"""NumPy restatement of rc_jpeg_encode (include/realcam_hip.h): the sample step, the integer DCT, the quantiser, the baseline Huffman coder
with restart intervals and byte stuffing -- and, independent of the coder, a small Huffman decoder that gives the quantised coefficients of
a stream back.  Shared by tests/test_jpeg_host.py and tests/test_jpeg_gpu.py; also holds the cases both run, so the host tests can show
that the GPU tests' inputs reach every branch of the coder."""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
BITS_DC_L = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
BITS_DC_C = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
VALS_DC = list(range(12))
BITS_AC_L = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
VALS_AC_L = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
BITS_AC_C = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
VALS_AC_C = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
# M[u][x] = rint(2^14 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2: the constant table (make_m regenerates it)
M = np.array([[5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793], [8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035],
              [7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568], [6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811],
              [5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793], [4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551],
              [3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135], [1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598]], dtype=np.int64)
MCU = {"420": 16, "444": 8}
HEADER_BYTES = 613


def make_m():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(2.0 ** 14 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def tables(quality):
    """The two 8-bit tables in natural order: the IJG rule in integers."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a BITS / HUFFVAL pair (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(BITS_DC_L, VALS_DC), huff_codes(BITS_DC_C, VALS_DC))
AC_CODES = (huff_codes(BITS_AC_L, VALS_AC_L), huff_codes(BITS_AC_C, VALS_AC_C))


def plan(sub, restart, h, w):
    mcu = MCU[sub]
    cols, rows = -(-w // mcu), -(-h // mcu)
    intervals = -(-cols * rows // restart)
    area = cols * rows * mcu * mcu
    return cols, rows, intervals, HEADER_BYTES + (3 * area if sub == "444" else 3 * area // 2) + 2 * intervals + 2


def header(quality, sub, restart, h, w):
    ql, qc = tables(quality)
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    o += b"\xff\xdb" + (132).to_bytes(2, "big") + b"\x00" + bytes(ql[ZIGZAG].tolist()) + b"\x01" + bytes(qc[ZIGZAG].tolist())
    o += b"\xff\xc0" + (17).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03"
    o += bytes([1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    o += b"\xff\xc4" + (418).to_bytes(2, "big")
    for tc_th, bits, vals in ((0x00, BITS_DC_L, VALS_DC), (0x01, BITS_DC_C, VALS_DC), (0x10, BITS_AC_L, VALS_AC_L), (0x11, BITS_AC_C, VALS_AC_C)):
        o += bytes([tc_th] + bits + vals)
    o += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    o += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(o) == HEADER_BYTES
    return bytes(o)


# ---- step 1: samples --------------------------------------------------------------------------------------------------------------------------
def _f(v):
    return np.float32(v)


KR, KB = 0.299, 0.114
K = (_f(KR), _f(1.0 - KR - KB), _f(KB), _f(0.5 / (1.0 - KB)), _f(0.5 / (1.0 - KR)))          # Kr, Kg, Kb, sb, sr: double, rounded to fp32 once


def _code(v, offset):
    return np.clip(np.rint(v * _f(255.0) + _f(offset)), 0, 255).astype(np.int64)


def samples(rgb, sub):
    """rgb (3, h, w) float32 (the source's values) -> the code planes of the padded MCU grid: Y (hp, wp) and Cb, Cr (hp, wp) at 4:4:4 or
    (hp / 2, wp / 2) at 4:2:0.  fp32, every product and sum rounded on its own."""
    rgb = np.asarray(rgb, dtype=np.float32)
    _, h, w = rgb.shape
    mcu = MCU[sub]
    hp, wp = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    rgb = rgb[:, np.minimum(np.arange(hp), h - 1)][:, :, np.minimum(np.arange(wp), w - 1)]
    with np.errstate(invalid="ignore"):
        rgb = np.where(rgb > 0, np.where(rgb < 1, rgb, _f(1)), _f(0)).astype(np.float32)       # NaN compares false: 0
    r, g, b = rgb
    y = (K[0] * r + K[1] * g) + K[2] * b
    cb, cr = (b - y) * K[3], (r - y) * K[4]
    assert y.dtype == np.float32 and cb.dtype == np.float32
    if sub == "420":
        cb, cr = (((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * _f(0.25) for c in (cb, cr))
    return _code(y, 0.0), _code(cb, 128.0), _code(cr, 128.0)


# ---- steps 2 and 3: DCT and quantiser -------------------------------------------------------------------------------------------------------
def fdct(codes):
    """codes (..., 8, 8) ints -> (R', F) of step 2, int64 (the caller may check that they fit int32)."""
    s = np.asarray(codes, dtype=np.int64) - 128
    r = (s @ M.T + 256) >> 9                       # R[y][u] = sum_x M[u][x] s[y][x]
    return r, M @ r                                # F[v][u] = sum_y M[v][y] R'[y][u]


def quantise(f, q):
    a = (np.abs(f) + (q << 18)) // (q << 19)
    return np.where(f < 0, -a, a)


def blocks_in_order(planes, sub):
    """The quantiser's inputs in coding order: [(component, codes (8, 8))] MCU by MCU."""
    y, cb, cr = planes
    mcu = MCU[sub]
    out = []
    for my in range(y.shape[0] // mcu):
        for mx in range(y.shape[1] // mcu):
            if sub == "420":
                for by in range(2):
                    for bx in range(2):
                        out.append((0, y[my * 16 + by * 8:my * 16 + by * 8 + 8, mx * 16 + bx * 8:mx * 16 + bx * 8 + 8]))
            else:
                out.append((0, y[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]))
            out.append((1, cb[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]))
            out.append((2, cr[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]))
    return out


def coefficients(rgb, quality, sub):
    """[(component, q (64,) in zigzag order)] in coding order."""
    ql, qc = tables(quality)
    out = []
    for comp, codes in blocks_in_order(samples(rgb, sub), sub):
        q = quantise(fdct(codes)[1], (qc if comp else ql).reshape(8, 8))
        out.append((comp, q.reshape(64)[ZIGZAG]))
    return out


# ---- step 4: the entropy coder ------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, code, length):
        self.v, self.n = (self.v << length) | code, self.n + length


def _category(v):
    return int(abs(int(v))).bit_length()


def _magnitude(v, cat):
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def encode(rgb, quality=90, sub="420", restart=8, stats=None):
    """rgb (3, h, w) float32 -> the complete file.  stats, a dict, collects what the coder met."""
    rgb = np.asarray(rgb, dtype=np.float32)
    _, h, w = rgb.shape
    st = stats if stats is not None else {}
    for k in ("stuffed", "zrl", "no_eob", "all_eob", "max_dc_cat", "max_ac_cat", "short_last", "rst_wrap"):
        st.setdefault(k, 0)
    coefs = coefficients(rgb, quality, sub)
    per_mcu = 6 if sub == "420" else 3
    nmcu = len(coefs) // per_mcu
    out = bytearray(header(quality, sub, restart, h, w))
    nint = -(-nmcu // restart)
    if nmcu % restart:
        st["short_last"] += 1
    for i in range(nint):
        bits, pred = Bits(), [0, 0, 0]
        for comp, q in coefs[i * restart * per_mcu:(i + 1) * restart * per_mcu]:
            t = 1 if comp else 0
            d = int(q[0]) - pred[comp]
            pred[comp] = int(q[0])
            cat = _category(d)
            st["max_dc_cat"] = max(st["max_dc_cat"], cat)
            bits.put(*DC_CODES[t][cat])
            bits.put(_magnitude(d, cat), cat)
            run = 0
            for k in range(1, 64):
                if q[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    bits.put(*AC_CODES[t][0xf0])
                    st["zrl"] += 1
                    run -= 16
                cat = _category(q[k])
                st["max_ac_cat"] = max(st["max_ac_cat"], cat)
                bits.put(*AC_CODES[t][(run << 4) | cat])
                bits.put(_magnitude(q[k], cat), cat)
                run = 0
            if q[63] == 0:
                bits.put(*AC_CODES[t][0x00])
                if not np.any(q[1:]):
                    st["all_eob"] += 1
            else:
                st["no_eob"] += 1
        pad = -bits.n % 8
        bits.put((1 << pad) - 1, pad)
        raw = bits.v.to_bytes(bits.n // 8, "big")
        st["stuffed"] += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
        if i < nint - 1:
            out += bytes([0xff, 0xd0 + i % 8])
            if i >= 8:
                st["rst_wrap"] += 1
    out += b"\xff\xd9"
    return bytes(out)


# ---- a decoder of its own: the stream's quantised coefficients back ---------------------------------------------------------------------------
def decode_coefficients(data):
    """A baseline file with three components and restart intervals -> [(component, q (64,) zigzag)] in coding order.  Reads every table from
    the file's own segments; shares nothing with `encode` but the zigzag order."""
    pos, huff, comps, restart = 2, {}, None, 0
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[pos] == 0xff, pos
        marker, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xc4:
            k = 0
            while k < len(seg):
                bits, n = list(seg[k + 1:k + 17]), sum(seg[k + 1:k + 17])
                huff[seg[k]] = {(length_, code): sym for sym, (code, length_) in huff_codes(bits, list(seg[k + 17:k + 17 + n])).items()}
                k += 17 + n
        elif marker == 0xc0:
            hh, ww = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c]) for c in range(seg[5])]
        elif marker == 0xdd:
            restart = int.from_bytes(seg, "big")
        elif marker == 0xda:
            break
    hs, vs = comps[0][1] >> 4, comps[0][1] & 15
    nmcu = -(-ww // (8 * hs)) * -(-hh // (8 * vs))
    layout = [0] * (hs * vs) + [1, 2]
    intervals, cur, k = [], bytearray(), pos
    while True:
        if data[k] != 0xff:
            cur.append(data[k]); k += 1
        elif data[k + 1] == 0x00:
            cur.append(0xff); k += 2
        elif 0xd0 <= data[k + 1] <= 0xd7:
            assert data[k + 1] == 0xd0 + len(intervals) % 8
            intervals.append(bytes(cur)); cur = bytearray(); k += 2
        else:
            assert data[k + 1] == 0xd9 and k + 2 == len(data)
            intervals.append(bytes(cur))
            break
    out, left = [], nmcu
    for chunk in intervals:
        v, n, at, pred = int.from_bytes(chunk, "big"), 8 * len(chunk), 0, [0, 0, 0]

        def take(m):
            nonlocal at
            at += m
            assert at <= n
            return (v >> (n - at)) & ((1 << m) - 1)

        def symbol(table):
            code, length = 0, 0
            while True:
                code, length = (code << 1) | take(1), length + 1
                if (length, code) in table:
                    return table[(length, code)]
                assert length < 16

        def extend(m):
            b = take(m) if m else 0
            return b if m == 0 or b >> (m - 1) else b - (1 << m) + 1

        for _ in range(min(restart or left, left)):
            for comp in layout:
                t = 1 if comp else 0
                q = np.zeros(64, dtype=np.int64)
                pred[comp] += extend(symbol(huff[t]))
                q[0] = pred[comp]
                j = 1
                while j < 64:
                    rs = symbol(huff[0x10 | t])
                    if rs == 0:
                        break
                    if rs == 0xf0:
                        j += 16
                        continue
                    j += rs >> 4
                    q[j] = extend(rs & 15)
                    j += 1
                out.append((comp, q))
        left -= min(restart or left, left)
        rest = n - at
        assert rest < 8 and take(rest) == (1 << rest) - 1                  # padded with 1-bits to the byte
    assert left == 0
    return out


def psnr(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


# ---- the cases of the GPU tests (tests/test_jpeg_host.py runs the reference and Pillow on every one of them) -----------------------------------
def noise(shape, seed, nan=True):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)
    if nan:
        a.reshape(-1)[rng.choice(a.size, size=max(1, a.size // 50), replace=False)] = np.nan
    return a


def flat(shape, rgb=(0.25, 0.5, 0.75)):
    return np.broadcast_to(np.array(rgb, dtype=np.float32).reshape(1, 3, 1, 1), shape).copy()


def checker(shape, cell):
    """Full swing: squares of `cell` pixels, 0 and 1, the three planes alike."""
    b, _, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((yy // cell) + (xx // cell)) % 2).astype(np.float32), shape).copy()


def smooth(shape):
    """A smooth scene: low-frequency gradients and a soft disc, different in the three planes."""
    b, _, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w] / np.array([h, w], dtype=np.float64).reshape(2, 1, 1)
    r = 0.5 + 0.45 * np.sin(2.1 * np.pi * xx + 0.3) * np.cos(1.3 * np.pi * yy)
    g = 0.15 + 0.7 * yy * (1 - 0.5 * xx)
    bl = 0.5 + 0.4 * np.exp(-((xx - 0.6) ** 2 + (yy - 0.4) ** 2) / 0.05) - 0.2 * xx
    return np.broadcast_to(np.stack([r, g, bl]).astype(np.float32), shape).copy()


# name: (subsampling, quality, restart, dtype, (B, H, W), crop (h, w) or None, content)
CASES = {
    "420_one_mcu": ("420", 90, 8, "float32", (1, 16, 16), None, lambda s: noise(s, 1)),
    "420_padded": ("420", 10, 8, "bfloat16", (1, 17, 23), None, lambda s: noise(s, 2)),
    "420_rows_wrap": ("420", 100, 3, "float16", (1, 40, 136), None, lambda s: noise(s, 3)),
    "444_one_mcu": ("444", 90, 8, "float32", (1, 8, 8), None, lambda s: noise(s, 4)),
    "444_short_last": ("444", 10, 4, "bfloat16", (1, 24, 80), None, lambda s: noise(s, 5)),
    "444_padded": ("444", 100, 8, "float16", (1, 9, 13), None, lambda s: noise(s, 6)),
    "420_flat": ("420", 90, 1, "float32", (1, 48, 64), None, lambda s: flat(s)),
    "444_flat_wrap": ("444", 50, 1, "bfloat16", (1, 24, 40), None, lambda s: flat(s, (1.0, 0.0, 0.5))),
    "444_checker": ("444", 100, 2, "float32", (1, 32, 48), None, lambda s: checker(s, 8)),
    "420_checker": ("420", 100, 2, "float32", (1, 32, 48), None, lambda s: checker(s, 3)),
    "444_checker_fine": ("444", 100, 8, "float32", (1, 16, 24), None, lambda s: checker(s, 1)),
    "420_crop": ("420", 90, 2, "bfloat16", (1, 50, 72), (37, 52), lambda s: noise(s, 7)),
    "444_crop": ("444", 90, 5, "float32", (1, 30, 44), (21, 33), lambda s: noise(s, 8, nan=False)),
    "444_many_intervals": ("444", 50, 1, "bfloat16", (1, 136, 136), None, lambda s: smooth(s)),       # 289 intervals: the scan walks two chunks
    "420_batch": ("420", 90, 4, "float16", (2, 32, 48), None, lambda s: np.concatenate([noise((1,) + s[1:], 9), smooth((1,) + s[1:])])),
}


def case_source(name):
    """(subsampling, quality, restart, dtype name, source (B,3,H,W) float32 before the dtype's rounding, (h, w))."""
    sub, quality, restart, dtype, (b, hh, ww), crop, make = CASES[name]
    return sub, quality, restart, dtype, make((b, 3, hh, ww)), crop or (hh, ww)
