"""CPU yardsticks for the three kernels that hold several layers in one launch: rc_lsc_chain (csrc/gma_fused.hip, lsc_chain_kernel<C, HEAD>), rc_pointwise_chain48
(csrc/chain.hip) and rc_conv_pair (csrc/conv_pair.hip, `pair` and `pair2`).  Plain torch; round_to / within_rounding / gamma / TINY and the stage helpers are those of
streaming_ref.py, groupmix_ref.py and conv_ref.py.

ref64_* / slack64_* / model64_* come out of ONE pipeline per entry point whose stages return (value, bound) (groupmix_ref.py): every fp32 accumulation of k terms
adds gamma_k * sum |terms|, every bf16 rounding point adds 2^-9 |v| (model64: rounds v to bf16 instead), both carried through the later layers by |W|.  The weights
are rounded to bf16 in all three, as rc_lsc_pack / rc_chain_pack_weights / rc_conv_pack_weights round them (host_f32_to_bf16, round-to-nearest-even); biases,
FiLM vectors and gates stay fp32.  The same pipeline on fp32 tensors is the CPU restatement test_fused_host.py holds against model64.

Rounding points, read from the sources:

  chains (both)   layer 0 and every layer but the last: the bias is the MFMA chain's initial C operand (k = cin + 1), LeakyReLU as med3(v, v * slope, big) = max(v, fl(v * slope))
                  for 0 <= slope <= 1 -- one fp32 rounding, on the negative side only --, then ONE rounding to bf16 (pack_pair / pack_tail / pack_bf16x2): the next
                  layer's B fragments.  The last layer's accumulator has no activation.
  rc_lsc_chain    HEAD: the last layer's value is rounded to bf16 (qa_pack: the lens-shading map where the two-launch path stores it), widened again, and
                  out = fma(h, l, h) with h = conv3x3(raw) + bias in fp32 (bias first, k = 9 raw_c + 1): one rounding for the product and the sum, then the store's.
  rc_conv_pair    in_gate: in0 * gate + in1 as an fp32 product and an fp32 sum (two roundings, -ffp-contract=off) and one cast to bf16: that value feeds conv1 AND is
                  what in_store receives (conv_ref.gated_input restates it bit for bit, so it is an input of the pipeline below, not a stage with a bound).
                  mid = act1(conv1(x) + b1): FiLM v * fs + ft + v (three roundings) and the LeakyReLU above, or ReLU, rounded to bf16 in LDS, and ZERO outside the
                  image (conv2 pads its own input; here: the second convolution's zero padding).  out = conv2(mid) + b2 (+ residual, one more fp32 sum), stored bf16.
                  chan_sums: both kernels add the fp32 value v they are about to store -- BEFORE its rounding to bf16 -- over the valid pixels of one output row of a
                  tile (2 x 16 lanes: 32 terms, `valid ? v : 0`), one slot per (tile, row).  The slots of an image added in float64 are compared with the float64
                  sum of ref64 inside sum(slack64) + gamma_32 * sum |ref64|.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_ref
from groupmix_ref import BF16, F32, F64, UB, e_linear, e_round, flip_share, randn, rb, real_map  # noqa: F401  (re-exported to the tests)
from streaming_ref import TINY, U32, gamma, int_view, round_to, same_bits, within_rounding  # noqa: F401

LSC_WIDTHS = (32, 48, 64, 128)
PAIR_MODES = ("plain", "sums", "gated", "gated_sums", "gated_nostore", "film", "film_res")      # every conv_pair_kernel<GATED, E1, E2> the entry point dispatches to
PAIR_C, PAIR_TH, PAIR_TW = 48, 8, 32                                                              # pair::C, OTH, OTW
PAIR_K = 9 * PAIR_C + 1                                                                           # terms of one 3x3 x 48 dot product + the bias


# ---- stages ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _w(w, dtype):
    """A weight as the packers store it: rounded to bf16."""
    return rb(w.float()).to(dtype)


def _b(b, dtype):
    return None if b is None else b.to(dtype)


def _zero(x, model):
    return None if model else torch.zeros_like(x)


def _slope(slope):
    return float(torch.tensor(slope, dtype=F32))


def e_leaky(v, e, slope):
    """max(v, fl(v * slope)), 0 <= slope <= 1: Lipschitz constant 1, one fp32 rounding on the negative side."""
    s = _slope(slope)
    y = torch.where(v > 0, v, v * s)
    if e is None:
        return y, None
    return y, e + U32 * s * (v.abs() + e) + TINY


def _conv3(x, w, b=None):
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)


def e_conv3(x, e, w, b, k, res=None):
    """3x3 convolution of NHWC x with zero padding (+ b) (+ res): k roundings on the longest path of a term."""
    y = _conv3(x, w, b)
    if res is not None:
        y = y + res
    if e is None:
        return y, None
    mag = _conv3(x.abs() + e, w.abs(), None if b is None else b.abs())
    if res is not None:
        mag = mag + res.abs()
    return y, _conv3(e, w.abs()) + gamma(k) * mag + TINY


def _point(v, e, model, trace):
    """One bf16 rounding point."""
    if trace is not None:
        trace.append(("point", v))
    return e_round(v, e, model)


def _acc(trace, mag):
    if trace is not None:
        trace.append(("acc", mag))


# ---- the chains ------------------------------------------------------------------------------------------------------------------------------------------------------
def _chain_pipe(model, dtype, x, w0, b0, wmid, bmid, slope, whead=None, bhead=None, raw=None, trace=None):
    c = w0.shape[0]
    cin0 = w0.numel() // c
    v = x.to(dtype)
    e = _zero(v, model)
    W = _w(w0.reshape(c, cin0), dtype)
    _acc(trace, F.linear(v.abs(), W.abs(), None if b0 is None else b0.to(dtype).abs()))
    v, e = e_linear(v, e, W, _b(b0, dtype), cin0 + 1)                       # layer 0: bias = the initial C operand, cin0 products
    v, e = _point(*e_leaky(v, e, slope), model, trace)                      # bf16 after the LeakyReLU
    for l, (w, b) in enumerate(zip(wmid, bmid)):
        W = _w(w.reshape(c, c), dtype)
        _acc(trace, F.linear(v.abs(), W.abs(), None if b is None else b.to(dtype).abs()))
        v, e = e_linear(v, e, W, _b(b, dtype), c + 1)
        if l + 1 < len(wmid):
            v, e = _point(*e_leaky(v, e, slope), model, trace)              # bf16 after every LeakyReLU between layers; none after the last layer
    if whead is None:
        return v, e
    lm, el = _point(v, e, model, trace)                                     # the lens-shading map, rounded to bf16 in front of the head
    r = raw.to(dtype)
    Wh = _w(whead, dtype)
    _acc(trace, _conv3(r.abs(), Wh.abs(), None if bhead is None else bhead.to(dtype).abs()))
    h, eh = e_conv3(r, _zero(r, model), Wh, _b(bhead, dtype), 9 * raw.shape[-1] + 1)
    y = h * lm + h                                                          # the device: one fma; a CPU fp32 run: product and sum -- gamma_2 bounds both
    _acc(trace, h.abs() * (lm.abs() + 1))
    if e is None:
        return y, None
    return y, eh * (lm.abs() + el + 1) + h.abs() * el + gamma(2) * (h.abs() + eh) * (lm.abs() + el + 1) + TINY


def _run(model, dtype, d, trace=None):
    with torch.no_grad():
        return _chain_pipe(model, dtype, d["x"], d["w0"], d["b0"], d["wmid"], d["bmid"], d["slope"], d.get("whead"), d.get("bhead"), d.get("raw"), trace)


def ref64_lsc_chain(x, w0, b0, wmid, bmid, slope, whead=None, bhead=None, raw=None):
    """rc_lsc_chain in float64 from the bf16 inputs and the bf16-rounded weights, no intermediate rounding: (B, H, W, C)."""
    return _chain_pipe(False, F64, x, w0, b0, wmid, bmid, slope, whead, bhead, raw)[0]


def slack64_lsc_chain(x, w0, b0, wmid, bmid, slope, whead=None, bhead=None, raw=None):
    return _chain_pipe(False, F64, x, w0, b0, wmid, bmid, slope, whead, bhead, raw)[1]


def model64_lsc_chain(x, w0, b0, wmid, bmid, slope, whead=None, bhead=None, raw=None, dtype=F64):
    return _chain_pipe(True, dtype, x, w0, b0, wmid, bmid, slope, whead, bhead, raw)[0]


def ref64_chain48(x, w0, b0, wmid, bmid, slope):
    """rc_pointwise_chain48: the same chain at width 48 without a head (cin0 <= 8; layer 0 is one zero-padded MFMA step with the bias as its C operand)."""
    return ref64_lsc_chain(x, w0, b0, wmid, bmid, slope)


def slack64_chain48(x, w0, b0, wmid, bmid, slope):
    return slack64_lsc_chain(x, w0, b0, wmid, bmid, slope)


def model64_chain48(x, w0, b0, wmid, bmid, slope, dtype=F64):
    return model64_lsc_chain(x, w0, b0, wmid, bmid, slope, dtype=dtype)


def chain_yardsticks(d):
    """(ref64, slack64, model64) of a chain data set (exact_chain / real_chain)."""
    ref, slack = _run(False, F64, d)
    return ref, slack, _run(True, F64, d)[0]


def chain_restated32(d):
    """The pipeline with fp32 tensors in torch's own summation order, rounding points included; the stored value is round_to(., bf16) of it."""
    return _run(True, F32, d)[0]


def _sparse(g, cout, cin, nnz=2, p_more=0.5):
    """Small-integer rows with at most `nnz` non-zeros in {-1, 1, 2}.  Row r's first entry sits in column (5 r + 3) mod cin -- seeded from the channel index: a column
    of its own while cout <= cin (5 divides none of the widths) --, the further ones (there in a share p_more of the rows) in drawn columns.  So the pattern differs
    from row to row, per 16-channel tile and per lane group, and a swapped tile, tap or channel changes the result."""
    w = torch.zeros(cout, cin)
    rows = torch.arange(cout)
    more = torch.randint(0, cin, (cout, nnz - 1), generator=g)
    vals = torch.tensor([1.0, -1.0, 1.0, -1.0, 2.0])[torch.randint(0, 5, (cout, nnz), generator=g)]
    vals[:, 1:] *= (torch.rand(cout, nnz - 1, generator=g) < p_more).float()
    for j in range(nnz - 1):
        w[rows, more[:, j]] = vals[:, j + 1]
    w[rows, (5 * rows + 3) % cin] = vals[:, 0]
    return w


def exact_chain(c, cin0, n_mid, shape, slope, raw_c=0, seed=0, bias=True):
    """Data whose every intermediate is exactly representable (exact_headroom_chain proves it per set): integer coordinates and RAW values in -2 .. 2, sparse
    integer weights (_sparse), biases in -1 .. 2, a dyadic slope (0, 0.5, 1).  raw_c > 0: with a head.  bias False: NULL biases."""
    assert slope in (0.0, 0.5, 1.0)
    g = torch.Generator().manual_seed(7000 + 131 * seed + c + 17 * cin0 + 3 * n_mid + 5 * raw_c)
    B, H, W = shape
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    # a slope of one half adds a fractional bit per LeakyReLU: the deeper chains then get fewer second entries and coordinates in -1 .. 1, which keeps them inside 8 bits
    deep = slope == 0.5 and n_mid >= 3
    p, top = (0.125, 1) if deep else (0.5, 2)
    d = dict(c=c, slope=slope, x=ints(-top, top, B, H, W, cin0).to(BF16), w0=_sparse(g, c, cin0, 2, p), b0=ints(-1, top, c) if bias else None,
             wmid=[_sparse(g, c, c, 2, p) for _ in range(n_mid)], bmid=[ints(-1, top, c) if bias else None for _ in range(n_mid)])
    if raw_c:
        d.update(raw=ints(-2, 2, B, H, W, raw_c).to(BF16), whead=_sparse(g, c, 9 * raw_c, 3).reshape(c, raw_c, 3, 3), bhead=ints(-2, 3, c) if bias else None)
    return d


def exact_headroom_chain(d):
    """(values at a bf16 rounding point that are not bf16 numbers, the largest sum of absolute terms of any accumulation in units of the data's finest bit).  Zero and
    below 2^24: every stored or packed value is exact in bf16 and every partial sum exact in fp32 in any order, the head's fma included."""
    trace = []
    _run(True, F64, d, trace)
    n_leaky = len(d["wmid"])                                                       # LeakyReLUs: after layer 0 and after every mid layer but the last
    frac = n_leaky if d["slope"] == 0.5 else 0
    inexact = sum(int((v != rb(v)).sum()) for kind, v in trace if kind == "point")
    return inexact, max(float(v.max()) for kind, v in trace if kind == "acc") * 2.0 ** frac


def _init(shape, seed, fan_in):
    """nn.Conv2d's default initialisation, weights and biases alike: uniform in +-1 / sqrt(fan_in)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)


def real_chain(c, cin0, n_mid, shape, slope, raw_c=0, seed=0, bias=True):
    """Weights at the initialisation scale (_init), the initialised biases perturbed by 0.1 randn, randn coordinates and RAW values with one outlier pixel x 25."""
    s = 9000 + 131 * seed + c + 17 * cin0 + 3 * n_mid + 5 * raw_c
    B, H, W = shape
    b_ = lambda k, fan: (_init((c,), k, fan) + randn((c,), k + 50, 0.1)) if bias else None
    d = dict(c=c, slope=slope, x=real_map((B, H, W, cin0), s), w0=_init((c, cin0), s + 1, cin0), b0=b_(s + 2, cin0),
             wmid=[_init((c, c), s + 10 + l, c) for l in range(n_mid)], bmid=[b_(s + 20 + l, c) for l in range(n_mid)])
    if raw_c:
        d.update(raw=real_map((B, H, W, raw_c), s + 3), whead=_init((c, raw_c, 3, 3), s + 4, 9 * raw_c), bhead=b_(s + 5, 9 * raw_c))
    return d


# ---- rc_lsc_pack's blob ----------------------------------------------------------------------------------------------------------------------------------------------
def row_channel(m, R, mt):
    """MFMA row R of output tile m -> channel (gma_fused.hip: pair-packed rows; an unpaired last tile keeps natural order)."""
    return 32 * (m >> 1) + 8 * (R >> 2) + 4 * (m & 1) + (R & 3) if m < (mt & ~1) else 16 * m + R


def tile_bytes(cin):
    return (cin // 32) * 1024 + (512 if cin % 32 else 0)


def lsc_packed_bytes(c, n_mid, head):
    """The documented sum: layer 0's half-filled K-step (512 bytes a tile), n_mid rc_chain_pack_weights matrices, the head's 1.5 K-steps, the fp32 bias rows."""
    mt = c // 16
    return mt * 512 + n_mid * mt * tile_bytes(c) + (mt * 1536 if head else 0) + (1 + n_mid + (1 if head else 0)) * mt * 16 * 4


def _bf16_of(u16):
    return torch.from_numpy((u16.astype(np.uint32) << 16).view(np.float32).copy())


def unpack_lsc_blob(blob, c, cin0, n_mid, raw_c=0):
    """rc_lsc_pack's output (uint8 numpy array) taken apart by the layout its comments document -> dict(w0 (c, cin0), wmid [n_mid x (c, c)], whead (c, raw_c, 3, 3) or
    None, biases [(c,) fp32 ...] in blob order, padding_zero: were all the unused fragment slots zero).
      layer 0     tile m at m * 512, lane (R = lane & 15, q = lane >> 4): 4 bf16 values, k = 4 q + i, zero where k >= cin0
      mid layers  rc_chain_pack_weights: tile m at m * tile_bytes(c), K-step s: 8 values a lane, k = 32 s + 8 q + i; a trailing 16 channels: 4 values, k = 32 KS + 4 q + i
      head        tile m at m * 1536: 8 values a lane, k = 8 q + i -> tap 2 q + i / 4, channel i % 4; then at + 1024 4 values a lane: tap 8 in lane group 0
      biases      fp32 [tile][row], one block of c values per layer (+ the head's)"""
    mt, tb, ks = c // 16, tile_bytes(c), c // 32
    blob = np.ascontiguousarray(blob)
    assert blob.dtype == np.uint8 and blob.size == lsc_packed_bytes(c, n_mid, raw_c > 0), (blob.size, lsc_packed_bytes(c, n_mid, raw_c > 0))
    u16 = blob.view(np.uint16)
    seen = np.zeros(u16.size, dtype=bool)
    ch = np.array([[row_channel(m, lane & 15, mt) for lane in range(64)] for m in range(mt)])          # (mt, 64)
    q = np.arange(64) >> 4

    def gather(dst, base, per_lane, col_of):
        """dst[ch, col] = value i of every lane's `per_lane` values at u16 offset base(m) + lane * per_lane + i, where col_of(q, i) gives the column (or -1: padding)."""
        for m in range(mt):
            for i in range(per_lane):
                idx = base(m) + np.arange(64) * per_lane + i
                col = col_of(q, i)
                live = col >= 0
                dst[ch[m][live], col[live]] = u16[idx[live]]
                seen[idx[live]] = True

    pos = 0
    w0 = np.zeros((c, cin0), dtype=np.uint16)
    gather(w0, lambda m: pos + m * 256, 4, lambda q, i: np.where(4 * q + i < cin0, 4 * q + i, -1))
    pos += mt * 256
    wmid = []
    for _ in range(n_mid):
        w = np.zeros((c, c), dtype=np.uint16)
        for s in range(ks):
            gather(w, lambda m, s=s, pos=pos: pos + m * tb // 2 + s * 512, 8, lambda q, i, s=s: 32 * s + 8 * q + i)
        if c % 32:
            gather(w, lambda m, pos=pos: pos + m * tb // 2 + ks * 512, 4, lambda q, i: 32 * ks + 4 * q + i)
        wmid.append(_bf16_of(w))
        pos += mt * tb // 2
    whead = None
    if raw_c:
        wh = np.zeros((c, 9 * 4), dtype=np.uint16)                                                   # [ch][tap][4 channel slots]
        gather(wh, lambda m: pos + m * 768, 8, lambda q, i: np.where((i & 3) < raw_c, 4 * (2 * q + (i >> 2)) + (i & 3), -1))
        gather(wh, lambda m: pos + m * 768 + 512, 4, lambda q, i: np.where((q == 0) & (i < raw_c), 32 + i, -1))
        whead = _bf16_of(wh).reshape(c, 9, 4)[:, :, :raw_c].permute(0, 2, 1).reshape(c, raw_c, 3, 3).contiguous()
        pos += mt * 768
    padding_zero = bool((u16[:pos][~seen[:pos]] == 0).all())
    f32 = blob[2 * pos:].view(np.float32)
    order = ch[:, :16].reshape(-1)                                                                  # row m * 16 + R -> channel
    biases = []
    for l in range(1 + n_mid + (1 if raw_c else 0)):
        b = np.zeros(c, dtype=np.float32)
        b[order] = f32[l * c:(l + 1) * c]
        biases.append(torch.from_numpy(b))
    return dict(w0=_bf16_of(w0), wmid=wmid, whead=whead, biases=biases, padding_zero=padding_zero)


# ---- rc_conv_pair ----------------------------------------------------------------------------------------------------------------------------------------------------
def pair_flags(mode):
    """-> dict(gated, store, sums, film, res) of a PAIR_MODES name."""
    assert mode in PAIR_MODES, mode
    return dict(gated=mode.startswith("gated"), store=mode in ("gated", "gated_sums"), sums=mode in ("sums", "gated_sums", "gated_nostore"),
                film=mode.startswith("film"), res=mode == "film_res")


def _pair_pipe(model, dtype, d, trace=None):
    f = pair_flags(d["mode"])
    xin = conv_ref.gated_input(d, "bf16")                                   # in0, or in0 * gate + in1 rounded where in_store stores it
    v = xin.to(dtype)
    per_image = lambda t: t.to(dtype)[:, None, None, :]                     # noqa: E731
    W1, W2 = _w(d["w1"], dtype), _w(d["w2"], dtype)
    _acc(trace, _conv3(v.abs(), W1.abs(), None if d["b1"] is None else d["b1"].to(dtype).abs()))
    v, e = e_conv3(v, _zero(v, model), W1, _b(d["b1"], dtype), PAIR_K)
    if f["film"]:
        fs, ft = per_image(d["fs"]), per_image(d["ft"])
        _acc(trace, v.abs() * (fs.abs() + 1) + ft.abs())
        y = v * fs + ft + v                                                 # three fp32 roundings
        e = None if e is None else e * (fs.abs() + 1) + gamma(3) * ((v.abs() + e) * (fs.abs() + 1) + ft.abs()) + TINY
        v, e = e_leaky(y, e, d["slope"])
    else:
        v = v.clamp_min(0)                                                  # ReLU (on the rounded bits in the kernel: the same value)
    mid, e = _point(v, e, model, trace)                                     # mid: bf16 in LDS; zero outside the image = the second convolution's own padding
    res = d["res"].to(dtype) if f["res"] else None
    _acc(trace, _conv3(mid.abs(), W2.abs(), None if d["b2"] is None else d["b2"].to(dtype).abs()) + (0 if res is None else res.abs()))
    out, e = e_conv3(mid, e, W2, _b(d["b2"], dtype), PAIR_K + (1 if f["res"] else 0), res)
    return out, e, xin


def pair_yardsticks(d):
    """-> dict(ref, slack, model: (B, H, W, 48) float64; stored: the bf16 tensor in_store must hold, or None; sums, sums_slack: (B, 48) float64 or None)."""
    with torch.no_grad():
        ref, slack, xin = _pair_pipe(False, F64, d)
        model = _pair_pipe(True, F64, d)[0]
    f = pair_flags(d["mode"])
    out = dict(ref=ref, slack=slack, model=model, stored=xin if f["store"] else None, sums=None, sums_slack=None)
    if f["sums"]:
        out["sums"] = ref.sum(dim=(1, 2))                                   # of the fp32 values in front of the store's rounding
        out["sums_slack"] = slack.sum(dim=(1, 2)) + gamma(32) * ref.abs().sum(dim=(1, 2))
    return out


def ref64_conv_pair(d):
    return pair_yardsticks(d)["ref"]


def slack64_conv_pair(d):
    return pair_yardsticks(d)["slack"]


def model64_conv_pair(d, dtype=F64):
    with torch.no_grad():
        return _pair_pipe(True, dtype, d)[0]


def exact_pair(mode, shape, seed=0):
    """conv_ref.exact_data-style operands: x (and the skip tensor) in halves |x| <= 2, gates / FiLM scales in {0, 1, 2}, integer weights -- conv1's sparse (one in
    eight entries, +-1) so that mid stays inside bf16's 8 bits, conv2's dense in -2 .. 2 --, integer biases; b1 in -6 .. 10, so relu(b1) != 0 on most channels and a
    kernel that computed conv1 on the padding ring instead of zeroing mid there differs at every border pixel.  Slope 0.5."""
    f = pair_flags(mode)
    g = torch.Generator().manual_seed(5000 + 17 * seed + PAIR_MODES.index(mode))
    B, H, W = shape
    C = PAIR_C
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    d = dict(mode=mode, slope=0.5, x=(ints(-4, 4, B, H, W, C) / 2).to(BF16))
    d["w1"] = ints(-1, 1, C, C, 3, 3) * (torch.rand(C, C, 3, 3, generator=g) < (0.09375 if f["film"] else 0.1875)).float()      # FiLM triples conv1's value
    d["w2"] = ints(-2, 2, C, C, 3, 3)
    d["b1"], d["b2"] = ints(-6, 10, C), ints(-8, 8, C)
    if f["gated"]:
        d["gate"] = conv_ref._choice(g, (B, C), [0.0, 1.0, 2.0], [1, 3, 3])
        d["skip"] = (ints(-4, 4, B, H, W, C) / 2).to(BF16)
    if f["film"]:
        d["fs"], d["ft"] = conv_ref._choice(g, (B, C), [0.0, 1.0, 2.0]), ints(-8, 8, B, C)
    if f["res"]:
        d["res"] = (ints(-16, 16, B, H, W, C) / 2).to(BF16)
    return d


def exact_headroom_pair(d):
    """(mid values that are not bf16 numbers, the largest sum of absolute terms in units of the finest bit -- halves, times the slope's half --, the same for a
    channel-sum slot: 32 pixels of the largest output)."""
    trace = []
    with torch.no_grad():
        out = _pair_pipe(True, F64, d, trace)[0]
    unit = 4.0 if pair_flags(d["mode"])["film"] else 2.0
    inexact = sum(int((v != rb(v)).sum()) for kind, v in trace if kind == "point")
    return inexact, max(float(v.max()) for kind, v in trace if kind == "acc") * unit, 32 * float(out.abs().max()) * unit


def real_pair(mode, shape, seed=0):
    """Weights at the initialisation scale (_init, fan_in 432), the initialised biases perturbed by 0.1 randn, randn maps with one outlier pixel x 25, gates in
    [0, 1), FiLM vectors 0.5 randn, slope 0.01 (Res_GFM's)."""
    f = pair_flags(mode)
    s = 6000 + 17 * seed + PAIR_MODES.index(mode)
    B, H, W = shape
    C = PAIR_C
    d = dict(mode=mode, slope=0.01, x=real_map((B, H, W, C), s), w1=_init((C, C, 3, 3), s + 1, 9 * C), w2=_init((C, C, 3, 3), s + 2, 9 * C),
             b1=_init((C,), s + 3, 9 * C) + randn((C,), s + 53, 0.1), b2=_init((C,), s + 4, 9 * C) + randn((C,), s + 54, 0.1))
    if f["gated"]:
        d["gate"] = torch.rand((B, C), generator=torch.Generator().manual_seed(s + 5))
        d["skip"] = real_map((B, H, W, C), s + 6)
    if f["film"]:
        d["fs"], d["ft"] = randn((B, C), s + 7, 0.5), randn((B, C), s + 8, 0.5)
    if f["res"]:
        d["res"] = real_map((B, H, W, C), s + 9)
    return d


def sharp_pair(mode, shape, seed=0):
    """The sharpness set: real_pair with conv2's weights, its bias and the residual made non-negative (|.|).  With signed weights an output can be a small difference
    of large terms, and ONE flipped mid value (2^-8 of its own term) then moves it by several of its own bf16 steps -- 8 of 106 080 outputs did on an MI355X, in both
    implementations alike.  A sum of non-negative terms (mid >= 0 behind the ReLU; behind the LeakyReLU its negative side is 0.01 of the value) moves by at most
    2^-8 of itself, so "only to an adjacent value" holds by construction (codec_ref.wmsa_sharp_inputs makes the same choice).  The signed set keeps the window."""
    d = real_pair(mode, shape, seed)
    d["w2"], d["b2"] = d["w2"].abs(), d["b2"].abs()
    if "res" in d:
        d["res"] = d["res"].abs()
    return d


def pair_sum_slots(H, W):
    """rc_conv_pair_sum_slots: one slot per output row of every 8 x 32 tile."""
    return 8 * (-(-H // PAIR_TH)) * (-(-W // PAIR_TW))
