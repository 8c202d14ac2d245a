"""CPU: the C-ABI library loads, exports every declared symbol, and its host-side packing matches the
fragment layout the kernel documents (checked by emulating the MFMA dataflow in NumPy)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F32, RC_OUT_NHWC, RC_OUT_PIXEL_SHUFFLE2


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/realcam_hip.h but not exported"
    assert set(declared) == set(_lib._SIGS), "ctypes binding table out of sync with the header"
    assert lib.rc_abi_version() == _lib.ABI_VERSION
    assert b"gfx950" in lib.rc_build_info()


def test_conv_desc_layout_matches_header():
    lib = _lib.load()
    assert lib.rc_conv_desc_size() == C.sizeof(_lib.ConvDesc)


def test_bad_arguments_are_reported_not_fixed():
    lib = _lib.load()
    assert lib.rc_conv_packed_bytes(16, 16, 7, RC_F32, RC_OUT_NHWC) == 0          # 7x7 unsupported (5x5: the folded tail only, cout <= 16)
    assert lib.rc_conv_packed_bytes(16, 32, 5, RC_F32, RC_OUT_NHWC) == 0
    assert b"bad shape" in lib.rc_last_error()
    assert lib.rc_conv2d(None, None) < 0
    assert lib.rc_bayer_unshuffle(None, RC_F32, None, RC_F32, 1, 4, 4, 4, 4, None) < 0
    assert b"null" in lib.rc_last_error()
    assert lib.rc_dwt_forward(1, 1, 1, 1, RC_F32, 1, 5, 4, 8, None) < 0              # odd height
    assert lib.rc_conv_sum_tiles(1088, 1920) == 4 * 136 * 60


def _plan(cin, cout, dtype):
    unit = 4 if dtype == RC_F32 else 8
    if dtype == RC_BF16:
        ck = 8 if cin <= 8 else 64 if cin % 64 == 0 else 48 if cin % 48 == 0 else 32 if cin == 32 else 16      # 3x3 (the emulated case)
    else:
        ck = 4 if cin <= 4 else 16
    nt = (3 if (cout % 48 == 0 and dtype == RC_BF16 and cin == 48) else 2 if (dtype == RC_BF16 and cin == 32 and cout == 32) else
          4 if cout % 64 == 0 else 3 if cout % 48 == 0 else 1)
    return unit, ck, nt


def _unit_map(upt, taps, s, q):
    """Python mirror of unit_map() in realcamnet_amd/csrc/conv_kernel.hpp: (live, tap, channel-unit)."""
    if upt == 6:
        if s < taps:
            return True, s, q
        tap = 2 * (s - taps) + (q >> 1)
        return tap < taps, tap, 4 + (q & 1)
    u = 4 * s + q
    return u < taps * upt, u // upt, u % upt


def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def _emulate(w, x, dtype, out_mode, ks=3):
    """Re-run the kernel's dataflow on the host-packed weights: returns conv output (cout', H, W) for one
    8x32 tile, following realcamnet_amd/csrc/conv_kernel.hpp's documented lane mapping."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    unit, ck, nt = _plan(cin, cout, dtype)
    if out_mode == RC_OUT_PIXEL_SHUFFLE2:
        cps = cout // 4
        nt = 3 if (cps % 48 == 0 and (cps % 64 != 0 or (dtype == RC_BF16 and cin == 48))) else 4 if cps % 64 == 0 else 1
    upt = ck // unit
    taps = ks * ks
    steps = taps + (taps + 1) // 2 if upt == 6 else (taps * upt + 3) // 4
    n_chunks = -(-cin // ck)
    n_ct = -(-cout // (16 * nt))
    nbytes = lib.rc_conv_packed_bytes(cin, cout, ks, dtype, out_mode)
    assert nbytes == n_ct * n_chunks * steps * nt * 1024
    buf = np.empty(nbytes, np.uint8)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.rc_conv_pack_weights(wc.ctypes.data, cin, cout, ks, dtype, out_mode, buf.ctypes.data) == 0
    pk = buf.view(np.float32) if dtype == RC_F32 else _bf16_to_f32(buf.view(np.uint16))
    pk = pk.reshape(n_ct, n_chunks, steps, nt, 64, unit)
    halo = ks // 2
    H, W = 8, 32
    xp = np.zeros((n_chunks * ck, H + 2 * halo, W + 2 * halo), np.float32)
    xp[:cin, halo:halo + H, halo:halo + W] = x
    nv = 4 * nt
    out = np.zeros((n_ct * 16 * nt, H, W), np.float64)   # indexed by PACKED cout
    lanes = np.arange(64)
    m_of, q_of, n_of = lanes & 15, lanes >> 4, lanes & 15
    for ct in range(n_ct):
        for wave in range(4):
            for pt in range(4):
                row, col0 = 2 * wave + (pt >> 1), (pt & 1) * 16
                for t in range(nt):
                    D = np.zeros((16, 16))      # D[m][n]
                    for chunk in range(n_chunks):
                        for s in range(steps):
                            A = np.zeros((16, 4, unit)); B = np.zeros((4, unit, 16))
                            for lane in range(64):
                                A[m_of[lane], q_of[lane]] = pk[ct, chunk, s, t, lane]
                                live, tap, cu = _unit_map(upt, taps, s, q_of[lane])
                                if live:
                                    dy, dx = divmod(tap, ks)
                                    c0 = chunk * ck + cu * unit
                                    B[q_of[lane], :, n_of[lane]] = xp[c0:c0 + unit, row + dy, col0 + n_of[lane] + dx]
                            D += np.einsum("mqe,qen->mn", A, B)
                    for lane in range(64):       # C/D layout: col = lane&15, row = 4*(lane>>4) + r
                        for r in range(4):
                            j = ct * 16 * nt + q_of[lane] * nv + t * 4 + r
                            out[j, row, col0 + n_of[lane]] = D[4 * q_of[lane] + r, n_of[lane]]
    return out, nt


@pytest.mark.parametrize("cin,cout,dtype", [(4, 48, RC_BF16), (48, 48, RC_BF16), (16, 32, RC_F32), (64, 64, RC_BF16), (32, 32, RC_BF16), (32, 64, RC_BF16),
                                            (4, 16, RC_F32), (48, 3, RC_BF16), (80, 16, RC_F32)])
def test_packed_weight_layout_reproduces_conv(cin, cout, dtype):
    rng = np.random.default_rng(0)
    w = rng.integers(-4, 5, size=(cout, cin, 3, 3)).astype(np.float32) / 4      # exactly representable in bf16
    x = rng.integers(-4, 5, size=(cin, 8, 32)).astype(np.float32) / 4
    out, nt = _emulate(w, x, dtype, RC_OUT_NHWC)
    ref = F.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), padding=1)[0].numpy()
    np.testing.assert_allclose(out[:cout], ref, atol=1e-4)
    assert np.all(out[cout:] == 0)


def test_pixel_shuffle_packing_permutation():
    lib = _lib.load()
    cin, cout = 16, 64
    rng = np.random.default_rng(1)
    w = rng.integers(-4, 5, size=(cout, cin, 3, 3)).astype(np.float32) / 4
    x = rng.integers(-4, 5, size=(cin, 8, 32)).astype(np.float32) / 4
    out, nt = _emulate(w, x, RC_F32, RC_OUT_PIXEL_SHUFFLE2)
    assert nt == 1                    # cout/4 = 16 out channels -> 16-wide tiles, one per sub-pixel
    tile = 16 * nt
    ref = F.pixel_shuffle(F.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), padding=1), 2)[0].numpy()
    got = np.zeros_like(ref)
    for j in range(cout):            # kernel epilogue: packed j -> (cout tile ct = cb*4 + sub-pixel, out channel)
        ct, within = divmod(j, tile)
        cb, sub = ct >> 2, ct & 3
        got[cb * tile + within, (sub >> 1)::2, (sub & 1)::2] = out[j]
    np.testing.assert_allclose(got, ref, atol=1e-4)
    bias = np.arange(cout, dtype=np.float32)
    dst = np.zeros(lib.rc_conv_packed_cout(cin, cout, 3, RC_F32, RC_OUT_PIXEL_SHUFFLE2), np.float32)
    assert lib.rc_conv_pack_bias(bias.ctypes.data, cin, cout, 3, RC_F32, RC_OUT_PIXEL_SHUFFLE2, dst.ctypes.data) == 0
    for j in range(cout):
        ct, within = divmod(j, tile)
        assert dst[j] == 4 * ((ct >> 2) * tile + within) + (ct & 3)


# ---- 32x32x16 form (realcamnet_amd/csrc/conv32_kernel.hpp) ---------------------------------------------------------------------
def _emulate32(w, x, out_mode, ck32=32):
    """Host-packed weights of the 32x32x16 conv replayed through v_mfma_f32_32x32x16_bf16's documented lane maps (A: lane = (row m = l & 31,
    k group l >> 5), B: lane = (column n = l & 31, k group l >> 5), D: lane (n, h) register i <- row (i & 3) + 8 (i >> 2) + 4 h) for one
    8 x 32 pixel tile.  Returns {(packed channel j): (8, 32) map} in PACKED order plus the plan (ck, nt32, n_ct)."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    ck = 48 if cin == 48 else ck32
    nt = 3 if cin == 48 else 2
    spt, steps = ck // 16, 9 * (ck // 16)
    n_chunks, n_ct = cin // ck, cout // (32 * nt)
    nbytes = lib.rc_conv_packed_bytes(cin, cout, 3, RC_BF16, out_mode)
    assert nbytes == n_ct * n_chunks * steps * nt * 1024
    assert lib.rc_conv_packed_cout(cin, cout, 3, RC_BF16, out_mode) == cout
    buf = np.empty(nbytes, np.uint8)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.rc_conv_pack_weights(wc.ctypes.data, cin, cout, 3, RC_BF16, out_mode, buf.ctypes.data) == 0
    pk = _bf16_to_f32(buf.view(np.uint16)).reshape(n_ct, n_chunks, steps, nt, 64, 8)
    H, W = 8, 32
    xp = np.zeros((cin, H + 2, W + 2), np.float32)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.zeros((cout, H, W), np.float64)          # indexed by PACKED channel
    m_of, kg_of = np.arange(64) & 31, np.arange(64) >> 5
    for ct in range(n_ct):
        for row in range(H):
            for t in range(nt):
                D = np.zeros((32, 32))
                for chunk in range(n_chunks):
                    for s in range(steps):
                        tap, j = divmod(s, spt)
                        dy, dx = divmod(tap, 3)
                        A = np.zeros((32, 2, 8)); B = np.zeros((2, 8, 32))
                        for lane in range(64):
                            A[m_of[lane], kg_of[lane]] = pk[ct, chunk, s, t, lane]
                            c0 = chunk * ck + (2 * j + kg_of[lane]) * 8
                            B[kg_of[lane], :, m_of[lane]] = xp[c0:c0 + 8, row + dy, m_of[lane] + dx]
                        D += np.einsum("mke,ken->mn", A, B)
                for lane in range(64):
                    n, h = lane & 31, lane >> 5
                    for i in range(16):
                        out[ct * 32 * nt + 32 * t + 16 * h + i, row, n] = D[(i & 3) + 8 * (i >> 2) + 4 * h, n]
    return out, nt, n_ct


@pytest.mark.parametrize("cin,cout,knob", [(128, 64, 2), (128, 64, 1), (48, 96, 4)])
def test_packed_weight_layout_32x32_reproduces_conv(cin, cout, knob):
    """knob = rc_debug_set("conv32"): 2 -> 32-channel chunks (two-barrier form), 1 -> 16-channel chunks (staged-output form), 0 = the default (none), 4 = the one-chunk 48 -> 96k NHWC layers only."""
    rng = np.random.default_rng(2)
    w = rng.integers(-2, 3, size=(cout, cin, 3, 3)).astype(np.float32) / 2
    x = rng.integers(-2, 3, size=(cin, 8, 32)).astype(np.float32) / 2
    lib = _lib.load()
    assert lib.rc_debug_set(b"conv32", knob) == 0
    try:
        out, nt, n_ct = _emulate32(w, x, RC_OUT_NHWC, ck32=16 if knob == 1 else 32)
    finally:
        lib.rc_debug_set(b"conv32", 0)
    ref = F.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), padding=1)[0].numpy()
    np.testing.assert_allclose(out, ref, atol=1e-4)             # NHWC: packed order == channel order


def test_pixel_shuffle_packing_32x32():
    lib = _lib.load()
    cin, cout = 48, 192                                          # the flagship tail: 48 -> 4 x 48, PixelShuffle(2)
    rng = np.random.default_rng(3)
    w = rng.integers(-2, 3, size=(cout, cin, 3, 3)).astype(np.float32) / 2
    x = rng.integers(-2, 3, size=(cin, 8, 32)).astype(np.float32) / 2
    assert lib.rc_debug_set(b"conv32", 1) == 0      # the PixelShuffle tail stays on the 16x16x32 kernel by default (measured a tie)
    try:
        out, nt, n_ct = _emulate32(w, x, RC_OUT_PIXEL_SHUFFLE2)
        bias = np.arange(cout, dtype=np.float32)
        dst = np.zeros(cout, np.float32)
        assert lib.rc_conv_pack_bias(bias.ctypes.data, cin, cout, 3, RC_BF16, RC_OUT_PIXEL_SHUFFLE2, dst.ctypes.data) == 0
    finally:
        lib.rc_debug_set(b"conv32", 0)
    assert (nt, n_ct) == (3, 2)
    ref = F.pixel_shuffle(F.conv2d(torch.from_numpy(x)[None], torch.from_numpy(w), padding=1), 2)[0].numpy()
    got = np.zeros_like(ref)
    cps = cout // 4
    for j in range(cout):   # kernel epilogue: cout tile ct = (out-channel block ct>>1, sub-row ct&1); row tile t; lane half h = sub-column
        ct, within = divmod(j, 32 * nt)
        t, c = divmod(within, 32)
        h, e = divmod(c, 16)
        oc = (ct >> 1) * 16 * nt + 16 * t + e
        assert oc < cps
        got[oc, (ct & 1)::2, h::2] = out[j]
    np.testing.assert_allclose(got, ref, atol=1e-4)
    for j in range(cout):
        ct, within = divmod(j, 32 * nt)
        t, c = divmod(within, 32)
        h, e = divmod(c, 16)
        assert dst[j] == 4 * ((ct >> 1) * 16 * nt + 16 * t + e) + 2 * (ct & 1) + h


def test_conv32_knob_switches_the_packed_layout():
    """rc_debug_set("conv32", 2) routes the multi-chunk layers to the 32x32x16 kernel: the packed size is the same, the order is not."""
    lib = _lib.load()
    w = np.random.default_rng(4).standard_normal((64, 128, 3, 3)).astype(np.float32)
    n = lib.rc_conv_packed_bytes(128, 64, 3, RC_BF16, RC_OUT_NHWC)
    a, b = np.empty(n, np.uint8), np.empty(n, np.uint8)
    assert lib.rc_conv_pack_weights(w.ctypes.data, 128, 64, 3, RC_BF16, RC_OUT_NHWC, a.ctypes.data) == 0     # default: 16x16x32 order
    assert lib.rc_debug_set(b"conv32", 2) == 0
    try:
        assert lib.rc_conv_packed_bytes(128, 64, 3, RC_BF16, RC_OUT_NHWC) == n
        assert lib.rc_conv_pack_weights(w.ctypes.data, 128, 64, 3, RC_BF16, RC_OUT_NHWC, b.ctypes.data) == 0
    finally:
        lib.rc_debug_set(b"conv32", 0)
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.sort(b))


def test_bench_path_kernels_do_not_spill_and_the_count_cannot_grow():
    """hipcc's per-kernel resource remarks of the built library (realcamnet_amd/_build/resources.json, written by build()): a kernel whose accumulators or
    staging registers land in scratch passes every parity test and silently runs 20-50 % slower (round 1: the fp32 fast-epilogue switch; round 3: the first
    GDN chain), and the count of such instantiations drifted 62 -> 71 -> 82 over rounds 2-4.  Round 5: the gated forms of kernels 2 / 4 and two unused
    instantiations are gone (81 -> 25); every kernel the cfg3 / cfg5 bench paths launch must be spill-free, and the total may only go down."""
    from realcamnet_amd import build
    res = build.kernel_resources()
    assert len(res) > 500
    spilled = {k: v for k, v in res.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0)}
    bench_path = [
        "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEELb0ELb1E",    # 48 -> 48 (kernel 2), fast epilogues
        "conv_mfma_auto_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEE",               # 48 -> 48 (kernel 6), all three modes
        "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi32ELi4ELi3ELi8EEELb0ELb1E",        # the multi-chunk layers
        "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi32ELi3ELi3ELi8EEELb0ELb1E",        # 192 -> 48
        "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEELb0ELb1E",        # 48 -> 192 (+ PixelShuffle: the tail ring)
        "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi5ELi8EEELb0ELb1E",    # the folded 5x5 tail (generic epilogue: planar pixel-shuffled store)
        "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi5ELi8EEELb0ELb0E",
        "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi3ELi8EEELb0ELb0E",    # 48 -> 3 on the ring strips
        "conv_mfma_kernelINS_7ConvCfgIDF16bLi64ELi5ELi1ELi8EEELb0E",                 # GroupMix in-projection 192 -> 80
        "wino_f32_kernelILi4ELi",                                                   # fp32 Winograd F(2x2,3x3): cfg2's 64 -> 64 / 128 -> 128 layers
        "conv_mfma_wst_kernel",                                                       # kernel 4b, every instantiation (the codec's folded stride-2 layers, 16-wide cout tiles, 16-channel chunks)
        "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi32ELi4ELi2ELi8EEELb0ELb1E",        # ... and kernel 4 on the same folded layers (`thin` 0)
        "2gf", "ca_gate", "ca_reduce", "color_", "instance_stats", "gfm_vector", "dwt_", "raw_ingest", "tail_ring", "nchw_to_nhwc", "nhwc_to_nchw",
        "wmsa", "3ans", "entropy_bottleneck", "gaussian_conditional", "channel_concat", "pointwise_chain",
    ]
    hits = {p: [k for k in res if p in k] for p in bench_path}
    assert all(hits[p] for p in bench_path), [p for p in bench_path if not hits[p]]            # the patterns still name real kernels
    bad = sorted(k for p in bench_path for k in hits[p] if k in spilled)
    assert not bad, [(k, spilled[k]) for k in bad]
    assert len(spilled) <= 25, sorted((v["tu"], v["vgpr_spill"], k[:90]) for k, v in spilled.items())


def test_cout_tile_override_packs_the_same_bytes_in_another_order():
    """rc_conv_desc.cout_tile (ABI 11) / the *_ct packers: a caller-chosen cout tile width changes the packed ORDER ([ct][chunk][step][nt]), not the content -- same
    byte count and the same multiset of values when the automatic width divides cout; widths the layout cannot express and the pixel-shuffle stores are rejected."""
    lib = _lib.load()
    cin, cout = 128, 128
    w = np.random.default_rng(5).standard_normal((cout, cin, 3, 3)).astype(np.float32)
    n0 = lib.rc_conv_packed_bytes(cin, cout, 3, RC_F32, RC_OUT_NHWC)
    assert n0 == lib.rc_conv_packed_bytes_ct(cin, cout, 3, RC_F32, RC_OUT_NHWC, 0) == lib.rc_conv_packed_bytes_ct(cin, cout, 3, RC_F32, RC_OUT_NHWC, 16) > 0
    a, b = np.empty(n0, np.uint8), np.empty(n0, np.uint8)
    assert lib.rc_conv_pack_weights(w.ctypes.data, cin, cout, 3, RC_F32, RC_OUT_NHWC, a.ctypes.data) == 0
    assert lib.rc_conv_pack_weights_ct(w.ctypes.data, cin, cout, 3, RC_F32, RC_OUT_NHWC, 16, b.ctypes.data) == 0
    fa, fb = a.view(np.float32), b.view(np.float32)
    assert not np.array_equal(fa, fb) and np.array_equal(np.sort(fa), np.sort(fb))
    assert lib.rc_conv_packed_cout_ct(cin, cout, 3, RC_F32, RC_OUT_NHWC, 16) == cout
    bias = np.arange(cout, dtype=np.float32)
    pb = np.empty(cout, np.float32)
    assert lib.rc_conv_pack_bias_ct(bias.ctypes.data, cin, cout, 3, RC_F32, RC_OUT_NHWC, 16, pb.ctypes.data) == 0 and np.array_equal(pb, bias)
    for bad_tile, mode in ((24, RC_OUT_NHWC), (96, RC_OUT_NHWC), (16, RC_OUT_PIXEL_SHUFFLE2)):
        assert lib.rc_conv_packed_bytes_ct(cin, cout, 3, RC_F32, mode, bad_tile) == 0


def test_debug_knobs_have_their_documented_defaults():
    """The A/B switches the header documents (include/realcam_hip.h, rc_debug_set) read back their defaults, round-trip, and reject unknown keys: a default that
    drifted would silently change which kernel the parity tests and the bench exercise."""
    lib = _lib.load()
    for key, default in ((b"persist", 1), (b"conv32", 0), (b"pss", 0), (b"persist_auto", 1), (b"sums_compact", 1), (b"thin", 2), (b"lds_poison", 0), (b"conv_flags", 0),
                         (b"pw_grid_cap", 1 << 22)):
        assert lib.rc_debug_get(key) == default, key
    for key, v in ((b"thin", 0), (b"lds_poison", 1), (b"persist_auto", 2), (b"pw_grid_cap", 3)):
        old = lib.rc_debug_get(key)
        try:
            assert lib.rc_debug_set(key, v) == 0 and lib.rc_debug_get(key) == v
        finally:
            lib.rc_debug_set(key, old)
    assert lib.rc_debug_set(b"pw_grid_cap", 0) == 0 and lib.rc_debug_get(b"pw_grid_cap") == 1 << 22       # 0 restores the default
    assert lib.rc_debug_get(b"no_such_knob") == -1 and lib.rc_debug_set(b"no_such_knob", 1) != 0


def test_sum_slot_query_follows_the_dispatch():
    """rc_conv_sum_slots asks the launcher itself which kernel a launch will take (nothing is launched: works without a GPU): the carried-sums kernels report
    grid x waves slots per image, everything else -- and every kernel when the per-tile layout is smaller -- rc_conv_sum_tiles()."""
    lib = _lib.load()

    def q(cin, cout, H, W, B=8, act=1, dtype=RC_BF16, residual=False):
        d = _lib.ConvDesc()
        d.batch, d.height, d.width, d.cin, d.cout, d.ksize, d.dtype = B, H, W, cin, cout, 3, dtype
        d.in0 = d.wpacked = d.out = d.chan_sums = 4096
        if residual:
            d.residual = 4096
        d.act, d.out_dtype = act, dtype
        return lib.rc_conv_sum_slots(C.byref(d))
    legacy = lib.rc_conv_sum_tiles(1088, 1920)
    try:
        assert q(48, 48, 1088, 1920) == 2048 and q(64, 64, 1088, 1920) == 2048 and legacy == 32640      # kernels 6 / 7 at 256 CUs: 256 x 8
        assert q(48, 48, 16, 40, B=2) == lib.rc_conv_sum_tiles(16, 40)                                  # small image: the per-tile layout is the smaller one
        assert q(128, 128, 272, 480) == lib.rc_conv_sum_tiles(272, 480)                                  # multi-chunk kernel: per tile
        assert q(32, 32, 64, 64, dtype=RC_F32) == lib.rc_conv_sum_tiles(64, 64)                          # fp32: per tile
        assert lib.rc_debug_set(b"persist_auto", 0) == 0
        assert q(48, 48, 1088, 1920) == 2048 and q(64, 64, 1088, 1920) == legacy                        # kernel 2: 512 blocks x 4 waves; 64 channels: general kernel
        assert lib.rc_debug_set(b"persist", 0) == 0
        assert q(48, 48, 1088, 1920) == legacy                                                           # general kernel only
        assert lib.rc_debug_set(b"persist", 1) == 0 and lib.rc_debug_set(b"sums_compact", 0) == 0
        assert q(48, 48, 1088, 1920) == legacy
    finally:
        lib.rc_debug_set(b"persist", 1); lib.rc_debug_set(b"persist_auto", 1); lib.rc_debug_set(b"sums_compact", 1)
    d = _lib.ConvDesc()
    assert lib.rc_conv_sum_slots(C.byref(d)) == -1 and lib.rc_conv_sum_slots(None) == -1


def test_no_new_mfma_accumulator_revisit_after_one_mfma(tmp_path):
    """on gfx950 an MFMA whose SrcC is the result of the MFMA issued TWO slots earlier (two accumulators alternating) read stale partial sums in the first build of
    rc_gma_in_cpe -- 40 of 40 launches differed from the first; each accumulator's K-steps back to back: 0 of 80 (tools/ubench/gi_experiment.hip).  Neither the hardware interlock nor
    hipcc's hazard recogniser covers it, and the instruction scheduler is free to produce that order again, so the ISA of the fused GroupMix / chain kernels is scanned here
    (tools/mfma_hazard_scan.py): rc_gma_in_cpe's kernel must have NO revisit with one MFMA and fewer than four other instructions in between, and the set of kernels that have one is
    frozen at the two that are stress-tested bitwise stable (gma_tail<192>, gma_qkv_agg: tools/dbg/block_stress.py, 300 forwards at the cfg3 size)."""
    import os, shutil, subprocess, sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from mfma_hazard_scan import scan
    from realcamnet_amd import build
    out = tmp_path / "gma_fused.s"
    flags = [f for f in build.FLAGS if not f.startswith("-Rpass")]
    r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "realcamnet_amd", "csrc", "gma_fused.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    close = {k: [p for p in v if p[0] == 1 and p[1] < 4] for k, v in scan(str(out), 1).items()}
    close = {k: v for k, v in close.items() if v}
    assert not any("gma_in_cpe" in k for k in close), close
    known = ("gma_tail_kernelILi192", "gma_qkv_agg_kernel")
    assert all(any(n in k for n in known) for k in close), sorted(close)
    assert sum(len(v) for v in close.values()) <= 3, {k: len(v) for k, v in close.items()}
