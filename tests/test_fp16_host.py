"""CPU: the fp16 (RC_F16) form of the ISP path at the ABI level -- exported constants, the host weight packer's fp32 -> fp16
rounding and fragment layout, packed sizes, and the compiled kernels' resources and MFMA accumulator schedule."""
import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32, RC_OUT_NCHW, RC_OUT_NHWC, RC_OUT_PIXEL_SHUFFLE2, RC_OUT_PIXEL_SHUFFLE2_NCHW
from conftest import NET_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realcamnet_amd", "csrc")


def test_abi_15_exports_rc_f16():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15
    assert (RC_F32, RC_BF16, _lib.RC_U16, RC_F16) == (0, 1, 2, 3)
    with open(os.path.join(ROOT, "include", "realcam_hip.h")) as f:
        assert "RC_F16 = 3" in f.read()


def _bf16_tags(n):
    """n distinct finite, normal bf16 values (as fp32): a tag per weight position that survives bf16 packing bit for bit."""
    pos = np.arange(0x0080, 0x7f80, dtype=np.uint32)                         # positive normal bf16 patterns
    pats = np.concatenate([pos, pos | 0x8000])
    assert n <= pats.size
    return (pats[:n] << 16).view(np.float32), pats[:n].astype(np.uint16)


def _pack(w, cin, cout, k, dtype, mode):
    lib = _lib.load()
    n = lib.rc_conv_packed_bytes(cin, cout, k, dtype, mode)
    assert n > 0, lib.rc_last_error()
    dst = np.zeros(n, np.uint8)
    w = np.ascontiguousarray(w, np.float32)
    assert lib.rc_conv_pack_weights(w.ctypes.data, cin, cout, k, dtype, mode, dst.ctypes.data) == 0, lib.rc_last_error()
    return dst.view(np.uint16)


def _special_weights(shape, seed):
    """Random fp32 weights (most of them round in fp16) with fp16 subnormals, ties, the overflow boundary and NaN-free extremes mixed in."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(shape) * 0.3).astype(np.float32).reshape(-1)
    specials = np.array([6e-8, -6e-8, 2.9802322e-08, 5.9604645e-08, 1e-6, -3.1e-5, 6.1e-5, 6.103515625e-05, 65504.0, 65519.0, 65520.0, -7e4, 1e6,
                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0, 0.0, -0.0, 1e-30], np.float32)
    idx = rng.choice(w.size, size=min(w.size, 6 * specials.size), replace=False)
    w[idx] = np.resize(specials, idx.size)
    w[idx[::3]] *= rng.uniform(0.5, 3.0, size=idx[::3].size).astype(np.float32)     # scaled specials: more subnormals / overflows / roundings
    return w.reshape(shape)


@pytest.mark.parametrize("cout,cin,k,mode", [(48, 48, 3, RC_OUT_NHWC), (48, 4, 3, RC_OUT_NHWC), (32, 32, 3, RC_OUT_NHWC), (64, 64, 1, RC_OUT_NHWC),
                                             (48, 2, 1, RC_OUT_NHWC), (64, 16, 3, RC_OUT_PIXEL_SHUFFLE2), (3, 48, 3, RC_OUT_NCHW),
                                             (12, 48, 5, RC_OUT_PIXEL_SHUFFLE2_NCHW), (12, 32, 5, RC_OUT_PIXEL_SHUFFLE2_NCHW), (48, 96, 3, RC_OUT_NHWC)])
def test_f16_packing_is_torch_half_in_the_bf16_layout(cout, cin, k, mode):
    """The fp16 packing of fp32 weights holds, at every position, torch's w.half() of the weight the bf16 packing places there (located by packing
    distinct bf16 tags): same layout, and the host converter rounds to nearest even, keeps subnormals and overflows to inf exactly like torch."""
    shape = (cout, cin, k, k)
    n = int(np.prod(shape))
    tags, tag_bits = _bf16_tags(n)
    placed = _pack(tags.reshape(shape), cin, cout, k, RC_BF16, mode)
    where = {int(b): i for i, b in enumerate(tag_bits)}
    src = np.array([where.get(int(b), -1) for b in placed])                   # weight index per packed position, -1 = padding (0)
    assert np.all((src >= 0) | (placed == 0))
    assert np.unique(src[src >= 0]).size == n                                 # every weight is placed exactly once
    w = _special_weights(shape, seed=cout * 100 + cin + k)
    got = _pack(w, cin, cout, k, RC_F16, mode)
    want_all = torch.from_numpy(w.reshape(-1)).half().view(torch.int16).numpy().view(np.uint16)
    want = np.where(src >= 0, want_all[np.maximum(src, 0)], 0).astype(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), w.reshape(-1)[src[i]] if src[i] >= 0 else 0.0, hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert np.isinf(want_all.view(np.float16)).any() and (np.abs(want_all.view(np.float16)) < 6.1e-5).any()   # the specials are in play


def _layer_shapes():
    """(cout, cin, k) of every convolution / Linear in the 13 ISP networks, and the folded-tail 5x5 shapes."""
    import realcamnet_amd as M
    shapes = set()
    for name in NET_NAMES:
        net = getattr(M, name)()
        for mod in net.modules():
            w = getattr(mod, "weight", None)
            if not isinstance(w, torch.Tensor) or w.dim() not in (2, 4):
                continue
            if w.dim() == 2:
                shapes.add((w.shape[0], w.shape[1], 1))
            elif w.shape[2] == w.shape[3] and w.shape[2] in (1, 3):
                shapes.add((w.shape[0], w.shape[1], w.shape[2]))
        tail = getattr(net, "tail", None)
        if tail is not None and hasattr(tail[0], "weight") and hasattr(tail[-1], "weight"):
            shapes.add((4 * tail[-1].weight.shape[0], tail[0].weight.shape[1], 5))
    return sorted(shapes)


def test_f16_packed_sizes_equal_bf16_for_every_isp_layer():
    lib = _lib.load()
    shapes = _layer_shapes()
    assert len(shapes) > 20
    checked = 0
    for cout, cin, k in shapes:
        modes = [RC_OUT_PIXEL_SHUFFLE2_NCHW] if k == 5 else [RC_OUT_NHWC, RC_OUT_NCHW] + ([RC_OUT_PIXEL_SHUFFLE2] if cout % 4 == 0 else [])
        for mode in modes:
            b = lib.rc_conv_packed_bytes(cin, cout, k, RC_BF16, mode)
            f = lib.rc_conv_packed_bytes(cin, cout, k, RC_F16, mode)
            assert f == b, (cout, cin, k, mode, f, b)
            assert lib.rc_conv_packed_cout(cin, cout, k, RC_F16, mode) == lib.rc_conv_packed_cout(cin, cout, k, RC_BF16, mode)
            checked += b > 0
    assert checked > 20


def test_off_path_entry_points_refuse_f16():
    lib = _lib.load()
    assert lib.rc_conv_packed_bytes(64, 64, 2, RC_F16, RC_OUT_NHWC) == 0                     # the codec's 2x2 stride-2 window: bf16 only
    assert lib.rc_wino_packed_bytes(64, 64, RC_F16) == 0                                      # Winograd: fp32 only
    assert lib.rc_layernorm(1, 1, RC_F16, 8, 64, 1, 1, 1e-5, None) < 0                         # GroupMix / codec LayerNorm
    assert b"bad dtype" in lib.rc_last_error()


# the conv patterns of tests/test_abi_host.py's bench-path list that the ISP networks launch (bf16 names; the fp16 twin has DF16_ for DF16b)
ISP_BENCH_PATTERNS = [
    "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEELb0ELb1E",
    "conv_mfma_auto_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEE",
    "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi32ELi4ELi3ELi8EEELb0ELb1E",
    "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi32ELi3ELi3ELi8EEELb0ELb1E",
    "conv_mfma_wsm_kernelINS_7ConvCfgIDF16bLi48ELi3ELi3ELi8EEELb0ELb1E",
    "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi5ELi8EEELb0ELb1E",
    "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi5ELi8EEELb0ELb0E",
    "conv_mfma_persist_kernelINS_7ConvCfgIDF16bLi48ELi1ELi3ELi8EEELb0ELb0E",
]


def test_f16_twins_of_the_isp_bench_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    res = build.kernel_resources()
    spilled = lambda v: v.get("scratch", 0) or v.get("vgpr_spill", 0)
    for p in ISP_BENCH_PATTERNS:
        twins = [k for k in res if p.replace("DF16b", "DF16_") in k]
        assert twins, p
        assert not [k for k in twins if spilled(res[k])], [(k, res[k]) for k in twins if spilled(res[k])]
    # every fp16 instantiation that spills is the twin of a bf16 one that spills the same way (no new spill form)
    for k, v in res.items():
        if "DF16_" in k and spilled(v):
            twin = res.get(k.replace("DF16_", "DF16b"))
            assert twin is not None and spilled(twin) and twin.get("vgpr_spill", 0) >= v.get("vgpr_spill", 0), (k, v, twin)


def _listing(tu, out_dir):
    from realcamnet_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(out_dir, tu.replace(".hip", ".s"))
    flags = [f for f in build.FLAGS if not f.startswith("-Rpass")]
    r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_f16_conv_units_add_no_mfma_accumulator_revisit(tmp_path):
    """tools/mfma_hazard_scan.py on every fp16 conv translation unit and its bf16 twin: an fp16 kernel may have a one-MFMA accumulator revisit
    (the pattern that read stale partial sums on gfx950) only where its bf16 twin has the same number of them."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from mfma_hazard_scan import scan
    f16 = sorted(f for f in os.listdir(CSRC) if f.startswith("conv_inst_f16_"))
    assert len(f16) >= 8
    tus = f16 + [f.replace("_f16_", "_bf16_") for f in f16]
    with cf.ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        listings = dict(zip(tus, ex.map(lambda t: _listing(t, str(tmp_path)), tus)))

    def close(tu):
        return {k: len([p for p in v if p[0] == 1 and p[1] < 4]) for k, v in scan(listings[tu], 1).items()}
    for tu in f16:
        mine, twin = close(tu), close(tu.replace("_f16_", "_bf16_"))
        extra = {k: n for k, n in mine.items() if n > twin.get(k.replace("DF16_", "DF16b"), 0)}
        assert not extra, (tu, extra)
