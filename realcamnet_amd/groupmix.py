"""HIP-backed mirror of the GroupMix attention block (upstream models/groupmix.py:21-299; the identical copy in
models/raw2bit.py:98-142 is what RealCamNet imports).  Same class names, constructor signatures and attribute
names, so reference state_dicts load unchanged; forward(x (B,N,C), size=(H,W)) keeps the reference signature.

Only the classes on the path are built (Mlp, Agg_0, Aggregator, ConvRelPosEnc, EfficientAtt, ConvPosEnc,
SeparableConv2d, GMA_Block); the ImageNet classifier around them (ConvStem, PatchEmbedLayer, GMA_Stage,
GroupMixFormer) is out of scope.  Inference only: BatchNorm uses running statistics,
Dropout / DropPath are identities.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class Mlp(nn.Module):
    """fc1 -> GELU -> fc2 (upstream groupmix.py:21-38); both Linears run as MFMA 1x1 convs."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if act_layer is not nn.GELU:
            raise NotImplementedError("Mlp: only nn.GELU is on the hot path")
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def _nhwc(self, a, residual=None):
        h = ops.conv2d(a, self.fc1, act="gelu")
        return ops.conv2d(h, self.fc2, residual=residual)

    def forward(self, x):
        return self._nhwc(_as_nhwc(x, None)).reshape(x.shape[0], -1, self.fc2.out_features)


class SeparableConv2d(nn.Module):
    """Depth-wise kxk + point-wise 1x1, both without bias (upstream groupmix.py:240-249).  Parameter holder:
    executed fused inside Aggregator."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False):
        super().__init__()
        if stride != 1 or dilation != 1 or bias or padding != kernel_size // 2:
            raise NotImplementedError("SeparableConv2d: stride 1, 'same' padding, no bias only")
        self.conv1 = nn.Conv2d(in_channels, in_channels, kernel_size, stride, padding, dilation, groups=in_channels, bias=bias)
        self.pointwise_conv = nn.Conv2d(in_channels, out_channels, 1, 1, 0, 1, 1, bias=bias)


class Agg_0(nn.Module):
    """Local branch: sep-conv(3seg -> seg) -> LayerNorm(seg) -> Hardswish (upstream groupmix.py:41-53)."""

    def __init__(self, seg_dim):
        super().__init__()
        self.conv = SeparableConv2d(seg_dim * 3, seg_dim, 3, 1, 1)
        self.norm = nn.LayerNorm(seg_dim)
        self.act = nn.Hardswish()


class Aggregator(nn.Module):
    """Multi-scale depth-wise aggregators over 5 channel groups (upstream groupmix.py:56-105)."""

    def __init__(self, dim, seg=4):
        super().__init__()
        self.dim = dim
        self.seg = seg
        seg_dim = self.dim // self.seg
        self.norm0 = nn.SyncBatchNorm(seg_dim)
        self.act0 = nn.Hardswish()
        self.agg1 = SeparableConv2d(seg_dim, seg_dim, 3, 1, 1)
        self.norm1 = nn.SyncBatchNorm(seg_dim)
        self.act1 = nn.Hardswish()
        self.agg2 = SeparableConv2d(seg_dim, seg_dim, 5, 1, 2)
        self.norm2 = nn.SyncBatchNorm(seg_dim)
        self.act2 = nn.Hardswish()
        self.agg3 = SeparableConv2d(seg_dim, seg_dim, 7, 1, 3)
        self.norm3 = nn.SyncBatchNorm(seg_dim)
        self.act3 = nn.Hardswish()
        self.agg0 = Agg_0(seg_dim)

    def _run(self, qkv):
        """qkv NHWC (B,H,W,3C) -> qkvp (B,H,W,3,4seg) [q|k|v, channel = head*Ch + i], loc (B,H,W,seg)."""
        if self.seg != 5:
            raise NotImplementedError("Aggregator: seg=5 only (as EfficientAtt builds it)")
        if qkv.dim() == 5:                                 # segment-planar (15, B, H, W, 16) from realcam::gma_ln_qkv
            return self._run_fused(qkv)[:2]
        b, H, W, c3 = qkv.shape
        c, seg = c3 // 3, c3 // 15
        dev, dt = qkv.device, qkv.dtype
        # all four depth-wise stages (groups 1..3: k = 3, 5, 7 shared by q/k/v; group 4: the local branch's own 3x3 per
        # q/k/v) in ONE launch: taps zero-padded to 7x7, the true window per weight vector in kvec (padded taps are
        # skipped, never multiplied), output (B,H,W,3,4seg) = [rep][g1 | g2 | g3 | g4] -- qkv is read once, not 4 times
        def taps(w1, w2, w3, w0):
            cols = []
            for r in range(3):
                cols += [ops.dw_taps(w1, 7), ops.dw_taps(w2, 7), ops.dw_taps(w3, 7), ops.dw_taps(w0[r * seg:(r + 1) * seg], 7)]
            unit = 8 if dt == torch.bfloat16 else 4
            kv = torch.tensor(([3] * (seg // unit) + [5] * (seg // unit) + [7] * (seg // unit) + [3] * (seg // unit)) * 3, dtype=torch.int32)
            return torch.cat(cols, dim=1).contiguous(), kv
        wT, kvec = ops.host_cached(self, f"taps7_{dt}", [self.agg1.conv1.weight, self.agg2.conv1.weight, self.agg3.conv1.weight,
                                                       self.agg0.conv.conv1.weight], taps)
        dwc = ops.dwconv2d(qkv, seg, (3, 4 * seg), 0, 4 * seg, 7, wT, n_rep=3, x_rep=c, y_rep=4 * seg, w_rep=4 * seg, kvec=kvec)

        scale, shift, pw, pwl = self._folded()
        ln = self.agg0.norm
        qkvp, loc = torch.ops.realcam.gma_pointwise(qkv, dwc, pw, scale, shift, pwl, ops.f32_param(ln, "weight"), ops.f32_param(ln, "bias"))
        return qkvp, loc


    def _folded(self):
        """BatchNorm(eval) -> per-channel scale / shift (4,16); point-wise weights as dense matrices (3,16,16), (16,48)."""
        def fold(*p):
            bn = [p[4 * i:4 * i + 4] for i in range(4)]
            scale = torch.stack([w / torch.sqrt(v + 1e-5) for (w, _, _, v) in bn])
            shift = torch.stack([bb - m * (w / torch.sqrt(v + 1e-5)) for (w, bb, m, v) in bn])
            pw = torch.stack([q[:, :, 0, 0] for q in p[16:19]])
            return scale, shift, pw, p[19][:, :, 0, 0]

        norms = (self.norm0, self.norm1, self.norm2, self.norm3)
        params = [t for n in norms for t in (n.weight, n.bias, n.running_mean, n.running_var)]
        params += [self.agg1.pointwise_conv.weight, self.agg2.pointwise_conv.weight, self.agg3.pointwise_conv.weight,
                   self.agg0.conv.pointwise_conv.weight]
        for n in norms:
            if abs(n.eps - 1e-5) > 0:
                raise NotImplementedError("Aggregator: BatchNorm eps must be the default 1e-5")
        return ops.host_cached(self, "fold", params, fold)

    def _run_fused(self, qkv):
        """dim 80, bf16: depth-wise, point-wise, BatchNorm, Hardswish and the local branch in ONE launch (rc_gma_aggregate);
        qkv in the segment-planar layout (15, B, H, W, 16) that realcam::gma_ln_qkv writes.  -> (qkvp, loc, kmax): kmax (B, 64) is the
        per-channel maximum of the aggregated k, reduced by the same launch (the shift of softmax_N(k))."""
        seg = 16

        def taps(w1, w2, w3, w0):
            return (ops.dw_taps(w1), ops.dw_taps(w2), ops.dw_taps(w3),
                    ops.dw_taps(w0).reshape(9, 3, seg).permute(1, 0, 2).contiguous())      # local: (which, tap, channel)
        dw3, dw5, dw7, dwl = ops.host_cached(self, "taps_exact", [self.agg1.conv1.weight, self.agg2.conv1.weight, self.agg3.conv1.weight,
                                                                 self.agg0.conv.conv1.weight], taps)
        scale, shift, pw, pwl = self._folded()
        ln = self.agg0.norm
        if abs(ln.eps - 1e-5) > 0:
            raise NotImplementedError("Aggregator: LayerNorm eps must be the default 1e-5")
        return torch.ops.realcam.gma_aggregate(qkv, dw3, dw5, dw7, dwl, pw, pwl, scale, shift, ops.f32_param(ln, "weight"),
                                               ops.f32_param(ln, "bias"))

    def _run_front(self, x, norm1, qkv_linear):
        """x (B,H,W,80) bf16 -> (qkvp, loc, kmax) = _run_fused(qkv(LayerNorm1(x))) in ONE launch (rc_gma_qkv_aggregate): the 240-channel qkv map is
        produced 16 channels at a time into LDS and consumed there, the depth-wise windows as banded Toeplitz products on the matrix cores
        (upstream groupmix.py:178 after :293, then :56-105)."""
        seg = 16
        dws = [self.agg1.conv1.weight, self.agg2.conv1.weight, self.agg3.conv1.weight, self.agg0.conv.conv1.weight]

        def pack():
            with torch.no_grad():
                w1, w2, w3, w0 = [p.detach().float().cpu() for p in dws]
                return torch.ops.realcam.gma_toeplitz_pack(ops.dw_taps(w1).to(x.device), ops.dw_taps(w2).to(x.device), ops.dw_taps(w3).to(x.device),
                                                           ops.dw_taps(w0).reshape(9, 3, seg).permute(1, 0, 2).contiguous().to(x.device))
        toeplitz = ops.derived(self, "toeplitz", dws, pack)
        scale, shift, pw, pwl = self._folded()
        ln = self.agg0.norm
        if abs(ln.eps - 1e-5) > 0:
            raise NotImplementedError("Aggregator: LayerNorm eps must be the default 1e-5")
        f32 = ops.f32_param
        return torch.ops.realcam.gma_qkv_aggregate(x, ops.packed_chain_natural(qkv_linear), f32(qkv_linear, "bias") if qkv_linear.bias is not None else None,
                                                   f32(norm1, "weight"), f32(norm1, "bias"), float(norm1.eps), toeplitz, pw, pwl,
                                                   scale, shift, f32(ln, "weight"), f32(ln, "bias"))


class ConvRelPosEnc(nn.Module):
    """q * depth-wise conv(v) with per-head-group windows (upstream groupmix.py:108-156)."""

    def __init__(self, Ch, h, window):
        super().__init__()
        if isinstance(window, int):
            window = {window: h}
        elif not isinstance(window, dict):
            raise ValueError()
        self.window = window
        self.conv_list = nn.ModuleList()
        self.head_splits = []
        for cur_window, cur_head_split in window.items():
            padding_size = cur_window // 2
            self.conv_list.append(nn.Conv2d(cur_head_split * Ch, cur_head_split * Ch, kernel_size=(cur_window, cur_window),
                                            padding=(padding_size, padding_size), dilation=(1, 1), groups=cur_head_split * Ch))
            self.head_splits.append(cur_head_split)
        self.channel_splits = [x * Ch for x in self.head_splits]

    def _conv_v(self, qkvp):
        """depth-wise conv of v (channels 2ct..3ct of qkvp) with every window zero-padded to a centred 7x7."""
        planar = qkvp.dim() == 5 and qkvp.shape[0] == 12 and qkvp.shape[-1] == 16      # realcam::gma_aggregate's segment planes
        ct = 64 if planar else qkvp.shape[-1]
        kmax = max(self.window.keys())
        if kmax > 7 or any(k % 2 == 0 for k in self.window):
            raise NotImplementedError("ConvRelPosEnc: odd windows up to 7")
        params = [t for cv in self.conv_list for t in (cv.weight, cv.bias)]
        if planar:
            if list(self.window.items()) != [(3, 2), (5, 3), (7, 3)] or self.channel_splits != [16, 24, 24]:
                raise NotImplementedError("fused ConvRelPosEnc: windows {3: 2, 5: 3, 7: 3} over 8 heads of 8 channels")
            def seg_taps(*p):   # 16-channel segments: [conv3 (16)] [conv5 0..16] [conv5 16..24 padded to 7x7 | conv7 0..8] [conv7 8..24]
                w3, w5, w7 = p[0], p[2], p[4]
                t2 = torch.cat([ops.dw_taps(w5[16:24], pad_to=7), ops.dw_taps(w7[0:8])], dim=1)
                return (ops.dw_taps(w3), ops.dw_taps(w5[0:16]), t2.contiguous(), ops.dw_taps(w7[8:24]), torch.cat([p[1], p[3], p[5]]))
            t0, t1, t2, t3, bias = ops.host_cached(self, "seg_taps", params, seg_taps)
            return torch.ops.realcam.gma_crpe(qkvp, t0, t1, t2, t3, bias)

        unit = 8 if qkvp.dtype == torch.bfloat16 else 4
        wins = list(self.window.keys())

        def build(*p):
            taps = torch.cat([ops.dw_taps(p[2 * i], pad_to=7) for i in range(len(self.conv_list))], dim=1)
            kch = torch.cat([torch.full((p[2 * i].shape[0],), float(wins[i])) for i in range(len(self.conv_list))])
            kvec = kch.reshape(-1, unit).max(dim=1).values      # a vector spanning two head groups takes the larger window
            return taps, torch.cat([p[2 * i + 1] for i in range(len(self.conv_list))]), kvec.to(torch.int32)

        wT, bias, kvec = ops.host_cached(self, f"taps7_{unit}", params, build)
        return ops.dwconv2d(qkvp, 2 * ct, (ct,), 0, ct, 7, wT, bias=bias, kvec=kvec)


class EfficientAtt(nn.Module):
    """Linear attention with multi-scale aggregators (upstream groupmix.py:159-200)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.aggregator = Aggregator(dim=dim, seg=5)
        trans_dim = dim // 5 * 4
        self.crpe = ConvRelPosEnc(Ch=trans_dim // num_heads, h=num_heads, window={3: 2, 5: 3, 7: 3})

    def _geometry(self, c):
        heads = self.num_heads
        if c % 5 or (c // 5 * 4) % heads or sum(self.crpe.head_splits) != heads:
            raise ValueError(f"EfficientAtt: dim {c} / heads {heads} do not tile (upstream needs dim % 10 == 0, heads == 8)")
        return c // 5, c // 5 * 4, (c // 5 * 4) // heads                # seg, ct, ch

    def _context(self, qkv):
        """qkv (B,H,W,3C) -> (qkvp, loc, convv, ktv): aggregators, crpe's depth-wise conv of v, softmax_N(k)^T v."""
        seg, ct, ch = self._geometry(80 if qkv.dim() == 5 else qkv.shape[-1] // 3)
        if qkv.dim() == 5 and self.num_heads == 8 and ch == 8:          # fused path: max folded into the aggregator, k^T v on the matrix cores
            qkvp, loc, kmax = self.aggregator._run_fused(qkv)
            convv = self.crpe._conv_v(qkvp)
            return qkvp, loc, convv, torch.ops.realcam.gma_kv_mfma(qkvp, kmax, float(self.scale))
        qkvp, loc = self.aggregator._run(qkv)
        convv = self.crpe._conv_v(qkvp)
        ktv = torch.ops.realcam.gma_kv(qkvp, self.num_heads, ch, float(self.scale))
        return qkvp, loc, convv, ktv

    def _nhwc(self, a, residual=None):
        seg, ct, ch = self._geometry(a.shape[-1])
        qkv = ops.conv2d(a, self.qkv)                                   # (B,H,W,3C), channel = which*C + c
        qkvp, loc, convv, ktv = self._context(qkv)
        y = torch.ops.realcam.gma_apply(qkvp, convv, loc, ktv, self.num_heads, ch, seg)
        return ops.conv2d(y, self.proj, residual=residual)

    def forward(self, x, size):
        return self._nhwc(_as_nhwc(x, size)).reshape(x.shape)


class ConvPosEnc(nn.Module):
    """Depth-wise 3x3 conv + identity (upstream groupmix.py:203-217)."""

    def __init__(self, dim, k=3):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, k, 1, k // 2, groups=dim)

    def _nhwc(self, a):
        k = self.proj.kernel_size[0]
        (wT,) = ops.host_cached(self, "taps", [self.proj.weight], lambda w: ops.dw_taps(w))
        return ops.dwconv2d(a, 0, (a.shape[-1],), 0, a.shape[-1], k, wT, bias=ops.f32_param(self.proj, "bias"), add_identity=True)

    def forward(self, x, size):
        return self._nhwc(_as_nhwc(x, size)).reshape(x.shape)


SUPPORTED_DTYPES = (torch.float32, torch.bfloat16)     # no fp16 kernels for the GroupMix stages (fp16 is built for the ISP path)


class GMA_Block(nn.Module):
    """cpe -> LN -> EfficientAtt -> + ; LN -> Mlp -> +   (upstream groupmix.py:274-299)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path_rate=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        if drop_path_rate > 0.:
            raise NotImplementedError("GMA_Block: inference path, drop_path_rate must be 0 (identity upstream too)")
        self.cpe = ConvPosEnc(dim=dim, k=3)
        self.norm1 = norm_layer(dim)
        self.att = EfficientAtt(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path_rate = nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)

    def _fusable(self, a) -> bool:
        """csrc/gma_fused.hip is built for the cfg3 shape: dim 80 (5 x 16), 8 heads, MLP ratio 4, bf16."""
        return (ops.FUSE_GMA and a.dtype == torch.bfloat16 and a.shape[-1] == 80 and self.att.num_heads == 8 and
                self.mlp.fc1.out_features == 320 and self.att.qkv.in_features == 80 and self.norm1.eps == self.norm2.eps)

    def _entry(self, a, pre):
        """cpe(pre(a)): the 1x1 convolution in front of the block (the cfg3 net's gma_in, 192 -> 80) and ConvPosEnc as ONE launch (realcam::gma_in_cpe) where that
        form exists (bf16, 192 -> 80, the block's fused path), else the two launches."""
        w = pre.weight
        if (ops.FUSE_GMA_ENTRY and a.dtype == torch.bfloat16 and tuple(w.shape) == (80, 192, 1, 1) and tuple(self.cpe.proj.weight.shape) == (80, 1, 3, 3) and
                a.shape[0] * a.shape[1] * a.shape[2] > 0 and a.shape[1] * a.shape[2] * 192 * 2 < 2 ** 31):
            dw = self.cpe.proj.weight
            toeplitz = ops.derived(self.cpe, "toeplitz3", (dw,), lambda: torch.ops.realcam.dw_toeplitz_pack(ops.dw_taps(dw.detach().float()).to(a.device), 3))
            return torch.ops.realcam.gma_in_cpe(ops._req(a, "gma_in input"), ops.packed_chain_natural(pre), ops.f32_param(pre, "bias") if pre.bias is not None else None,
                                                toeplitz, ops.f32_param(self.cpe.proj, "bias") if self.cpe.proj.bias is not None else None)
        return self.cpe._nhwc(pre._nhwc(a))

    def _nhwc(self, a, post=None, pre=None):
        """post = (conv1x1 module, residual): fold `conv(block(a)) + residual` into the block's last launch (the cfg3 net's gma_out).
        pre = the conv1x1 module in front of the block (gma_in): `a` is ITS input, and conv + ConvPosEnc run as one launch where possible."""
        if self.training:
            raise RuntimeError("realcamnet_amd is an inference path: call .eval() first")
        ops.require_dtype(a, SUPPORTED_DTYPES, "GMA_Block")
        if pre is not None:
            x = self._entry(a, pre)
            a = x                                   # (only its dtype / width matter below)
        else:
            x = self.cpe._nhwc(a)
        if self._fusable(a) and (post is None or post[0].weight.shape[0] == 192):
            R = torch.ops.realcam
            f32 = ops.f32_param
            if ops.FUSE_GMA_FRONT:                                          # LayerNorm1 + qkv + aggregators: one launch, qkv stays on chip
                qkvp, loc, kmax = self.att.aggregator._run_front(x, self.norm1, self.att.qkv)
                convv = self.att.crpe._conv_v(qkvp)
                ktv = R.gma_kv_mfma(qkvp, kmax, float(self.att.scale))
            else:
                wq, bq = ops.packed_chain(self.att.qkv)
                qkv = R.gma_ln_qkv(x, wq, bq, f32(self.norm1, "weight"), f32(self.norm1, "bias"), float(self.norm1.eps))
                qkvp, loc, convv, ktv = self.att._context(qkv)
            wp, bp = ops.packed_chain(self.att.proj)
            w1, b1 = ops.packed_chain(self.mlp.fc1)
            w2, b2 = ops.packed_chain(self.mlp.fc2)
            wo, bo, res = (*ops.packed_chain(post[0]), ops._req(post[1], "residual")) if post is not None else (None, None, None)
            return R.gma_tail(qkvp, convv, loc, x, ktv, wp, bp, f32(self.norm2, "weight"), f32(self.norm2, "bias"), float(self.norm2.eps),
                              w1, b1, w2, b2, res, wo, bo)
        x = self.att._nhwc(ops.layernorm(x, self.norm1), residual=x)
        y = self.mlp._nhwc(ops.layernorm(x, self.norm2), residual=x)
        return y if post is None else ops.conv2d(y, post[0], residual=post[1])

    def forward(self, x_input, size):
        return self._nhwc(_as_nhwc(x_input, size)).reshape(x_input.shape)


def _as_nhwc(x, size):
    """(B,N,C) tokens -> the same memory viewed as NHWC (B,H,W,C)."""
    x = ops._req(x, "tokens")
    b, n, c = x.shape
    if size is None:
        return x.reshape(b, 1, n, c)
    H, W = size
    if H * W != n:
        raise ValueError(f"size {size} does not match {n} tokens")
    return x.reshape(b, H, W, c)
