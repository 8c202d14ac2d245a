"""GPU (-m gpu): rc_conv2d form by form against the float64 yardstick of conv_ref.py, every case in two data regimes.

  exact        small dyadic operands (conv_ref.exact_data): every intermediate is exact in fp32, so the result must equal round_to(ref64, dtype) bit for bit in
               any summation order -- this pins the single round-to-nearest-even at the store.  (The sign of a zero is not compared: the float64 reference and the
               kernels' med3-based ReLU may legitimately disagree on max(-0, +0).  GELU is transcendental: its "exact" run is checked like a real-valued one.)
  real-valued  conv_ref.real_data: within_rounding(got, ref64, slack64_conv) everywhere, and a second launch gives the same bits.

Coverage (form, dtypes, reached instantiation by conv_ref.plan, test).  test_conv_host.py checks this table, and that the cases below reach every
launch_conv<ConvCfg<...>> of csrc/conv_inst_*.hip.

  form                                   dtypes          instantiation                      test
  instantiation plain                    bf16 f16 f32    every ConvCfg<T, CK, NT, KS>       test_every_instantiation_plain_and_relu_bias
  instantiation relu+bias                bf16 f16 f32    every ConvCfg<T, CK, NT, KS>       test_every_instantiation_plain_and_relu_bias
  named shapes                           bf16 f16 f32    80->80 240->64 320->64 k5 160->224 test_named_layer_shapes
  cout_tile widths                       bf16 f16 f32    ConvCfg<T, 16|64, 1..5, 1|3>       test_named_layer_shapes
  key 0                                  bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 1                                  bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 2                                  bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 16                                 bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 32                                 bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 8                                  bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 6                                  bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 33                                 bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 34                                 bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  key 80                                 bf16 f16 f32    48->48 32->32 64->64 64->128       test_fast_epilogue_keys
  generic gelu                           bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic relu_post                      bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic film                           bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic film misaligned                bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic leaky slope                    bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic res+relu                       bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic mul+res                        bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  generic scale                          bf16 f16 f32    48->48 64->128                     test_generic_epilogue_forms
  ragged cout                            bf16 f16 f32    48->20 48->36 (NT 1)               test_ragged_cout_stores_nothing_past_cout
  routes one tile                        bf16 f16        48->48 32->32 64->64               test_kernel_routes_agree
  routes cout tiles                      bf16 f16        48->192 64->128                    test_kernel_routes_agree
  routes resident weights                bf16 f16 f32    16->32 (kernel 2, w_resident)      test_kernel_routes_agree
  routes fp32                            f32             16->16 16->64 (kernels 1 / 2 / 3)  test_kernel_routes_agree
  routes chunks                          bf16 f16        128->64 96->48                     test_kernel_routes_agree
  routes pss                             bf16            48->192 PixelShuffle(2)            test_kernel_routes_agree
  routes strip heights                   bf16 f16        48->48 128->64, H 3 4 5 15 16 17   test_kernel_routes_agree
  scalar staging offset                  bf16 f16 f32    48->32 16->32                      test_scalar_staging
  scalar staging cin                     bf16 f16 f32    3 5 12 6 ->32                      test_scalar_staging
  scalar staging gated                   bf16 f16 f32    12->32 48->32 (+store_input)       test_scalar_staging
  cin 4                                  bf16 f16 f32    4->32 aligned and not              test_scalar_staging
  ragged chunk                           bf16 f16 f32    24 40 104 ->32                     test_ragged_last_chunk_in_every_persist_mode
  planar NCHW                            bf16 f16 f32    48->3 48->12 48->48                test_planar_stores
  planar PixelShuffle NCHW               bf16 f16 f32    48->12 48->48                      test_planar_stores
  PixelShuffle NHWC                      bf16 f16 f32    48->192 16->64                     test_named_layer_shapes
  ksize 2                                bf16            ConvCfg<bf16_t, 16|32|64, NT, 2>   test_every_instantiation_plain_and_relu_bias
  ksize 2 src_h src_w                    bf16            64->64 128->48 192->16 stride 2    test_stride2_window_reading_its_own_input
  several tiles kernel 2                 bf16            48->48 persist_auto 0              test_persistent_blocks_walk_several_tiles
  several tiles kernel 2 resident        bf16            16->32 persist 3                   test_persistent_blocks_walk_several_tiles
  several tiles kernel 3                 bf16            48->48 persist 2                   test_persistent_blocks_walk_several_tiles
  several tiles kernel 4                 bf16            128->16 thin 0                     test_persistent_blocks_walk_several_tiles
  several tiles kernel 4b                bf16            128->16 thin 2                     test_persistent_blocks_walk_several_tiles
  several tiles kernel 6                 bf16            32->32 persist_auto 2              test_persistent_blocks_walk_several_tiles
  several tiles kernel 7                 bf16            64->64 persist_auto 2              test_persistent_blocks_walk_several_tiles
  sum slots refusal                      bf16            48->48 relu+sums                   test_a_sum_slot_count_of_neither_layout_is_refused

Knob combinations dropped as no-ops (launch_conv_g): `persist_auto` under persist 0 (nothing persistent is considered) and under persist 2 (kernel 3 is tried first
on every one-chunk, one-cout-tile layer); `thin` on one-chunk, one-cout-tile layers, under persist 0, and on 48 -> 192 + residual (that key stays on kernel 2); `pss`
on anything but the bf16 one-chunk PixelShuffle(2) layer of four cout tiles with keys 0 / 1 / 2, and under persist 0; persist 2 on layers with several chunks or cout
tiles (kernel 3 needs one of each: same route as persist 1); persist 3 on multi-chunk layers (same route as 1); for fp32 `persist_auto`, `thin` and `pss` (kernels 4 to 7 are 16-bit forms).  conv32 is left alone.

Which kernel a setting reaches is read from launch_conv_g; where the launcher reveals it -- the slot count rc_conv_sum_slots reports for the carried-sums kernels 2 / 6 / 7 --
test_persistent_blocks_walk_several_tiles compares it with the count that kernel's grid implies."""
import contextlib

import pytest
import torch

import conv_ref as R
from conv_ref import NCHW, NHWC, PS2, PS2_NCHW, Case
from realcamnet_amd import ops, torch_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = R.DTYPES
KNOBS = ("persist", "persist_auto", "thin", "pss", "lds_poison")
LAST = {}                  # what the last launch() saw beside its results: the channel-sum slot count the launcher asked for
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 7, 31), (3, 8, 32), (1, 9, 33), (3, 17, 65)]
GUARD = 64                 # sentinel elements in front of and behind an output that a partial store must leave alone


# ---- the table of cases ------------------------------------------------------------------------------------------------------------------------------------
def instantiations():
    """Every launch_conv<ConvCfg<T, CK, NT, KS>> line of csrc/conv_inst_*.hip as (dtype, ksize, ck, nt); test_conv_host.py compares it with the sources."""
    out = []
    for dt in ("bf16", "f16"):
        out += [(dt, 3, ck, nt) for ck in (8, 16, 32, 48, 64) for nt in ((1, 2, 3, 4) if ck == 32 else (1, 3, 4))]
        out += [(dt, 5, ck, 1) for ck in (32, 48)]
        out += [(dt, 1, ck, nt) for ck in (8, 16, 48, 64) for nt in ((1, 3, 4, 5) if dt == "bf16" else (1, 3, 4))]
    out += [("bf16", 1, 80, nt) for nt in (1, 3, 4, 5)] + [("bf16", 2, ck, nt) for ck in (16, 32, 64) for nt in (1, 3, 4)]
    out += [("f32", 3, ck, nt) for ck in (4, 16) for nt in (1, 3, 4)] + [("f32", 1, ck, nt) for ck in (4, 16) for nt in (1, 3, 4, 5)] + [("f32", 5, 16, 1)]
    return out


def shape_reaching(dt, ks, ck, nt):
    """The smallest (cin, cout, cout_tile) whose plan is that instantiation; the automatic cout tile width where one reaches it."""
    for ct in (0, 16, 32, 48, 64, 80):
        for cin in (16, 8, 4, 32, 48, 64, 80, 128):
            for cout in (16, 32, 48, 64, 80):
                p = R.plan(cin, cout, ks, dt, NHWC, ct)
                if p is not None and (p["ck"], p["nt"]) == (ck, nt):
                    return cin, cout, ct
    return None


def instantiation_cases():
    cases = []
    for i, (dt, ks, ck, nt) in enumerate(instantiations()):
        cin, cout, ct = shape_reaching(dt, ks, ck, nt)
        kw = dict(k=ks, shape=SHAPES[i % len(SHAPES)], cout_tile=ct, dtypes=(dt,))
        cases.append(Case(f"{dt}-k{ks}-ck{ck}-nt{nt}-plain", cin, cout, bias=False, **kw))
        cases.append(Case(f"{dt}-k{ks}-ck{ck}-nt{nt}-relu", cin, cout, act="relu", **kw))
    return cases


def named_cases():
    c = []
    h16, bf = ("bf16", "f16"), ("bf16",)
    for cin, cout in ((80, 80), (240, 64), (320, 64)):                                  # the GroupMix Linears: 80-wide chunks, 80-wide cout tiles
        c.append(Case(f"k1-{cin}-{cout}", cin, cout, k=1, shape=(3, 9, 33), act="relu", dtypes=bf))
    for cin in (48, 96, 32):                                                            # the folded tail's 5 x 5 window
        c.append(Case(f"k5-{cin}", cin, 12, k=5, shape=(1, 9, 33), dtypes=h16))
        c.append(Case(f"k5-{cin}-planar", cin, 12, k=5, shape=(1, 9, 33), out_mode=PS2_NCHW, crop=(17, 65), out_dtype="f32", dtypes=h16))
    c.append(Case("k5-16-f32", 16, 12, k=5, shape=(1, 9, 33), dtypes=("f32",)))
    for cin in (1, 3, 4):
        c.append(Case(f"f32-cin{cin}", cin, 32, shape=(3, 9, 33), act="relu", dtypes=("f32",)))
        c.append(Case(f"f32-cin{cin}-k1", cin, 32, k=1, shape=(1, 7, 31), dtypes=("f32",)))
    c.append(Case("codec-160-224", 160, 224, shape=(1, 9, 33), act="leaky", slope=0.25, dtypes=h16))        # ck 32, nt 2: seven 32-wide cout tiles
    for ct in (16, 32, 48, 64, 80):                                                     # every caller-chosen width that has a kernel
        c.append(Case(f"cout-tile-{ct}-k3", 16, 240, shape=(1, 9, 33), cout_tile=ct, act="relu", dtypes=("bf16", "f16", "f32") if ct not in (32, 80) else ()))
        c.append(Case(f"cout-tile-{ct}-k1", 64, 240, k=1, shape=(1, 9, 33), cout_tile=ct, dtypes=() if ct == 32 else (("bf16", "f32") if ct == 80 else ("bf16", "f16", "f32"))))
    c.append(Case("cout-tile-32-k3", 32, 96, shape=(1, 9, 33), cout_tile=32, act="relu", dtypes=h16))                   # nt 2 exists on 32-channel chunks only
    c.append(Case("shuffle-48-192", 48, 192, shape=(3, 9, 33), out_mode=PS2, act="relu"))
    c.append(Case("shuffle-16-64", 16, 64, shape=(1, 7, 31), out_mode=PS2))
    c.append(Case("shuffle-64-256", 64, 256, shape=(1, 9, 33), out_mode=PS2, act="leaky", slope=0.5))
    return [x for x in c if x.dtypes]


FAST_KEYS = {0: dict(), 1: dict(act="relu"), 2: dict(act="leaky", slope=0.25), 16: dict(res=True), 32: dict(sums=True), 8: dict(mul=True),
             6: dict(act="leaky", slope=0.5, film=True), 33: dict(act="relu", sums=True), 34: dict(act="leaky", slope=0.25, sums=True), 80: dict(scale=True, res=True)}
EPILOGUE_LAYERS = ((48, 48), (32, 32), (64, 64), (64, 128))


def fast_key_cases():
    return [Case(f"key{key}-{cin}-{cout}", cin, cout, shape=(3, 9, 33) if (key + cin) % 2 else (1, 17, 65), **kw)
            for cin, cout in EPILOGUE_LAYERS for key, kw in FAST_KEYS.items()]


GENERIC_FORMS = {"gelu": dict(act="gelu"), "relu_post": dict(act="relu_post", res=True), "film": dict(film=True),
                 "film-misaligned": dict(film=True, act="leaky", slope=0.5, film_offset=1), "leaky-slope-2": dict(act="leaky", slope=2.0),
                 "leaky-slope-neg": dict(act="leaky", slope=-0.5), "res+relu": dict(act="relu", res=True), "mul+res": dict(mul=True, res=True),
                 "mul+relu": dict(mul=True, act="relu"), "scale": dict(scale=True), "scale+relu+sums": dict(scale=True, act="relu", sums=True)}


def generic_cases():
    return [Case(f"{name}-{cin}-{cout}", cin, cout, shape=(3, 9, 33) if cout == 48 else (1, 17, 65), **kw)
            for cin, cout in ((48, 48), (64, 128)) for name, kw in GENERIC_FORMS.items()]


def ragged_cout_cases():
    forms = {"plain": dict(), "res": dict(res=True), "mul": dict(mul=True), "film": dict(film=True, act="leaky", slope=0.25), "relu_post": dict(act="relu_post", res=True),
             "sums": dict(act="relu", sums=True)}
    return [Case(f"cout{cout}-{name}", 48, cout, shape=(3, 9, 33), **kw) for cout in (20, 36) for name, kw in forms.items()]


def _grid(*axes):
    out = [{}]
    for name, vals in axes:
        out = [dict(o, **{name: v}) for o in out for v in vals]
    return out


ONE_TILE_ROUTES = [dict(persist=0), dict(persist=2)] + _grid(("persist", (1, 3)), ("persist_auto", (0, 1, 2)))
COUT_TILE_ROUTES = [dict(persist=0), dict(persist=3)] + _grid(("persist", (1,)), ("thin", (0, 1, 2)))
F32_ROUTES = [dict(persist=p) for p in (0, 1, 2, 3)]
CHUNK_ROUTES = [dict(persist=0)] + _grid(("persist", (1,)), ("thin", (0, 1, 2)))
PSS_ROUTES = [dict(persist=0), dict(persist=1, pss=0), dict(persist=1, pss=1)]
ROUTE_KEYS = {"plain": dict(), "res": dict(res=True), "gate+res": dict(scale=True, res=True), "leaky+sums": dict(act="leaky", slope=0.25, sums=True),
              "relu+sums": dict(act="relu", sums=True)}


def route_cases():
    """(case, the knob settings that change the launched kernel)."""
    out = []
    h16 = ("bf16", "f16")
    for cin, cout in ((48, 48), (32, 32), (64, 64)):
        out += [(Case(f"route-{cin}-{cout}-{n}", cin, cout, shape=(3, 17, 65), dtypes=h16, **kw), ONE_TILE_ROUTES) for n, kw in ROUTE_KEYS.items()]
    # one chunk, two cout tiles whose weights all fit beside the tile (16 -> 32: about 5 KB a tile in 16-bit, 9 KB in fp32): kernel 2 keeps them resident (w_resident) and
    # drops the per-cout-tile barrier.  16-bit: persist 3 for every key, persist 1 for the residual key (res_pre_form); plain / sums under persist 1 go to kernels 4 / 4b.
    # fp32: persist 1 and 3 (no kernel 4 there).  persist 0 is kernel 1.
    for n in ("plain", "res", "relu+sums", "gate+res"):
        out.append((Case(f"route-16-32-{n}", 16, 32, shape=(3, 17, 65), **ROUTE_KEYS[n]), COUT_TILE_ROUTES))
    for cin, cout in ((16, 16), (16, 64)):                                              # fp32, full tiles, one 16-channel chunk, one cout tile: kernels 1 / 2 / 3 / 2
        out += [(Case(f"route-f32-{cin}-{cout}-{n}", cin, cout, shape=(3, 17, 65), dtypes=("f32",), **ROUTE_KEYS[n]), F32_ROUTES) for n in ("plain", "res", "relu+sums")]
    for cin, cout in ((48, 192), (64, 128)):                                            # one chunk, several cout tiles too large to stay resident: kernels 1 / 2 (48 -> 192: residual prefetch) / 4 / 4b
        out += [(Case(f"route-{cin}-{cout}-{n}", cin, cout, shape=(1, 17, 65), dtypes=h16, **ROUTE_KEYS[n]), COUT_TILE_ROUTES) for n in ("plain", "res", "relu+sums")]
    for cin, cout in ((128, 64), (96, 48)):                                             # several chunks: kernels 1 / 4 / 4b
        out += [(Case(f"route-{cin}-{cout}-{n}", cin, cout, shape=(1, 17, 65), dtypes=h16, **ROUTE_KEYS[n]), CHUNK_ROUTES) for n in ("plain", "res", "gate+res")]
    for H in (3, 4, 5, R.WSM_TH - 1, R.WSM_TH, R.WSM_TH + 1):                         # a row under / at / over the 4-row wave strips (kernel 6) and the 16-row strips (kernels 4, 4b, 6)
        out.append((Case(f"route-h{H}-48-48-res", 48, 48, shape=(1, H, 33), dtypes=h16, res=True), ONE_TILE_ROUTES))
        out.append((Case(f"route-h{H}-48-48-relu+sums", 48, 48, shape=(3, H, 33), dtypes=h16, act="relu", sums=True), ONE_TILE_ROUTES))
        out.append((Case(f"route-h{H}-128-64", 128, 64, shape=(1, H, 33), dtypes=h16, act="relu"), CHUNK_ROUTES))
    for n, kw in (("plain", dict()), ("relu", dict(act="relu")), ("leaky", dict(act="leaky", slope=0.5))):
        out.append((Case(f"route-pss-{n}", 48, 192, shape=(1, 33, 65), out_mode=PS2, dtypes=("bf16",), **kw), PSS_ROUTES))
    return out


def staging_cases():
    c = []
    for cin in (48, 16):                                                                # a contiguous view at element offset 1: the scalar path on a vectorisable layer
        c.append(Case(f"offset1-{cin}", cin, 32, offset=1, poison=True, act="relu"))
        c.append(Case(f"offset1-{cin}-gated", cin, 32, offset=1, poison=True, gated=True, store=True))
        c.append(Case(f"offset1-{cin}-gated-nostore", cin, 32, offset=1, poison=True, gated=True))
    for cin, dts in ((3, ("bf16", "f16", "f32")), (5, ("bf16", "f16", "f32")), (12, ("bf16", "f16")), (6, ("f32",))):
        c.append(Case(f"cin{cin}", cin, 32, shape=(3, 9, 33), poison=True, act="leaky", slope=0.5, dtypes=dts))
        c.append(Case(f"cin{cin}-gated", cin, 32, shape=(3, 9, 33), poison=True, gated=True, store=True, dtypes=dts))
        c.append(Case(f"cin{cin}-gated-nostore", cin, 32, poison=True, gated=True, dtypes=dts))
    for off in (0, 1, 2, 4):                                                            # 16-bit: 8-byte aligned (the one-load-per-pixel branch) at 0 and 4, not at 1 and 2
        c.append(Case(f"cin4-offset{off}", 4, 32, shape=(3, 9, 33), offset=off, poison=True, act="relu"))
    c.append(Case("cin4-gated", 4, 32, poison=True, gated=True, store=True))
    return c


def ragged_chunk_cases():
    return [Case(f"chunk-{cin}-{n}", cin, 32, shape=(1, 17, 65), poison=True, **kw) for cin in (24, 40, 104)
            for n, kw in (("relu", dict(act="relu")), ("res", dict(res=True)), ("gated", dict(gated=True, store=True)))]


def planar_cases():
    c = []
    crops = {NCHW: (None, (1, 1), (5, 7), (9, 33), (8, 31)), PS2_NCHW: (None, (1, 1), (5, 7), (17, 65), (18, 66), (16, 63))}
    for mode, couts in ((NCHW, (3, 12, 48)), (PS2_NCHW, (12, 48))):
        for cout in couts:
            for i, crop in enumerate(crops[mode]):
                for od in ("f32", "16"):
                    c.append(Case(f"planar{mode}-{cout}-{'full' if crop is None else 'x'.join(map(str, crop))}-{od}", 48, cout, shape=(3, 9, 33), out_mode=mode, crop=crop,
                                  out_dtype=od, act=("relu", None, "leaky")[i % 3], slope=0.5))
    return c


def multi_tile_cases(cus=256):
    """One shape per persistent kernel whose work items exceed twice that kernel's grid (sized as launch_conv_g sizes it from the CU count)."""
    def rows_for(items, tiles_x, batch, rows_per_item):
        return rows_per_item * (items // (tiles_x * batch) + 1)
    c = []
    keys = (("plain", dict()), ("res", dict(res=True)), ("relu+sums", dict(act="relu", sums=True)))
    W, B = 96, 3
    for n, kw in keys:
        # kernel 2: grid = blocks per CU (3: NT <= 2 ... else 2; take 3) x CUs over 8 x 32 tiles
        c.append((2, Case(f"tiles-k2-{n}", 48, 48, shape=(B, rows_for(2 * 3 * cus, 3, B, 8), W), dtypes=("bf16",), **kw), dict(persist=1, persist_auto=0)))
        # kernel 3: grid = CUs over 8 x 32 tiles
        # kernel 2 with both cout tiles' weights resident: the block's later tiles reuse them and skip the per-cout-tile barrier
        c.append(("2r", Case(f"tiles-k2r-{n}", 16, 32, shape=(B, rows_for(2 * 3 * cus, 3, B, 8), W), dtypes=("bf16",), **kw), dict(persist=3)))
        c.append((3, Case(f"tiles-k3-{n}", 48, 48, shape=(B, rows_for(2 * cus, 3, B, 8), W), dtypes=("bf16",), **kw), dict(persist=2)))
        # kernel 6 / 7: grid = CUs over 16 x 32 regions / pairs of tiles.  The map of kernel 2 (2 CUs + 3 tiles an image): more than twice the grid here too, and its
        # per-tile slot count (8 CUs + 12) exceeds the compact one (8 x grid), so the relu+sums case takes the compact layout of the carried sums
        c.append((6, Case(f"tiles-k6-{n}", 32, 32, shape=(B, rows_for(2 * 3 * cus, 3, B, 8), W), dtypes=("bf16",), **kw), dict(persist=1, persist_auto=2)))
        c.append((7, Case(f"tiles-k7-{n}", 64, 64, shape=(B, rows_for(2 * 3 * cus, 3, B, 8), W), dtypes=("bf16",), **kw), dict(persist=1, persist_auto=2)))
    for n, kw in keys:
        # kernels 4 / 4b: grid = CUs over 16 x 32 regions (x cout tiles); their sums are per tile
        c.append((4, Case(f"tiles-k4-{n}", 128, 16, shape=(B, rows_for(2 * cus, 3, B, 16), W), dtypes=("bf16",), **kw), dict(persist=1, thin=0)))
        c.append(("4b", Case(f"tiles-k4b-{n}", 128, 16, shape=(B, rows_for(2 * cus, 3, B, 16), W), dtypes=("bf16",), **kw), dict(persist=1, thin=2)))
    return c


def all_cases():
    """Every case of this file (the multi-tile shapes for 256 CUs): test_conv_host.py checks the generators, the packing and the coverage on these."""
    return (instantiation_cases() + named_cases() + fast_key_cases() + generic_cases() + ragged_cout_cases() + [c for c, _ in route_cases()] + staging_cases() +
            ragged_chunk_cases() + planar_cases() + [c for _, c, _ in multi_tile_cases()])


def out_dtype_of(c, dtype):
    """The torch dtype the launch stores: the activation dtype, or for planar stores fp32 / the 16-bit planar type (the activation type; bf16 from an fp32 net)."""
    if c.out_dtype is None:
        return dtype
    return "f32" if c.out_dtype == "f32" else ("f16" if dtype == "f16" else "bf16")


# ---- launching ---------------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def knobs(hip, **kv):
    wino, small = ops.WINOGRAD, ops.SMALL_MAP_COUT_TILE
    before = {k: hip.rc_debug_get(k.encode()) for k in KNOBS}
    try:
        ops.WINOGRAD = False                      # fp32 3x3 layers stay on the implicit GEMM (wino.hip has test_winograd.py)
        ops.SMALL_MAP_COUT_TILE = False           # and on the cout tile width the case names
        for k, v in kv.items():
            assert k in KNOBS and hip.rc_debug_set(k.encode(), v) == 0, k
        yield
    finally:
        ops.WINOGRAD, ops.SMALL_MAP_COUT_TILE = wino, small
        for k, v in before.items():
            hip.rc_debug_set(k.encode(), v)


def _dev(t, offset=0):
    """The tensor on the device; with `offset`, as a contiguous view at that element offset of a larger (512-byte aligned) buffer."""
    if t is None:
        return None
    if offset == 0:
        return t.to(DEV).contiguous()
    buf = torch.zeros(t.numel() + offset + 16, dtype=t.dtype, device=DEV)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def launch(c, d, dtype):
    """-> (out on the CPU, stored input or None, channel-sum totals (B, cout) float64 or None, guard intact?)."""
    T = DT[dtype]
    x = _dev(d["x"], c.offset)
    if c.offset:
        assert (x.data_ptr() % 16 != 0) == ((c.offset * x.element_size()) % 16 != 0) and x.is_contiguous()
    mod = ops._ConvView(d["w"].to(DEV), _dev(d.get("bias")))
    film = (_dev(d["fs"], c.film_offset), _dev(d["ft"], c.film_offset)) if c.film else None
    if c.film_offset:
        assert film[0].data_ptr() % 16 != 0
    kw = dict(act=c.act, slope=c.slope, residual=_dev(d.get("res")), mul_plus1=_dev(d.get("mul")), film=film, gate=_dev(d.get("gate")), skip=_dev(d.get("skip")),
              store_input=c.store, out_mode=c.out_mode, want_sums=c.sums, crop_hw=c.crop, out_scale=_dev(d.get("scale")))
    To = DT[out_dtype_of(c, dtype)]
    planar = c.out_mode in (NCHW, PS2_NCHW)
    guarded = planar or c.cout_tile or c.film_offset or R.plan(c.cin, c.cout, c.k, dtype, c.out_mode, c.cout_tile)["cout_packed"] != c.cout
    intact = True
    with torch.no_grad():
        if not guarded:
            r = ops.conv2d(x, mod, **kw)                                                # the production path: pack cache, slot query, dispatcher op
            r = list(r) if isinstance(r, tuple) else [r]
            out = r.pop(0)
            stored = r.pop(0) if (c.gated and c.store) else None
            sums = r.pop(0) if c.sums else None
        else:
            # what ops.conv2d cannot express (a cout tile width of the caller's, an output inside sentinels): the same packing cache and dispatcher-op functions
            pc = ops.packed_conv(mod, T, c.out_mode, c.cout_tile)
            ch, cw = c.crop if (planar and c.crop) else (0, 0)
            args = (x, pc.wpacked, pc.bias, pc.cout, pc.ksize, ops._ACT[c.act], float(c.slope), kw["residual"], kw["mul_plus1"], film[0] if film else None,
                    film[1] if film else None, kw["gate"], kw["skip"], c.store, c.out_mode, c.sums, ch, cw, To if planar else None, kw["out_scale"], c.cout_tile, 0)
            o0, stored, sums = torch_ops._conv_alloc(*args)
            buf = torch.full((o0.numel() + 2 * GUARD,), -12345.0 if To == torch.float32 else -123.0, dtype=To, device=DEV)      # the sentinel
            out = buf[GUARD:GUARD + o0.numel()].view(o0.shape)
            assert out.data_ptr() % 16 == 0
            torch_ops._conv_launch((out, stored, sums), *args)
            torch.cuda.synchronize()
            fill = buf[0].item()
            intact = bool((buf[:GUARD] == fill).all() and (buf[GUARD + o0.numel():] == fill).all())
            stored = stored if (c.gated and c.store) else None
            sums = sums if c.sums else None
    torch.cuda.synchronize()
    LAST["slots"] = None if sums is None else sums.shape[1]
    return out.cpu(), None if stored is None else stored.cpu(), None if sums is None else sums.double().sum(1).cpu(), intact


def _canon(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def check_exact(c, dtype, seed=0):
    d = R.exact_data(c, dtype, seed)
    ref = R.ref64_conv(c, d, dtype)
    out, stored, sums, intact = launch(c, d, dtype)
    To = DT[out_dtype_of(c, dtype)]
    tag = (c.name, dtype, "exact")
    assert intact, tag
    assert out.dtype == To and out.shape == ref["out"].shape, tag
    if c.act == "gelu":
        assert bool(R.within_rounding(out, ref["out"], ref["slack"], To).all()), tag
    else:
        want = R.round_to(ref["out"], To)
        bad = _canon(out) != _canon(want)
        assert R.same_bits(_canon(out), _canon(want)), (tag, int(bad.sum()), out[bad][:4], want[bad][:4])
    if ref["stored"] is not None:
        assert R.same_bits(stored, ref["stored"]), tag
    if c.sums and c.act != "gelu":
        assert torch.equal(sums, ref["sums"]), (tag, (sums - ref["sums"]).abs().max())
    return out, stored, sums


def check_real(c, dtype, seed=0):
    d = R.real_data(c, dtype, seed)
    ref = R.ref64_conv(c, d, dtype)
    out, stored, sums, intact = launch(c, d, dtype)
    out2, stored2, sums2, _ = launch(c, d, dtype)
    To = DT[out_dtype_of(c, dtype)]
    tag = (c.name, dtype, "real")
    assert intact, tag
    ok = R.within_rounding(out, ref["out"], ref["slack"], To)
    assert bool(ok.all()), (tag, int((~ok).sum()), out[~ok][:4], ref["out"][~ok][:4], ref["slack"][~ok][:4])
    assert R.same_bits(out, out2), tag
    if ref["stored"] is not None:
        assert R.same_bits(stored, ref["stored"]) and R.same_bits(stored, stored2), tag
    if c.sums:
        assert bool(((sums - ref["sums"]).abs() <= ref["sums_slack"]).all()), (tag, (sums - ref["sums"]).abs().max())
        assert torch.equal(sums, sums2), tag
    return out


def check_both(hip, c, **kn):
    for dtype in c.dtypes:
        with knobs(hip, lds_poison=1 if c.poison else 0, **kn):
            check_exact(c, dtype)
            check_real(c, dtype)


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. instantiations -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", instantiation_cases(), ids=_ids(instantiation_cases()))
def test_every_instantiation_plain_and_relu_bias(hip, c):
    (dt,) = c.dtypes
    p = R.plan(c.cin, c.cout, c.k, dt, c.out_mode, c.cout_tile)
    assert f"{dt}-k{c.k}-ck{p['ck']}-nt{p['nt']}-" in c.name
    check_both(hip, c)


@pytest.mark.parametrize("c", named_cases(), ids=_ids(named_cases()))
def test_named_layer_shapes(hip, c):
    check_both(hip, c)


# ---- 2. epilogues ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fast_key_cases(), ids=_ids(fast_key_cases()))
def test_fast_epilogue_keys(hip, c):
    check_both(hip, c)


@pytest.mark.parametrize("c", generic_cases(), ids=_ids(generic_cases()))
def test_generic_epilogue_forms(hip, c):
    check_both(hip, c)


@pytest.mark.parametrize("c", ragged_cout_cases(), ids=_ids(ragged_cout_cases()))
def test_ragged_cout_stores_nothing_past_cout(hip, c):
    """cout 20 and 36 on 16-wide cout tiles: the 4-channel lane groups past cout must not store (the output sits between sentinels, and every element of it is compared)."""
    assert R.plan(c.cin, c.cout, 3, "bf16", NHWC)["cout_packed"] != c.cout
    check_both(hip, c)


# ---- 3. kernel routes --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,routes", route_cases(), ids=[c.name for c, _ in route_cases()])
def test_kernel_routes_agree(hip, c, routes):
    """Every route of a case gives the yardstick's bits on exact data, and one and the same result (output bits, sums totals within rounding) on real-valued data."""
    for dtype in c.dtypes:
        first = None
        for kn in routes:
            with knobs(hip, **kn):
                check_exact(c, dtype)
                out = check_real(c, dtype)
            if first is None:
                first = out
            assert R.same_bits(out, first), (c.name, dtype, kn)


# ---- 4. staging --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", staging_cases(), ids=_ids(staging_cases()))
def test_scalar_staging(hip, c):
    """cin_vec_ok == 0: in0 at a storage offset that is not 16-byte aligned, or cin % unit != 0; gated or not, with and without store_input, two cout tiles (cout 32 on
    16-wide tiles: only tile 0 may materialise the stored input), LDS poisoned first."""
    check_both(hip, c)


@pytest.mark.parametrize("c", ragged_chunk_cases(), ids=_ids(ragged_chunk_cases()))
def test_ragged_last_chunk_in_every_persist_mode(hip, c):
    for dtype in c.dtypes:
        assert c.cin % R.plan(c.cin, c.cout, 3, dtype, NHWC)["ck"] != 0
        first = None
        for persist in (0, 1, 2, 3):
            with knobs(hip, persist=persist, lds_poison=1):
                check_exact(c, dtype)
                out = check_real(c, dtype)
            first = out if first is None else first
            assert R.same_bits(out, first), (c.name, dtype, persist)


# ---- 5. planar stores --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", planar_cases(), ids=_ids(planar_cases()))
def test_planar_stores(hip, c):
    check_both(hip, c)


# ---- 6. several tiles per block ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(multi_tile_cases())), ids=[c.name for _, c, _ in multi_tile_cases()])
def test_persistent_blocks_walk_several_tiles(hip, idx):
    """Each persistent kernel on a map whose work items exceed twice its grid, so the state a block carries from tile to tile (the prefetched residual, carried sums,
    first_tile; for 16 -> 32 under persist 3 the resident weights of both cout tiles) is used at least twice.  Exact regime; sums compared as float64 totals over the
    slots.  For relu+sums the slot count the launcher chose must be the compact count of the kernel meant (grid x waves), or the per-tile count for the others."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kernel, c, kn = multi_tile_cases(cus)[idx]
    B, H, W = c.shape
    per_item = 16 if kernel in (4, "4b", 6) else 8
    items = B * ((W + 31) // 32) * ((H + per_item - 1) // per_item)
    grid = {2: 3 * cus, "2r": 3 * cus, 3: cus, 4: cus, "4b": cus, 6: cus, 7: cus}[kernel]
    assert (items // 2 if kernel == 7 else items) > 2 * grid, (items, grid)
    with knobs(hip, **kn):
        check_exact(c, "bf16")
    if c.sums:
        pgrid = lambda limit, n: (min(limit, n) + 7) // 8 * 8          # noqa: E731  persistent_grid of csrc/common.hpp
        tiles = B * ((W + 31) // 32) * ((H + 7) // 8)
        legacy = hip.rc_conv_sum_tiles(H, W)
        want = {2: 4 * pgrid(2 * cus, tiles),                          # 48 -> 48, NT 3: two blocks per CU, 4 waves
                6: 8 * pgrid(cus, items), 7: 8 * pgrid(cus, (tiles + 1) // 2)}.get(kernel, legacy)
        assert LAST["slots"] == want and (want < legacy or kernel not in (2, 6, 7)), (kernel, LAST["slots"], want, legacy)


def test_a_sum_slot_count_of_neither_layout_is_refused(hip):
    """chan_sums_slots that is neither the per-tile count nor the launched kernel's compact count: RC_ERR_INVALID from launch_conv_g, nothing launched (the buffer is
    larger than either layout all the same)."""
    c = Case("slots", 48, 48, shape=(1, 17, 65), act="relu", sums=True)
    d = R.exact_data(c, "bf16")
    x = _dev(d["x"])
    mod = ops._ConvView(d["w"].to(DEV), _dev(d["bias"]))
    pc = ops.packed_conv(mod, torch.bfloat16, NHWC, 0)
    legacy = hip.rc_conv_sum_tiles(17, 65)
    out = torch.full((1, 17, 65, 48), -123.0, dtype=torch.bfloat16, device=DEV)
    sums = torch.zeros((1, legacy + 3, 48), dtype=torch.float32, device=DEV)
    args = (x, pc.wpacked, pc.bias, 48, 3, ops._ACT["relu"], 0.0, None, None, None, None, None, None, False, NHWC, True, 0, 0, None, None, 0, 0)
    with knobs(hip):
        with pytest.raises(Exception, match="neither layout"):
            torch_ops._conv_launch((out, x.new_empty((0,)), sums), *args)
    torch.cuda.synchronize()
    assert bool((out == -123.0).all()) and bool((sums == 0).all())


@pytest.mark.parametrize("cin,cout,shape", [(64, 64, (1, 16, 24)), (128, 48, (3, 17, 33)), (192, 16, (1, 31, 65)), (64, 3, (1, 1, 1))])
def test_stride2_window_reading_its_own_input(hip, cin, cout, shape):
    """rc_conv_desc.src_h / src_w: the ksize-2 launch gathers the space-to-depth channels of its own input while staging (even and odd source sizes: the phase-1 row and
    column beyond the edge read zero).  Both regimes against the float64 stride-2 convolution, with and without a LeakyReLU."""
    B, H, W = shape
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 1)
    for regime in ("exact", "real"):
        g = torch.Generator().manual_seed(cin + cout + H)
        if regime == "exact":
            x = (torch.randint(-4, 5, (B, H, W, cin), generator=g).float() / 2).bfloat16()
            w = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
            bias = torch.randint(96, 160, (cout,), generator=g).float() + (2 * torch.randint(0, 32, (cout,), generator=g).float() + 1) / 64
            bias = bias * torch.where(torch.arange(cout) % 2 == 1, -1.0, 1.0)
        else:
            x = R.values((B, H, W, cin), torch.bfloat16, 5, span=2)
            w = R.values((cout, cin, 3, 3), torch.float32, 6, span=2, specials=False) / 8
            bias = R.values((cout,), torch.float32, 7, span=2, specials=False)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(bias)
        mod = conv.to(DEV, torch.bfloat16).eval()                     # bf16 weights select the 2 x 2 window; rounded as the packer rounds them
        mod.bias = torch.nn.Parameter(bias.to(DEV))                   # the bias stays fp32, as rc_conv_pack_bias takes it
        for act, slope in ((None, 0.0), ("leaky", 0.25)):
            ref, slack = R.ref64_conv_stride2(x, w, bias, "bf16", act, slope)
            with knobs(hip), torch.no_grad():
                assert ops.FOLD_STRIDE2
                y = ops.conv_stride2(x.to(DEV), mod, act=act, slope=slope)
                y2 = ops.conv_stride2(x.to(DEV), mod, act=act, slope=slope)
            torch.cuda.synchronize()
            y, y2 = y.cpu(), y2.cpu()
            assert y.shape == ref.shape and R.same_bits(y, y2), (regime, act)
            if regime == "exact":
                assert R.same_bits(_canon(y), _canon(R.round_to(ref, torch.bfloat16))), (regime, act)
            assert bool(R.within_rounding(y, ref, slack, torch.bfloat16).all()), (regime, act)
