"""When is a value derived from a module's parameters (host-built taps, conv views, GDN's effective gamma / beta, the entropy bottleneck's
58-column table, the coder's CDF tables, the Haar-tap verdict) rebuilt, and when is the kept one returned?  Everything here runs on CPU tensors.

The contract, for every site: a second call returns the SAME object; an in-place write, a new nn.Parameter and a dtype cast rebuild; an edit
through `.data` does not (the documented limit) until ops.invalidate_caches(module); nothing derived ever shows up in the state_dict; modules
made of fake tensors neither crash nor touch a real module's entries."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch._subclasses.fake_tensor import FakeTensor, FakeTensorMode

from realcamnet_amd import bitstream, networks, ops, tcm


def _tensors(v):
    """The tensors of a derived value, whatever its shape: a tensor, a tuple / list of values, a conv view."""
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (tuple, list)):
        return [t for e in v for t in _tensors(e)]
    if isinstance(v, ops._ConvView):
        return [t for t in (v.weight, v.bias) if t is not None]
    raise TypeError(type(v))


def _same_values(a, b):
    a, b = _tensors(a), _tensors(b)
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


# name -> (module factory, the cached call, the parameter the tests write to)
SITES = {
    "host_cached": (lambda: nn.Conv2d(4, 4, 3), lambda m: ops.host_cached(m, "twice", [m.weight, m.bias], lambda w, b: (w * 2, b + 1)), "weight"),
    "split_conv_views": (lambda: nn.Conv2d(4, 6, 3), lambda m: ops.split_conv_views(m, (2, 4)), "weight"),
    "split_conv_input_views": (lambda: nn.Conv2d(4, 6, 3), lambda m: ops.split_conv_input_views(m, (1, 3)), "bias"),
    "gdn_effective": (lambda: tcm.GDN(4), lambda m: m._effective(), "gamma"),
    "bottleneck_packed": (lambda: tcm.EntropyBottleneck(4), lambda m: m._packed()[0], "_bias1"),
}
site = pytest.mark.parametrize("name", sorted(SITES))


def _make(name):
    torch.manual_seed(7)
    make, call, pname = SITES[name]
    return make().eval(), call, pname


def _snapshot(v):
    """Copies of a derived value's tensors (views of a parameter follow its in-place writes; the copies do not)."""
    return [t.clone() for t in _tensors(v)]


def _rebuilt(m, call, old):
    """The call after a change: a new object whose values are those a module without any cache gives."""
    got = call(m)
    assert got is not old
    assert call(m) is got
    ops.invalidate_caches(m)
    assert _same_values(got, call(m))
    return got


@site
def test_second_call_returns_the_same_object(name):
    m, call, _ = _make(name)
    keys = list(m.state_dict())
    v = call(m)
    assert call(m) is v and call(m) is v
    assert list(m.state_dict()) == keys and len(list(m.buffers())) + len(list(m.parameters())) == len(keys)      # never a buffer, never saved


@site
def test_in_place_write_rebuilds(name):
    m, call, pname = _make(name)
    v = call(m)
    old_vals = _snapshot(v)
    with torch.no_grad():
        getattr(m, pname).add_(0.25)
    got = _rebuilt(m, call, v)
    assert not _same_values(got, old_vals)
    v, old_vals = got, _snapshot(got)
    with torch.no_grad():
        getattr(m, pname).copy_(torch.randn_like(getattr(m, pname)))
    got = _rebuilt(m, call, v)
    assert not _same_values(got, old_vals)


@site
def test_new_parameter_rebuilds(name):
    m, call, pname = _make(name)
    v = call(m)
    old_vals = _snapshot(v)
    setattr(m, pname, nn.Parameter(torch.randn_like(getattr(m, pname))))
    got = _rebuilt(m, call, v)
    assert not _same_values(got, old_vals)


@site
def test_dtype_cast_rebuilds(name):
    m, call, _ = _make(name)
    v = call(m)
    m.to(torch.bfloat16)
    v = _rebuilt(m, call, v)
    m.double()
    _rebuilt(m, call, v)


@site
def test_data_edit_is_not_seen_until_invalidate_caches(name):
    m, call, pname = _make(name)
    v = call(m)
    old_vals = _snapshot(v)
    getattr(m, pname).data.add_(0.25)                      # does not move `_version`: the documented limit
    assert call(m) is v
    ops.invalidate_caches(m)
    got = call(m)
    assert got is not v and not _same_values(got, old_vals)


def test_invalidate_caches_reaches_every_submodule():
    torch.manual_seed(1)
    net = nn.Sequential(nn.Conv2d(4, 6, 3), nn.Sequential(tcm.GDN(4), nn.Conv2d(4, 4, 3))).eval()
    calls = (lambda: ops.split_conv_views(net[0], (3, 3)), lambda: net[1][0]._effective(),
             lambda: ops.host_cached(net[1][1], "w", [net[1][1].weight], lambda w: w + 1))
    before = [c() for c in calls]
    assert all(c() is b for c, b in zip(calls, before))
    ops.invalidate_caches(net)
    after = [c() for c in calls]
    assert all(a is not b and _same_values(a, b) for a, b in zip(after, before))


def test_host_cached_values():
    """host_cached: built under no_grad from detached fp32 host copies, returned as a tuple on the parameters' device (a lone tensor is wrapped)."""
    m = nn.Conv2d(2, 2, 1).to(torch.bfloat16)
    seen = []

    def build(w):
        seen.append((w.dtype, w.device.type, w.requires_grad, torch.is_grad_enabled()))
        return w.permute(1, 0, 2, 3)
    out = ops.host_cached(m, "t", [m.weight], build)
    assert seen == [(torch.float32, "cpu", False, False)]
    assert isinstance(out, tuple) and len(out) == 1 and out[0].is_contiguous() and out[0].dtype == torch.float32
    assert torch.equal(out[0], m.weight.detach().float().permute(1, 0, 2, 3))
    assert ops.host_cached(m, "t", [m.weight], build) is out and len(seen) == 1
    other = ops.host_cached(m, "u", [m.weight], lambda w: (w, w + 1))        # another name on the same module: an entry of its own
    assert len(other) == 2 and ops.host_cached(m, "t", [m.weight], build) is out and len(seen) == 1


def test_split_views_sizes():
    m = nn.Conv2d(4, 6, 3)
    a = ops.split_conv_views(m, (2, 4))
    assert [tuple(v.weight.shape) for v in a] == [(2, 4, 3, 3), (4, 4, 3, 3)] and torch.equal(a[1].bias, m.bias.detach()[2:])
    b = ops.split_conv_views(m, (3, 3))                                      # other sizes: other views
    assert b is not a and [v.weight.shape[0] for v in b] == [3, 3]
    with pytest.raises(ValueError):
        ops.split_conv_views(m, (2, 2))
    assert [v.weight.shape[0] for v in ops.split_conv_views(m, (3, 3))] == [3, 3]
    i = ops.split_conv_input_views(m, (1, 3))
    assert [tuple(v.weight.shape) for v in i] == [(6, 1, 3, 3), (6, 3, 3, 3)] and i[0].bias is not None and i[1].bias is None
    assert ops.split_conv_input_views(m, (1, 3)) is i and ops.split_conv_input_views(m, (2, 2)) is not i
    with pytest.raises(ValueError):
        ops.split_conv_input_views(m, (1, 1))


# ---- the coder's CDF tables ---------------------------------------------------------------------------------------------------------------
def _gc():
    gc = tcm.GaussianConditional(None)
    assert gc.update_scale_table(bitstream.get_scale_table()) is True
    return gc


def _eb():
    torch.manual_seed(2)
    eb = tcm.EntropyBottleneck(4)
    assert eb.update() is True
    return eb


def _same_tables(a, b):
    return torch.equal(a.cdf, b.cdf) and torch.equal(a.sizes, b.sizes) and torch.equal(a.offsets, b.offsets)


@pytest.mark.parametrize("make", [_gc, _eb])
def test_coder_tables_are_kept_and_rebuilt(make):
    m = make()
    keys = list(m.state_dict())
    t = tcm._coder_tables(m)
    assert tcm._coder_tables(m) is t and str(t.cdf.device) == "cpu" and torch.equal(t.cdf, m._quantized_cdf)
    assert list(m.state_dict()) == keys

    cdf0 = m._quantized_cdf.clone()                                        # (on the host a Tables object may share the buffer's memory)
    m._quantized_cdf.add_(1)                                               # in-place write
    t2 = tcm._coder_tables(m)
    assert t2 is not t and torch.equal(t2.cdf, cdf0 + 1)
    m._quantized_cdf.data.sub_(1)                                          # through .data: not seen ...
    assert tcm._coder_tables(m) is t2
    ops.invalidate_caches(m)                                               # ... until the caches are dropped
    t3 = tcm._coder_tables(m)
    assert t3 is not t2 and torch.equal(t3.cdf, cdf0)

    m._quantized_cdf = m._quantized_cdf.clone()                            # a new buffer tensor
    t4 = tcm._coder_tables(m)
    assert t4 is not t3 and _same_tables(t4, t3)
    for cast in (lambda: m.to(torch.bfloat16), lambda: m.double()):        # the int tables do not change, but the tables object is rebuilt
        cast()
        t5 = tcm._coder_tables(m)
        assert t5 is not t4 and _same_tables(t5, t4) and tcm._coder_tables(m) is t5
        t4 = t5


def test_new_coder_buffers_give_new_tables():
    gc = _gc()
    t = tcm._coder_tables(gc)
    gc.update()                                                            # _set_coder_buffers: fresh buffer tensors
    t2 = tcm._coder_tables(gc)
    assert t2 is not t and _same_tables(t2, t)
    assert gc.update_scale_table(bitstream.get_scale_table()[:32], force=True) is True
    t3 = tcm._coder_tables(gc)
    assert t3 is not t2 and t3.cdf.shape[0] == 32 and tcm._coder_tables(gc) is t3
    tcm._set_coder_buffers(gc, gc._offset.clone(), gc._quantized_cdf.clone(), gc._cdf_length.clone())
    assert tcm._coder_tables(gc) is not t3

    eb = _eb()
    t = tcm._coder_tables(eb)
    assert eb.update() is False and tcm._coder_tables(eb) is t             # nothing rebuilt: the same tables
    with torch.no_grad():
        eb.quantiles.mul_(2.0)
    assert eb.update(force=True) is True
    t2 = tcm._coder_tables(eb)
    assert t2 is not t and torch.equal(t2.cdf, eb._quantized_cdf) and tuple(t2.cdf.shape) != tuple(t.cdf.shape)


def test_resized_coder_buffers_give_new_tables():
    """The codec's load_state_dict sizes the table buffers from the checkpoint (new tensors) before nn.Module copies into them."""
    src, dst = tcm.GaussianConditional(None), _gc()
    src.update_scale_table(bitstream.get_scale_table()[:32])
    t = tcm._coder_tables(dst)
    sd = {"gc." + k: v for k, v in src.state_dict().items()}
    tcm._resize_coder_buffers(dst, "gc", tcm._CODER_BUFFERS + ("scale_table",), sd)
    dst.load_state_dict(src.state_dict())
    t2 = tcm._coder_tables(dst)
    assert t2 is not t and t2.cdf.shape[0] == 32 and torch.equal(t2.cdf, src._quantized_cdf) and tcm._coder_tables(dst) is t2


# ---- conv -> DWT: the Haar-tap verdict ----------------------------------------------------------------------------------------------------
def _dwt_case():
    return torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16), networks.Conv2d(32, 32, 3, padding=1), networks.DWTForward(32)


def test_haar_tap_verdict_follows_the_taps():
    x, conv, dwt = _dwt_case()
    assert ops.conv_dwt_ok(x, conv, dwt) is True and ops.conv_dwt_ok(x, conv, dwt) is True
    with torch.no_grad():
        dwt.weight.mul_(2.0)                                               # in-place write: looked at again
    assert ops.conv_dwt_ok(x, conv, dwt) is False
    with torch.no_grad():
        dwt.weight.copy_(networks.DWTForward(32).weight)
    assert ops.conv_dwt_ok(x, conv, dwt) is True
    dwt.weight = nn.Parameter(dwt.weight.detach() * 3.0, requires_grad=False)      # a new parameter
    assert ops.conv_dwt_ok(x, conv, dwt) is False
    dwt.weight = nn.Parameter(networks.DWTForward(32).weight.detach().clone(), requires_grad=False)
    assert ops.conv_dwt_ok(x, conv, dwt) is True

    dwt.weight.data.mul_(2.0)                                              # through .data: the kept verdict ...
    assert ops.conv_dwt_ok(x, conv, dwt) is True
    ops.invalidate_caches(dwt)                                             # ... until the caches are dropped
    assert ops.conv_dwt_ok(x, conv, dwt) is False
    dwt.weight.data.mul_(0.5)
    assert ops.conv_dwt_ok(x, conv, dwt) is False                          # (kept again)
    dwt.to(torch.bfloat16)                                                 # a cast: looked at again (+-0.5 are exact in bf16)
    assert ops.conv_dwt_ok(x, conv, dwt) is True
    dwt.weight.data.mul_(2.0)
    assert ops.conv_dwt_ok(x, conv, dwt) is True
    dwt.double()
    assert ops.conv_dwt_ok(x, conv, dwt) is False
    assert list(dwt.state_dict()) == ["weight"]


# ---- fake tensors ---------------------------------------------------------------------------------------------------------------------------
@site
def test_fake_module_neither_crashes_nor_touches_a_real_modules_entries(name):
    real, call, pname = _make(name)
    v = call(real)
    vals = _snapshot(v)
    with FakeTensorMode():
        fake, _, _ = _make(name)
        assert isinstance(getattr(fake, pname), FakeTensor)
        f = call(fake)
        assert all(isinstance(t, FakeTensor) for t in _tensors(f))
        assert [(t.shape, t.dtype) for t in _tensors(f)] == [(t.shape, t.dtype) for t in _tensors(v)]
        if name != "bottleneck_packed":                                    # (shape tracing: nothing is packed, nothing kept)
            assert call(fake) is f
        assert call(real) is v                                             # the real module's entry is looked up, not rebuilt, inside the mode
    assert call(real) is v and _same_values(v, vals) and not any(isinstance(t, FakeTensor) for t in _tensors(v))
    with torch.no_grad():
        getattr(real, pname).add_(1.0)
    assert call(real) is not v


def test_fake_taps_pass_and_leave_the_real_verdict_alone():
    x, conv, dwt = _dwt_case()
    with torch.no_grad():
        dwt.weight.mul_(2.0)
    assert ops.conv_dwt_ok(x, conv, dwt) is False
    with FakeTensorMode():
        fx, fconv, fdwt = _dwt_case()
        assert isinstance(fdwt.weight, FakeTensor)
        assert ops.conv_dwt_ok(fx, fconv, fdwt) is True and ops.conv_dwt_ok(fx, fconv, fdwt) is True      # a DWTForward is built with these taps and frozen
    assert ops.conv_dwt_ok(x, conv, dwt) is False


# ---- the helper itself ----------------------------------------------------------------------------------------------------------------------
class _Builds:
    """A build function that counts its calls."""
    def __init__(self, fail=False):
        self.n, self.fail = 0, fail

    def __call__(self):
        self.n += 1
        if self.fail:
            raise NotImplementedError("no such kernel")
        return object()


def test_derived_rebuilds_when_extra_changes():
    m, build = nn.Conv2d(2, 2, 1), _Builds()
    a = ops.derived(m, "slot", (m.weight, m.bias), build, extra=(1, "x"))
    assert ops.derived(m, "slot", (m.weight, m.bias), build, extra=(1, "x")) is a and build.n == 1
    b = ops.derived(m, "slot", (m.weight, m.bias), build, extra=(2, "x"))
    assert b is not a and build.n == 2
    assert ops.derived(m, "slot", (m.weight, m.bias), build, extra=(2, "x")) is b and build.n == 2
    assert ops.derived(m, "slot", (m.weight, m.bias), build) is not b and build.n == 3                      # no extra is not that extra
    assert ops.derived(m, ("slot", 1), (m.weight, m.bias), build) is not ops.derived(m, "slot", (m.weight, m.bias), build) and build.n == 4


def test_a_raising_build_leaves_no_entry():
    m, bad, good = nn.Conv2d(2, 2, 1), _Builds(fail=True), _Builds()
    for n in (1, 2):
        with pytest.raises(NotImplementedError):
            ops.derived(m, "slot", (m.weight,), bad)
        assert bad.n == n                                                  # asked again: the failure was not kept
    v = ops.derived(m, "slot", (m.weight,), good)
    assert ops.derived(m, "slot", (m.weight,), bad) is v and bad.n == 2    # a hit never builds, so never raises
    with torch.no_grad():
        m.weight.add_(1.0)
    with pytest.raises(NotImplementedError):
        ops.derived(m, "slot", (m.weight,), bad)
    assert ops.derived(m, "slot", (m.weight,), good) is not v and good.n == 2      # nor is the value of the older weights handed out after it
    assert list(m.state_dict()) == ["weight", "bias"]


def test_drop_derived_drops_one_slot_or_all():
    m, build = nn.Conv2d(2, 2, 1), _Builds()
    get = lambda slot: ops.derived(m, slot, (m.weight,), build)
    a, b, c = get("a"), get("b"), get(("c", 1))
    ops.drop_derived(m, "a")
    assert get("b") is b and get(("c", 1)) is c and get("a") is not a
    a = get("a")
    ops.drop_derived(m, "b", ("c", 1), "never built")
    assert get("a") is a and get("b") is not b and get(("c", 1)) is not c
    a, b, c = get("a"), get("b"), get(("c", 1))
    ops.drop_derived(m)
    assert get("a") is not a and get("b") is not b and get(("c", 1)) is not c
    ops.drop_derived(nn.Conv2d(2, 2, 1))                                   # nothing derived yet: nothing to do
    ops.drop_derived(nn.Conv2d(2, 2, 1), "a")


def test_none_in_params():
    m, build = nn.Conv2d(2, 2, 1, bias=False), _Builds()
    a = ops.derived(m, "slot", (m.weight, m.bias), build)
    assert m.bias is None and ops.derived(m, "slot", (m.weight, m.bias), build) is a and build.n == 1
    m.bias = nn.Parameter(torch.zeros(2))                                  # None -> a tensor and back: not the same parameters
    b = ops.derived(m, "slot", (m.weight, m.bias), build)
    assert b is not a and ops.derived(m, "slot", (m.weight, m.bias), build) is b
    m.bias = None
    assert ops.derived(m, "slot", (m.weight, m.bias), build) is not b
    assert ops.derived(m, "none", (None,), build) is ops.derived(m, "none", (None,), build)


def test_an_entry_holds_its_tensors():
    import weakref
    m = nn.Conv2d(2, 2, 1)
    old = weakref.ref(m.weight)
    ops.derived(m, "slot", (m.weight,), _Builds())
    m.weight = nn.Parameter(torch.zeros(2, 2, 1, 1))
    assert old() is not None                                               # kept by the entry, so its address cannot be handed out again ...
    ops.derived(m, "slot", (m.weight,), _Builds())
    assert old() is None                                                   # ... until the entry is replaced


def test_another_tensor_at_the_same_address_rebuilds():
    """A parameter replaced by a fresh tensor that lands on the freed one's address with the same version counter, dtype and device is not the
    tensor the value was derived from.  Made deterministic without an allocator: two tensors wrapped, one after the other, around ONE numpy array.
    NOTE: the code before ops.derived keyed on (address, _version, dtype, device) alone and handed out the first tensor's value here."""
    arr = np.arange(8, dtype=np.float32).reshape(2, 4, 1, 1).copy()
    view = ops._ConvView(torch.from_numpy(arr), None)
    first = (view.weight.data_ptr(), view.weight._version, view.weight.dtype, str(view.weight.device))
    a = ops.split_conv_views(view, (1, 1))
    a_vals = _snapshot(a)
    (t,) = ops.host_cached(view, "twice", [view.weight], lambda w: w * 2)
    assert torch.equal(t, torch.from_numpy(arr) * 2)
    view.weight = None
    arr[...] = -arr - 1.0                                                  # written through numpy: no tensor, no version counter
    view.weight = torch.from_numpy(arr)
    assert (view.weight.data_ptr(), view.weight._version, view.weight.dtype, str(view.weight.device)) == first
    b = ops.split_conv_views(view, (1, 1))
    assert b is not a and not _same_values(b, a_vals) and torch.equal(b[1].weight, view.weight[1:])
    (t2,) = ops.host_cached(view, "twice", [view.weight], lambda w: w * 2)
    assert t2 is not t and torch.equal(t2, torch.from_numpy(arr) * 2)
