"""The binding layer's shared helpers (marf_hip) without a GPU: the parameter flattener, the packed-weight
cache, the shard scatter, the stale-buffer check and the refused-size helper.  Each of them stands once in
marf_hip.py; the planar launches, both fused steps, the render and the mask net go through them."""
import ctypes

import pytest
import torch


def _layers():
    torch.manual_seed(0)
    return [torch.nn.Linear(5, 7), torch.nn.Linear(7, 4), torch.nn.Linear(4, 3)]


def _params(layers):
    return [p for lay in layers for p in lay.parameters()]


def test_flatten_params_keeps_objects_and_values():
    import marf_hip
    layers = _layers()
    before = _params(layers)
    want = [p.detach().clone() for p in before]
    assert marf_hip.flat_view(before) is None  # (torch allocates every Linear parameter on its own)
    ps = marf_hip.flatten_params(p for lay in layers for p in lay.parameters())
    flat = marf_hip.flat_view(ps)
    assert flat is not None and flat.numel() == sum(p.numel() for p in want)
    assert len(ps) == len(before) and all(a is b for a, b in zip(ps, before))
    assert all(a is b for a, b in zip(_params(layers), before))  # the modules still hold them
    assert all(torch.equal(p, w) and p.shape == w.shape for p, w in zip(ps, want))
    assert torch.equal(flat, torch.cat([w.reshape(-1) for w in want]))


def test_flatten_params_only_when_needed():
    import marf_hip
    layers = _layers()
    ps = marf_hip.flatten_params(_params(layers))
    ptrs = [p.data_ptr() for p in ps]
    again = marf_hip.flatten_params(_params(layers))
    assert [p.data_ptr() for p in again] == ptrs  # already one buffer: nothing moves
    # another allocation between two layers' .data (what a device move or a load does)
    layers[1].weight.data = layers[1].weight.data.clone()
    want = [p.detach().clone() for p in _params(layers)]
    assert marf_hip.flat_view(_params(layers)) is None
    third = marf_hip.flatten_params(_params(layers))
    assert marf_hip.flat_view(third) is not None
    assert all(a is b for a, b in zip(third, ps))
    assert third[0].data_ptr() != ptrs[0]  # a new buffer
    assert all(torch.equal(p, w) for p, w in zip(third, want))


class _Pack:
    """A pack callable that counts its calls and records what it was given."""

    def __init__(self):
        self.calls = 0
        self.flat = None

    def __call__(self, flat, buf):
        self.calls += 1
        self.flat = flat.clone()
        assert buf.dtype == torch.uint8 and buf.numel() == 24


def test_packed_cache_packs_once_per_parameter_version():
    import marf_hip
    ps = marf_hip.flatten_params(_params(_layers()))
    pack = _Pack()
    sizes = []
    cache = marf_hip._PackedCache(lambda: sizes.append(24) or 24, pack)
    assert pack.calls == 0 and not sizes  # nothing is asked or packed before the first use
    buf = cache.get(ps)
    assert pack.calls == 1 and sizes == [24]
    assert torch.equal(pack.flat, torch.cat([p.detach().reshape(-1) for p in ps]))
    assert cache.get(ps) is buf and cache.get(list(ps)) is buf
    assert pack.calls == 1
    with torch.no_grad():
        ps[2].add_(1.0)  # an in-place update (torch's optimizers): the version counter moves
    assert cache.get(ps) is buf and pack.calls == 2
    assert torch.equal(pack.flat, torch.cat([p.detach().reshape(-1) for p in ps]))
    assert cache.get(ps) is buf and pack.calls == 2
    marf_hip.PARAM_GENERATION[0] += 1  # an in-library update (marf Adam writes through raw pointers)
    assert cache.get(ps) is buf and pack.calls == 3
    assert cache.get(ps) is buf and pack.calls == 3
    cache.invalidate()
    assert cache.get(ps) is buf and pack.calls == 4
    assert cache.get(ps) is buf and pack.calls == 4
    assert sizes == [24]  # one buffer all along


def test_packed_cache_concatenates_separate_parameters():
    import marf_hip
    ps = _params(_layers())  # not flattened
    assert marf_hip.flat_view(ps) is None
    pack = _Pack()
    cache = marf_hip._PackedCache(lambda: 24, pack)
    cache.get(ps)
    assert pack.calls == 1 and torch.equal(pack.flat, torch.cat([p.detach().reshape(-1) for p in ps]))


def test_packed_cache_forgets_a_pack_that_raised():
    import marf_hip
    ps = marf_hip.flatten_params(_params(_layers()))
    state = {"fail": False, "calls": 0}

    def pack(flat, buf):
        state["calls"] += 1
        if state["fail"]:
            raise RuntimeError("refused")

    cache = marf_hip._PackedCache(lambda: 8, pack)
    cache.get(ps)
    state["fail"] = True
    with torch.no_grad():
        ps[0].add_(1.0)
    with pytest.raises(RuntimeError, match="refused"):
        cache.get(ps)
    state["fail"] = False
    cache.get(ps)
    assert state["calls"] == 3  # the same versions again: still packed, the failed attempt cached nothing


def test_scatter_rows():
    import marf_hip
    w = torch.randn(4, 8)
    d = torch.randn(4, 8)
    assert marf_hip._scatter_rows(d, w, 0, 4) is d
    d2 = torch.randn(2, 8)
    out = marf_hip._scatter_rows(d2, w, 1, 3)
    assert out.shape == w.shape and out.dtype == w.dtype
    assert torch.equal(out[1:3], d2)
    assert not out[0].any() and not out[3].any()


def test_buffers_check_raises_after_a_second_get():
    import marf_hip
    bufs = marf_hip._Buffers()
    a = bufs.get("saved", 16, "cpu")
    gen = bufs.generation("saved", "cpu")
    bufs.check("saved", gen, "cpu", "the test's saved bytes were")  # the buffer is still this forward's
    bufs.get("other", 16, "cpu")
    bufs.check("saved", gen, "cpu", "the test's saved bytes were")  # another buffer does not count
    assert bufs.get("saved", 8, "cpu") is a  # handed out again
    with pytest.raises(RuntimeError, match="the test's saved bytes were reused by a later forward"):
        bufs.check("saved", gen, "cpu", "the test's saved bytes were")
    bufs.check("saved", bufs.generation("saved", "cpu"), "cpu", "the test's saved bytes were")


def test_nbytes_raises_with_the_librarys_reason():
    import marf_hip
    L = marf_hip.lib()
    g = marf_hip.grid_geometry(64, 512, 512, 256, 256, None)
    g.d_H = 1  # (planning reads no device memory)
    dims = [66, 256, 256, 256, 256, 3]
    ok = marf_hip.Net(dims, 16, marf_hip.MARF_BF16X3)
    n = marf_hip._nbytes(L.marf_warp_step_saved_bytes, ok.handle, ctypes.byref(g))
    assert n == L.marf_warp_step_saved_bytes(ok.handle, ctypes.byref(g)) > 0
    refused = marf_hip.Net(dims, 16, marf_hip.MARF_FP16X2)
    assert L.marf_warp_step_saved_bytes(refused.handle, ctypes.byref(g)) == 0
    with pytest.raises(RuntimeError, match="libmarf: .*fp16x2"):
        marf_hip._nbytes(L.marf_warp_step_saved_bytes, refused.handle, ctypes.byref(g))
    # the two Net methods on top of it (fp16x2 has no Gauss-Newton path either)
    for query in (lambda: refused.warp_step_saved_bytes(g), refused.gn_packed_bytes):
        msg = _message(query)
        assert msg == "libmarf: " + L.marf_last_error().decode() and len(msg) > len("libmarf: ")


def _message(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


def test_net_and_mask_net_share_one_handle_base():
    """The attributes tests and bench.py read, on both kinds of net, and the entry points named once."""
    import marf_hip
    n = marf_hip.Net([34, 64, 64, 3], 8, marf_hip.MARF_FP32)
    k = marf_hip.MaskNet(2, marf_hip.MARF_FP32)
    for net in (n, k):
        assert isinstance(net, marf_hip._NativeNet) and net.handle and net.param_count > 0 and net.packed_bytes > 0
        for name in (net.DESTROY, net.PACK, net.SAVED_BYTES, net.WORKSPACE_BYTES):
            assert name in marf_hip._SIGS, name
    assert n.step_kernel and n.layer_spans and (n.dims, n.L, n.dtype, n.skip) == ([34, 64, 64, 3], 8, marf_hip.MARF_FP32, [])
    assert (k.n_vocab, k.embed_dim, k.n_freqs, k.width, k.n_layers, k.in_dim) == (2, 128, 10, 256, 5, 426)
    g = marf_hip.grid_geometry(3, 36, 48, 18, 24, None)
    g.d_H = 1
    L = marf_hip.lib()
    assert n.saved_bytes(g) == L.marf_saved_bytes(n.handle, ctypes.byref(g)) > 0
    assert n.workspace_bytes(g) == L.marf_workspace_bytes(n.handle, ctypes.byref(g)) > 0
    assert k.saved_bytes(g) == L.marf_mask_saved_bytes(k.handle, ctypes.byref(g)) > 0
    assert k.workspace_bytes(g) == L.marf_mask_workspace_bytes(k.handle, ctypes.byref(g)) > 0
