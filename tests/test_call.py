"""sugar_amd._call: the pointer / stream / guard / CSR helpers every module shares, and `call`'s error path.  No GPU: the
CSR runs on CPU tensors and the one library call is refused by its argument check before anything is enqueued."""
import ctypes

import pytest
import torch

from sugar_amd import _call


def _brute_csr(flat, n_rows):
    rows = [[i for i, v in enumerate(flat) if v == r] for r in range(n_rows)]
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + len(r))
    return offsets, [i for r in rows for i in r]


def _old_csr(flat, n_rows):
    """the argsort / bincount / cumsum construction that mesh_bind carried before the helpers were shared"""
    flat = flat.reshape(-1).to(torch.int64)
    items = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=n_rows)[:n_rows]
    offsets = torch.zeros(n_rows + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32), items.to(torch.int32)


@pytest.mark.parametrize("flat,n_rows", [
    (torch.tensor([2, 0, 2, 2, 5, 0]), 7),                                            # rows 1, 3, 4 and 6 are empty
    (torch.zeros(0, dtype=torch.int64), 3),
    (torch.tensor([[0, 1, 2], [2, 1, 3], [3, 1, 0], [0, 2, 3]], dtype=torch.int32), 4),   # a faces tensor
])
def test_csr_matches_enumeration_and_the_old_construction(flat, n_rows):
    offsets, items = _call.csr(flat, n_rows)
    assert offsets.dtype == torch.int32 and items.dtype == torch.int32
    assert offsets.shape == (n_rows + 1,) and items.shape == (flat.numel(),)
    want_offsets, want_items = _brute_csr(flat.reshape(-1).tolist(), n_rows)
    assert offsets.tolist() == want_offsets and items.tolist() == want_items
    for r in range(n_rows):
        row = items[offsets[r]:offsets[r + 1]].tolist()
        assert row == sorted(row)
    old_offsets, old_items = _old_csr(flat, n_rows)
    assert torch.equal(offsets, old_offsets) and torch.equal(items, old_items)


def test_ptr():
    null = _call.ptr(None)
    assert isinstance(null, ctypes.c_void_p) and not null.value
    t = torch.arange(4.0)
    p = _call.ptr(t)
    assert isinstance(p, ctypes.c_void_p) and p.value == t.data_ptr()


def test_need_gpu_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call.need_gpu("x", a=torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call.need_gpu("x", a=None)


def test_call_surfaces_a_refusal(hip_lib, monkeypatch):
    """nx = 0 is refused by the entry point's dimension check before anything is enqueued: no device is touched"""
    monkeypatch.setattr(_call, "stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: __import__("contextlib").nullcontext())
    with pytest.raises(RuntimeError) as info:
        _call.call("sgr_marching_cubes_count", None, 0, 1, 1, None, 0.0, None, None)
    assert "sgr_marching_cubes_count" in str(info.value) and "must be positive" in str(info.value)
