"""CPU: the owner of the operators' scratch buffers (stp3_amd/scratch.py) -- keys, floors, growth and the retire rule, on
plain CPU tensors with the "is the stream capturing" predicate patched."""
import gc
import weakref

import pytest
import torch

from stp3_amd import scratch

CPU = torch.device('cpu')
_REAL_CAPTURING = scratch.capturing


@pytest.fixture(autouse=True)
def fresh_owner(monkeypatch):
    monkeypatch.setattr(scratch, '_BUFFERS', {})
    monkeypatch.setattr(scratch, '_RETAINED', [])
    monkeypatch.setattr(scratch, 'capturing', lambda: False)


def _retained_ptrs(device=CPU):
    return [t.data_ptr() for t in scratch.retained(device)]


def test_same_request_same_tensor():
    a = scratch.get('a', 1000, CPU)
    assert a.dtype == torch.uint8 and a.numel() >= 1000 and a.device == CPU
    assert scratch.get('a', 1000, CPU) is a
    assert scratch.get('a', 10, CPU) is a
    assert scratch.get('a', 0, CPU) is a


def test_names_are_distinct_buffers():
    a = scratch.get('a', 256, CPU)
    b = scratch.get('b', 256, CPU)
    assert a is not b and a.data_ptr() != b.data_ptr()
    assert scratch.get('a', 256, CPU) is a and scratch.get('b', 256, CPU) is b


def test_floor_on_first_allocation_and_on_growth():
    a = scratch.get('a', 100, CPU, floor=4096)
    assert a.numel() == 4096
    assert scratch.get('a', 4096, CPU, floor=4096) is a
    b = scratch.get('a', 4097, CPU, floor=4096)                # past the floor: the exact size
    assert b is not a and b.numel() == 4097
    c = scratch.get('c', 100, CPU)
    assert c.numel() == 100
    d = scratch.get('c', 200, CPU, floor=1 << 16)              # a growth below the floor allocates the floor
    assert d is not c and d.numel() == 1 << 16


def test_growth_drops_a_buffer_no_capture_has_seen():
    old = weakref.ref(scratch.get('a', 1 << 12, CPU))
    new = scratch.get('a', 1 << 16, CPU)
    gc.collect()
    assert old() is None
    assert new.numel() == 1 << 16 and scratch.retained(CPU) == []


def test_growth_retains_a_buffer_handed_out_under_capture(monkeypatch):
    first = scratch.get('a', 1 << 12, CPU)                     # allocated outside the capture (the warm-up) ...
    monkeypatch.setattr(scratch, 'capturing', lambda: True)
    assert scratch.get('a', 1 << 12, CPU) is first             # ... handed out inside it
    monkeypatch.setattr(scratch, 'capturing', lambda: False)
    ptr, old = first.data_ptr(), weakref.ref(first)
    del first
    new = scratch.get('a', 1 << 16, CPU)
    gc.collect()
    assert new.data_ptr() != ptr and new.numel() == 1 << 16
    assert old() is not None and ptr in _retained_ptrs()
    # the mark belongs to the buffer, not to the name: the new one was never captured and is dropped when outgrown
    newer_old = weakref.ref(new)
    del new
    scratch.get('a', 1 << 17, CPU)
    gc.collect()
    assert newer_old() is None and _retained_ptrs() == [ptr]


def test_buffer_allocated_under_capture_is_retained(monkeypatch):
    monkeypatch.setattr(scratch, 'capturing', lambda: True)
    ptr = scratch.get('a', 1 << 12, CPU).data_ptr()
    monkeypatch.setattr(scratch, 'capturing', lambda: False)
    scratch.get('a', 1 << 16, CPU)
    assert ptr in _retained_ptrs()


class _Stream:
    """What the dry-run drivers put in the place of a stream (tests/model_trace.py): an object with a handle."""

    def __init__(self, handle=0):
        self.cuda_stream = handle


def test_stream_objects_of_one_handle_share_the_key(monkeypatch):
    """``torch.cuda.Stream()`` wraps round its pool of 32: the 33rd stream object carries the handle of the first."""
    gpu = torch.device('cuda', 0)
    current = [_Stream(0x1000)]
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: current[0])
    k_first = scratch.key(gpu)
    current[0] = _Stream(0x2000)
    k_other = scratch.key(gpu)
    current[0] = _Stream(0x1000)                               # another object, the same handle
    assert scratch.key(gpu) == k_first and hash(scratch.key(gpu)) == hash(k_first)
    assert k_other != k_first
    assert scratch.key(torch.device('cuda', 1)) != k_first


def test_streams_key_the_buffers(monkeypatch):
    """The owner end to end with a handle in the key: CPU tensors stand in for the device's (``torch.empty`` patched)."""
    gpu = torch.device('cuda', 0)
    current = [_Stream(0x1000)]
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: current[0])
    empty = torch.empty
    monkeypatch.setattr(torch, 'empty', lambda n, dtype, device: empty(n, dtype=dtype))
    a = scratch.get('a', 512, gpu)
    current[0] = _Stream(0x2000)
    b = scratch.get('a', 512, gpu)
    current[0] = _Stream(0x1000)
    assert b is not a and scratch.get('a', 512, gpu) is a
    # the wrap-around case: the first engine's graph holds ``a``; the 33rd engine asks its stream for more
    monkeypatch.setattr(scratch, 'capturing', lambda: True)
    scratch.get('a', 512, gpu)
    monkeypatch.setattr(scratch, 'capturing', lambda: False)
    current[0] = _Stream(0x1000)
    grown = scratch.get('a', 4096, gpu)
    assert grown is not a and a.data_ptr() in [t.data_ptr() for t in scratch._RETAINED]


def test_non_cuda_device_with_the_dry_run_patches(monkeypatch):
    """tests/model_trace.py: ``torch.cuda.current_stream`` returns a stand-in; a CPU device never asks for it."""
    def no_stream(*a, **k):
        raise AssertionError('a non-CUDA device has no stream in its key')
    monkeypatch.setattr(torch.cuda, 'current_stream', no_stream)
    assert scratch.key('cpu') == CPU
    a = scratch.get('a', 128, 'cpu')
    assert a.device == CPU and scratch.get('a', 128, CPU) is a
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: _Stream())
    assert scratch.get('a', 128, 'cpu') is a
    assert scratch.get('a', 256, 'cpu', floor=1024).numel() == 1024


def test_real_predicate_outside_a_capture():
    """The unpatched predicate: no GPU, or a GPU whose current stream is not capturing -- False either way."""
    assert _REAL_CAPTURING() is False
