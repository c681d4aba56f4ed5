"""MI355X: the scratch owner under a real capture (stp3_amd/scratch.py).  A buffer that a captured graph was handed keeps its
address when a later, larger request on the same stream outgrows it.  Both tests assert ON THE HOST that the old buffer is
retained BEFORE they replay: a broken owner fails there and never replays into freed memory."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _retained_ptrs(dev):
    from stp3_amd import scratch
    return [t.data_ptr() for t in scratch.retained(dev)]


def test_captured_buffer_outlives_its_growth():
    """The owner alone, torch operators only."""
    from stp3_amd import scratch
    dev = torch.device('cuda', 0)
    name = 'test_scratch_gpu.t'
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        first = scratch.get(name, 4096, dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        inside = scratch.get(name, 4096, dev)
        inside.fill_(0x5a)
    torch.cuda.synchronize(dev)
    assert inside is first
    with torch.cuda.stream(stream):
        first.zero_()                                          # (the capture ran nothing: whatever fills it is the replay)
        grown = scratch.get(name, max(1 << 20, first.numel() + 1), dev)
    assert grown is not first and grown.data_ptr() != first.data_ptr() and grown.numel() >= 1 << 20
    assert first.data_ptr() in _retained_ptrs(dev)
    old = next(t for t in scratch.retained(dev) if t.data_ptr() == first.data_ptr())
    del first, inside
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert bool((old == 0x5a).all())


# the smallest shape the kernels take, and the smallest one whose statistics are not degenerate
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 8, 3, 3)])
def test_bn_act_replays_into_its_retained_scratch(shape):
    """One operator through the owner: ``ops.bn_act`` in training mode, captured at a small shape; an eager call on the same
    stream then needs more than the reduction scratch holds (N * 128 * 3 * C * 4 bytes against the 8 MiB floor)."""
    from stp3_amd import ops
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(5)
    c = shape[1]
    x = torch.randn(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(dev), torch.randn(c, generator=gen).to(dev)
    mean, var = torch.zeros(c, device=dev), torch.ones(c, device=dev)

    def small():
        return ops.bn_act(x, gamma, beta, mean, var, True, 0.1, 1e-5, act=ops.ACT_RELU)

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream), torch.no_grad():
        small()                                                # warm-up: allocates this stream's buffer
        captured_ws = ops._bn_workspace(shape[0], c, dev)[0]
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream), torch.no_grad():
        y_graph = small()
    torch.cuda.synchronize(dev)
    ptr = captured_ws.data_ptr()
    # an eager call that outgrows the buffer: N * C >= 5462 at the floor (N = 16, C = 512), more if an earlier user of this
    # pooled stream left a larger one
    big_c = 512
    big_n = max(16, captured_ws.numel() // (128 * 3 * big_c * 4) + 1)
    assert big_n * 128 * 3 * big_c * 4 > captured_ws.numel()
    del captured_ws
    with torch.cuda.stream(stream), torch.no_grad():
        xb = torch.randn(big_n, big_c, 2, 2, device=dev).contiguous(memory_format=torch.channels_last)
        ones, zeros = torch.ones(big_c, device=dev), torch.zeros(big_c, device=dev)
        ops.bn_act(xb, ones, zeros, zeros.clone(), ones.clone(), True, 0.1, 1e-5)
        new_ws = ops._bn_workspace(shape[0], c, dev)[0]
    torch.cuda.synchronize(dev)
    assert new_ws.data_ptr() != ptr and new_ws.numel() >= big_n * 128 * 3 * big_c * 4
    assert ptr in _retained_ptrs(dev)
    y_graph.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream), torch.no_grad():
        y_eager = small()
    torch.cuda.synchronize(dev)
    assert torch.isfinite(y_graph).all()
    assert torch.equal(y_graph, y_eager)
