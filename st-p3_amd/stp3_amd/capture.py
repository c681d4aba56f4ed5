"""Warm-up and capture of a hipGraph, as ``graph.GraphedTrainStep`` and the engines of ``inference`` do it.

Warm-up AND capture run on one private stream: scratch buffers are per stream (``scratch.py`` states the contract), so the
warm-up grows every buffer the body uses and the capture names addresses that stay."""
import torch


def warm_up(body, device, n, log=None):
    """Run ``body()`` ``n`` times on a new stream that waits for the current one and is waited for; returns the stream."""
    stream = torch.cuda.Stream(device=device)
    cur = torch.cuda.current_stream(device)
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        for i in range(n):
            body()
            if log is not None:
                log(f'graph: eager warm-up {i} done')
    cur.wait_stream(stream)
    torch.cuda.synchronize(device)
    return stream


def capture(body, stream, device, capture_error_mode='global'):
    """Capture ``body()`` on ``stream`` (the one ``warm_up`` returned); returns (graph, what ``body`` returned)."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode=capture_error_mode):
        result = body()
    torch.cuda.synchronize(device)
    return graph, result
