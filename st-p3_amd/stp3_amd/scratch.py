"""The one owner of the operators' scratch buffers: grow-on-demand ``uint8`` device buffers, one per name, device AND stream.

Per stream, because operators of independent branches are queued on different HIP streams (the encoder's two heads, the weight
gradients beside the data gradients) and must not share scratch.  Per name, because an operator may hold several at once (the
fused convolution + BatchNorm: 'bn' and 'fused').

THE CAPTURE CONTRACT.  A captured graph (``capture.py``) names the addresses of the buffers its operators were handed, for as
long as it is replayed.  Two rules keep those addresses good:
  * warm-up and capture run on ONE private stream (``capture.warm_up`` / ``capture.capture``), so the warm-up grows every buffer
    of that stream to its final size and the capture allocates none;
  * a buffer that was handed out while its stream was capturing is never freed: when a later, larger request outgrows it, it
    moves to ``retained``.  ``torch.cuda.Stream()`` hands out its streams round-robin from a pool of 32 per device, so the 33rd
    engine of a process shares the key of the first -- its larger request must not free what the first one's graph replays into.
A buffer no capture has seen is dropped when it is outgrown.
"""
import torch

_BUFFERS = {}          # key -> [tensor, handed out under capture]
_RETAINED = []         # outgrown buffers a captured graph may still name: never freed


def key(device):
    """What distinguishes the scratch of two callers: the device and, on a GPU, the handle of the current stream (the handle,
    not the stream object: two objects of one pooled stream share their scratch)."""
    device = torch.device(device)
    if device.type != 'cuda':
        return device
    return (device, torch.cuda.current_stream().cuda_stream)


def capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def get(name, nbytes, device, floor=0):
    """The buffer ``name`` of ``device`` and the current stream, at least ``nbytes`` long (``max(nbytes, floor)`` when it has to
    be allocated)."""
    k = (name, key(device))
    entry = _BUFFERS.get(k)
    if entry is None or entry[0].numel() < nbytes:
        if entry is not None and entry[1]:
            _RETAINED.append(entry[0])
        entry = _BUFFERS[k] = [torch.empty(max(nbytes, floor), dtype=torch.uint8, device=torch.device(device)), False]
    if capturing():
        entry[1] = True
    return entry[0]


def retained(device):
    """The retained buffers of ``device`` (for tests)."""
    device = torch.device(device)
    return [t for t in _RETAINED if t.device.type == device.type and device.index in (None, t.device.index)]
