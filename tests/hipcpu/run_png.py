"""TEST INFRASTRUCTURE -- run stp3_png_unfilter (csrc/stp3_png.hip) on CPU tensors through libstp3hip_cpu.so
(tests/hipcpu/build.py) and store what the kernel wrote.

    python tests/hipcpu/run_png.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_png_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Per supported case of tests/png_cases.py: ``<case>`` = what ``PngDecoder.unfilter_device`` wrote for the
scanlines ``PngDecoder.inflate`` produced, into an output with a guard ring of 77s (``<case>/guard``: whether it survived), and
``replay`` = static scanline / output tensors of the three-image case, launched, rewritten in place with the replay case and
launched again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import png_cases as PC  # noqa: E402

GUARD = 64


def setup(lib_path):
    """As tests/hipcpu/run_jpeg.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_png_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0


def guarded(shape):
    """A contiguous uint8 view of `shape` in the middle of a buffer of 77s, and the buffer."""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), 77, dtype=torch.uint8)
    return buf[GUARD:GUARD + size].view(shape), buf


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd.datas import PngDecoder, _png_shape
    fixture = PC.load()
    dec = PngDecoder(workers=2)
    out = {}
    for name in PC.SUPPORTED:
        batch = dec.inflate(PC.streams(fixture, name))
        assert batch.fallback == {} and len(batch.groups) == 1, name
        grp = batch.groups[0]
        held, buf = guarded((len(grp.indices),) + _png_shape(grp.geometry))
        dec.unfilter_device(grp.geometry, grp.rows, held)
        out[name] = held.numpy().copy()
        out[f'{name}/guard'] = np.array(bool((buf[:GUARD] == 77).all() and (buf[-GUARD:] == 77).all()))
    first, second = (dec.inflate(PC.streams(fixture, k)) for k in ('three_images', 'three_images_replay'))
    grp = first.groups[0]
    rows = grp.rows.clone()
    held = torch.full((3,) + _png_shape(grp.geometry), 77, dtype=torch.uint8)
    dec.unfilter_device(grp.geometry, rows, held)
    assert np.array_equal(held.numpy(), out['three_images'])
    rows.copy_(second.groups[0].rows)
    dec.unfilter_device(grp.geometry, rows, held)
    out['replay'] = held.numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
