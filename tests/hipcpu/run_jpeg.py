"""TEST INFRASTRUCTURE -- run stp3_jpeg_reconstruct (csrc/stp3_jpeg.hip) on CPU tensors through libstp3hip_cpu.so
(tests/hipcpu/build.py) and store what the kernel wrote.

    python tests/hipcpu/run_jpeg.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_jpeg_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Per case of tests/jpeg_cases.py: ``<case>`` = what ``JpegDecoder()(streams, device)`` returned with the kernel
behind it (the unsupported streams through the fallback), and ``replay`` = static coefficient / table / output tensors of the
N = 3 case, launched, rewritten in place with the replay case and launched again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import jpeg_cases as JC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_augment.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_jpeg_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd.datas import JpegDecoder
    fixture = JC.load()
    dec = JpegDecoder(workers=2)
    out = {}
    for name in JC.CASES:
        out[name] = dec(JC.streams(fixture, name), 'cpu').numpy()
    first, second = (dec.entropy(JC.streams(fixture, k)) for k in ('s420_32x48_n3', 's420_32x48_n3_replay'))
    grp = first.groups[0]
    coef, quant = grp.coef.clone(), grp.quant.clone()
    held = torch.full((3, 32, 48, 3), 77, dtype=torch.uint8)
    dec.reconstruct_device(grp.geometry, coef, quant, held)
    assert np.array_equal(held.numpy(), out['s420_32x48_n3'])
    coef.copy_(second.groups[0].coef)
    quant.copy_(second.groups[0].quant)
    dec.reconstruct_device(grp.geometry, coef, quant, held)
    out['replay'] = held.numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
