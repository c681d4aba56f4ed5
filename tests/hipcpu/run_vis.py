"""TEST INFRASTRUCTURE -- run csrc/stp3_vis.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and store what
the kernels wrote.

    python tests/hipcpu/run_vis.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_visualisation_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from
the environment.  Per case of visualisation_cases, sample and head dtype: ``<name>/<sample>/<f32|bf16>``, the video FOLLOWED BY
a guard band of GUARD bytes (value FILL) that the kernels must leave alone; ``full/0/unaligned``: the same video painted one byte
into the buffer (FILL, video, guard), which takes the byte stores at an even W."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import visualisation_cases as VC  # noqa: E402

GUARD, FILL = 64, 0xA5


def setup(lib_path):
    """As tests/hipcpu/run_depth.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_vis_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd import visualisation as V
    out = {}
    for name, c in VC.CASES.items():
        cfg = VC.cfg_of(name)
        shape = (1, c['T'], 3, 7 * c['H'], 2 * c['W'])
        n = int(np.prod(shape))
        for tag, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
            labels, output, consistent = VC.stored(name, head_dtype=dtype)
            for sample in c['samples']:
                runs = [(f'{name}/{sample}/{tag}', 0)] + ([('full/0/unaligned', 1)] if (name, sample, tag) == ('full', 0, 'f32') else [])
                for key, lead in runs:
                    buf = torch.full((lead + n + GUARD,), FILL, dtype=torch.uint8)
                    got = V.visualise_output(labels, output, cfg, sample=sample, consistent_instance_seg=consistent,
                                             out=buf[lead:lead + n].view(shape))
                    assert got.data_ptr() == buf.data_ptr() + lead
                    out[key] = buf.numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
