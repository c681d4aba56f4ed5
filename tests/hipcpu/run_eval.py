"""TEST INFRASTRUCTURE -- run csrc/stp3_eval.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and store the
states the scorer holds afterwards.

    python tests/hipcpu/run_eval.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_eval_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  The runs are those of tests/eval_cases.py (``run_semantic``, ``run_planning``, ``run_panoptic``) with an
``EvalScorer`` whose CPU tensors take the kernel route."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import eval_cases as EC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_instance.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def main(lib_path, out_path):
    setup(lib_path)
    out = {}
    out.update(EC.run_semantic('cpu'))
    out.update(EC.run_planning('cpu'))
    out.update(EC.run_panoptic('cpu'))
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
