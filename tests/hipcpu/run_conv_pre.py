"""TEST INFRASTRUCTURE -- run the operand-side BatchNorm cases of csrc/stp3_conv.hip (tests/conv_pre_cases.py) on CPU tensors
through libstp3hip_cpu.so (tests/hipcpu/build.py) and print the bit comparisons as JSON.

    python tests/hipcpu/run_conv_pre.py <libstp3hip_cpu.so> <case name> [<case name> ...]

Driver of tests/test_conv_pre_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import torch  # noqa: E402

from tests import conv_pre_cases as PC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_eval.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def main(lib_path, names):
    ops = setup(lib_path)
    cases = dict(PC.case_list())
    print('RESULT', json.dumps({name: PC.run_case(ops, 'cpu', **cases[name]) for name in names}))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2:])
