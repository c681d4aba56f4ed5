"""TEST INFRASTRUCTURE -- run csrc/stp3_depth.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and
store what the kernels wrote.

    python tests/hipcpu/run_depth.py <libstp3hip_cpu.so> <out.npz> [real]

Driver of tests/test_depth_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Per lidar case of depth_cases (without ``real``: every case but 'real'; with it: that case alone):
``<name>/pixels``, ``/depth``, ``/keep`` of DepthLabeller.project, ``/from_pixels`` (float64 output), ``/from_lidar`` (float32),
``/labels`` (the one-launch labels kernel, one band), ``/labels_banded`` (two bands), ``/labels_table`` (labels through the
winner table in global memory).  Per map case: ``<name>/depths`` and ``/labels``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import depth_cases as DC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_sampler.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    # the test builds csrc/stp3_depth.hip alone (seconds instead of minutes): bind its entries only
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_depth_') and k != 'stp3_depth_softmax'}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def cloud(case):
    return (torch.from_numpy(case['points']), torch.from_numpy(case['offsets']), torch.from_numpy(case['steps']), DC.BEFORE,
            torch.from_numpy(case['intrinsics']))


def main(lib_path, out_path, real=False):
    setup(lib_path)
    from stp3_amd.datas import DepthLabeller
    out = {}
    for name in (['real'] if real else [n for n in DC.LIDAR_CASES if n != 'real']):
        case = DC.build_lidar(name)
        lab = DepthLabeller(**DC.geometry(case))
        args = cloud(case)
        pixels, depth, keep = lab.project(*args)
        out[f'{name}/pixels'], out[f'{name}/depth'], out[f'{name}/keep'] = pixels.numpy(), depth.numpy(), keep.numpy()
        out[f'{name}/from_pixels'] = lab.from_pixels(pixels, depth, keep, args[1], out_dtype=torch.float64).numpy()
        out[f'{name}/from_lidar'] = lab.from_lidar(*args).numpy()
        out[f'{name}/labels'] = lab.from_lidar(*args, labels=True, fused=True).numpy()
        lab.label_bands = 2
        out[f'{name}/labels_banded'] = lab.from_lidar(*args, labels=True, fused=True).numpy()
        out[f'{name}/labels_table'] = lab.from_lidar(*args, labels=True).numpy()
    if not real:
        for name in DC.MAP_CASES:
            case = DC.build_map(name)
            lab = DepthLabeller(**DC.geometry(case))
            maps = torch.from_numpy(case['maps'])
            out[f'{name}/depths'] = lab.from_maps(maps, out_dtype=torch.float64).numpy()
            out[f'{name}/labels'] = lab.from_maps(maps, labels=True).numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == 'real')
