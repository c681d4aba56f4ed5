"""TEST INFRASTRUCTURE -- run csrc/stp3_sampler.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) on the
cases of tests/golden/sampler.npz and store what the kernel wrote.

    python tests/hipcpu/run_sampler.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_sampler_cpu.py (which holds the checks).  Per case ``c<i>_``: ``unsorted`` (sort = 0), ``sorted`` and
``order`` (sort = 1) of stp3_amd.ops_plan.sample_trajectories on its GPU route; ``batch_*``: the three 1 800-row cases in one
launch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_case.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
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
    from stp3_amd import ops_plan
    from tests import helpers as H
    g = H.load('sampler.npz')
    out = {}
    cases = sorted(int(k[1:-7]) for k in g.files if k.endswith('_params'))
    for i in cases:
        v0, kappa, m, nf = g[f'c{i}_params']
        args = (torch.tensor([v0]), torch.tensor([kappa]), int(nf), int(m))
        draws = torch.from_numpy(g[f'c{i}_draws'])[None]
        out[f'c{i}_unsorted'] = ops_plan.sample_trajectories(*args, draws=draws, sort=False)[0].numpy()
        rows, order = ops_plan.sample_trajectories(*args, draws=draws, sort=True, return_order=True)
        out[f'c{i}_sorted'], out[f'c{i}_order'] = rows[0].numpy(), order[0].numpy()
    same = [i for i in cases if tuple(g[f'c{i}_params'][2:]) == tuple(g[f'c{cases[0]}_params'][2:])]
    p = np.stack([g[f'c{i}_params'] for i in same])
    rows, order = ops_plan.sample_trajectories(torch.from_numpy(p[:, 0].copy()), torch.from_numpy(p[:, 1].copy()), int(p[0, 3]),
                                               int(p[0, 2]), draws=torch.from_numpy(np.stack([g[f'c{i}_draws'] for i in same])),
                                               sort=True, return_order=True)
    out['batch_cases'], out['batch_sorted'], out['batch_order'] = np.array(same), rows.numpy(), order.numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
