"""Trajectory sampler on the MI355X: stp3_traj_sample (csrc/stp3_sampler.hip) at the sizes of nuscenes/Planning.yml (batch 4,
1 800 trajectories, 6 future frames).  Prints the time per call by stream events; run under
``rocprofv3 --kernel-trace --stats`` it shows the kernel's own time and that a call is exactly one dispatch
(``calls`` launches of traj_sample_kernel, nothing else besides the one torch.rand fill of the draws).

    python scripts/time_sampler.py [batch] [calls]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd import ops_plan  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    M, T = 1800, 6
    v0 = torch.tensor([5.0, 8.3, 0.0, 12.0] * B, dtype=torch.float64)[:B].cuda()
    kappa = torch.tensor([0.0, 0.05, -0.3, 0.004] * B, dtype=torch.float64)[:B].cuda()
    draws = torch.rand(B, 3 * M + 2 * (M * 4 // 5), dtype=torch.float64, device='cuda', generator=torch.Generator('cuda').manual_seed(0))
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = ops_plan.sample_trajectories(v0, kappa, T, M, draws=draws)                         # first call: loads the code object
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls - 1):
        out = ops_plan.sample_trajectories(v0, kappa, T, M, draws=draws)
    b.record()
    torch.cuda.synchronize()
    print(f'B={B} M={M} n_future={T}: {calls} calls of stp3_traj_sample, {a.elapsed_time(b) / (calls - 1) * 1e3:.1f} us per call '
          f'(stream events, launch overhead included); output {tuple(out.shape)} finite: {bool(torch.isfinite(out).all())}')


if __name__ == '__main__':
    main()
