"""Instance post-processing on the MI355X: stp3_amd.instance.predict_instance_segmentation_and_trajectories (csrc/
stp3_instance.hip) at the shape of nuscenes/Prediction.yml's validation batch (4 samples x 7 frames x 200 x 200) on the clean
and the crowded scene of tests/instance_cases.py.  Prints the time per call by stream events after warm-up and the number of
device operations of one call (torch profiler: kernels and memsets, the dtype conversions included); run under
``rocprofv3 --kernel-trace --stats`` it shows the two kernels' own times.

    python scripts/time_instance.py [calls]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd import instance  # noqa: E402
from tests import instance_cases as IC  # noqa: E402


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for name in ('clean', 'crowded'):
        case = IC.build(name, B=4, S=7)
        out = {k: torch.from_numpy(case[k]).cuda() for k in ('segmentation', 'instance_center', 'instance_offset', 'instance_flow')}
        ids = instance.predict_instance_segmentation_and_trajectories(out, check=True)       # first call: loads the code object
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            ids = instance.predict_instance_segmentation_and_trajectories(out)
        b.record()
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            instance.predict_instance_segmentation_and_trajectories(out)
            torch.cuda.synchronize()
        ops = [e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA for _ in range(e.count)]
        ours = sum('segment_kernel' in k or 'track_kernel' in k for k in ops)
        print(f'{name}: 4 x 7 x 200 x 200, {calls} calls, {a.elapsed_time(b) / calls * 1e3:.0f} us per call (stream events, launch '
              f'overhead included); one call = {len(ops)} device operations, {ours} of them stp3_instance kernels; ids up to '
              f'{int(ids.max())}')


if __name__ == '__main__':
    main()
