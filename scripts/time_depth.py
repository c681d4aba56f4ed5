"""Depth labels on the MI355X: the routes of stp3_amd.datas.DepthLabeller (csrc/stp3_depth.hip) at the shape bench.py
trains -- B T = 12 frames x 6 cameras, 900 x 1600 -> 224 x 480 maps -> 28 x 60 labels, 35 000 points per frame (the 'real'
geometry of tests/depth_cases.py, 12 frames).

    python scripts/time_depth.py [--calls 20] [--repeats 5] [--kernels-only]

Per route the time per call by stream events after a warm-up, ``repeats`` windows of ``calls`` calls, the routes alternating
inside every repeat (median, and the spread min .. max over the repeats): the kernel routes (full map; labels only in one
launch with 1 .. 7 bands of label rows per image; labels through the winner table in global memory; project + from_pixels;
stored float32 maps) and the torch-operator path (``reference_*``) on the same GPU -- the parent of this work has no such
path, so that is the comparison.  Outputs of the routes are compared at this size before anything is timed.
``--kernels-only`` runs a few calls of the kernel routes and nothing else: the form to put under
``rocprofv3 --kernel-trace --stats`` (a run of its own).  The reference's own function on the host cores:
``python scripts/make_golden_depth.py --time``."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd.datas import DepthLabeller  # noqa: E402
from tests import depth_cases as DC  # noqa: E402

FRAMES = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_depth.py measures on the GPU; there is no other mode'
    case = DC.build_lidar('real', F=FRAMES, counts=(35000,) * FRAMES, repeats=2000 * FRAMES)
    lab = DepthLabeller(**DC.geometry(case))
    args = tuple(torch.from_numpy(case[k]).cuda() for k in ('points', 'offsets', 'steps')) + (DC.BEFORE,
            torch.from_numpy(case['intrinsics']).cuda())
    offsets = args[1]
    pixels, depth, keep = lab.project(*args)
    full = lab.from_lidar(*args)
    maps32 = torch.zeros(FRAMES, 6, 900, 1600, device='cuda')

    def banded(b):
        def run():
            lab.label_bands = b
            return lab.from_lidar(*args, labels=True, fused=True)
        return run
    routes = {
        'kernels: full map (scatter + resample)': lambda: lab.from_lidar(*args),
        'kernels: labels, winner table in global memory': lambda: lab.from_lidar(*args, labels=True),
        **{f'kernels: labels, one launch, >= {b} band(s) per image': banded(b) for b in (1, 2, 4, 7)},
        'kernels: project + from_pixels (full map)': lambda: lab.from_pixels(*lab.project(*args), offsets),
        'kernels: stored float32 maps -> full map': lambda: lab.from_maps(maps32),
    }
    if not a.kernels_only:
        routes.update({
            'torch operators: full map': lambda: lab.reference_from_lidar(*args),
            'torch operators: labels': lambda: lab.reference_from_lidar(*args, labels=True),
            'torch operators: stored float32 maps -> full map': lambda: lab.reference_from_maps(maps32),
        })
        want, want_labels = lab.reference_from_lidar(*args), lab.reference_from_lidar(*args, labels=True)
        assert torch.equal(full, want) and torch.equal(lab.class_ids(full), want_labels)
        assert torch.equal(lab.from_pixels(pixels, depth, keep, offsets), want)
        for name, fn in routes.items():
            if 'labels' in name:
                assert torch.equal(fn(), want_labels), name
        print(f'{FRAMES} frames x 6 cameras, {case["points"].shape[0]} points, {int(keep.sum())} kept (point, camera) pairs, '
              f'{int((want > 0).sum())} non-zero of {want.numel()} outputs; all routes equal the torch path exactly')
    for fn in routes.values():                                  # warm-up: code objects, allocator, tables
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if a.kernels_only:
        for fn in routes.values():
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        print(f'{a.calls} calls of each of {len(routes)} kernel routes done')
        return
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.calls):
                fn()
            end.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(end) / a.calls * 1e3)
    print(f'{torch.cuda.get_device_name(0)}; us per call, stream events, {a.repeats} windows of {a.calls} calls, routes alternating')
    for name, t in times.items():
        print(f'  {name:58s} median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}')


if __name__ == '__main__':
    main()
