"""Depth labels under the per-image augmentation on the MI355X: ``DepthLabeller`` with ``params``
(csrc/stp3_depth_augment.hip) against the plain routes (csrc/stp3_depth.hip) and against the torch statements, at the shape
bench.py trains -- B T = 12 frames x 6 cameras, 900 x 1600 -> 224 x 480 maps -> 28 x 60 labels, 35 000 points per frame.

    python scripts/time_depth_augment.py [--calls 20] [--repeats 5]

Per route the time per call by stream events after a warm-up, ``repeats`` windows of ``calls`` calls, the routes alternating
inside every repeat (median, and the spread min .. max over the repeats), all in one run:
  plain      the parent's routes: full map, labels through the winner table, stored float32 maps
  fixed      the augmented entries with ``sample(train=False)`` parameters (the same result as the plain routes)
  drawn      the augmented entries with parameters drawn inside the limits of scripts/time_augment.py: full map, labels,
             stored float32 maps -- each call builds its plan (tables on the host, one upload), as a training step would;
             ``drawn, prepared plan`` leaves that out
  torch      ``reference_*`` with the drawn parameters on the same GPU
  host       the host time of ``augment_plan`` per batch (perf_counter, the upload's enqueue included)
Outputs are compared before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from stp3_amd.config import perception_cfg  # noqa: E402
from stp3_amd.datas import DepthLabeller, ImageAugmenter  # noqa: E402
from tests import depth_cases as DC  # noqa: E402
from time_augment import LIMITS  # noqa: E402

FRAMES, CAMERAS = 12, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_depth_augment.py measures on the GPU; there is no other mode'
    cfg = perception_cfg(**{'LIFT.GT_DEPTH': True})
    lab, aug = DepthLabeller(cfg), ImageAugmenter(cfg, **LIMITS)
    case = DC.build_lidar('real', F=FRAMES, counts=(35000,) * FRAMES, repeats=2000 * FRAMES, crop=(0, 0, 480, 270))
    args = tuple(torch.from_numpy(case[k]).cuda() for k in ('points', 'offsets', 'steps')) + (DC.BEFORE,
            torch.from_numpy(case['intrinsics']).cuda())
    n = FRAMES * CAMERAS
    pairs = case['points'].shape[0] * CAMERAS
    maps32 = torch.rand(FRAMES, CAMERAS, 900, 1600, device='cuda') * 70.0
    fixed, drawn = aug.sample(n, train=False), aug.sample(n, torch.Generator().manual_seed(1))
    plans = {k: lab.augment_plan(drawn, 'cuda', **kw) for k, kw in (('full', dict(points=pairs)), ('labels', dict(labels=True, points=pairs)),
                                                                     ('maps', dict(maps=torch.float32)))}
    routes = {
        'plain: full map': lambda: lab.from_lidar(*args),
        'plain: labels, winner table': lambda: lab.from_lidar(*args, labels=True),
        'plain: stored float32 maps': lambda: lab.from_maps(maps32),
        'fixed parameters: full map': lambda: lab.from_lidar(*args, params=fixed),
        'fixed parameters: labels': lambda: lab.from_lidar(*args, params=fixed, labels=True),
        'fixed parameters: stored float32 maps': lambda: lab.from_maps(maps32, params=fixed),
        'drawn: full map': lambda: lab.from_lidar(*args, params=drawn),
        'drawn: labels': lambda: lab.from_lidar(*args, params=drawn, labels=True),
        'drawn: stored float32 maps': lambda: lab.from_maps(maps32, params=drawn),
        'drawn, prepared plan: full map': lambda: lab.from_lidar(*args, plan=plans['full']),
        'drawn, prepared plan: labels': lambda: lab.from_lidar(*args, labels=True, plan=plans['labels']),
        'drawn, prepared plan: stored float32 maps': lambda: lab.from_maps(maps32, plan=plans['maps']),
        'torch operators, drawn: full map': lambda: lab.reference_from_lidar(*args, params=drawn),
        'torch operators, drawn: labels': lambda: lab.reference_from_lidar(*args, params=drawn, labels=True),
        'torch operators, drawn: stored float32 maps': lambda: lab.reference_from_maps(maps32, params=drawn),
    }
    want = {k: routes[f'torch operators, drawn: {k}']() for k in ('full map', 'labels', 'stored float32 maps')}
    for name, fn in routes.items():
        kind = name.split(': ')[1]
        if name.startswith('drawn'):
            assert torch.equal(fn(), want[kind]), name
        if name.startswith('fixed'):
            assert torch.equal(fn(), routes['plain: ' + {'labels': 'labels, winner table'}.get(kind, kind)]()), name
    print(f'{FRAMES} frames x {CAMERAS} cameras, {case["points"].shape[0]} points, {int((want["full map"] > 0).sum())} non-zero of '
          f'{want["full map"].numel()} outputs (drawn parameters); the augmented entries equal the torch statements, and the plain '
          f'entries with the fixed parameters, exactly')
    for fn in routes.values():                                  # warm-up: code objects, allocator, tables
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
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
    host = {}
    for k, kw in (('full map', dict()), ('labels', dict(labels=True)), ('stored float32 maps', dict(maps=torch.float32))):
        host[k] = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                lab.augment_plan(drawn, 'cuda', like=plans[{'full map': 'full', 'labels': 'labels'}.get(k, 'maps')], **kw)
            host[k].append((time.perf_counter() - t0) / a.calls * 1e6)
            torch.cuda.synchronize()
    print(f'{torch.cuda.get_device_name(0)}; us per call, stream events, {a.repeats} windows of {a.calls} calls, routes alternating')
    for name, t in times.items():
        print(f'  {name:48s} median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}')
    print(f'host time of augment_plan(like=) per batch of {n} parameter sets (perf_counter, us)')
    for k, t in host.items():
        print(f'  {k:48s} median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}')


if __name__ == '__main__':
    main()
