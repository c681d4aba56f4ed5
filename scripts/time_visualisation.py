"""The training video on the MI355X: what ``visualise_output`` costs once per VIS_INTERVAL steps, on the two routes, at the shape
a Prediction run logs -- B = 4 samples of 200 x 200 cells, T = 7 frames, every head on (sample 0 is rendered, as in the reference).

    python scripts/time_visualisation.py [--runs 30]

  host route    what the reference does: the tensors are pulled to the host (``.cpu()`` copies, each a synchronisation of the
                stream) and coloured with numpy -- ``visualisation.visualise_output_reference`` on the copies; the copies are
                inside the timed region
  kernel route  ``visualisation.visualise_output`` on the GPU tensors: ``stp3_vis_render`` (csrc/stp3_vis.hip), two launches,
                the video stays on the device; timed to the end of the kernels (a synchronise closes the timed region, it is
                not part of the route)
The instance ids of the predictions are given to both routes (the post-processing is neither route's work).  The routes
alternate, ``runs`` times, after a warm-up; per route the median and the spread (min .. max) of the host clock, and for the
kernel route the stream-event time of the render alone.  The tensors pulled and the host synchronisations are counted in an
untimed run by wrapping ``Tensor.cpu`` / ``Tensor.item`` / ``torch.cuda.synchronize``.  The two videos are compared under the rule
of tests/visualisation_cases.py before anything is timed.  No threshold: this records a cost, it does not judge one."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd import visualisation as V  # noqa: E402
from tests import visualisation_cases as VC  # noqa: E402

B, T, H, W = 4, 7, 200, 200


def count_host_traffic(fn):
    """{name: calls} of Tensor.cpu / Tensor.item / torch.cuda.synchronize during ``fn()``."""
    counts, saved = {}, []

    def wrap(owner, attr):
        inner = getattr(owner, attr)
        saved.append((owner, attr, inner))

        def counting(*args, **kwargs):
            counts[attr] = counts.get(attr, 0) + 1
            return inner(*args, **kwargs)
        setattr(owner, attr, counting)
    wrap(torch.Tensor, 'cpu')
    wrap(torch.Tensor, 'item')
    wrap(torch.cuda, 'synchronize')
    try:
        fn()
    finally:
        for owner, attr, inner in saved:
            setattr(owner, attr, inner)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_visualisation.py measures on the GPU; there is no other mode'
    host_labels, host_output, host_ids, cfg = VC.random_case(B, T, H, W, seed=5)
    labels, output = ({k: v.cuda() for k, v in d.items()} for d in (host_labels, host_output))
    ids = host_ids.cuda()
    out = torch.empty(1, T, 3, 7 * H, 2 * W, dtype=torch.uint8, device='cuda')

    def host_route():
        pulled_l = {k: v.cpu() for k, v in labels.items()}
        pulled_o = {k: v.cpu() for k, v in output.items()}
        return V.visualise_output_reference(pulled_l, pulled_o, cfg, consistent_instance_seg=ids.cpu())

    def kernel_route():
        return V.visualise_output(labels, output, cfg, consistent_instance_seg=ids, out=out)

    want = host_route().numpy()
    share = VC.compare_videos(kernel_route().cpu().numpy(), want, VC.flow_sources(host_labels, host_output, 0),
                              VC.planning_panels(host_labels, host_output, 0, cfg), 'kernel route against host route')
    print(f'B = {B}, T = {T}, {H} x {W} cells: video {tuple(out.shape)} uint8, {out.numel()} bytes; the routes agree under the rule of '
          f'tests/visualisation_cases.py ({share:.3%} of a flow panel fragile at most)')
    print(f'host route:   {count_host_traffic(host_route)} calls (every .cpu() of a device tensor waits for the stream)')
    print(f'kernel route: {count_host_traffic(kernel_route) or "no"} such calls; 2 launches (vis_prepare_kernel, vis_paint_kernel)')
    for _ in range(3):
        host_route()
        kernel_route()
    torch.cuda.synchronize()
    times = {'host route': [], 'kernel route': [], 'kernel route, stream events': []}
    for _ in range(a.runs):
        t0 = time.perf_counter()
        host_route()
        times['host route'].append((time.perf_counter() - t0) * 1e6)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        kernel_route()
        end.record()
        torch.cuda.synchronize()
        times['kernel route'].append((time.perf_counter() - t0) * 1e6)
        times['kernel route, stream events'].append(start.elapsed_time(end) * 1e3)
    print(f'{torch.cuda.get_device_name(0)}; us per video, {a.runs} runs, the routes alternating')
    for name, t in times.items():
        print(f'  {name:30s} median {statistics.median(t):10.1f}   min {min(t):10.1f}   max {max(t):10.1f}')


if __name__ == '__main__':
    main()
