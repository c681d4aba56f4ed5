"""The metric update of one validation sample on the MI355X: the three metric classes of stp3_amd/metrics.py behind their
``argmax`` / ``logical_or`` front, as ``TrainingModule.shared_step`` runs them, against ``EvalScorer.update`` (stp3_amd/evaluation.py;
csrc/stp3_eval.hip) on the same inputs, in one process, alternating, after warm-up.  B = 1, S = 7, receptive field 3, 200 x 200,
pedestrian head and two hd-map elements, instance and planning on.  Prints the median and the spread of the wall time of
one update up to a final synchronise, and per side the device operations (torch profiler: kernels, copies, memsets) and the
host synchronisations (torch's sync debug mode: every call that waits for the device warns) of one update.

    python scripts/time_eval.py [repeats]
"""
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd.config import perception_cfg  # noqa: E402
from stp3_amd.evaluation import EvalScorer  # noqa: E402
from stp3_amd.metrics import IntersectionOverUnion, PanopticMetric, PlanningMetric  # noqa: E402
from tests import eval_cases as EC  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import instance_cases as IC  # noqa: E402
from tests.test_planning_cpu import PLANNING  # noqa: E402


def inputs():
    updates, labels = EC.planning_inputs('cuda')
    labels = {k: v[:1].contiguous() for k, v in labels.items()}
    rs = np.random.RandomState(500)
    output = {'segmentation': torch.from_numpy(EC._logits(rs, (1, 7, 2, 200, 200))).cuda().to(torch.bfloat16),
              'pedestrian': torch.from_numpy(EC._logits(rs, (1, 7, 2, 200, 200))).cuda().to(torch.bfloat16),
              'hdmap': torch.from_numpy(EC._logits(rs, (1, 4, 200, 200))).cuda().to(torch.bfloat16)}
    labels['hdmap'] = torch.from_numpy(EC._labels(rs, (1, 2, 200, 200), 2)).cuda()
    labels['instance'] = torch.from_numpy(IC.build('clean')['gt_instance'][:1]).cuda()
    labels['gt_trajectory'] = updates[0][1][:1].contiguous()
    instance = torch.from_numpy(H.load('instance.npz')['clean/tracked'][:1].astype(np.int64)).cuda()
    return output, labels, updates[0][0][:1].contiguous(), instance


class Classes:
    """trainer.py:160-189: the evaluation branch of ``shared_step`` behind the forward, the planner's trajectory given."""

    def __init__(self, cfg):
        self.rf = int(cfg.TIME_RECEPTIVE_FIELD)
        self.vehicle, self.pedestrian = IntersectionOverUnion(2).cuda(), IntersectionOverUnion(2).cuda()
        self.hdmap = [IntersectionOverUnion(2, absent_score=1).cuda() for _ in range(2)]
        self.panoptic, self.planning = PanopticMetric(2).cuda(), PlanningMetric(cfg, cfg.N_FUTURE_FRAMES).cuda()

    @torch.no_grad()
    def update(self, output, labels, final_traj, instance):
        rf = self.rf
        seg_pred = torch.argmax(output['segmentation'].detach(), dim=2, keepdim=True)
        self.vehicle(seg_pred[:, rf - 1:], labels['segmentation'][:, rf - 1:])
        ped_pred = torch.argmax(output['pedestrian'].detach(), dim=2, keepdim=True)
        self.pedestrian(ped_pred[:, rf - 1:], labels['pedestrian'][:, rf - 1:])
        for i in range(2):
            hd_pred = torch.argmax(output['hdmap'][:, 2 * i:2 * (i + 1)].detach(), dim=1, keepdim=True)
            self.hdmap[i](hd_pred, labels['hdmap'][:, i:i + 1])
        self.panoptic(instance[:, rf - 1:], labels['instance'][:, rf - 1:])
        occupancy = seg_pred.bool() | ped_pred.bool()                                   # (the planner's input: part of the front)
        truth = labels['segmentation'][:, rf:].squeeze(2).bool() | labels['pedestrian'][:, rf:].squeeze(2).bool()
        self.planning(final_traj, labels['gt_trajectory'][:, 1:], truth)
        return occupancy


def census(update, args):
    """(device operations, host synchronisations) of one update."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        update(*args)
        torch.cuda.synchronize()
    ops = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            update(*args)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return ops, sum('synchroniz' in str(w.message).lower() for w in caught)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    cfg = perception_cfg(**{**PLANNING, 'INSTANCE_SEG.ENABLED': True})
    args = inputs()
    sides = {'metric classes': Classes(cfg).update, 'EvalScorer': EvalScorer(cfg, 'cuda').update}
    times = {k: [] for k in sides}
    for r in range(5 + repeats):
        for name, update in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            update(*args)
            torch.cuda.synchronize()
            if r >= 5:
                times[name].append((time.perf_counter() - t0) * 1e6)
    print(f'one update, B 1, S 7, receptive field 3, 200 x 200, 2 hd-map elements, instance and planning on; {repeats} repeats, '
          f'alternating, after 5 warm-up rounds; wall time to a final synchronise')
    for name, update in sides.items():
        t = sorted(times[name])
        ops, syncs = census(update, args)
        print(f'{name:>15}: median {statistics.median(t):8.0f} us, min {t[0]:8.0f}, max {t[-1]:8.0f}, quartiles '
              f'{t[len(t) // 4]:.0f} .. {t[3 * len(t) // 4]:.0f}; {ops} device operations, {syncs} host synchronisations per update')
    a, b = statistics.median(times['metric classes']), statistics.median(times['EvalScorer'])
    print(f'ratio of the medians (metric classes / EvalScorer): {a / b:.2f}')


if __name__ == '__main__':
    main()
