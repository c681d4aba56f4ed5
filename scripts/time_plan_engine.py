"""Time one closed-loop tick -- forward AND planner -- as a caller runs it today against the one-launch planner (``Planning.drive``).

    python scripts/time_plan_engine.py [--legs baseline,drive] [--batches 1,4] [--calls 200] [--repeats 5]
                                       [--out profiles/plan_drive_timing.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \
        python scripts/time_plan_engine.py --trace baseline|drive --batch 1 --calls K

* ``baseline``: the engine's replay of the forward, then the eager statements of evaluate.py:96-132 -- two ``argmax``, a
  ``logical_or``, ``model.planning(...)`` -- under the same autocast.
* ``drive``: the same replay, then ``ops_plan.plan_scene`` and ``Planning.drive`` (stp3_plan_scene, reduce_channel, stp3_plan_drive).
(profiles/plan_engine_timing.txt holds the measurement of a third variant, that tail CAPTURED into the engine's graph, which did
not beat the baseline and was not merged.)
Configuration: nuscenes/Planning.yml's planner sizes (N = 1 800 candidates, T = 6 future steps, receptive field 3: nine frames)
at B = 1 and B = 4, seeded random weights, bf16 autocast.  Every call ends in a device synchronise (the trajectory is what the
caller waits for).  Reported per leg and batch: the median wall time per call of ``calls`` calls after warm-up, ``repeats`` times
(median and min .. max of the repeats); the TAIL alone after a synchronise: host issue time, first-to-last-kernel time and the
device kernels it launches (torch.profiler).  ``--trace`` runs warm-up and K calls of one leg, nothing else."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'st-p3_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

PLANNING = {'N_FUTURE_FRAMES': 6, 'PLANNING.ENABLED': True, 'PLANNING.SAMPLE_NUM': 1800, 'PROBABILISTIC.ENABLED': False,
            'SEMANTIC_SEG.PEDESTRIAN.ENABLED': True, 'SEMANTIC_SEG.HDMAP.ENABLED': True, 'INSTANCE_FLOW.ENABLED': False,
            'INSTANCE_SEG.ENABLED': False}
COMMANDS = ['LEFT', 'FORWARD', 'RIGHT', 'FORWARD']


def build(b):
    import warnings
    import torch
    from stp3_amd import synthetic
    from stp3_amd.config import perception_cfg
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    torch.manual_seed(0)
    cfg = perception_cfg(**PLANNING)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = to_channels_last(STP3(cfg).eval().cuda())
    batch = synthetic.make_batch(batch=b, seq=9, seed=1, with_labels=False, planning=(6, 1800))
    batch['command'] = COMMANDS[:b]
    return model, batch


def forward_inputs(batch):
    return batch['image'].cuda(), batch['intrinsics'], batch['extrinsics'], batch['future_egomotion']


def eager_tail(model, out, trajs, commands, target):
    """evaluate.py:96-132 on the forward's outputs."""
    import torch
    n_present = model.receptive_field
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        seg = torch.argmax(out['segmentation'].detach(), dim=2, keepdim=True)
        ped = torch.argmax(out['pedestrian'].detach(), dim=2, keepdim=True)
        occupancy = torch.logical_or(seg, ped)
        _, final = model.planning(cam_front=out['cam_front'].detach(), trajs=trajs[:, :, 1:], gt_trajs=None,
                                  cost_volume=out['costvolume'][:, n_present:].detach(),
                                  semantic_pred=occupancy[:, n_present:].squeeze(2), hd_map=out['hdmap'].detach(),
                                  commands=commands, target_points=target)
    return final


def drive_tail(model, out, trajs, codes, target):
    """The same step through the one-launch planner."""
    import torch
    from stp3_amd import ops_plan
    n_present = model.receptive_field
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        occupancy, lane, drivable = ops_plan.plan_scene(out['segmentation'], out['pedestrian'], out['hdmap'], n_present)
        final, _, _ = model.planning.drive(out['cam_front'], trajs[:, :, 1:], out['costvolume'][:, n_present:], occupancy, lane, drivable,
                                           codes, target)
    return final


def make_leg(leg, model, batch):
    """(one call of the leg without the final synchronise, the leg's tail on given forward outputs, the engine)."""
    import torch
    from stp3_amd.inference import InferenceEngine
    trajs, target, commands = batch['sample_trajectory'].cuda(), batch['target_point'].cuda(), batch['command']
    engine = InferenceEngine(model, batch, autocast_dtype=torch.bfloat16)
    image = engine.image
    poses = [batch[k] for k in ('intrinsics', 'extrinsics', 'future_egomotion')]
    if leg == 'baseline':
        tail = lambda out: eager_tail(model, out, trajs, commands, target)                             # noqa: E731
    else:
        from stp3_amd import ops_plan
        codes = ops_plan.command_codes(commands, device='cuda')
        tail = lambda out: drive_tail(model, out, trajs, codes, target)                                # noqa: E731
    return (lambda: tail(engine(image, *poses))), tail, engine


def per_call_medians(call, calls, repeats):
    import torch
    out = []
    for _ in range(repeats):
        samples = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            samples.append(time.perf_counter() - t)
        out.append(statistics.median(samples))
    return out


def kernels_per_call(call, calls=5):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
            and 'memset' not in e.name.lower())
    return n / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='baseline,drive')
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', default=None)
    ap.add_argument('--batch', type=int, default=1)
    args = ap.parse_args()
    import torch
    if args.trace:
        model, batch = build(args.batch)
        call, _, _ = make_leg(args.trace, model, batch)
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        for _ in range(args.calls):
            call()
            torch.cuda.synchronize()
        print(f'traced {args.calls} calls of {args.trace} at B = {args.batch} after {args.warmup} warm-up calls')
        return
    lines = [f'# scripts/time_plan_engine.py --legs {args.legs} --batches {args.batches} --calls {args.calls} --repeats {args.repeats}',
             f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; N = 1800, T = 6, nine frames, bf16 autocast; times in ms']
    for b in (int(v) for v in args.batches.split(',')):
        model, batch = build(b)
        for leg in args.legs.split(','):
            call, tail_of, engine = make_leg(leg, model, batch)
            for _ in range(args.warmup):
                call()
            meds = [1e3 * v for v in per_call_medians(call, args.calls, args.repeats)]
            line = (f'B={b} {leg}: wall per call median {statistics.median(meds):.3f} (repeats min {min(meds):.3f} .. max {max(meds):.3f}; '
                    f'{args.repeats} x median of {args.calls})')
            lines.append(line)
            print(line, flush=True)
            poses = [batch[k] for k in ('intrinsics', 'extrinsics', 'future_egomotion')]
            out = engine(engine.image, *poses)
            tail = lambda: tail_of(out)                                                                # noqa: E731
            host, dev = [], []
            for _ in range(args.calls):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                e0.record()
                tail()
                e1.record()
                issued = time.perf_counter() - t
                torch.cuda.synchronize()
                host.append(1e3 * issued)
                dev.append(e0.elapsed_time(e1))
            line = (f'B={b} {leg} tail alone: host issue time median {statistics.median(host):.3f}, first to last kernel '
                    f'{statistics.median(dev):.3f}; device kernels {kernels_per_call(tail):.1f}')
            lines.append(line)
            print(line, flush=True)
            del engine, call
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
