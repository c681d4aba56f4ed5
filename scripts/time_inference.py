"""Time the eval forward: plain eager ``model.eval()(...)`` against ``InferenceEngine`` replay, in one process.

    python scripts/time_inference.py [--legs perception_b1,perception_b4,prediction_b1] [--block 50] [--repeats 3]
                                     [--out profiles/inference_timing.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \
        python scripts/time_inference.py --trace plain|engine --leg perception_b1 --forwards K
    python scripts/time_inference.py --kernel-stats DIR [--out profiles/inference_kernel_stats.txt]

Timing protocol: sizes users run (Perception.yml 224 x 480, T = 3, at B = 1 and B = 4; a Prediction.yml leg at B = 1); both
paths warmed; a host clock around ``block`` forwards that end in a device synchronise; the two paths ALTERNATE block by block,
``repeats`` times; reported: the median and the spread (min .. max) of the per-forward time of each path's blocks, their ratio,
and whether the engine's slowest block beats the plain path's fastest one.  The plain path is what ``model.eval()(...)`` runs
outside the engine -- the path the engine's outputs are bit-equal to (tests/test_inference_gpu.py).

Kernel trace (a run of its own: tracing slows the host): ``--trace PATH --forwards K`` runs the warm-up (and the capture) and
then K forwards of one path, nothing else.  Two traced runs with different K give, by difference, the dispatches and the summed
kernel time PER FORWARD, whatever the set-up launched; ``--kernel-stats DIR`` reads the kernel_trace CSVs
``DIR/<leg>_<path>_<K>/**/*kernel_trace.csv`` and writes that table.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'st-p3_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = {'perception_b1': ('perception', 1), 'perception_b4': ('perception', 4), 'prediction_b1': ('prediction', 1)}


def build_leg(name):
    """(model on the GPU in eval mode, batch) of a leg; seeded random weights (timing does not depend on their values)."""
    import torch
    from stp3_amd import synthetic
    from stp3_amd.config import perception_cfg
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    kind, b = LEGS[name]
    torch.manual_seed(0)
    if kind == 'perception':
        cfg, seq = perception_cfg(), 3
    else:
        # nuscenes/Prediction.yml: four future frames, GAUSSIAN present distribution, instance + flow heads
        cfg = perception_cfg(**{'N_FUTURE_FRAMES': 4, 'PROBABILISTIC.ENABLED': True, 'PROBABILISTIC.METHOD': 'GAUSSIAN',
                                'SEMANTIC_SEG.PEDESTRIAN.ENABLED': False, 'SEMANTIC_SEG.HDMAP.ENABLED': False,
                                'INSTANCE_FLOW.ENABLED': True, 'INSTANCE_SEG.ENABLED': True, 'FUTURE_DISCOUNT': 0.95})
        seq = 7
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = to_channels_last(STP3(cfg).eval().cuda())
    batch = synthetic.make_batch(batch=b, seq=seq, seed=1, with_labels=False)
    return model, batch


def paths(model, batch):
    """{'plain': fn, 'engine': fn}: one forward each, on a resident batch (images on the device, poses on the host)."""
    import torch
    from stp3_amd.inference import InferenceEngine
    image = batch['image'].cuda()
    poses = (batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'])

    def plain():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return model(image, *poses)

    engine = InferenceEngine(model, (image,) + poses, autocast_dtype=torch.bfloat16)

    def replay():
        return engine(engine.image, *poses)

    return {'plain': plain, 'engine': replay}


def time_block(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def run_timing(args):
    import torch
    assert torch.cuda.is_available(), 'time_inference.py measures on the GPU; there is no fallback'
    lines = [f'# scripts/time_inference.py --block {args.block} --repeats {args.repeats}: ms per eval forward, host clock around '
             f'{args.block} forwards ending in a device synchronise, paths alternating block by block',
             f'# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             '# leg             path    median   min      max      blocks']
    for leg in args.legs.split(','):
        model, batch = build_leg(leg)
        fns = paths(model, batch)
        for fn in fns.values():                                   # warm both paths
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                times[k].append(time_block(fn, args.block))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            lines.append(f'{leg:15s} {k:7s} {med[k]:8.3f} {min(v):8.3f} {max(v):8.3f}  ' + ' '.join(f'{t:.3f}' for t in v))
        spread = max(max(v) - min(v) for v in times.values())
        beats = med['plain'] - med['engine'] > spread
        lines.append(f'{leg:15s} ratio plain / engine = {med["plain"] / med["engine"]:.2f}x; difference of the medians '
                     f'{med["plain"] - med["engine"]:.3f} ms against a spread (largest max - min of a path) of {spread:.3f} ms: '
                     f'{"engine faster beyond the spread" if beats else "NOT separated from the spread"}; slowest engine block '
                     f'{max(times["engine"]):.3f} ms, fastest plain block {min(times["plain"]):.3f} ms')
        del model, fns
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


def run_trace(args):
    """Under rocprofv3: warm-up (+ capture), then ``forwards`` forwards of ONE path."""
    import torch
    assert torch.cuda.is_available()
    model, batch = build_leg(args.leg)
    if args.trace == 'plain':
        image = batch['image'].cuda()
        poses = (batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'])

        def fn():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return model(image, *poses)
        for _ in range(3):                                        # (the engine's constructor runs 3 warm-up forwards too)
            fn()
    else:
        fn = paths(model, batch)['engine']
    for _ in range(args.forwards):
        fn()
    torch.cuda.synchronize()
    print(f'traced {args.forwards} forwards of {args.leg} / {args.trace}')
    return 0


def read_trace(pattern):
    """(dispatches, summed kernel nanoseconds, {kernel name: (n, ns)}) of the kernel_trace CSVs that match."""
    n, total, by = 0, 0, {}
    files = glob.glob(pattern, recursive=True)
    assert files, f'no kernel trace under {pattern}'
    for path in files:
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                d = int(row['End_Timestamp']) - int(row['Start_Timestamp'])
                n += 1
                total += d
                e = by.setdefault(row['Kernel_Name'], [0, 0])
                e[0] += 1
                e[1] += d
    return n, total, by


def family(name):
    for key, fam in (('conv2d_igemm', 'dense convolution, tiled'), ('pointwise_rows', 'dense convolution, pointwise rows'),
                     ('pointwise_direct', 'dense convolution, pointwise direct'), ('dwconv', 'depthwise convolution'),
                     ('bn_apply_fwd', 'BatchNorm apply (stand-alone)'), ('se_pool', 'squeeze-excite'), ('se_reduce', 'squeeze-excite'),
                     ('se_mlp', 'squeeze-excite'), ('se_scale', 'squeeze-excite'), ('lift_', 'voxel pool'), ('depth_softmax', 'voxel pool'),
                     ('plan_', 'voxel-pool plan'), ('voxel_index', 'voxel-pool plan'), ('upsample', 'up-sampling'),
                     ('linear_fwd', 'small linear'), ('causal_pair', 'causal frame pairing')):
        if key in name:
            return fam
    return 'torch (element-wise, copies, reductions)'


def run_kernel_stats(args):
    lines = ['# rocprofv3 --kernel-trace --stats, one traced run per (leg, path, K forwards); per forward = (run with K2 - run with K1) '
             '/ (K2 - K1)', '# leg             path    dispatches/forward   kernel ms/forward']
    legs = sorted({os.path.basename(d).rsplit('_', 2)[0] for d in glob.glob(os.path.join(args.kernel_stats, '*_*_*')) if os.path.isdir(d)})
    for leg in legs:
        per = {}
        for path in ('plain', 'engine'):
            runs = sorted((int(os.path.basename(d).rsplit('_', 1)[1]), d)
                          for d in glob.glob(os.path.join(args.kernel_stats, f'{leg}_{path}_*')) if os.path.isdir(d))
            (k1, d1), (k2, d2) = runs[0], runs[-1]
            n1, t1, by1 = read_trace(os.path.join(d1, '**', '*kernel_trace.csv'))
            n2, t2, by2 = read_trace(os.path.join(d2, '**', '*kernel_trace.csv'))
            fam = {}
            for name, (n, ns) in by2.items():
                a = by1.get(name, (0, 0))
                e = fam.setdefault(family(name), [0.0, 0.0])
                e[0] += (n - a[0]) / (k2 - k1)
                e[1] += (ns - a[1]) / (k2 - k1) / 1e6
            per[path] = ((n2 - n1) / (k2 - k1), (t2 - t1) / (k2 - k1) / 1e6, fam)
            lines.append(f'{leg:15s} {path:7s} {per[path][0]:12.1f} {per[path][1]:18.3f}')
        if len(per) == 2:
            lines.append(f'{leg:15s} engine / plain: {per["plain"][0] - per["engine"][0]:.1f} fewer dispatches per forward, kernel time '
                         f'x{per["engine"][1] / per["plain"][1]:.3f}')
            for key in sorted(set(per['plain'][2]) | set(per['engine'][2])):
                a, b = per['plain'][2].get(key, (0, 0)), per['engine'][2].get(key, (0, 0))
                lines.append(f'    {key:42s} plain {a[0]:7.1f} x {a[1]:8.3f} ms   engine {b[0]:7.1f} x {b[1]:8.3f} ms')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--legs', default='perception_b1,perception_b4,prediction_b1')
    ap.add_argument('--block', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', choices=('plain', 'engine'), default=None)
    ap.add_argument('--leg', default='perception_b1')
    ap.add_argument('--forwards', type=int, default=10)
    ap.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.kernel_stats:
        return run_kernel_stats(args)
    if args.trace:
        return run_trace(args)
    assert args.block >= 50 and args.repeats >= 3, 'the protocol asks for blocks of >= 50 forwards, repeated >= 3 times'
    return run_timing(args)


if __name__ == '__main__':
    sys.exit(main())
