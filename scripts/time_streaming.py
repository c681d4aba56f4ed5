"""Time the closed-loop tick: the full-window ``InferenceEngine`` against ``StreamingEngine``, in one process.

    python scripts/time_streaming.py [--legs perception_b1,perception_b4,prediction_b1] [--block 50] [--repeats 3]
                                     [--out profiles/streaming_timing.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \
        python scripts/time_streaming.py --trace full|streaming --leg perception_b1 --ticks K
    python scripts/time_streaming.py --kernel-stats DIR [--out profiles/streaming_kernel_stats.txt]

What a tick of the simulator loop costs (carla_agent.py:408-445: a new camera frame joins a window of T = 3).  Both paths do ALL
of a tick's work: the image copy from a PINNED host tensor (full: the window's B T N images; streaming: the B N newest), the plan
rebuild and the ego-motion upload, the replay.  Protocol of scripts/time_inference.py (whose legs these are): both paths warmed on
every shape, a host clock around ``block`` ticks that end in a device synchronise, the two paths ALTERNATING block by block,
``repeats`` times; reported: median, minimum and maximum per path, the ratio, and whether the difference of the medians exceeds
the spread.

Kernel trace (a run of its own, tracing only, no counters): ``--trace PATH --ticks K`` builds the engine and runs K ticks of one
path; two traced runs with different K give, by difference, the dispatches and the kernel time PER TICK by kernel family
(``--kernel-stats DIR`` reads ``DIR/<leg>_<path>_<K>/**/*kernel_trace.csv``).
"""
import argparse
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'st-p3_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

import time_inference as TI  # noqa: E402

PATHS = ('full', 'streaming')


def paths(model, batch, which=PATHS):
    """{'full': fn, 'streaming': fn}: one tick each -- image copy from pinned host memory, plan rebuild, replay."""
    import torch
    from stp3_amd.inference import InferenceEngine, StreamingEngine
    rf = model.receptive_field
    poses = (batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'])
    window = batch['image'][:, :rf].contiguous().pin_memory()
    newest = batch['image'][:, rf - 1].contiguous().pin_memory()
    out = {}
    if 'full' in which:
        full = InferenceEngine(model, (window,) + poses, autocast_dtype=torch.bfloat16)
        out['full'] = lambda: full(window, *poses)
    if 'streaming' in which:
        streaming = StreamingEngine(model, (window,) + poses, autocast_dtype=torch.bfloat16)
        for _ in range(rf):                                       # fill the window: every timed tick returns outputs
            streaming.step(newest, *poses)
        out['streaming'] = lambda: streaming.step(newest, *poses)
    return out


def run_timing(args):
    import torch
    assert torch.cuda.is_available(), 'time_streaming.py measures on the GPU; there is no fallback'
    lines = [f'# scripts/time_streaming.py --block {args.block} --repeats {args.repeats}: ms per tick (image copy from pinned host memory '
             f'+ plan rebuild + replay), host clock around {args.block} ticks ending in a device synchronise, paths alternating block by block',
             f'# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             '# full: InferenceEngine on the whole window (B T N images per tick); streaming: StreamingEngine.step (B N images per tick)',
             '# leg             path       median   min      max      blocks']
    for leg in args.legs.split(','):
        model, batch = TI.build_leg(leg)
        fns = paths(model, batch)
        for fn in fns.values():                                   # warm both paths at this shape
            for _ in range(args.warmup):
                assert fn() is not None
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                times[k].append(TI.time_block(fn, args.block))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            lines.append(f'{leg:15s} {k:10s} {med[k]:8.3f} {min(v):8.3f} {max(v):8.3f}  ' + ' '.join(f'{t:.3f}' for t in v))
        spread = max(max(v) - min(v) for v in times.values())
        beats = med['full'] - med['streaming'] > spread
        lines.append(f'{leg:15s} ratio full / streaming = {med["full"] / med["streaming"]:.2f}x; difference of the medians '
                     f'{med["full"] - med["streaming"]:.3f} ms against a spread (largest max - min of a path) of {spread:.3f} ms: '
                     f'{"streaming faster beyond the spread" if beats else "NOT separated from the spread"}; slowest streaming block '
                     f'{max(times["streaming"]):.3f} ms, fastest full-window block {min(times["full"]):.3f} ms')
        del model, fns
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


def run_trace(args):
    """Under rocprofv3: construction (warm-up + capture), then ``ticks`` ticks of ONE path."""
    import torch
    assert torch.cuda.is_available()
    model, batch = TI.build_leg(args.leg)
    fn = paths(model, batch, which=(args.trace,))[args.trace]
    for _ in range(args.ticks):
        fn()
    torch.cuda.synchronize()
    print(f'traced {args.ticks} ticks of {args.leg} / {args.trace}')
    return 0


def family(name):
    if 'window_push' in name:
        return 'window push'
    return TI.family(name)


def run_kernel_stats(args):
    lines = ['# rocprofv3 --kernel-trace --stats (tracing only), one traced run per (leg, path, K ticks); per tick = (run with K2 - run '
             'with K1) / (K2 - K1)', '# leg             path       dispatches/tick   kernel ms/tick']
    legs = sorted({os.path.basename(d).rsplit('_', 2)[0] for d in glob.glob(os.path.join(args.kernel_stats, '*_*_*')) if os.path.isdir(d)})
    for leg in legs:
        per = {}
        for path in PATHS:
            runs = sorted((int(os.path.basename(d).rsplit('_', 1)[1]), d)
                          for d in glob.glob(os.path.join(args.kernel_stats, f'{leg}_{path}_*')) if os.path.isdir(d))
            if len(runs) < 2:
                continue
            (k1, d1), (k2, d2) = runs[0], runs[-1]
            n1, t1, by1 = TI.read_trace(os.path.join(d1, '**', '*kernel_trace.csv'))
            n2, t2, by2 = TI.read_trace(os.path.join(d2, '**', '*kernel_trace.csv'))
            fam = {}
            for name, (n, ns) in by2.items():
                a = by1.get(name, (0, 0))
                e = fam.setdefault(family(name), [0.0, 0.0])
                e[0] += (n - a[0]) / (k2 - k1)
                e[1] += (ns - a[1]) / (k2 - k1) / 1e6
            per[path] = ((n2 - n1) / (k2 - k1), (t2 - t1) / (k2 - k1) / 1e6, fam)
            lines.append(f'{leg:15s} {path:10s} {per[path][0]:12.1f} {per[path][1]:18.3f}')
        if len(per) == 2:
            lines.append(f'{leg:15s} streaming / full: {per["full"][0] - per["streaming"][0]:.1f} fewer dispatches per tick, kernel time '
                         f'x{per["streaming"][1] / per["full"][1]:.3f}')
            for key in sorted(set(per['full'][2]) | set(per['streaming'][2])):
                a, b = per['full'][2].get(key, (0, 0)), per['streaming'][2].get(key, (0, 0))
                lines.append(f'    {key:42s} full {a[0]:7.1f} x {a[1]:8.3f} ms   streaming {b[0]:7.1f} x {b[1]:8.3f} ms')
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
    ap.add_argument('--trace', choices=PATHS, default=None)
    ap.add_argument('--leg', default='perception_b1')
    ap.add_argument('--ticks', type=int, default=10)
    ap.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.kernel_stats:
        return run_kernel_stats(args)
    if args.trace:
        return run_trace(args)
    assert args.block >= 50 and args.repeats >= 3, 'the protocol asks for blocks of >= 50 ticks, repeated >= 3 times'
    return run_timing(args)


if __name__ == '__main__':
    sys.exit(main())
