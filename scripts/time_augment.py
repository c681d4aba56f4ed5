"""stp3_image_augment on the MI355X against the plain stp3_image_prep on the same bytes: 72 camera images (4 samples x 3 frames
x 6 cameras) of 900 x 1600 x 3 bytes -> 224 x 480, the augmentation parameters drawn per image at resize_lim = (0.193, 0.225),
bot_pct_lim = (0, 0.22), rot_lim = (-5.4, 5.4) degrees, flip on.

    python scripts/time_augment.py [out.txt]            (default: profiles/augment_timing.txt)

Device time from events around CALLS launches on one stream, REPEATS times per variant, the variants alternating inside every
repeat so that drift of the machine hits all of them alike; median, minimum, maximum and the interquartile range are written.
The plan (parameter table + coefficient tables, host work and two host-to-device copies) is built once outside the timed
window and timed on its own with the host clock.  If Pillow is importable the reference's chain is timed on one host core."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, ROOT)
from stp3_amd.config import perception_cfg  # noqa: E402
from stp3_amd.datas import IMAGENET_MEAN, IMAGENET_STD, ImageAugmenter, ImagePreprocessor  # noqa: E402

N, CALLS, REPEATS = 72, 10, 30
LIMITS = dict(resize_lim=(0.193, 0.225), bot_pct_lim=(0.0, 0.22), rot_lim=(-5.4, 5.4), rand_flip=True)


def summary(us):
    q = statistics.quantiles(us, n=4)
    return f'median {statistics.median(us):8.1f} us  min {min(us):8.1f}  max {max(us):8.1f}  iqr {q[2] - q[0]:6.1f}  ({len(us)} repeats x {CALLS} calls)'


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'augment_timing.txt')
    assert torch.cuda.is_available(), 'time_augment.py measures on the GPU; there is no fallback'
    cfg = perception_cfg()
    prep, aug = ImagePreprocessor(cfg), ImageAugmenter(cfg, **LIMITS)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (N, 900, 1600, 3), dtype=torch.uint8, generator=g).cuda()
    params = aug.sample(N, torch.Generator().manual_seed(1))
    fixed = aug.sample(N, train=False)
    unrotated = [dict(p, rotate=0.0) for p in params]
    t0 = time.perf_counter()
    plan = aug.plan(params, images.device)
    torch.cuda.synchronize()
    first_plan = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(5):
        aug.plan(params, images.device)
    torch.cuda.synchronize()
    warm_plan = (time.perf_counter() - t0) / 5
    plans = {'fixed': aug.plan(fixed, images.device), 'unrotated': aug.plan(unrotated, images.device)}
    variants = {}
    for dtype in (torch.float32, torch.bfloat16):
        tag = str(dtype)[6:]
        variants[f'ImagePreprocessor {tag}'] = lambda d=dtype: prep(images, out_dtype=d)
        variants[f'ImageAugmenter {tag} (drawn: resize, crop, flip, rotate; 2 launches)'] = lambda d=dtype: aug.run(images, plan, d)
        variants[f'ImageAugmenter {tag} (drawn, rotation 0; 1 launch)'] = lambda d=dtype: aug.run(images, plans['unrotated'], d)
        variants[f'ImageAugmenter {tag} (train=False parameters; 1 launch)'] = lambda d=dtype: aug.run(images, plans['fixed'], d)
    assert torch.equal(aug.run(images, plans['fixed']), prep(images))
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(REPEATS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / CALLS * 1e3)
    lines = [f'{N} images 900 x 1600 x 3 uint8 -> (3, 224, 480); parameters drawn at {LIMITS}',
             f'  distinct resized sizes in the call: {len({p["resize_dims"] for p in params})}; ksize {plan.ksize}, columns in LDS {plan.cols}, strip rows '
             f'{plan.strip_rows}, coefficient tables {plan.coef.numel() * 4 / 1e3:.0f} KB, workspace {plan.workspace.numel() / 1e6:.1f} MB']
    for name, us in times.items():
        lines.append(f'{name:75s} {summary(us)}')
    for tag in ('float32', 'bfloat16'):
        base = statistics.median(times[f'ImagePreprocessor {tag}'])
        full = statistics.median(times[f'ImageAugmenter {tag} (drawn: resize, crop, flip, rotate; 2 launches)'])
        same = statistics.median(times[f'ImageAugmenter {tag} (train=False parameters; 1 launch)'])
        lines.append(f'ratio to the plain kernel, {tag}: drawn parameters {full / base:.2f}x, train=False parameters {same / base:.2f}x')
    lines.append(f'building the plan on the host (tables + copies): first {first_plan * 1e3:.1f} ms, with the axis tables cached '
                 f'{warm_plan * 1e3:.2f} ms per call')
    try:
        from PIL import Image
    except ImportError:
        Image = None
        lines.append('Pillow is not importable here: the host chain was not measured')
    if Image is not None:
        host = images[:12].cpu().numpy()
        mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
        t0 = time.perf_counter()
        for a, p in zip(host, params):
            img = Image.fromarray(a).resize(p['resize_dims'], resample=Image.BILINEAR).crop(p['crop'])
            if p['flip']:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            img = img.rotate(p['rotate'])
            t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)
            t = (t - mean) / std
        dt = (time.perf_counter() - t0) / len(host)
        lines.append(f'the same chain with Pillow + torch on one host core: {dt * 1e3:.2f} ms per image = {dt * N * 1e3:.0f} ms per {N} images')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
