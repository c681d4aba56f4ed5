"""JpegDecoder against Pillow on 72 camera-sized frames (4 samples x 3 frames x 6 cameras): 900 x 1600, 4:2:0, quality 90.

    python scripts/time_jpeg.py [out.txt]            (default: profiles/jpeg_timing.txt)

The frames are synthetic but photo-like -- low-pass noise at several scales plus hard edges; white noise would have several
times a photograph's bit rate and is no proxy for the Huffman work -- generated here from a seed and encoded with Pillow (which
this script therefore needs).  Host times with the host clock (device work inside them ends in a synchronise), device times
from events around CALLS launches; every line is the median of REPEATS repeats with minimum, maximum and interquartile range.
(a) Pillow's full decode, (b) the host entropy decode, (c) the host-to-device copy of the coefficients, (d) the kernel and its
share of 8 TB/s on the compulsory 6 bytes per pixel, (e) JpegDecoder.__call__ against JpegDecoder.reference + upload."""
import concurrent.futures
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, ROOT)
from stp3_amd.datas import JpegDecoder  # noqa: E402

N, H, W, DISTINCT, CALLS, REPEATS, THREADS = 72, 900, 1600, 8, 10, 9, 16
PEAK = 8e12


def frame(seed):
    """Low-pass noise at four scales (bilinear up-sampling of coarse grids), a horizon, and rectangles with hard edges."""
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(1, 3, H, W)
    for cells, gain in ((6, 70.0), (24, 40.0), (96, 20.0), (400, 8.0)):
        coarse = torch.randn(1, 3, cells * 9 // 16 + 2, cells + 2, generator=g)
        img += gain * torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False)
    img += torch.linspace(60, -40, H).view(1, 1, H, 1) + 128
    img += 2.0 * torch.randn(1, 3, H, W, generator=g)                       # sensor noise
    rng = np.random.RandomState(seed)
    for _ in range(25):
        y, x, h, w = rng.randint(0, H), rng.randint(0, W), rng.randint(10, 200), rng.randint(10, 300)
        img[0, :, y:y + h, x:x + w] = img[0, :, y:y + h, x:x + w] * 0.5 + torch.tensor(rng.randint(0, 256, 3)).float().view(3, 1, 1) * 0.5
    return img[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()


def summary(values, unit, scale):
    v = [x * scale for x in values]
    q = statistics.quantiles(v, n=4)
    return f'median {statistics.median(v):9.2f} {unit}  min {min(v):9.2f}  max {max(v):9.2f}  iqr {q[2] - q[0]:7.2f}  ({len(v)} repeats)'


def host_time(fn):
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def device_time(fn, calls=CALLS):
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls * 1e-3)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'jpeg_timing.txt')
    assert torch.cuda.is_available(), 'time_jpeg.py measures on the GPU; there is no fallback'
    from PIL import Image
    torch.set_num_threads(THREADS)
    distinct = []
    for k in range(DISTINCT):
        buf = io.BytesIO()
        Image.fromarray(frame(k)).save(buf, 'JPEG', quality=90, subsampling=2)
        distinct.append(buf.getvalue())
    streams = [distinct[i % DISTINCT] for i in range(N)]
    one, many = JpegDecoder(workers=1), JpegDecoder(workers=THREADS)
    info = one.info(streams[0])
    batch = many.entropy(streams)
    grp = batch.groups[0]
    assert not batch.fallback and len(batch.groups) == 1
    want = one.reference(distinct)
    got = many(distinct, 'cuda')
    differ = int((got.cpu() != want).sum())

    def pillow(s):
        return np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))

    pool = concurrent.futures.ThreadPoolExecutor(max_workers=THREADS)
    coef_d, quant_d = grp.coef.cuda(), grp.quant.cuda()
    out_d = torch.empty(N, H, W, 3, dtype=torch.uint8, device='cuda')
    pinned = torch.empty(N, H, W, 3, dtype=torch.uint8, pin_memory=True)

    staging = pinned.numpy()                                                # (a view of the pinned buffer)

    def decode_into(i):                                                     # Pillow's decode, copied into its pinned frame
        np.copyto(staging[i], pillow(streams[i]))                          # (one memcpy, outside the interpreter lock)

    def reference_upload(threads):
        if threads > 1:
            list(pool.map(decode_into, range(N)))                           # (the staging copy runs in the worker threads too)
        else:
            for i in range(N):
                decode_into(i)
        out_d.copy_(pinned, non_blocking=True)

    for _ in range(2):                                                      # warm-up of everything timed below
        many.reconstruct_device(grp.geometry, coef_d, quant_d, out_d)
        many(streams, 'cuda', out=out_d)
        coef_d.copy_(grp.coef, non_blocking=True)
    torch.cuda.synchronize()
    t = {}
    t['a1'] = host_time(lambda: [pillow(s) for s in streams])
    t['a16'] = host_time(lambda: list(pool.map(pillow, streams)))
    t['b1'] = host_time(lambda: one.entropy(streams, out=batch))
    t['b16'] = host_time(lambda: many.entropy(streams, out=batch))
    t['c'] = device_time(lambda: coef_d.copy_(grp.coef, non_blocking=True))
    t['d'] = device_time(lambda: many.reconstruct_device(grp.geometry, coef_d, quant_d, out_d))
    t['e_dec'] = host_time(lambda: many(streams, 'cuda', out=out_d))
    t['e_ref1'] = host_time(lambda: reference_upload(1))
    t['e_ref16'] = host_time(lambda: reference_upload(THREADS))
    med = {k: statistics.median(v) for k, v in t.items()}
    coef_bytes = grp.coef.numel() * 2
    lines = [f'{N} frames {H} x {W}, 4:2:0, quality 90 ({DISTINCT} distinct synthetic frames: low-pass noise + edges); MCU grid '
             f'{info.mcus_y} x {info.mcus_x}, {info.coef_count} coefficients per frame',
             f'bytes per frame: ' + ', '.join(str(len(s)) for s in distinct) + f' (mean {sum(map(len, distinct)) / DISTINCT / 1e3:.0f} KB = '
             f'{sum(map(len, distinct)) * 8 / DISTINCT / (H * W):.2f} bit/px)',
             f'bytes that differ between JpegDecoder on the GPU and Pillow on the {DISTINCT} distinct frames: {differ}',
             f'(a) Pillow full decode, 1 thread            per frame  {summary(t["a1"], "ms", 1e3 / N)}',
             f'(a) Pillow full decode, {THREADS} threads          per frame  {summary(t["a16"], "ms", 1e3 / N)}',
             f'(b) host entropy decode, 1 thread           per frame  {summary(t["b1"], "ms", 1e3 / N)}',
             f'(b) host entropy decode, {THREADS} threads         per frame  {summary(t["b16"], "ms", 1e3 / N)}',
             f'    ratio (a) / (b): 1 thread {med["a1"] / med["b1"]:.2f}x, {THREADS} threads {med["a16"] / med["b16"]:.2f}x',
             f'(c) host-to-device copy of the coefficients ({coef_bytes / 1e6:.0f} MB, pinned)  {summary(t["c"], "us", 1e6)} = '
             f'{coef_bytes / med["c"] / 1e9:.1f} GB/s',
             f'(d) stp3_jpeg_reconstruct, {N} frames                       {summary(t["d"], "us", 1e6)} = '
             f'{N * H * W * 6 / med["d"] / 1e12:.2f} TB/s on 6 B/px = {N * H * W * 6 / med["d"] / PEAK:.3f} of 8 TB/s',
             f'(e) JpegDecoder.__call__ ({THREADS} threads), {N} frames         {summary(t["e_dec"], "ms", 1e3)}',
             f'(e) reference + upload, 1 thread, {N} frames            {summary(t["e_ref1"], "ms", 1e3)}',
             f'(e) reference + upload, {THREADS} threads, {N} frames          {summary(t["e_ref16"], "ms", 1e3)}',
             f'    ratio reference + upload / JpegDecoder: {med["e_ref16"] / med["e_dec"]:.2f}x at {THREADS} threads']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
