"""PngDecoder against Pillow on the PNG files of one CARLA sample (T = 3 past frames, S = 7 frames): 12 camera images and 12
depth images of 300 x 400 RGB, 3 hd-map images and 7 top-down class maps -- and on B = 4 such samples in one call.

    python scripts/time_png.py [out.txt]            (default: profiles/png_timing.txt)

The files are synthetic, generated here from a seed and written by Pillow at its default level (which this script therefore
needs): photo-like cameras (low-pass noise at several scales plus hard edges), depth coded in 24 bits over three bytes (a
smooth range image: the low byte is close to noise, as in the simulator's files), flat-colour hd maps, grey class maps.  Host
times with the host clock (device work inside them ends in a synchronise), device times from events around CALLS launches;
every line is the median of REPEATS repeats with minimum, maximum and interquartile range.  (a) Pillow's full decode, (b)
PngDecoder.inflate (chunks, CRC, zlib, the copy into pinned scanlines), (c) the host-to-device copy of the scanlines, (d) the
kernel per kind with the bytes it must move (scanlines in, pixels out) over its time, (e) PngDecoder.__call__ against Pillow +
upload, (f) carla.load_carla_sample against the Pillow route into carla.assemble_carla_sample."""
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
from stp3_amd import carla  # noqa: E402
from stp3_amd.datas import PngDecoder  # noqa: E402

T, S, H, W, BATCH, CALLS, REPEATS, THREADS = 3, 7, 300, 400, 4, 20, 9, 16
MAP_HW, TOP_HW = (400, 400), (300, 400)
KINDS = ('camera', 'depth', 'hdmap', 'topdown')


def smooth(seed, h, w, channels, scales=((6, 70.0), (24, 40.0), (96, 20.0))):
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(1, channels, h, w)
    for cells, gain in scales:
        coarse = torch.randn(1, channels, cells * h // w + 2, cells + 2, generator=g)
        img += gain * torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=False)
    return img, g


def camera(seed):
    img, g = smooth(seed, H, W, 3)
    img += torch.linspace(60, -40, H).view(1, 1, H, 1) + 128 + 2.0 * torch.randn(1, 3, H, W, generator=g)
    rng = np.random.RandomState(seed)
    for _ in range(10):
        y, x, h, w = rng.randint(0, H), rng.randint(0, W), rng.randint(5, 80), rng.randint(5, 120)
        img[0, :, y:y + h, x:x + w] = img[0, :, y:y + h, x:x + w] * 0.5 + torch.tensor(rng.randint(0, 256, 3)).float().view(3, 1, 1) * 0.5
    return img[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()


def depth(seed):
    """A smooth range image in metres, coded as the simulator codes it: R + 256 G + 65536 B = range / 1000 * (2^24 - 1)."""
    img, _ = smooth(1000 + seed, H, W, 1, scales=((4, 30.0), (16, 10.0)))
    metres = (img[0, 0] + torch.linspace(80, 3, H).view(H, 1)).clamp(0.5, 999.0).double()
    code = (metres / 1000.0 * 16777215.0).long().numpy()
    return np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=2).astype(np.uint8)


def hdmap(seed):
    rng = np.random.RandomState(2000 + seed)
    img = np.zeros(MAP_HW + (3,), dtype=np.uint8)
    for _ in range(6):
        y, x, h, w = rng.randint(0, MAP_HW[0]), rng.randint(0, MAP_HW[1]), rng.randint(20, 200), rng.randint(20, 200)
        img[y:y + h, x:x + w] = carla.DRIVABLE_COLOUR
        img[y:y + h, x + w // 2:x + w // 2 + 2] = carla.LANE_COLOUR
    return img


def topdown(seed):
    rng = np.random.RandomState(3000 + seed)
    img = np.full(TOP_HW, 7, dtype=np.uint8)
    for _ in range(12):
        y, x = rng.randint(0, TOP_HW[0]), rng.randint(0, TOP_HW[1])
        img[y:y + rng.randint(4, 12), x:x + rng.randint(4, 24)] = rng.choice([carla.VEHICLE_CLASS, carla.PEDESTRIAN_CLASS, 1, 8])
    return img


def png(array):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(array).save(buf, 'PNG')
    return buf.getvalue()


def summary(values, unit, scale):
    v = [x * scale for x in values]
    q = statistics.quantiles(v, n=4)
    return f'median {statistics.median(v):9.3f} {unit}  min {min(v):9.3f}  max {max(v):9.3f}  iqr {q[2] - q[0]:7.3f}  ({len(v)} repeats)'


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'png_timing.txt')
    assert torch.cuda.is_available(), 'time_png.py measures on the GPU; there is no fallback'
    from PIL import Image
    torch.set_num_threads(THREADS)
    makers = dict(camera=(camera, 4 * T), depth=(depth, 4 * T), hdmap=(hdmap, T), topdown=(topdown, S))
    sample = {k: [png(fn(BATCH * 100 + i)) for i in range(n)] for k, (fn, n) in makers.items()}       # one sample
    batch = {k: [png(fn(b * 100 + i)) for b in range(BATCH) for i in range(n)] for k, (fn, n) in makers.items()}
    one, many = PngDecoder(workers=1), PngDecoder(workers=THREADS)
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=THREADS)
    pillow = lambda s: np.asarray(Image.open(io.BytesIO(s)))
    lines, differ = [], 0
    for k in KINDS:
        got = many(sample[k], 'cuda').cpu().numpy()
        differ += sum(int((a != b).sum()) for a, b in zip(got, one.reference(sample[k])))
    types = np.bincount(np.concatenate([g.rows[:, :, 0].reshape(-1).numpy() for k in KINDS for g in one.inflate(sample[k]).groups]), minlength=5)
    lines.append(f'one CARLA sample: T = {T}, S = {S}: {4 * T} camera + {4 * T} depth files {H} x {W} RGB, {T} hd maps {MAP_HW[0]} x '
                 f'{MAP_HW[1]} RGB, {S} top-down maps {TOP_HW[0]} x {TOP_HW[1]} grey; synthetic, Pillow\'s encoder at its default level')
    lines.append('bytes per file (mean): ' + ', '.join(f'{k} {sum(map(len, sample[k])) / len(sample[k]) / 1e3:.1f} KB' for k in KINDS) +
                 f'; scanlines by filter type 0..4: {types.tolist()}')
    lines.append(f'bytes that differ between PngDecoder on the GPU and Pillow on the sample\'s {sum(len(v) for v in sample.values())} files: {differ}')

    measurements = dict(seq_x=[0.5 * i for i in range(S)], seq_y=[0.1 * i for i in range(S)], seq_theta=[0.01 * i for i in range(S)],
                        x_command=3.0, y_command=-2.0, command=2, steer=0.05, throttle=0.4, brake=0.0, velocity=4.5,
                        receptive_field=T, sample_num=30)
    cdec = carla.CarlaDecoder(crop=256, bev_crop=200)

    for label, files in (('1 sample', sample), (f'{BATCH} samples', batch)):
        flat = [s for k in KINDS for s in files[k]]
        n = len(flat)
        held = {k: many.inflate(files[k]) for k in KINDS}
        rows_d = {k: held[k].groups[0].rows.cuda() for k in KINDS}
        outs_d = {k: many.unfilter_device(held[k].groups[0].geometry, rows_d[k]) for k in KINDS}
        pinned = {k: torch.empty(outs_d[k].shape, dtype=torch.uint8, pin_memory=True) for k in KINDS}

        def inflate_all(dec):
            for k in KINDS:
                dec.inflate(files[k], out=held[k])

        def upload():
            for k in KINDS:
                rows_d[k].copy_(held[k].groups[0].rows, non_blocking=True)

        def call_all():
            for k in KINDS:
                many(files[k], 'cuda', out=outs_d[k])

        def reference_upload(threads):
            for k in KINDS:
                staging = pinned[k].numpy()

                def decode_into(i, staging=staging, k=k):
                    np.copyto(staging[i], pillow(files[k][i]))
                if threads > 1:
                    list(pool.map(decode_into, range(len(files[k]))))
                else:
                    for i in range(len(files[k])):
                        decode_into(i)
                outs_d[k].copy_(pinned[k], non_blocking=True)

        for _ in range(2):                                                      # warm-up of everything timed below
            call_all(), upload(), reference_upload(THREADS)
        torch.cuda.synchronize()
        t = {}
        t['a1'] = host_time(lambda: [pillow(s) for s in flat])
        t['a16'] = host_time(lambda: list(pool.map(pillow, flat)))
        t['b1'] = host_time(lambda: inflate_all(one))
        t['b16'] = host_time(lambda: inflate_all(many))
        t['c'] = device_time(upload)
        for k in KINDS:
            t['d_' + k] = device_time(lambda k=k: many.unfilter_device(held[k].groups[0].geometry, rows_d[k], outs_d[k]))
        t['e_dec'] = host_time(call_all)
        t['e_ref1'] = host_time(lambda: reference_upload(1))
        t['e_ref16'] = host_time(lambda: reference_upload(THREADS))
        med = {k: statistics.median(v) for k, v in t.items()}
        row_bytes = sum(rows_d[k].numel() for k in KINDS)
        lines += ['', f'---- {label}: {n} files per call ----',
                  f'(a) Pillow full decode, 1 thread             per file  {summary(t["a1"], "ms", 1e3 / n)}',
                  f'(a) Pillow full decode, {THREADS} threads           per file  {summary(t["a16"], "ms", 1e3 / n)}',
                  f'(b) PngDecoder.inflate, 1 thread             per file  {summary(t["b1"], "ms", 1e3 / n)}',
                  f'(b) PngDecoder.inflate, {THREADS} threads           per file  {summary(t["b16"], "ms", 1e3 / n)}',
                  f'    ratio (a) / (b): 1 thread {med["a1"] / med["b1"]:.2f}x, {THREADS} threads {med["a16"] / med["b16"]:.2f}x',
                  f'(c) host-to-device copy of the scanlines ({row_bytes / 1e6:.1f} MB, pinned, 4 copies)  {summary(t["c"], "us", 1e6)} = '
                  f'{row_bytes / med["c"] / 1e9:.1f} GB/s']
        for k in KINDS:
            moved = rows_d[k].numel() + outs_d[k].numel()
            lines.append(f'(d) stp3_png_unfilter, {k:8s} {rows_d[k].shape[0]:3d} x {tuple(rows_d[k].shape[1:])}  {summary(t["d_" + k], "us", 1e6)} = '
                         f'{moved / med["d_" + k] / 1e9:.2f} GB/s on {moved / 1e6:.2f} MB in + out')
        lines += [f'(e) PngDecoder.__call__ x 4 kinds ({THREADS} threads)       {summary(t["e_dec"], "ms", 1e3)}',
                  f'(e) Pillow + upload, 1 thread                      {summary(t["e_ref1"], "ms", 1e3)}',
                  f'(e) Pillow + upload, {THREADS} threads                    {summary(t["e_ref16"], "ms", 1e3)}',
                  f'    ratio Pillow + upload / PngDecoder at {THREADS} threads: {med["e_ref16"] / med["e_dec"]:.2f}x']
        if files is sample:
            nested = dict(image_files=[files['camera'][4 * i:4 * i + 4] for i in range(T)],
                          depth_files=[files['depth'][4 * i:4 * i + 4] for i in range(T)], hdmap_files=files['hdmap'],
                          topdown_files=files['topdown'])

            def pillow_route():
                decoded = {k: torch.from_numpy(np.stack(list(pool.map(pillow, files[k])))).cuda() for k in KINDS}
                return carla.assemble_carla_sample(cdec, decoded['camera'].view(T, 4, H, W, 3), decoded['depth'].view(T, 4, H, W, 3),
                                                   decoded['hdmap'], decoded['topdown'], **measurements)

            def byte_route():
                return carla.load_carla_sample(cdec, many, **nested, **measurements, device='cuda')

            for _ in range(2):
                pillow_route(), byte_route()
            f_ref, f_dec = [], []
            for _ in range(REPEATS):                                            # alternating: the host is shared
                f_ref.append(once(pillow_route))
                f_dec.append(once(byte_route))
            lines += [f'(f) carla.load_carla_sample ({THREADS} threads)              {summary(f_dec, "ms", 1e3)}',
                      f'(f) Pillow ({THREADS} threads) -> assemble_carla_sample       {summary(f_ref, "ms", 1e3)}',
                      f'    ratio Pillow route / load_carla_sample: {statistics.median(f_ref) / statistics.median(f_dec):.2f}x']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text, end='')


def once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if __name__ == '__main__':
    main()
