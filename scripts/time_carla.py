"""The CARLA decoder on the MI355X against the host routes it replaces (stp3_amd.carla.CarlaDecoder; csrc/stp3_carla.hip).

    python scripts/time_carla.py [--repeats 30] [--out profiles/carla_timing.txt]

Two comparisons, wall clock around a device synchronisation (both sides end with the tensors on the GPU or, for the sample, where
the reference leaves them), after a warm-up, ``repeats`` repeats with the routes alternating inside every repeat; median and range:
  per tick    the agent's own host route (carla_agent.py:326-329,409-432): per camera BGR -> RGB, PIL crop, ToTensor, Normalize,
              ``.to('cuda')`` -- four times -- against ONE pinned-memory copy of the four BGRA frames + ``stp3_carla_frames``
  per sample  T = 3 frames x four cameras, seven top-down frames (CarlaData.py:355-450 after the PNG decoder): the reference-style
              numpy / PIL statements on decoded arrays, results left on the host as the loader leaves them, against the four
              launches on bytes that are already on the device, and against the same plus the pinned copies of the bytes
torchvision and cv2 are not dependencies of this repository: ToTensor / Normalize / cvtColor are their published statements in
torch / numpy (as in scripts/make_golden_carla.py).  Outputs of the two sides are compared before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from stp3_amd.carla import CarlaDecoder  # noqa: E402
from tests import carla_cases as CC  # noqa: E402

MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def crop_of(image, crop):
    """scale_and_crop_image at scale 1 (CarlaData.py:454-464)."""
    width, height = int(image.width // 1.), int(image.height // 1.)
    arr = np.asarray(image.resize((width, height)))
    y0, x0 = height // 2 - crop // 2, width // 2 - crop // 2
    return arr[y0:y0 + crop, x0:x0 + crop]


def normalise(pic):
    x = torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1)))).to(dtype=torch.float32).div(255)
    return x.sub_(MEAN).div_(STD)


def host_tick(frames):
    """frames: four (300, 400, 4) BGRA arrays -> (1, 1, 4, 3, 256, 256) on the GPU, the agent's statements."""
    out = []
    for bgra in frames:
        rgb = np.ascontiguousarray(bgra[:, :, :3][:, :, ::-1])                          # cv2.cvtColor(.., COLOR_BGR2RGB)
        x = normalise(np.array(crop_of(Image.fromarray(rgb), 256))).unsqueeze(0).unsqueeze(0).unsqueeze(0)
        out.append(x.to('cuda', dtype=torch.float32))
    return torch.cat(out, dim=2)


def host_sample(s):
    """The loader's statements on decoded arrays (CarlaData.py:355-450 without Image.open)."""
    images = torch.cat([torch.cat([normalise(np.array(crop_of(Image.fromarray(s['images'][t, n]), 256))).unsqueeze(0) for n in range(4)],
                                  dim=0).unsqueeze(0) for t in range(3)], dim=0)
    depths = []
    for t in range(3):
        row = []
        for n in range(4):
            data = np.array(crop_of(Image.fromarray(s['depths'][t, n]), 256)).astype(np.float32)
            normalized = np.dot(data, [65536.0, 256.0, 1.0])
            normalized /= (256 * 256 * 256 - 1)
            row.append(torch.from_numpy(normalized * 1000).unsqueeze(0))
        depths.append(torch.cat(row, dim=0).unsqueeze(0))
    hdmaps = []
    for t in range(3):
        c = crop_of(Image.fromarray(s['hdmaps'][t]), 200)
        lane = np.all(c == [255, 0, 255], axis=2).astype(np.float64)
        drivable = np.logical_or(np.all(c == [54, 52, 46], axis=2), lane)
        hdmaps.append(torch.from_numpy(np.concatenate([lane[::-1, ::-1][None], drivable[::-1, ::-1][None]], axis=0)).unsqueeze(0))
    seg, ped = [], []
    for t in range(7):
        image = Image.fromarray(s['topdowns'][t])
        width, height = int(image.width // 1.1), int(image.height // 1.1)
        arr = np.asarray(image.resize((width, height), resample=Image.NEAREST))
        y0, x0 = height // 2 - 100, width // 2 - 100
        c = arr[y0:y0 + 200, x0:x0 + 200]
        vehicle = (c == 10).astype(np.float64)
        vehicle[89:112, 96:105] = 0
        pedestrian = (c == 4).astype(np.float64)
        seg.append(torch.from_numpy(vehicle[::-1, ::-1].copy()).unsqueeze(0).unsqueeze(0))
        ped.append(torch.from_numpy(pedestrian[::-1, ::-1].copy()).unsqueeze(0).unsqueeze(0))
    return images, torch.cat(depths, dim=0), torch.cat(hdmaps, dim=0), torch.cat(seg, dim=0), torch.cat(ped, dim=0)


def timed(routes, repeats):
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'carla_timing.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_carla.py measures on the GPU; there is no other mode'
    dec = CarlaDecoder(downsample=CC.DOWNSAMPLE, d_bound=CC.D_BOUND)
    lines = [f'# python scripts/time_carla.py   (one {torch.cuda.get_device_name(0)}; host: {os.cpu_count()} logical CPUs, torch on '
             f'{torch.get_num_threads()} threads, Pillow {PIL.__version__})',
             f'# wall clock around a device synchronisation, us per call, after 3 warm-up calls, {a.repeats} repeats, routes alternating']

    # ---- per tick
    bgra = np.random.RandomState(1).randint(0, 256, size=(4, 300, 400, 4)).astype(np.uint8)
    pinned = torch.from_numpy(bgra).pin_memory()
    staged = torch.empty(4, 300, 400, 4, dtype=torch.uint8, device='cuda')
    out = torch.empty(4, 3, 256, 256, device='cuda')

    def kernel_tick():
        staged.copy_(pinned, non_blocking=True)
        return dec.images(staged, order='bgr', out=out)
    assert torch.equal(kernel_tick(), host_tick(bgra)[0, 0])
    tick = {'agent host route: 4 x (BGR->RGB, PIL crop, ToTensor, Normalize, .to(cuda))': lambda: host_tick(bgra),
            'one pinned copy (1.9 MB) + stp3_carla_frames': kernel_tick}
    # ---- per sample
    s = CC.build_sample()
    keys = ('images', 'depths', 'hdmaps', 'topdowns')
    host_bytes = {k: torch.from_numpy(s[k]).pin_memory() for k in keys}
    dev_bytes = {k: v.cuda() for k, v in host_bytes.items()}

    def launches(b):
        return (dec.images(b['images']), dec.depths(b['depths'], out_dtype=torch.float64), dec.hdmap(b['hdmaps'], out_dtype=torch.float64),
                *dec.topdown(b['topdowns'], out_dtype=torch.float64))
    for got, want in zip(launches(dev_bytes), host_sample(s)):
        assert torch.equal(got.cpu(), want.to(got.dtype))
    sample = {'reference-style numpy / PIL route on decoded arrays (results on the host)': lambda: host_sample(s),
              'four launches, bytes already on the device': lambda: launches(dev_bytes),
              'pinned copies of the bytes (10.5 MB) + four launches': lambda: launches({k: v.cuda(non_blocking=True) for k, v in host_bytes.items()})}
    for title, routes in (('per tick: four 300 x 400 BGRA frames -> (4, 3, 256, 256) float32 on the GPU', tick),
                          ('per training sample: T = 3 x four cameras (images, depths), 3 hd maps, 7 top-down frames', sample)):
        for fn in routes.values():
            for _ in range(3):
                fn()
        times = timed(routes, a.repeats)
        lines.append(title)
        for name, t in times.items():
            lines.append(f'  {name:82s} median {statistics.median(t):9.1f}   min {min(t):9.1f}   max {max(t):9.1f}')
        names = list(times)
        slow, fast = times[names[0]], times[names[1]]
        verdict = ('faster beyond the spread of the repeats' if max(fast) < min(slow) else
                   'NOT faster beyond the spread of the repeats' if statistics.median(fast) < statistics.median(slow) else 'not faster')
        lines.append(f'  -> the kernel route is {verdict} (median ratio {statistics.median(slow) / statistics.median(fast):.1f})')
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
