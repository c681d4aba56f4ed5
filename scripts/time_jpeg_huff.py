"""JpegDecoder(entropy='device') against JpegDecoder() (entropy='host') on the 72 camera-sized frames of scripts/time_jpeg.py
(900 x 1600, 4:2:0, quality 90), and on the same frames with one restart interval per MCU row.

    python scripts/time_jpeg_huff.py [out.txt]          (default: profiles/jpeg_huff_timing.txt)
    python scripts/time_jpeg_huff.py --launches         (a few calls of stp3_jpeg_entropy_device on both data sets and nothing
                                                         else: the run to put under `rocprofv3 --kernel-trace --stats` for
                                                         the time of each pass)

The method of scripts/time_jpeg.py: warm-up, host times with the host clock (device work inside them ends in a synchronise),
device times from events around CALLS launches, every line the median of REPEATS repeats with minimum, maximum and
interquartile range.  The two modes of the whole call ALTERNATE inside one run; a difference counts beyond the printed spread."""
import io
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import time_jpeg as T  # noqa: E402
from stp3_amd.datas import JpegDecoder, _coef_count  # noqa: E402


def data_sets():
    from PIL import Image
    sets = {}
    for label, extra in (('no restart markers', {}), ('a restart interval per MCU row', {'restart_marker_rows': 1})):
        distinct = []
        for k in range(T.DISTINCT):
            buf = io.BytesIO()
            Image.fromarray(T.frame(k)).save(buf, 'JPEG', quality=90, subsampling=2, **extra)
            distinct.append(buf.getvalue())
        sets[label] = [distinct[i % T.DISTINCT] for i in range(T.N)]
    return sets


def staged(dec, streams):
    batch = dec.prepare(streams)
    grp = batch.groups[0]
    assert len(batch.groups) == 1 and not batch.fallback and not grp.host
    coef = torch.empty(T.N, _coef_count(grp.geometry), dtype=torch.int16, device='cuda')
    status = torch.empty(T.N, dtype=torch.int32, device='cuda')
    return batch, grp, grp.scans.cuda(), grp.descs.cuda(), coef, status


def launches():
    dec = JpegDecoder(workers=T.THREADS, entropy='device')
    for streams in data_sets().values():
        batch, grp, scans, descs, coef, status = staged(dec, streams)
        for _ in range(5):
            dec.entropy_device_launch(grp, scans, descs, coef, status)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * T.N


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'jpeg_huff_timing.txt')
    assert torch.cuda.is_available(), 'time_jpeg_huff.py measures on the GPU; there is no fallback'
    torch.set_num_threads(T.THREADS)
    host, one = JpegDecoder(workers=T.THREADS), JpegDecoder(workers=1, entropy='device')
    dev = JpegDecoder(workers=T.THREADS, entropy='device')
    dev.keep_flags = True
    lines = [f'{T.N} frames {T.H} x {T.W}, 4:2:0, quality 90 ({T.DISTINCT} distinct synthetic frames of scripts/time_jpeg.py); subsequences of '
             f'128 bytes, 256 per workgroup; sync_rounds {dev.sync_rounds}']
    out_d = torch.empty(T.N, T.H, T.W, 3, dtype=torch.uint8, device='cuda')
    for label, streams in data_sets().items():
        batch, grp, scans, descs, coef, status = staged(dev, streams)
        want = host.entropy(streams).groups[0]
        dev.entropy_device_launch(grp, scans, descs, coef, status)
        differ = int((coef.cpu() != want.coef).sum())
        for _ in range(2):                                                      # warm-up of everything timed below
            dev(streams, 'cuda', out=out_d)
            host(streams, 'cuda', out=out_d)
            scans.copy_(grp.scans, non_blocking=True)
        flags = np.concatenate(dev.last_flags)
        stats = dict(dev.last_stats)
        subs = grp.descs.numpy().view(np.int32)[:, 0]
        rounds = [int(np.argmax(f[:dev.sync_rounds + 1] == 0)) for f in flags]
        t = {'p1': T.host_time(lambda: one.prepare(streams, out=batch)), 'p16': T.host_time(lambda: dev.prepare(streams, out=batch)),
             'up': T.device_time(lambda: scans.copy_(grp.scans, non_blocking=True)),
             'dev': T.device_time(lambda: dev.entropy_device_launch(grp, scans, descs, coef, status)),
             'rec': T.device_time(lambda: dev.reconstruct_device(grp.geometry, coef, want.quant.cuda(), out_d), calls=3)}
        call = {'device': [], 'host': []}
        for _ in range(T.REPEATS):                                              # alternating
            call['device'] += once(lambda: dev(streams, 'cuda', out=out_d))
            call['host'] += once(lambda: host(streams, 'cuda', out=out_d))
        med = {k: statistics.median(v) for k, v in {**t, **call}.items()}
        used = int(grp.descs.numpy().view(np.int32)[:, 5].sum())
        lines += [f'---- {label}: stream bytes mean {sum(map(len, streams)) / T.N / 1e3:.0f} KB, {int(subs.mean())} subsequences and '
                  f'{int(grp.descs.numpy().view(np.int32)[:, 1].mean())} segments per frame',
                  f'coefficients that differ between the device decode and stp3_jpeg_entropy on all {T.N} frames: {differ}; images taken '
                  f'by the device / host / Pillow in a call: {stats["device"]} / {stats["host"]} / {stats["pillow"]}',
                  f'(a) stp3_jpeg_scan_prepare, 1 thread        per frame  {T.summary(t["p1"], "ms", 1e3 / T.N)}',
                  f'(a) stp3_jpeg_scan_prepare, {T.THREADS} threads      per frame  {T.summary(t["p16"], "ms", 1e3 / T.N)}',
                  f'(b) upload of the scans ({grp.scans.numel() / 1e6:.1f} MB pinned, {used / 1e6:.1f} MB used; coefficients would be '
                  f'{coef.numel() * 2 / 1e6:.0f} MB)  {T.summary(t["up"], "us", 1e6)} = {grp.scans.numel() / med["up"] / 1e9:.1f} GB/s',
                  f'(c) stp3_jpeg_entropy_device, all passes, {T.N} frames   {T.summary(t["dev"], "us", 1e6)}',
                  f'    stp3_jpeg_reconstruct behind it                     {T.summary(t["rec"], "us", 1e6)}',
                  f'(d) subsequences that decoded more than one further subsequence before their state repeated: {int(flags[:, -1].sum())} of '
                  f'{int(subs.sum())} = {flags[:, -1].sum() / subs.sum():.3f}; cross-workgroup launches that still changed an edge state, per '
                  f'frame: min {min(rounds)} max {max(rounds)} (sync_rounds must be at least the maximum)',
                  f'(e) JpegDecoder(entropy="device").__call__, {T.N} frames  {T.summary(call["device"], "ms", 1e3)}',
                  f'(e) JpegDecoder(entropy="host").__call__, {T.N} frames    {T.summary(call["host"], "ms", 1e3)}',
                  f'    ratio host / device: {med["host"] / med["device"]:.2f}x']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text, end='')


def once(fn):
    import time
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return [time.perf_counter() - t0]


if __name__ == '__main__':
    launches() if '--launches' in sys.argv else main()
