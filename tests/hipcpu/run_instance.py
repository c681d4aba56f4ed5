"""TEST INFRASTRUCTURE -- run csrc/stp3_instance.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and
store what the kernels wrote.

    python tests/hipcpu/run_instance.py <libstp3hip_cpu.so> <out.npz> [lsap]

Driver of tests/test_instance_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from
the environment.  Per case of instance_cases.HOST_KERNEL_CASES and for sample 0 of 'clean' (``clean0``): ``<name>/raw``,
``/centers``, ``/counts`` of stp3_amd.instance.segment_frames and ``/tracked`` of predict_instance_segmentation_and_trajectories
on their GPU route, with ``check=True``; ``random/*``: both kernels on random heads with plateaus, NaNs, infinities and empty
frames (the torch path is run on the same arrays by the test); ``errors``: the tracker's error words on inputs that break its
contract.  With ``lsap``: only the assignment, through the tracker, on the point scenes whose sizes the test supplies (``main_lsap``)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import instance_cases as IC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_sampler.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def random_heads(seed, n=6, h=24, w=40):
    """Heads that exercise the corners of the segment kernel: quantised centerness (plateaus, many candidates), a NaN, an
    infinity, a frame below the threshold, a frame that is all foreground."""
    rs = np.random.RandomState(seed)
    center = (rs.randint(0, 12, size=(n, h, w)) / 10.0).astype(np.float32)
    center[1, 5, 7] = np.nan
    center[1, 9, 9] = np.inf
    center[2] *= 0.05
    offset = (4.0 * rs.standard_normal((n, 2, h, w))).astype(np.float32)
    offset[3] = np.rint(offset[3])
    fg = rs.uniform(size=(n, h, w)) < 0.3
    fg[4] = True
    return center, offset, fg


def point_scene(rs, n0, n1, h=64, w=96, spread=3.0):
    """(raw (1, 2, h, w) int64, flow (1, 2, 2, h, w) float32): n0 single-pixel instances at random places in frame 0, n1 in frame 1, random
    flow of ``spread`` pixels: a dense assignment problem of n0 x n1."""
    raw = np.zeros((1, 2, h, w), np.int64)
    pix0 = rs.choice(h * w, size=n0, replace=False)
    pix1 = rs.choice(h * w, size=n1, replace=False)
    raw[0, 0].reshape(-1)[np.sort(pix0)] = np.arange(1, n0 + 1)
    raw[0, 1].reshape(-1)[np.sort(pix1)] = np.arange(1, n1 + 1)
    flow = (spread * rs.standard_normal((1, 2, 2, h, w))).astype(np.float32)
    return raw, flow


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd import instance as I
    out = {}
    jobs = [(name, IC.build(name)) for name in IC.HOST_KERNEL_CASES]
    clean = IC.build('clean')
    jobs.append(('clean0', {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in clean.items()}))
    for name, case in jobs:
        o = {k: None if case[k] is None else torch.from_numpy(case[k])
             for k in ('segmentation', 'instance_center', 'instance_offset', 'instance_flow')}
        b, s, _, h, w = o['segmentation'].shape
        fg = torch.argmax(o['segmentation'], dim=2) == 1
        raw, centers, counts = I.segment_frames(o['instance_center'].reshape(b * s, h, w), o['instance_offset'].reshape(b * s, 2, h, w),
                                                fg.reshape(b * s, h, w))
        out[f'{name}/raw'], out[f'{name}/centers'], out[f'{name}/counts'] = raw.view(b, s, h, w).numpy(), centers.numpy(), counts.numpy()
        res = I.predict_instance_segmentation_and_trajectories(o, compute_matched_centers=case['matched'],
                                                               make_consistent=case['make_consistent'], check=True)
        out[f'{name}/tracked'] = (res[0] if case['matched'] else res).numpy()
    center, offset, fg = random_heads(5)
    raw, centers, counts = I.segment_frames(torch.from_numpy(center), torch.from_numpy(offset), torch.from_numpy(fg))
    out['random/raw'], out['random/centers'], out['random/counts'] = raw.numpy(), centers.numpy(), counts.numpy()
    rs = np.random.RandomState(6)
    flow = (2.0 * rs.standard_normal((2, 3, 2, 24, 40))).astype(np.float32)
    tracked, err = I.track_frames(raw.view(2, 3, 24, 40), torch.from_numpy(flow))
    out['random/tracked'], out['random/err'] = tracked.numpy(), err.numpy()
    # contract violations: a missing id (1), no background (2), an id above 100 and an infinite flow on an instance (1, 3)
    bad = np.zeros((3, 2, 8, 8), np.int64)
    bad[:, :, 1, 1], bad[:, :, 5, 5] = 1, 2
    bad[0, 1, 5, 5] = 3
    bad[1, 0] = 1
    bad[2, 1, 6, 6] = 101
    flow = np.zeros((3, 2, 2, 8, 8), np.float32)
    words = []
    for i in range(3):
        f = flow[i:i + 1].copy()
        if i == 2:
            f[0, 0, 0, 1, 1] = np.inf
        words.append(I.track_frames(torch.from_numpy(bad[i:i + 1]), torch.from_numpy(f))[1].numpy())
    out['errors'] = np.stack(words)
    np.savez(out_path, **out)
    print('RESULT', out_path)


def main_lsap(lib_path, out_path):
    """The kernel's assignment on point scenes of every pair of sides the test asks for (sizes.npy next to ``out_path``)."""
    setup(lib_path)
    from stp3_amd import instance as I
    sizes = np.load(out_path + '.sizes.npy')
    out = {}
    for k, (n0, n1, seed) in enumerate(sizes):
        raw, flow = point_scene(np.random.RandomState(int(seed)), int(n0), int(n1))
        tracked, err = I.track_frames(torch.from_numpy(raw), torch.from_numpy(flow), matching_threshold=1e30)
        assert not err.numpy().any()
        out[f'p{k}'] = tracked.numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    (main_lsap if len(sys.argv) > 3 and sys.argv[3] == 'lsap' else main)(sys.argv[1], sys.argv[2])
