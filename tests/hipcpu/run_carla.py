"""TEST INFRASTRUCTURE -- run csrc/stp3_carla.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py) and store what
the kernels wrote.

    python tests/hipcpu/run_carla.py <libstp3hip_cpu.so> <out.npz> [real]

Driver of tests/test_carla_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Without ``real``: every case of tests/carla_cases.py but the ones at the real image size; with it: those alone.
Per case: ``frames/<name>/out`` (float32) and ``/bf16`` (bits); ``depth/<name>/f64``, ``/f32``, ``/labels``; ``hdmap/<name>/f32``,
``/f64``, ``/i64``; ``topdown/<name>/vehicle`` and ``/pedestrian`` (float64) and ``/vehicle_i64``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import carla_cases as CC  # noqa: E402


def setup(lib_path):
    """As tests/hipcpu/run_depth.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_carla_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)


def main(lib_path, out_path, real=False):
    setup(lib_path)
    from stp3_amd.carla import CarlaDecoder
    pick = lambda kind, cases: [n for n in cases if (n in CC.REAL_SIZE[kind]) == real]          # noqa: E731
    out = {}
    for name in pick('frames', CC.FRAME_CASES):
        c = CC.FRAME_CASES[name]
        dec = CarlaDecoder(crop=c['crop'])
        frames = torch.from_numpy(CC.build_frames(name))
        out[f'frames/{name}/out'] = dec.images(frames, order=c['order']).numpy()
        out[f'frames/{name}/bf16'] = dec.images(frames, order=c['order'], out_dtype=torch.bfloat16).view(torch.int16).numpy()
    for name in pick('depth', CC.DEPTH_CASES):
        c = CC.DEPTH_CASES[name]
        dec = CarlaDecoder(crop=c['crop'], downsample=c['ds'], d_bound=CC.D_BOUND)
        frames = torch.from_numpy(CC.build_depth(name))
        out[f'depth/{name}/f64'] = dec.depths(frames, out_dtype=torch.float64).numpy()
        out[f'depth/{name}/f32'] = dec.depths(frames).numpy()
        out[f'depth/{name}/labels'] = dec.depths(frames, labels=True).numpy()
    for name in pick('hdmap', CC.HDMAP_CASES):
        dec = CarlaDecoder(bev_crop=CC.HDMAP_CASES[name]['crop'])
        frames = torch.from_numpy(CC.build_hdmap(name))
        for key, dtype in (('f32', torch.float32), ('f64', torch.float64), ('i64', torch.int64)):
            out[f'hdmap/{name}/{key}'] = dec.hdmap(frames, out_dtype=dtype).numpy()
    for name in pick('topdown', CC.TOPDOWN_CASES):
        dec = CarlaDecoder(bev_crop=CC.TOPDOWN_CASES[name]['crop'], topdown_scale=CC.TOPDOWN_SCALE)
        frames = torch.from_numpy(CC.build_topdown(name))
        veh, ped = dec.topdown(frames, out_dtype=torch.float64)
        out[f'topdown/{name}/vehicle'], out[f'topdown/{name}/pedestrian'] = veh.numpy(), ped.numpy()
        out[f'topdown/{name}/vehicle_i64'] = dec.topdown(frames, out_dtype=torch.int64)[0].numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == 'real')
