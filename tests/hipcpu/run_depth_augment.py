"""TEST INFRASTRUCTURE -- run csrc/stp3_depth_augment.hip on CPU tensors through libstp3hip_cpu.so (tests/hipcpu/build.py)
and store what the kernels wrote.

    python tests/hipcpu/run_depth_augment.py <libstp3hip_cpu.so> <out.npz> [corrupt]

Driver of tests/test_depth_augment_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read
from the environment.  Per small case of depth_augment_cases: ``<name>/full`` (float64 output), ``/full32``, ``/labels`` (some
image rotates: the window's tables), ``/labels_norot`` and ``/full_norot`` (the same parameters without rotation: the label
rows' and columns' tables), ``/replay`` (the plan rewritten in place with the second parameter set).
With ``corrupt``: per case and per kind of damage ``<name>/<damage>/out`` of a call whose third image's record (or whose table
entries) hold impossible values, output and workspace between canaries -- ``/canaries`` says whether those are intact, ``/rc``
the entry's return value.  Host only: never on a GPU."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import depth_augment_cases as DA  # noqa: E402
from tests import depth_cases as DC  # noqa: E402

BAD = 2                                            # the image whose record is damaged
CANARY, PAD = 0x5a, 4096
I32 = np.iinfo(np.int32)


def setup(lib_path):
    """As tests/hipcpu/run_depth.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_augment_depth_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    torch.cuda.is_current_stream_capturing = lambda: False
    return ops


def inputs_of(name, seed_offset=0):
    built = DA.build(name, seed_offset)
    if 'maps' in built:
        return None, torch.from_numpy(built['maps'])
    return (torch.from_numpy(built['points']), torch.from_numpy(built['offsets']), torch.from_numpy(built['steps']), DC.BEFORE,
            torch.from_numpy(built['intrinsics'])), None


def call(lab, cloud, maps, **kw):
    return (lab.from_maps(maps, **kw) if cloud is None else lab.from_lidar(*cloud, **kw)).numpy()


def no_rotation(params):
    return [dict(p, rotate=0.0) for p in params]


def run_cases(out):
    for name in DA.SMALL:
        lab, params = DA.labeller(name), DA.params(name)
        cloud, maps = inputs_of(name)
        out[f'{name}/full'] = call(lab, cloud, maps, params=params, out_dtype=torch.float64)
        out[f'{name}/full32'] = call(lab, cloud, maps, params=params)
        out[f'{name}/labels'] = call(lab, cloud, maps, params=params, labels=True)
        out[f'{name}/full_norot'] = call(lab, cloud, maps, params=no_rotation(params))
        out[f'{name}/labels_norot'] = call(lab, cloud, maps, params=no_rotation(params), labels=True)
        # a plan made for the first set, rewritten in place for the second one and another cloud
        route = None if maps is None else maps.dtype
        plan = lab.augment_plan(params, 'cpu', maps=route)
        call(lab, cloud, maps, plan=plan)
        blob = plan.blob.data_ptr()
        lab.augment_plan(DA.replay_params(name), 'cpu', like=plan)
        assert plan.blob.data_ptr() == blob
        cloud2, maps2 = inputs_of(name, 1)
        out[f'{name}/replay'] = call(lab, cloud2, maps2, plan=plan)


def padded(nbytes):
    """(whole buffer filled with the canary, the view of its middle)."""
    whole = torch.full((nbytes + 2 * PAD,), CANARY, dtype=torch.uint8)
    return whole, whole[PAD:PAD + nbytes]


def intact(whole, nbytes):
    w = whole.numpy()
    return bool((w[:PAD] == CANARY).all() and (w[PAD + nbytes:] == CANARY).all())


DAMAGE = {
    'max': lambda rec, plan: rec.__setitem__(slice(None), I32.max),
    'min': lambda rec, plan: rec.__setitem__(slice(None), I32.min),
    'rotation': lambda rec, plan: rec.__setitem__(slice(0, 6), np.array([I32.max, I32.min, I32.max, I32.min, I32.max, I32.min])),
    'offsets': lambda rec, plan: rec.__setitem__(slice(6, 12), np.array([plan.part('tap_y').numel() // 2, plan.part('tap_x').numel() // 2 - 1,
                                                                          plan.part('slot_y').numel() - 1, plan.part('slot_x').numel(), 3, 0])),
    'lengths': lambda rec, plan: rec.__setitem__(slice(10, 12), np.array([I32.max, -1])),
    'entries': None,                                # the third image's taps and slot sources instead of its record
}


def run_corrupt(out):
    from stp3_amd import _lib
    lib = _lib.lib()
    for name in ('l24', 'l17', 'm64', 'm32'):
        lab, params = DA.labeller(name), DA.params(name)
        cloud, maps = inputs_of(name)
        n_frames, n_cam = DA.FRAMES_CAMERAS[name]
        ho, wo = DA.CASES[name]['final']
        for damage, fn in DAMAGE.items():
            route = None if maps is None else maps.dtype
            plan = lab.augment_plan(params, 'cpu', maps=route)
            records = plan.part('records').numpy().reshape(-1, 16)
            if fn is not None:
                fn(records[BAD], plan)
            else:
                ty, tx, sy, sx, nsy, nsx = records[BAD, 6:12]
                plan.part('tap_y').numpy().reshape(-1, 2)[ty:ty + ho:2] = np.array([I32.max, I32.min])
                plan.part('tap_x').numpy().reshape(-1, 2)[tx:tx + wo:2] = -7
                plan.part('slot_y').numpy()[sy:sy + nsy:2] = I32.max
                plan.part('slot_x').numpy()[sx:sx + nsx:3] = I32.min
            n_total = 0 if cloud is None else cloud[0].shape[0]
            d = lab._augment_dims(plan, n_frames, n_cam, n_total, _lib.DEPTH_OUT_F64)
            out_bytes = n_frames * n_cam * ho * wo * 8
            out_whole, out_view = padded(out_bytes)
            ok = True
            if cloud is None:
                rc = lib.stp3_augment_depth_from_maps(ctypes.byref(d), maps.data_ptr(), _lib.DEPTH_OUT_F64 if maps.dtype == torch.float64
                                                      else _lib.DEPTH_OUT_F32, out_view.data_ptr(), None)
            else:
                need = ctypes.c_size_t()
                assert lib.stp3_augment_depth_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == 0
                ws_whole, ws_view = padded(need.value)
                points, offsets, steps, before, k = cloud
                rc = lib.stp3_augment_depth_from_lidar(ctypes.byref(d), points.data_ptr(), offsets.data_ptr(), steps.data_ptr(),
                                                       lab._before_mask(before), k.data_ptr(), ws_view.data_ptr(), need.value,
                                                       out_view.data_ptr(), None)
                ok = intact(ws_whole, need.value)
            out[f'{name}/{damage}/rc'] = np.int64(rc)
            out[f'{name}/{damage}/canaries'] = np.bool_(ok and intact(out_whole, out_bytes))
            out[f'{name}/{damage}/out'] = out_view.numpy().view(np.float64).reshape(n_frames, n_cam, ho, wo).copy()


def main(lib_path, out_path, corrupt=False):
    setup(lib_path)
    out = {}
    (run_corrupt if corrupt else run_cases)(out)
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == 'corrupt')
