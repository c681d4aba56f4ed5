"""Writes tests/golden/depth_labels.npz: the reference's depth maps (stp3/datas/NuscenesData.py, unmodified and loaded from
the reference tree) on the cases of tests/depth_cases.py, for tests/test_depth_cpu.py / test_depth_gpu.py.

    python scripts/make_golden_depth.py [--time]

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, torch and Pillow.  Data only; the inputs are not stored:
the tests rebuild them with the same builder and check the sha256 stored here first.

Lidar cases (``<name>/``): ``FuturePredictionDataset.get_depth_from_lidar`` (:289-300) called unbound, per frame and camera,
on a namespace that carries ``cfg``, ``augmentation_parameters`` and a ``nusc_exp`` whose ``map_pointcloud_to_image`` hands
back the prepared (points, coloring, None).  THE PROJECTION IS NOT THE DEVKIT'S OWN CODE: the nuScenes devkit is not
installed here, ``depth_cases.project`` restates NuScenesExplorer.map_pointcloud_to_image from its published source --
PARITY UNPINNED (``meta/projection``).  Pinned by the reference: scatter (last point wins), bilinear resample, crop, round.
  sha      digests of points / offsets / steps / intrinsics        depths   int16 (F, N, Ho, Wo): the reference's rounded maps
  margin   float64: the smallest distance of a non-zero unrounded output from a half-integer (asserted > 1e-6)
  duplicates  how many kept points share their pixel with a later one

Map cases: the statements of :261-266 are executed through the reference's own ``get_input_data`` (:174-280), isolated: the
dataset tables, the quaternion class and the image normaliser it touches on the way are stand-ins, the camera image is a
grey PNG and the depth map an .npy file in a temporary data root (``meta/map_route`` says so).
  sha, depths  as above       margin   as above (float64 map)
  excluded  int32 (k, 4): (frame, camera, row, column) of the outputs of the float32 map whose unrounded value lies within 1e-3
            of a half-integer -- the tests compare those to +-1 and everything else exactly; at most 0.5 % of the pixels may
            be listed, and the reference alone must stay below that (asserted)

``labels``: the trainer's statement (stp3/trainer.py:269-276, restated here in one line of torch on the reference's map).
"""
import os
import sys
import tempfile
import time
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_stubs  # noqa: E402
from tests import depth_cases as DC  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'depth_labels.npz')
HALF_MARGIN_F64, HALF_MARGIN_F32, EXCLUDED_CAP = 1e-6, 1e-3, 0.005


def load_reference():
    """ref_stubs.install() plus empty stand-ins for what stp3/datas/NuscenesData.py imports and these methods never call."""
    ref_stubs.install()

    def mod(name, **attrs):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(sys.modules[name], k, v)

    dummy = type('Dummy', (), {'__init__': lambda self, *a, **k: None})
    mod('cv2')
    mod('tqdm', tqdm=lambda x, *a, **k: x)
    mod('matplotlib', use=lambda *a, **k: None)
    mod('matplotlib.pyplot')
    mod('nuscenes.nuscenes', NuScenes=dummy, NuScenesExplorer=dummy)
    mod('nuscenes.can_bus')
    mod('nuscenes.can_bus.can_bus_api', NuScenesCanBus=dummy)
    mod('nuscenes.utils.splits', create_splits_scenes=dummy)
    mod('nuscenes.eval')
    mod('nuscenes.eval.common')
    mod('nuscenes.eval.common.utils', quaternion_yaw=dummy)
    import stp3.datas.NuscenesData as ND
    return ND


def dataset_namespace(ND, geo):
    h, w = geo['source_hw']
    left, top, right, bottom = geo['crop']
    cfg = NS(IMAGE=NS(ORIGINAL_HEIGHT=h, ORIGINAL_WIDTH=w, RESIZE_SCALE=geo['scale'], TOP_CROP=top, FINAL_DIM=(bottom - top, right - left),
                      NAMES=[]),
             LIFT=NS(GT_DEPTH=True))
    hr, wr = int(h * geo['scale']), int(w * geo['scale'])
    aug = {'scale_width': geo['scale'], 'scale_height': geo['scale'], 'resize_dims': (wr, hr), 'crop': tuple(geo['crop'])}
    return NS(cfg=cfg, augmentation_parameters=aug)


def lidar_reference(ND, case):
    """(rounded maps (F, N, Ho, Wo) float64, unrounded maps, duplicates): get_depth_from_lidar per frame and camera."""
    ds = dataset_namespace(ND, case)
    pixels, depth, keep = DC.projected(case)
    # the unrounded value: the same call with torch.round of the module replaced by the identity for the second pass
    off, n_cam = case['offsets'], case['steps'].shape[1]
    rounded, raw, dup = [], [], 0
    for f in range(len(off) - 1):
        for c in range(n_cam):
            k = keep[off[f]:off[f + 1], c]
            u, v, z, _ = DC.project(case['points'][off[f]:off[f + 1]], case['steps'][f], case['intrinsics'][f], case['source_hw'])
            pts = np.stack([u[k, c], v[k, c], np.ones(k.sum())])                # (3, n) float64, as view_points returns
            col = z[k, c]                                                       # float32 depths
            ds.nusc_exp = NS(map_pointcloud_to_image=lambda a, b, pts=pts, col=col: (pts, col, None))
            rounded.append(ND.FuturePredictionDataset.get_depth_from_lidar(ds, None, None).numpy())
            keep_round = ND.torch.round
            ND.torch.round = lambda t: t                                        # (the module's attribute, for this call)
            try:
                raw.append(ND.FuturePredictionDataset.get_depth_from_lidar(ds, None, None).numpy())
            finally:
                ND.torch.round = keep_round
            lin = pts[1].astype(np.int64) * case['source_hw'][1] + pts[0].astype(np.int64)
            dup += len(lin) - len(np.unique(lin))
            assert np.array_equal(np.stack([pts[0].astype(np.int32), pts[1].astype(np.int32)], 1), pixels[off[f]:off[f + 1], c][k])
    shape = (len(off) - 1, n_cam) + rounded[0].shape
    return np.stack(rounded).reshape(shape), np.stack(raw).reshape(shape), dup


class _Quaternion:
    """Identity rotation with the attributes get_input_data reads."""
    def __init__(self, *a, **k):
        self.rotation_matrix = np.eye(3)
        self.yaw_pitch_roll = (0.0, 0.0, 0.0)

    @property
    def inverse(self):
        return self


def map_reference(ND, case):
    """(rounded, unrounded) maps of get_input_data's depth branch (:257-267) on the stored maps of a case."""
    from PIL import Image
    maps = case['maps']
    n_frames, n_cam = maps.shape[:2]
    h, w = case['source_hw']
    ds = dataset_namespace(ND, case)
    cams = [f'CAM_{c}' for c in range(n_cam)]
    ds.cfg.IMAGE.NAMES = cams
    ds.normalise_image = lambda img: torch.zeros(3, img.size[1], img.size[0])
    records = {'pose': {'rotation': [1, 0, 0, 0], 'translation': [0.0, 0.0, 0.0], 'ego_pose_token': 'pose'},
               'calib': {'rotation': [1, 0, 0, 0], 'translation': [0.0, 0.0, 0.0],
                         'camera_intrinsic': [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]}}
    keep_q, ND.Quaternion = ND.Quaternion, _Quaternion
    out = {}
    try:
        with tempfile.TemporaryDirectory() as root:
            ds.dataroot = root
            os.makedirs(os.path.join(root, 'samples'))
            Image.fromarray(np.full((h, w, 3), 128, np.uint8)).save(os.path.join(root, 'samples', 'grey.png'))
            for what, rnd in (('rounded', None), ('raw', lambda t: t)):
                frames = []
                for f in range(n_frames):
                    def get(table, token, f=f):
                        if table == 'sample_data':
                            return {'ego_pose_token': 'pose', 'calibrated_sensor_token': 'calib',
                                    'filename': f'samples/grey.png' if token == 'LIDAR' else f'samples/{token}.png'}
                        return records['pose' if table == 'ego_pose' else 'calib']
                    for c, cam in enumerate(cams):
                        os.makedirs(os.path.join(root, 'depths', cam, 'npy'), exist_ok=True)
                        np.save(os.path.join(root, 'depths', cam, 'npy', f'f{f}_{cam}.npy'), maps[f, c])
                        Image.fromarray(np.full((h, w, 3), 128, np.uint8)).save(os.path.join(root, 'samples', f'f{f}_{cam}.png'))
                    ds.nusc = NS(get=get)
                    rec = {'data': {'LIDAR_TOP': 'LIDAR', **{cam: f'f{f}_{cam}' for cam in cams}}}
                    keep_round = ND.torch.round
                    if rnd:
                        ND.torch.round = rnd
                    try:
                        depths = ND.FuturePredictionDataset.get_input_data(ds, rec)[3]
                    finally:
                        ND.torch.round = keep_round
                    assert depths.dtype == torch.from_numpy(maps).dtype
                    frames.append(depths.numpy().reshape((n_cam,) + tuple(depths.shape[-2:])))
                out[what] = np.stack(frames)
    finally:
        ND.Quaternion = keep_q
    return out['rounded'], out['raw']


def half_distance(raw):
    """Distance of every value from the nearest half-integer."""
    return np.abs(raw - np.floor(raw) - 0.5)


def labels_of(depths, geo):
    ds, (d0, d1, _) = geo['downsample'], geo['d_bound']
    t = torch.from_numpy(depths.astype(np.float32))
    return (torch.clamp(t[..., ::ds, ::ds], d0, d1 - 1) - d0).long().numpy()


def main():
    ND = load_reference()
    out = {'meta/projection': np.array('PARITY UNPINNED: nuScenes devkit map_pointcloud_to_image restated from its published source '
                                       '(tests/depth_cases.project); scatter, resample, crop and rounding are the reference\'s own'),
           'meta/map_route': np.array('get_input_data (NuscenesData.py:174-280) itself, isolated with stand-in tables, quaternion and '
                                      'normaliser; depth files in a temporary data root')}
    for name in DC.LIDAR_CASES:
        case = DC.build_lidar(name)
        rounded, raw, dup = lidar_reference(ND, case)
        nz = raw != 0
        margin = float(half_distance(raw[nz]).min()) if nz.any() else np.inf
        assert margin > HALF_MARGIN_F64, (name, margin)
        assert np.array_equal(rounded, np.rint(rounded)) and rounded.min() >= 0 and rounded.max() < 2 ** 15
        assert dup >= DC.LIDAR_CASES[name]['repeats'] * 0.75 and (name != 'small' or dup >= 100), (name, dup)   # (the builder keeps a prefix)
        out[f'{name}/sha'] = np.array(DC.digest(case, DC.LIDAR_KEYS))
        out[f'{name}/depths'] = rounded.astype(np.int16)
        out[f'{name}/labels'] = labels_of(rounded, case).astype(np.int16)
        out[f'{name}/margin'], out[f'{name}/duplicates'] = np.float64(margin), np.int64(dup)
        print(f'{name}: {rounded.shape}, {int((rounded > 0).sum())} non-zero outputs, margin {margin:.2e}, {dup} overwritten points')
    for name in DC.MAP_CASES:
        case = DC.build_map(name)
        rounded, raw = map_reference(ND, case)
        out[f'{name}/sha'] = np.array(DC.digest(case, ('maps',)))
        out[f'{name}/depths'] = rounded.astype(np.int16)
        out[f'{name}/labels'] = labels_of(rounded, case).astype(np.int16)
        dist = half_distance(raw.astype(np.float64))
        if case['maps'].dtype == np.float64:
            assert dist.min() > HALF_MARGIN_F64, (name, dist.min())
            out[f'{name}/margin'] = np.float64(dist.min())
            print(f'{name}: {rounded.shape}, margin {dist.min():.2e}')
        else:
            excluded = np.argwhere(dist < HALF_MARGIN_F32).astype(np.int32)
            assert len(excluded) <= EXCLUDED_CAP * raw.size, (name, len(excluded), raw.size)
            out[f'{name}/excluded'] = excluded.reshape(-1, 4)
            print(f'{name}: {rounded.shape}, {len(excluded)} of {raw.size} outputs excluded (cap {EXCLUDED_CAP * raw.size:.0f})')
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    if '--time' in sys.argv:
        case = DC.build_lidar('real')
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            lidar_reference(ND, case)
        dt = (time.perf_counter() - t0) / reps / 2                               # (lidar_reference calls the method twice)
        n_cam = case['steps'].shape[1]
        print(f'reference get_depth_from_lidar on this host ({os.cpu_count()} logical CPUs, torch threads {torch.get_num_threads()}): '
              f'{dt / n_cam * 1e3:.1f} ms per camera image, {dt * 12 * 1e3:.0f} ms for 12 frames x {n_cam} cameras '
              f'(projection excluded: prepared points)')


if __name__ == '__main__':
    main()
