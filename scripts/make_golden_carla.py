"""Writes tests/golden/carla.npz: the reference's CARLA loader and agent (stp3/datas/CarlaData.py, carla_agent.py, unmodified and
loaded from the reference tree) on the cases of tests/carla_cases.py, for tests/test_carla_cpu.py / test_carla_gpu.py.

    python scripts/make_golden_carla.py

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, torch and Pillow.  Data only; the inputs are not stored: the
tests rebuild them with the same builders and check the sha256 stored here first.  ``oracle.ref_stubs`` is used unchanged; cv2,
carla, leaderboard.*, team_code.* and stp3.trainer (imported by carla_agent.py, never used on these paths) get empty stand-ins
here.

What is called, unbound or on a bare namespace:
  frames/<case>   ``scale_and_crop_image(Image.fromarray(x), scale=1, crop=c)`` + the normaliser, per image; BGR(A) sources pass
                  through the agent's ``x[:, :, :3]`` reversed (cv2 is not installed: cv2.cvtColor(.., COLOR_BGR2RGB) of three
                  channels IS that reversal).  THE NORMALISER IS NOT TORCHVISION'S OWN CODE: torchvision is not installed, ToTensor
                  and Normalize are restated from their published source (uint8 HWC -> CHW float32 .div(255); (x - mean) / std
                  with float32 mean / std) -- ``meta/normaliser`` says so.  out: float32; bf16: its rounding (int16 bits)
  depth/<case>    ``CarlaDataset.get_depth(np.array(scale_and_crop_image(Image.open(png), 1., c)))``: metres float64; labels: the
                  trainer's statement (stp3/trainer.py:269-276, restated in one line of torch on the reference's float64 map)
  hdmap/<case>    ``CarlaDataset.get_hdmap(png, 1., c)``        topdown/<case>  ``CarlaDataset.get_labels(png, 1.1, c)``
  sample/         ``CarlaDataset.__getitem__`` itself on a namespace whose lists name lossless PNGs in a temporary directory;
                  its Quaternion is a stand-in (``extrinsics`` is therefore not stored: stp3_amd.carla.cam_para's rotation is pinned
                  against the closed form, parity with pyquaternion unpinned) and its sampled trajectories are random (not stored)
  host/           ``get_future_egomotion``, ``transform_2d_points``, the gt_trajectory / target_point statements (through
                  ``__getitem__``, with constant images) and the agent's command point (carla_agent.py:349-357, restated: it is
                  inline in ``tick``); ``PIDController.step`` and ``MVPAgent.control_pid`` over the 60 steps
Large outputs are stored as sha256 + every 97th element; 0 / 1 maps as bits."""
import os
import sys
import tempfile
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_stubs  # noqa: E402
from tests import carla_cases as CC  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'carla.npz')
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def load_reference():
    ref_stubs.install()

    def mod(name, **attrs):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(sys.modules[name], k, v)

    dummy = type('Dummy', (), {'__init__': lambda self, *a, **k: None})
    mod('cv2')
    mod('carla')
    mod('leaderboard')
    mod('leaderboard.autoagents')
    mod('leaderboard.autoagents.autonomous_agent', AutonomousAgent=dummy, Track=dummy)
    sys.modules['leaderboard.autoagents'].autonomous_agent = sys.modules['leaderboard.autoagents.autonomous_agent']
    mod('team_code')
    mod('team_code.planner', RoutePlanner=dummy)
    mod('stp3.trainer', TrainingModule=dummy)
    import stp3.datas.CarlaData as CD
    import carla_agent as CA
    return CD, CA


def normalise_image(pic):
    """torchvision.transforms.Compose([ToTensor(), Normalize(mean, std)]) on a uint8 HWC array, restated (see the module text)."""
    x = torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1)))).to(dtype=torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=x.dtype).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=x.dtype).view(-1, 1, 1)
    return x.sub_(mean).div_(std)


class _Quaternion:
    """Identity rotation with the attribute get_cam_para reads."""
    def __init__(self, *a, **k):
        self.rotation_matrix = np.eye(3)


def put(out, key, value):
    value = np.asarray(value)
    if value.size > CC.LARGE:
        out[f'{key}/sha'] = np.array(CC.digest(value))
        out[f'{key}/sample'] = CC.strided(value)
        out[f'{key}/shape'] = np.array(value.shape, dtype=np.int64)
    else:
        out[key] = value


def bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16).numpy()


def labels_of(metres, ds):
    d0, d1, _ = CC.D_BOUND
    t = torch.from_numpy(metres)
    return (torch.clamp(t[..., ::ds, ::ds], d0, d1 - 1) - d0).long().numpy()


def save_png(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)
    assert np.array_equal(np.asarray(Image.open(path)), array)             # lossless


def main():
    from PIL import Image
    CD, CA = load_reference()
    DS = CD.CarlaDataset
    out = {'meta/normaliser': np.array('PARITY UNPINNED: torchvision ToTensor + Normalize restated from their published source '
                                       '(scripts/make_golden_carla.normalise_image); window and channel order are the reference\'s own'),
           'meta/quaternion': np.array('get_cam_para ran with a stand-in Quaternion: extrinsics not stored, parity with pyquaternion '
                                       'unpinned; intrinsics are the reference\'s')}
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CC.FRAME_CASES.items():
            frames = CC.build_frames(name)
            res = []
            for img in frames:
                rgb = img[:, :, :3][:, :, ::-1] if c['order'] == 'bgr' else img[:, :, :3]
                res.append(normalise_image(np.array(CD.scale_and_crop_image(Image.fromarray(np.ascontiguousarray(rgb)), scale=1,
                                                                            crop=c['crop']))))
            res = torch.stack(res)
            assert tuple(res.shape) == (c['n'], 3, c['crop'], c['crop']) and res.dtype == torch.float32
            out[f'frames/{name}/sha'] = np.array(CC.digest(frames))
            put(out, f'frames/{name}/out', res.numpy())
            put(out, f'frames/{name}/bf16', bf16_bits(res))
        for name, c in CC.DEPTH_CASES.items():
            frames = CC.build_depth(name)
            res = []
            for i, img in enumerate(frames):
                path = os.path.join(tmp, f'depth_{name}_{i}.png')
                save_png(img, path)
                res.append(DS.get_depth(None, np.array(CD.scale_and_crop_image(Image.open(path), scale=1., crop=c['crop']))).numpy())
            res = np.stack(res)
            assert res.dtype == np.float64 and res.shape == (c['n'], c['crop'], c['crop'])
            out[f'depth/{name}/sha'] = np.array(CC.digest(frames))
            put(out, f'depth/{name}/metres', res)
            out[f'depth/{name}/labels'] = labels_of(res, c['ds']).astype(np.int16)
        ids = out['depth/planted/labels']
        assert set(range(48)) <= set(ids.reshape(-1).tolist())             # every class id is reached by a planted code
        for name, c in CC.HDMAP_CASES.items():
            frames = CC.build_hdmap(name)
            res = []
            for i, img in enumerate(frames):
                path = os.path.join(tmp, f'hdmap_{name}_{i}.png')
                save_png(img, path)
                res.append(DS.get_hdmap(None, path, 1., c['crop']))
            res = np.stack(res)
            assert res.shape == (c['n'], 2, c['crop'], c['crop']) and set(np.unique(res)) <= {0, 1}
            assert res[:, 0].sum() > 0 and (res[:, 1] >= res[:, 0]).all() and res[:, 1].sum() > res[:, 0].sum()
            out[f'hdmap/{name}/sha'] = np.array(CC.digest(frames))
            out[f'hdmap/{name}/out'] = CC.pack(res)
        for name, c in CC.TOPDOWN_CASES.items():
            frames = CC.build_topdown(name)
            veh, ped = [], []
            for i, img in enumerate(frames):
                path = os.path.join(tmp, f'topdown_{name}_{i}.png')
                save_png(img, path)
                v, p = DS.get_labels(None, path, CC.TOPDOWN_SCALE, c['crop'])
                veh.append(v)
                ped.append(p)
            veh, ped = np.stack(veh), np.stack(ped)
            assert veh.shape == (c['n'], c['crop'], c['crop']) and veh.dtype == np.float64 and veh.sum() > 0 and ped.sum() > 0
            out[f'topdown/{name}/sha'] = np.array(CC.digest(frames))
            out[f'topdown/{name}/vehicle'], out[f'topdown/{name}/pedestrian'] = CC.pack(veh), CC.pack(ped)

        # ---- one recorded sequence through __getitem__ itself, and the host arithmetic of the other pose sequences through it too
        s = CC.SAMPLE
        t, n = s['receptive_field'], s['receptive_field'] + s['n_future']
        sample, poses = CC.build_sample(), CC.host_poses()
        cams = ('front', 'left', 'right', 'rear')
        files = {k: [] for k in cams + tuple(f'{c}_depth' for c in cams) + ('hdmap', 'topdown')}
        for i in range(t):
            for j, cam in enumerate(cams):
                for kind, src in (('', sample['images']), ('_depth', sample['depths'])):
                    path = os.path.join(tmp, f'seq_{cam}{kind}_{i}.png')
                    save_png(src[i, j], path)
                    files[cam + kind].append(path)
            path = os.path.join(tmp, f'seq_hdmap_{i}.png')
            save_png(sample['hdmaps'][i], path)
            files['hdmap'].append(path)
        for i in range(n):
            path = os.path.join(tmp, f'seq_topdown_{i}.png')
            save_png(sample['topdowns'][i], path)
            files['topdown'].append(path)
        keep_q, CD.Quaternion = CD.Quaternion, _Quaternion
        try:
            for k, pose in enumerate(poses):
                cfg = NS(N_FUTURE_FRAMES=s['n_future'], TIME_RECEPTIVE_FIELD=t, PLANNING=NS(SAMPLE_NUM=30))
                ds = NS(cfg=cfg, receptive_field=t, sequence_length=n, n_samples=30, normalise_image=normalise_image,
                        SAMPLE_INTERVAL=DS.SAMPLE_INTERVAL,
                        x=[list(pose['x'])], y=[list(pose['y'])], theta=[list(pose['theta'])], x_command=[pose['x_command']],
                        y_command=[pose['y_command']], command=[pose['command']], steer=[pose['steer']],
                        throttle=[pose['throttle']], brake=[pose['brake']], velocity=[pose['velocity']],
                        topdown=[files['topdown']])
                for cam in cams:
                    setattr(ds, cam, [files[cam]])
                    setattr(ds, f'{cam}_depth', [files[f'{cam}_depth']])
                ds.hdmap = [files['hdmap']]
                for fn in ('get_depth', 'get_hdmap', 'get_labels', 'get_cam_para', 'get_future_egomotion', 'get_trajectory_sampling'):
                    setattr(ds, fn, types.MethodType(getattr(DS, fn), ds))
                data = DS.__getitem__(ds, 0)
                out[f'host/{k}/gt_trajectory'] = data['gt_trajectory'].numpy()
                out[f'host/{k}/target_point'] = data['target_point'].numpy()
                out[f'host/{k}/command'] = np.array(data['command'])
                out[f'host/{k}/future_egomotion'] = data['future_egomotion'].numpy()
                assert data['future_egomotion'].dtype == torch.float32 and data['gt_trajectory'].dtype == torch.float64
                # the agent's command point: carla_agent.py:349-357 (inline in tick), compass = the present theta
                theta_now = 0.0 if np.isnan(pose['theta'][t - 1]) else pose['theta'][t - 1]
                theta = theta_now + np.pi / 2
                R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
                point = np.array([pose['x_command'] - pose['x'][t - 1], pose['y_command'] - pose['y'][t - 1]])
                out[f'host/{k}/agent_point'] = R.T.dot(point) * [1.0, -1.0]
                if k == 0:
                    out['sample/sha'] = np.array(CC.digest(*(sample[key] for key in ('images', 'depths', 'hdmaps', 'topdowns'))))
                    put(out, 'sample/image', data['image'].numpy())
                    put(out, 'sample/depths', data['depths'].numpy())
                    for key in ('segmentation', 'pedestrian', 'hdmap'):
                        out[f'sample/{key}'] = CC.pack(data[key].numpy())
                    out['sample/intrinsics'] = data['intrinsics'].numpy()
                    out['sample/shapes'] = np.array(sorted(f'{key}:{tuple(v.shape)}:{v.dtype}' for key, v in data.items()
                                                           if torch.is_tensor(v)))
                    out['sample/keys'] = np.array(sorted(data))
        finally:
            CD.Quaternion = keep_q
    # transform_2d_points on points of its own
    pts = np.random.RandomState(5).uniform(-20, 20, size=(6, 3))
    out['host/transform/points'] = pts
    out['host/transform/out'] = CD.transform_2d_points(pts, 0.3, -4.0, 2.5, -1.1, 7.0, -3.0)
    # the agent's future_egomotion is the same function; called here on the window of the first poses
    agent = NS()
    out['host/agent_egomotion'] = CA.MVPAgent.get_future_egomotion(agent, poses[1]['x'][:3], poses[1]['y'][:3], poses[1]['theta'][:3]).numpy()
    # the controllers
    wp, speed = CC.control_sequence()
    agent = NS(turn_controller=CA.PIDController(K_P=1.25, K_I=0.75, K_D=0.3, n=40),
               speed_controller=CA.PIDController(K_P=5.0, K_I=0.5, K_D=1.0, n=40))
    rows, meta = [], []
    for i in range(len(wp)):
        steer, throttle, brake, metadata = CA.MVPAgent.control_pid(agent, torch.from_numpy(wp[i]), torch.from_numpy(speed[i:i + 1]),
                                                                    {'next_command': 4})
        rows.append([float(steer), float(throttle), float(brake)])
        meta.append([metadata[k] for k in ('speed', 'steer', 'throttle', 'brake', 'desired_speed', 'angle', 'delta')] +
                    list(metadata['aim']) + [v for k in ('wp_1', 'wp_2', 'wp_3', 'wp_4') for v in metadata[k]])
    out['host/control/sha'] = np.array(CC.digest(wp, speed))
    out['host/control/out'] = np.array(rows, dtype=np.float64)
    out['host/control/metadata'] = np.array(meta, dtype=np.float64)
    assert 5 < out['host/control/out'][:, 2].sum() < 55                     # both branches of the brake
    pid = CA.PIDController(K_P=1.25, K_I=0.75, K_D=0.3, n=40)
    errors = np.random.RandomState(6).uniform(-1, 1, size=60)
    out['host/pid/errors'] = errors
    out['host/pid/out'] = np.array([pid.step(e) for e in errors])
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'entries')


if __name__ == '__main__':
    main()
