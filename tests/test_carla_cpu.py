"""CPU: the CARLA decoder and host arithmetic (stp3_amd.carla; csrc/stp3_carla.hip) against the reference's own
stp3/datas/CarlaData.py and carla_agent.py, recorded by scripts/make_golden_carla.py in tests/golden/carla.npz on the cases of
tests/carla_cases.py (the inputs are rebuilt here; their sha256 is checked before anything else).

Everything is compared EXACTLY.  Camera images: the float32 statements x / 255, (x - mean) / std are two correctly rounded
divisions on both sides; bf16 is the rounding of that float32.  Depth: one IEEE float64 statement on both sides, so even the
planted codes either side of every class boundary need no exclusion list.  Maps are 0 / 1.  The host functions run the same numpy
and torch statements as the reference on the same machine.  The camera rotation is pinned against the closed form (a rotation by
yaw about z in float64, cast to float32) within 2**-23 -- the entries are at most 1 in magnitude and the only error is the cast;
parity with pyquaternion unpinned (the fixture's generator ran with a stand-in).  The resize tables are checked against Pillow's
``Image.resize(..., NEAREST)`` itself."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import carla_cases as CC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
MAP_DTYPES = {'f32': torch.float32, 'f64': torch.float64, 'i64': torch.int64}


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(H.load('carla.npz'))


@functools.lru_cache(maxsize=None)
def built(kind, name):
    """The input bytes of a case, after their digest has been compared with the fixture's."""
    frames = {'frames': CC.build_frames, 'depth': CC.build_depth, 'hdmap': CC.build_hdmap, 'topdown': CC.build_topdown}[kind](name)
    assert CC.digest(frames) == str(fixture()[f'{kind}/{name}/sha']), f'{kind}/{name}: the case builder drifted'
    return frames


def same(got, key, what):
    """``got`` against the fixture entry ``key``: the array itself, or its digest and strided sample for a large one."""
    g = fixture()
    got = np.asarray(got)
    if f'{key}/sha' in g:
        assert got.shape == tuple(g[f'{key}/shape']) and got.dtype == g[f'{key}/sample'].dtype, (what, key, got.shape, got.dtype)
        assert np.array_equal(CC.strided(got), g[f'{key}/sample']), f'{what}: {key} (sample)'
        assert CC.digest(got) == str(g[f'{key}/sha']), f'{what}: {key} (digest)'
    else:
        assert got.shape == g[key].shape and got.dtype == g[key].dtype, (what, key, got.shape, got.dtype)
        assert np.array_equal(got, g[key]), f'{what}: {key}, {int((got != g[key]).sum())} elements differ'


def same_bits(got, key, what):
    got = np.asarray(got)
    assert set(np.unique(got).tolist()) <= {0, 1}, (what, key)
    assert np.array_equal(CC.pack(got), fixture()[key]), f'{what}: {key}'


def decoder(kind, name):
    from stp3_amd.carla import CarlaDecoder
    if kind == 'frames':
        return CarlaDecoder(crop=CC.FRAME_CASES[name]['crop'])
    if kind == 'depth':
        return CarlaDecoder(crop=CC.DEPTH_CASES[name]['crop'], downsample=CC.DEPTH_CASES[name]['ds'], d_bound=CC.D_BOUND)
    if kind == 'hdmap':
        return CarlaDecoder(bev_crop=CC.HDMAP_CASES[name]['crop'])
    return CarlaDecoder(bev_crop=CC.TOPDOWN_CASES[name]['crop'], topdown_scale=CC.TOPDOWN_SCALE)


# ---- the checks shared with tests/test_carla_gpu.py: ``run`` maps a method name to the callable under test ----------------
def check_frames(name, images, what):
    c = CC.FRAME_CASES[name]
    frames = torch.from_numpy(built('frames', name))
    out = images(frames, order=c['order'])
    assert out.dtype == torch.float32 and tuple(out.shape) == (c['n'], 3, c['crop'], c['crop'])
    same(out.cpu().numpy(), f'frames/{name}/out', what)
    half = images(frames, order=c['order'], out_dtype=torch.bfloat16)
    assert half.dtype == torch.bfloat16
    same(half.cpu().view(torch.int16).numpy(), f'frames/{name}/bf16', what)


def check_depth(name, depths, what):
    c = CC.DEPTH_CASES[name]
    frames = torch.from_numpy(built('depth', name))
    d64 = depths(frames, out_dtype=torch.float64)
    assert d64.dtype == torch.float64 and tuple(d64.shape) == (c['n'], c['crop'], c['crop'])
    same(d64.cpu().numpy(), f'depth/{name}/metres', what)
    d32 = depths(frames)
    assert d32.dtype == torch.float32 and torch.equal(d32.cpu(), d64.cpu().float()), what
    ids = depths(frames, labels=True)
    side = -(-c['crop'] // c['ds'])
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (c['n'], side, side)
    assert np.array_equal(ids.cpu().numpy(), fixture()[f'depth/{name}/labels']), f'{what}: class ids of depth/{name}'
    assert torch.equal(ids.cpu(), decoder('depth', name).class_ids(d64.cpu())), what


def check_hdmap(name, hdmap, what):
    c = CC.HDMAP_CASES[name]
    frames = torch.from_numpy(built('hdmap', name))
    for key, dtype in MAP_DTYPES.items():
        out = hdmap(frames, out_dtype=dtype)
        assert out.dtype == dtype and tuple(out.shape) == (c['n'], 2, c['crop'], c['crop'])
        same_bits(out.cpu().numpy(), f'hdmap/{name}/out', f'{what} ({key})')
    assert bool((out[:, 1] >= out[:, 0]).all()) and int(out[:, 0].sum()) > 0         # a lane pixel is drivable


def check_topdown(name, topdown, what):
    c = CC.TOPDOWN_CASES[name]
    frames = torch.from_numpy(built('topdown', name))
    for key, dtype in MAP_DTYPES.items():
        veh, ped = topdown(frames, out_dtype=dtype)
        assert veh.dtype == dtype and tuple(veh.shape) == tuple(ped.shape) == (c['n'], 1, c['crop'], c['crop'])
        same_bits(veh.cpu().numpy(), f'topdown/{name}/vehicle', f'{what} ({key})')
        same_bits(ped.cpu().numpy(), f'topdown/{name}/pedestrian', f'{what} ({key})')


def check_all(kind, name, dec, what, device='cpu'):
    to = lambda fn: (lambda frames, **kw: fn(frames.to(device), **kw))                  # noqa: E731
    if kind == 'frames':
        check_frames(name, to(dec['images']), what)
    elif kind == 'depth':
        check_depth(name, to(dec['depths']), what)
    elif kind == 'hdmap':
        check_hdmap(name, to(dec['hdmap']), what)
    else:
        check_topdown(name, to(dec['topdown']), what)


ALL_CASES = ([('frames', n) for n in CC.FRAME_CASES] + [('depth', n) for n in CC.DEPTH_CASES] +
             [('hdmap', n) for n in CC.HDMAP_CASES] + [('topdown', n) for n in CC.TOPDOWN_CASES])


def test_fixture_holds_data_only_and_has_its_properties():
    g = fixture()
    assert os.path.getsize(os.path.join(H.GOLDEN, 'carla.npz')) <= 1 << 20
    assert all(v.dtype.kind in 'iufU' for v in g.values())                              # numbers and strings: no objects
    assert 'PARITY UNPINNED' in str(g['meta/normaliser']) and 'pyquaternion' in str(g['meta/quaternion'])
    assert sorted({k.split('/')[1] for k in g if k.startswith('frames/')}) == sorted(CC.FRAME_CASES)
    # every class id 0..47 is decided by a planted code, and neighbours one code apart fall into different classes
    ids = g['depth/planted/labels'].reshape(-1)[:98]
    assert ids[0] == 0 and ids[1] == 47 and all(ids[2 + 2 * j + 1] - ids[2 + 2 * j] == 1 for j in range(1, 48))
    assert g['depth/planted/metres'].shape == (11, 20, 20) and g['depth/planted/labels'].shape == (11, 3, 3)
    # the window of the 3-channel 11 x 13 source with crop 6 starts at an unaligned byte
    assert ((11 // 2 - 3) * 13 + (13 // 2 - 3)) * 3 % 4 != 0
    # the ego box matters where it lies inside the window: without it the vehicle map differs
    from stp3_amd import carla
    frames = torch.from_numpy(built('topdown', 't500_c100'))
    keep, carla.EGO_BOX = carla.EGO_BOX, (0, 0, 0, 0)
    try:
        veh = decoder('topdown', 't500_c100').reference_topdown(frames)[0]
    finally:
        carla.EGO_BOX = keep
    assert not np.array_equal(CC.pack(veh.numpy()), g['topdown/t500_c100/vehicle'])


@pytest.mark.parametrize('kind,name', ALL_CASES, ids=[f'{k}-{n}' for k, n in ALL_CASES])
def test_torch_statements_match_the_reference(kind, name):
    dec = decoder(kind, name)
    twins = {'images': dec.reference_images, 'depths': dec.reference_depths, 'hdmap': dec.reference_hdmap, 'topdown': dec.reference_topdown}
    check_all(kind, name, twins, 'reference_* twins')
    # CPU tensors take that route through the public methods
    check_all(kind, name, {'images': dec.images, 'depths': dec.depths, 'hdmap': dec.hdmap, 'topdown': dec.topdown}, 'CPU tensors')


def test_leading_dimensions_are_kept():
    dec = decoder('frames', 'f6_rgb3_n5')
    frames = torch.from_numpy(built('frames', 'f6_rgb3_n5'))[:4].reshape(2, 2, 11, 13, 3)
    assert tuple(dec.images(frames).shape) == (2, 2, 3, 6, 6)
    assert torch.equal(dec.images(frames).reshape(4, 3, 6, 6), dec.images(frames.reshape(4, 11, 13, 3)))
    dec = decoder('topdown', 't23_c7')
    frames = torch.from_numpy(built('topdown', 't23_c7')).reshape(2, 1, 23, 29)
    assert all(tuple(m.shape) == (2, 1, 1, 7, 7) for m in dec.topdown(frames))


@pytest.mark.parametrize('n_src,n_out', [(23, 20), (29, 26), (500, 454), (512, 465), (7, 7), (300, 272)])
def test_nearest_axis_is_pillows(n_src, n_out):
    Image = pytest.importorskip('PIL.Image')
    from stp3_amd.carla import CarlaDecoder
    tab = CarlaDecoder.nearest_axis(n_src, n_out)
    assert tab.dtype == np.int32 and tab.shape == (n_out,)
    ramp = np.arange(n_src, dtype=np.int32)
    along_x = np.asarray(Image.fromarray(np.tile(ramp, (3, 1))).resize((n_out, 3), resample=Image.NEAREST))
    along_y = np.asarray(Image.fromarray(np.tile(ramp[:, None], (1, 3))).resize((3, n_out), resample=Image.NEAREST))
    assert np.array_equal(along_x[0], tab) and np.array_equal(along_y[:, 0], tab)
    # and on bytes, both axes at once (the mode get_labels reads)
    img = np.random.RandomState(n_src).randint(0, 256, size=(n_src, n_src)).astype(np.uint8)
    want = np.asarray(Image.fromarray(img).resize((n_out, n_out), resample=Image.NEAREST))
    assert np.array_equal(img[tab][:, tab], want)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------
def test_host_functions_match_the_reference():
    from stp3_amd import carla
    g = fixture()
    for k, pose in enumerate(CC.host_poses()):
        theta = [0.0 if np.isnan(t) else t for t in pose['theta']]
        ego = carla.future_egomotion(pose['x'], pose['y'], theta)
        assert ego.dtype == torch.float32 and np.array_equal(ego.numpy(), g[f'host/{k}/future_egomotion'])
        gt = carla.gt_trajectory(pose['x'], pose['y'], pose['theta'], 3)               # (the nan theta is fixed inside)
        assert gt.dtype == torch.float64 and tuple(gt.shape) == (5, 3) and np.array_equal(gt.numpy(), g[f'host/{k}/gt_trajectory'])
        point = carla.local_command_point((pose['x'][2], pose['y'][2]), theta[2], (pose['x_command'], pose['y_command']))
        assert point.dtype == torch.float64 and np.array_equal(point.numpy(), g[f'host/{k}/target_point'])
        assert np.array_equal(point.numpy(), g[f'host/{k}/agent_point'])                # the agent's statement: the same numbers
        assert carla.command_name(pose['command']) == str(g[f'host/{k}/command'])
    assert [carla.command_name(c) for c in (1, 2, 3, 4, 0, -1)] == ['LEFT', 'RIGHT', 'FORWARD', 'LANE', 'LANE', 'LANE']
    pose = CC.host_poses()[1]
    assert np.array_equal(carla.future_egomotion(pose['x'][:3], pose['y'][:3], pose['theta'][:3]).numpy(), g['host/agent_egomotion'])
    out = carla.transform_2d_points(g['host/transform/points'], 0.3, -4.0, 2.5, -1.1, 7.0, -3.0)
    assert np.array_equal(out, g['host/transform/out'])


def test_pid_and_control_match_the_reference_over_60_steps():
    from stp3_amd import carla
    g = fixture()
    pid = carla.turn_controller()
    assert np.array_equal(np.array([pid.step(e) for e in g['host/pid/errors']]), g['host/pid/out'])
    wp, speed = CC.control_sequence()
    assert CC.digest(wp, speed) == str(g['host/control/sha'])
    turn, spd = carla.turn_controller(), carla.speed_controller()
    for i in range(60):
        steer, throttle, brake, meta = carla.control_pid(torch.from_numpy(wp[i]), torch.from_numpy(speed[i:i + 1]), turn, spd, command=4)
        assert [float(steer), float(throttle), float(brake)] == g['host/control/out'][i].tolist(), i
        row = ([meta[k] for k in ('speed', 'steer', 'throttle', 'brake', 'desired_speed', 'angle', 'delta')] + list(meta['aim']) +
               [v for k in ('wp_1', 'wp_2', 'wp_3', 'wp_4') for v in meta[k]])
        assert row == g['host/control/metadata'][i].tolist() and meta['command'] == 4, i
    # arrays are taken as well as tensors, and the controllers were advanced: a fresh pair repeats step 0 only
    again = carla.control_pid(wp[0], speed[0], carla.turn_controller(), carla.speed_controller())
    assert [float(v) for v in again[:3]] == g['host/control/out'][0].tolist()


def test_cam_para():
    """Rotation: the closed form, within the float32 cast (parity with pyquaternion unpinned).  Intrinsics: the fixture's."""
    from stp3_amd import carla
    extrinsics, intrinsics = carla.cam_para()
    assert extrinsics.dtype == torch.float32 and tuple(extrinsics.shape) == (4, 4, 4) and tuple(intrinsics.shape) == (4, 3, 3)
    for cam, (x, y, z, _, _, yaw) in zip(extrinsics, carla.CAMERAS):
        a = np.float64(yaw) * np.pi / 180
        want = np.array([[np.cos(a), -np.sin(a), 0, x], [np.sin(a), np.cos(a), 0, y], [0, 0, 1, z], [0, 0, 0, 1]]).astype(np.float32)
        assert np.abs(cam.numpy().astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    assert [c[5] for c in carla.CAMERAS] == [0.0, -60.0, 60.0, 180.0]
    assert intrinsics.dtype == torch.float32 and np.array_equal(intrinsics.numpy(), fixture()['sample/intrinsics'][0])


def test_assemble_carla_sample_is_getitem():
    from stp3_amd.carla import CarlaDecoder, assemble_carla_sample
    g = fixture()
    sample, pose = CC.build_sample(), CC.host_poses()[0]
    assert CC.digest(*(sample[k] for k in ('images', 'depths', 'hdmaps', 'topdowns'))) == str(g['sample/sha'])
    dec = CarlaDecoder(downsample=CC.DOWNSAMPLE, d_bound=CC.D_BOUND)
    data = assemble_carla_sample(dec, *(torch.from_numpy(sample[k]) for k in ('images', 'depths', 'hdmaps', 'topdowns')),
                                 pose['x'], pose['y'], pose['theta'], pose['x_command'], pose['y_command'], pose['command'],
                                 pose['steer'], pose['throttle'], pose['brake'], pose['velocity'], receptive_field=3, sample_num=30)
    assert sorted(data) == g['sample/keys'].tolist()
    shapes = sorted(f'{k}:{tuple(v.shape)}:{v.dtype}' for k, v in data.items() if torch.is_tensor(v))
    assert shapes == g['sample/shapes'].tolist()
    same(data['image'].numpy(), 'sample/image', 'assemble_carla_sample')
    same(data['depths'].numpy(), 'sample/depths', 'assemble_carla_sample')
    for k in ('segmentation', 'pedestrian', 'hdmap'):
        same_bits(data[k].numpy(), f'sample/{k}', 'assemble_carla_sample')
    assert np.array_equal(data['intrinsics'].numpy(), g['sample/intrinsics'])
    for k in ('gt_trajectory', 'target_point', 'future_egomotion'):
        assert np.array_equal(data[k].numpy(), g[f'host/0/{k}']), k
    assert data['command'] == 'LEFT' and (data['steer'], data['throttle'], data['brake'], data['velocity']) == \
        (pose['steer'], pose['throttle'], pose['brake'], pose['velocity'])
    assert tuple(data['sample_trajectory'].shape) == (30, 5, 3) and not data['sample_trajectory'][:, 0].any()


def test_wrapper_raises():
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(crop=6, bev_crop=4)
    ok = torch.zeros(1, 11, 13, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        dec.images(torch.zeros(1, 5, 13, 3, dtype=torch.uint8))                         # Hs < crop
    with pytest.raises(ValueError):
        dec.images(torch.zeros(1, 11, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        dec.hdmap(torch.zeros(1, 9, 11, 4, dtype=torch.uint8))                          # a 4-channel hd map
    with pytest.raises(ValueError):
        dec.images(ok.float())                                                          # not uint8
    with pytest.raises(ValueError):
        dec.depths(ok.to(torch.int32))
    with pytest.raises(ValueError):
        dec.topdown(torch.zeros(1, 9, 11))
    with pytest.raises(ValueError):
        dec.images(ok, order='gbr')
    with pytest.raises(ValueError):
        dec.images(ok, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        dec.images(torch.zeros(1, 11, 13, 2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        dec.depths(ok, labels=True)                                                     # no downsample / d_bound
    with pytest.raises(ValueError):
        dec.hdmap(torch.zeros(1, 9, 11, 3, dtype=torch.uint8), out_dtype=torch.int32)
    with pytest.raises(ValueError):
        dec.topdown(torch.zeros(1, 4, 4, dtype=torch.uint8))                            # resized 3 x 3 < 4
    with pytest.raises(ValueError):
        CarlaDecoder(scale=0.5)


def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                       # never dereferenced: every call below is refused first
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    frames = lambda **k: lib.stp3_carla_frames(*[{**dict(n=4, Hs=300, Ws=400, Cs=4, crop=256, bgr=1), **k}[a] for a in      # noqa: E731
                                                 ('n', 'Hs', 'Ws', 'Cs', 'crop', 'bgr')], mean, mean, k.get('dtype', 0), fake, fake, None)
    for bad in (dict(n=0), dict(Hs=255), dict(Ws=100), dict(Cs=2), dict(Cs=5), dict(crop=0), dict(bgr=2)):
        assert frames(**bad) == -10001, bad
    assert frames(dtype=2) == -10002 and frames(n=70000) == -10002
    assert lib.stp3_carla_frames(4, 300, 400, 4, 256, 1, mean, mean, 0, None, fake, None) == -10001
    assert lib.stp3_carla_depth(4, 300, 400, 256, 3, 8, 2.0, 49.0, fake, fake, None) == -10001             # unknown kind
    assert lib.stp3_carla_depth(4, 300, 400, 256, 2, 0, 2.0, 49.0, fake, fake, None) == -10001             # labels, downsample 0
    assert lib.stp3_carla_depth(4, 300, 400, 256, 2, 8, 50.0, 49.0, fake, fake, None) == -10001
    assert lib.stp3_carla_depth(4, 200, 400, 256, 0, 1, 0.0, 0.0, fake, fake, None) == -10001
    assert lib.stp3_carla_hdmap(1, 199, 300, 200, 0, fake, fake, None) == -10001
    assert lib.stp3_carla_hdmap(1, 300, 300, 200, 3, fake, fake, None) == -10001
    assert lib.stp3_carla_hdmap(1, 300, 300, 200, 0, fake, None, None) == -10001
    assert lib.stp3_carla_topdown(1, 500, 500, 454, 199, 200, fake, fake, 0, fake, fake, fake, None) == -10001
    assert lib.stp3_carla_topdown(1, 500, 500, 454, 454, 200, None, fake, 0, fake, fake, fake, None) == -10001
    assert lib.stp3_carla_topdown(1, 500, 500, 454, 454, 200, fake, fake, 0, fake, fake, None, None) == -10001


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
def run_host(tmp, lib, order, *extra):
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if order:
        env['HIPCPU_ORDER'] = order
    path = str(tmp / f'out_{order or "plain"}{"_".join(extra)}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_carla.py'), lib, path, *extra], env=env, capture_output=True,
                         text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(path))


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_carla')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_carla.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    return request.param or 'plain', run_host(*host_lib, request.param)


def check_host(out, real, what):
    for kind, name in ALL_CASES:
        if (name in CC.REAL_SIZE[kind]) != real:
            continue
        stored = lambda key: torch.from_numpy(out[f'{kind}/{name}/{key}'])                                   # noqa: E731
        if kind == 'frames':
            check_frames(name, lambda f, order, out_dtype=torch.float32: stored('out') if out_dtype == torch.float32
                         else stored('bf16').view(torch.bfloat16), what)
        elif kind == 'depth':
            check_depth(name, lambda f, labels=False, out_dtype=torch.float32: stored('labels') if labels
                        else stored('f64' if out_dtype == torch.float64 else 'f32'), what)
        elif kind == 'hdmap':
            check_hdmap(name, lambda f, out_dtype: stored({v: k for k, v in MAP_DTYPES.items()}[out_dtype]), what)
        else:
            want_v, want_p = fixture()[f'topdown/{name}/vehicle'], fixture()[f'topdown/{name}/pedestrian']
            assert out[f'topdown/{name}/vehicle'].dtype == np.float64 and out[f'topdown/{name}/vehicle_i64'].dtype == np.int64
            assert np.array_equal(CC.pack(out[f'topdown/{name}/vehicle']), want_v), (what, name)
            assert np.array_equal(CC.pack(out[f'topdown/{name}/vehicle_i64']), want_v), (what, name)
            assert np.array_equal(CC.pack(out[f'topdown/{name}/pedestrian']), want_p), (what, name)
            assert set(np.unique(out[f'topdown/{name}/vehicle']).tolist()) <= {0.0, 1.0}


def test_kernels_on_host_match_the_reference(host_kernel):
    order, out = host_kernel
    check_host(out, False, f'kernels on the host ({order} order)')


def test_kernels_on_host_match_the_reference_at_the_real_shapes(host_lib):
    """300 x 400 x 4 BGRA -> 256 x 256 (4 images), the depth images of that size, a 500 x 500 top-down image."""
    check_host(run_host(*host_lib, 'random', 'real'), True, 'kernels on the host (random order), real shapes')
