"""GPU: the CARLA decoder kernels (csrc/stp3_carla.hip through stp3_amd.carla.CarlaDecoder) and ``ClosedLoopDriver`` on the MI355X
(CPU side, fixture and comparison rules: tests/test_carla_cpu.py).

DECODER.  Every fixture case of tests/carla_cases.py on device tensors, EXACTLY; each kernel against its ``reference_*`` twin run on
the GPU on random bytes (unaligned windows, odd sizes, 3 and 4 channels, both channel orders, more than one workgroup per image,
the real shapes), bit for bit; a second call is bit-equal to the first; the four decode calls captured into ONE ``torch.cuda.graph``
and replayed on other bytes through the same buffers; a guard band behind every output stays untouched.

DRIVER.  THE ORACLE IS PARENT CODE: a Planning-shaped model (tests/test_planning_cpu.PLANNING at IMAGE.FINAL_DIM 256 x 256, the
CARLA window) with N = 4 cameras and T = 3; 7 ticks of seeded BGRA frames and poses.  Ticks 1-4 return zero control; on ticks 5-7
trajectory and control are bit-equal to the same tick written out here from existing public pieces: ``CarlaDecoder.reference_images``,
``model.eval()`` under bf16 autocast with the per-frame encoder shim of tests/test_streaming_gpu.py, argmax / logical_or /
``model.planning(...)``, and the fixture-checked ``control_pid``.  ``reset()`` mid-sequence restarts the warm-up.
One more case, beyond that: ``ClosedLoopDriver(planner='drive')`` against the same tick with ``ops_plan.plan_scene`` + ``Planning.drive``
as its planner step (bit-reproducible kernels), again bit for bit.  The two planner steps are NOT bit-equal to each other:
``Planning.drive`` refines in float32, ``model.planning`` under bf16 autocast in bf16 (measured here: way points differ by up to
2.4e-3 m); the largest difference is printed."""
import gc

import numpy as np
import pytest
import torch

from tests import carla_cases as CC
from tests import test_carla_cpu as TC

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.mark.parametrize('kind,name', TC.ALL_CASES, ids=[f'{k}-{n}' for k, n in TC.ALL_CASES])
def test_fixture_cases_on_the_device(kind, name):
    dec = TC.decoder(kind, name)
    TC.check_all(kind, name, {'images': dec.images, 'depths': dec.depths, 'hdmap': dec.hdmap, 'topdown': dec.topdown},
                 'kernels on the GPU', device='cuda')


def _bytes(shape, seed, values=None):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, size=shape).astype(np.uint8) if values is None else np.array(values, dtype=np.uint8)[rs.randint(0, len(values), size=shape)]
    return torch.from_numpy(a).cuda()


def _equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    print(f'[carla] {what}: {bad} of {got.numel()} elements differ from the torch statements on the GPU')
    assert bad == 0, what


@pytest.mark.parametrize('shape,crop', [((5, 11, 13, 3), 6), ((5, 11, 13, 4), 7), ((3, 37, 41, 3), 31), ((2, 40, 36, 4), 32),
                                        ((4, 300, 400, 4), 256), ((2, 300, 400, 3), 256)])
def test_frames_equal_the_torch_statements_on_the_gpu(shape, crop):
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(crop=crop)
    frames = _bytes(shape, seed=sum(shape) + crop)
    for order in ('rgb', 'bgr'):
        for dtype in (torch.float32, torch.bfloat16):
            got = dec.images(frames, order=order, out_dtype=dtype)
            _equal(got, dec.reference_images(frames, order=order, out_dtype=dtype), f'frames {shape} crop {crop} {order} {dtype}')
            _equal(dec.images(frames, order=order, out_dtype=dtype), got, 'second call')
    # an unaligned base pointer of a 4-channel source takes the byte route
    flat = torch.cat([torch.zeros(1, dtype=torch.uint8, device='cuda'), frames.reshape(-1)])
    shifted = flat[1:].view(shape)
    assert shifted.data_ptr() % 4 == 1
    _equal(dec.images(shifted, order='bgr'), dec.reference_images(frames, order='bgr'), 'unaligned base')


@pytest.mark.parametrize('shape,crop,ds', [((3, 11, 13, 3), 7, 2), ((2, 20, 24, 3), 20, 8), ((2, 33, 35, 3), 32, 5),
                                           ((4, 300, 400, 3), 256, 8)])
def test_depth_equals_the_torch_statements_on_the_gpu(shape, crop, ds):
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(crop=crop, downsample=ds, d_bound=CC.D_BOUND)
    frames = _bytes(shape, seed=sum(shape) + ds)
    frames[..., 0] %= 16
    for kw in (dict(out_dtype=torch.float64), dict(out_dtype=torch.float32), dict(labels=True)):
        got = dec.depths(frames, **kw)
        _equal(got, dec.reference_depths(frames, **kw), f'depth {shape} crop {crop} ds {ds} {kw}')
        _equal(dec.depths(frames, **kw), got, 'second call')
    assert torch.equal(dec.depths(frames, labels=True), dec.class_ids(dec.depths(frames, out_dtype=torch.float64)))


@pytest.mark.parametrize('shape,crop', [((3, 9, 11, 3), 4), ((2, 33, 37, 3), 33), ((2, 210, 214, 3), 200)])
def test_hdmap_equals_the_torch_statements_on_the_gpu(shape, crop):
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(bev_crop=crop)
    rs = np.random.RandomState(crop)
    frames = torch.from_numpy(np.array(CC.PALETTE, dtype=np.uint8)[rs.randint(0, len(CC.PALETTE), size=shape[:3])]).cuda()
    for dtype in TC.MAP_DTYPES.values():
        got = dec.hdmap(frames, out_dtype=dtype)
        _equal(got, dec.reference_hdmap(frames, out_dtype=dtype), f'hdmap {shape} crop {crop} {dtype}')
        _equal(dec.hdmap(frames, out_dtype=dtype), got, 'second call')
    assert int(got[:, 0].sum()) > 0 and bool((got[:, 1] >= got[:, 0]).all())


@pytest.mark.parametrize('shape,crop', [((3, 23, 29), 7), ((2, 23, 29), 20), ((2, 300, 250), 200), ((1, 512, 512), 100)])
def test_topdown_equals_the_torch_statements_on_the_gpu(shape, crop):
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(bev_crop=crop)
    frames = _bytes(shape, seed=crop + shape[1], values=CC.TOPDOWN_CLASSES)
    for dtype in TC.MAP_DTYPES.values():
        got = dec.topdown(frames, out_dtype=dtype)
        want = dec.reference_topdown(frames, out_dtype=dtype)
        again = dec.topdown(frames, out_dtype=dtype)
        for k, what in enumerate(('vehicle', 'pedestrian')):
            _equal(got[k], want[k], f'topdown {shape} crop {crop} {dtype} {what}')
            _equal(again[k], got[k], 'second call')


def _decode_all(dec, fr, dp, hd, td):
    return (dec.images(fr, order='bgr'), dec.depths(dp, labels=True), dec.hdmap(hd), *dec.topdown(td))


def _reference_all(dec, fr, dp, hd, td):
    return (dec.reference_images(fr, order='bgr'), dec.reference_depths(dp, labels=True), dec.reference_hdmap(hd),
            *dec.reference_topdown(td))


def test_the_four_decode_calls_in_one_graph():
    from stp3_amd.carla import CarlaDecoder
    dec = CarlaDecoder(crop=32, bev_crop=20, downsample=8, d_bound=CC.D_BOUND)
    shapes = ((4, 40, 36, 4), (4, 40, 36, 3), (3, 25, 27, 3), (7, 31, 29))
    static = [_bytes(s, seed=10 + i, values=v) for i, (s, v) in enumerate(zip(shapes, (None, None, None, CC.TOPDOWN_CLASSES)))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _decode_all(dec, *static)                                   # warm-up: the index tables reach the device
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _decode_all(dec, *static)
    for seed in (50, 60):
        fresh = [_bytes(shapes[0], seed), _bytes(shapes[1], seed + 1),
                 torch.from_numpy(np.array(CC.PALETTE, dtype=np.uint8)[np.random.RandomState(seed).randint(0, 10, size=(3, 25, 27))]).cuda(),
                 _bytes(shapes[3], seed + 2, values=CC.TOPDOWN_CLASSES)]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        for k, (got, want) in enumerate(zip(outs, _reference_all(dec, *fresh))):
            _equal(got, want, f'graph replay (bytes of seed {seed}), output {k}')


def _guarded(numel, dtype):
    buf = torch.full((numel + GUARD,), 7, dtype=dtype, device='cuda')
    return buf, buf[:numel]


def test_a_guard_band_behind_every_output_stays_untouched():
    from stp3_amd import _lib, ops
    from stp3_amd.carla import CarlaDecoder
    lib = _lib.lib()
    dec = CarlaDecoder(crop=7, bev_crop=7, downsample=2, d_bound=CC.D_BOUND)
    stream = ops._stream()
    frames = _bytes((5, 11, 13, 3), 1)
    for dtype in (torch.float32, torch.bfloat16):
        buf, out = _guarded(5 * 3 * 49, dtype)
        dec.images(frames, out_dtype=dtype, out=out.view(5, 3, 7, 7))
        _equal(out.view(5, 3, 7, 7), dec.reference_images(frames, out_dtype=dtype), f'images into a given buffer ({dtype})')
        assert bool((buf[out.numel():] == 7).all())
    for kind, dtype, side, kw in ((_lib.DEPTH_OUT_F64, torch.float64, 7, dict(out_dtype=torch.float64)),
                                  (_lib.DEPTH_OUT_F32, torch.float32, 7, dict(out_dtype=torch.float32)),
                                  (_lib.DEPTH_OUT_LABELS, torch.int64, 4, dict(labels=True))):
        buf, out = _guarded(5 * side * side, dtype)
        _lib.check(lib.stp3_carla_depth(5, 11, 13, 7, kind, 2, 2.0, 49.0, ops._ptr(frames), ops._ptr(out), stream), 'stp3_carla_depth')
        _equal(out.view(5, side, side), dec.reference_depths(frames, **kw), f'depth into a guarded buffer ({dtype})')
        assert bool((buf[out.numel():] == 7).all())
    hd = torch.from_numpy(np.array(CC.PALETTE, dtype=np.uint8)[np.random.RandomState(2).randint(0, 10, size=(5, 11, 13))]).cuda()
    td = _bytes((5, 11, 13), 3, values=CC.TOPDOWN_CLASSES)
    rows, cols = dec._tables(11, 13, td.device)
    hr, wr = dec.topdown_dims(11, 13)
    for key, dtype in TC.MAP_DTYPES.items():
        kind = getattr(_lib, f'CARLA_OUT_{key.upper()}')
        buf, out = _guarded(5 * 2 * 49, dtype)
        _lib.check(lib.stp3_carla_hdmap(5, 11, 13, 7, kind, ops._ptr(hd), ops._ptr(out), stream), 'stp3_carla_hdmap')
        _equal(out.view(5, 2, 7, 7), dec.reference_hdmap(hd, out_dtype=dtype), f'hdmap into a guarded buffer ({dtype})')
        assert bool((buf[out.numel():] == 7).all())
        vbuf, veh = _guarded(5 * 49, dtype)
        pbuf, ped = _guarded(5 * 49, dtype)
        _lib.check(lib.stp3_carla_topdown(5, 11, 13, hr, wr, 7, ops._ptr(rows), ops._ptr(cols), kind, ops._ptr(td), ops._ptr(veh),
                                          ops._ptr(ped), stream), 'stp3_carla_topdown')
        want = dec.reference_topdown(td, out_dtype=dtype)
        _equal(veh.view(5, 1, 7, 7), want[0], f'vehicle into a guarded buffer ({dtype})')
        _equal(ped.view(5, 1, 7, 7), want[1], f'pedestrian into a guarded buffer ({dtype})')
        assert bool((vbuf[veh.numel():] == 7).all()) and bool((pbuf[ped.numel():] == 7).all())


# ---- the driver -----------------------------------------------------------------------------------------------------------
TICKS, SEED = 7, 5


def _tick_inputs():
    """7 ticks: BGRA frames (7, 4, 300, 400, 4) uint8, positions, compass, speed, route command and command point."""
    g = torch.Generator().manual_seed(SEED)
    frames = torch.randint(0, 256, (TICKS, 4, 300, 400, 4), dtype=torch.uint8, generator=g)
    rs = np.random.RandomState(SEED)
    compass = (0.4 + np.cumsum(rs.uniform(-0.05, 0.05, size=TICKS))).tolist()
    step = rs.uniform(0.3, 1.2, size=TICKS)
    x = (12.0 + np.cumsum(step * np.cos(compass))).tolist()
    y = (-7.0 + np.cumsum(step * np.sin(compass))).tolist()
    speed = rs.uniform(1.0, 6.0, size=TICKS).tolist()
    commands = [4, 4, 3, 1, 1, 4, 2]
    wps = [(x[i] + float(rs.uniform(-15, 15)), y[i] + float(rs.uniform(5, 25))) for i in range(TICKS)]
    return frames, list(zip(x, y)), compass, speed, commands, wps


@pytest.fixture(scope='module')
def planning_model():
    from stp3_amd.config import perception_cfg
    from stp3_amd.cost import Cost_Function
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    from tests import helpers as H
    from tests.test_planning_cpu import PLANNING
    # the CARLA configs' window and GRU state: 256 x 256 images leave 4 x 4 x 8 = 128 features of the front camera
    c = perception_cfg(**PLANNING, **{'IMAGE.FINAL_DIM': (256, 256), 'PLANNING.GRU_STATE_SIZE': 128})
    model = H.fill_deterministic(STP3(c))
    model.planning.cost_function.load_state_dict(Cost_Function(c).state_dict())     # grid constants, not weights to randomise
    model = to_channels_last(model.eval().cuda())
    yield model
    del model
    gc.collect()                                   # the drivers' engines and captured graphs: freed here, not inside a later test


@torch.no_grad()
def _written_out_ticks(model, inputs, planner='forward'):
    """Ticks 5-7 from public pieces of the parent commit: per tick (trajectory (1, 4, 3) float32 numpy, steer, throttle, brake)."""
    from stp3_amd import carla, datas, ops_plan
    from tests.test_inference_gpu import _plain
    from tests.test_streaming_gpu import per_frame_encoder
    frames, pos, compass, speed, commands, wps = inputs
    dec = carla.CarlaDecoder(model.cfg)
    extrinsics, intrinsics = carla.cam_para(dec.crop)
    turn, spd, last_steer = carla.turn_controller(), carla.speed_controller(), 0
    twin = torch.Generator(device='cuda').manual_seed(SEED)
    rf, out = model.receptive_field, []
    for i in range(4, TICKS):
        window = range(i - 2, i + 1)
        images = torch.stack([dec.reference_images(frames[j].cuda(), order='bgr') for j in window]).unsqueeze(0)
        ego = carla.future_egomotion([pos[j][0] for j in window], [pos[j][1] for j in window], [compass[j] for j in window])
        batch = {'image': images, 'intrinsics': intrinsics.unsqueeze(0).expand(3, 4, 3, 3).unsqueeze(0).contiguous(),
                 'extrinsics': extrinsics.unsqueeze(0).expand(3, 4, 4, 4).unsqueeze(0).contiguous(),
                 'future_egomotion': torch.cat([ego, torch.zeros(1, 6)]).unsqueeze(0)}
        with per_frame_encoder(model, 1, 4):
            plain = _plain(model, batch)
        trajs = datas.trajectory_sampling(torch.tensor([speed[i]], dtype=torch.float64, device='cuda'),
                                          torch.tensor([last_steer], dtype=torch.float64, device='cuda'), model.cfg.N_FUTURE_FRAMES,
                                          model.cfg.PLANNING.SAMPLE_NUM, generator=twin)
        seg = torch.argmax(plain['segmentation'], dim=2, keepdim=True)
        ped = torch.argmax(plain['pedestrian'], dim=2, keepdim=True)
        occupancy = torch.logical_or(seg, ped)
        target = carla.local_command_point(pos[i], compass[i], wps[i]).to('cuda', dtype=torch.float32).unsqueeze(0)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            if planner == 'forward':
                _, final = model.planning(cam_front=plain['cam_front'], trajs=trajs[:, :, 1:], gt_trajs=None,
                                          cost_volume=plain['costvolume'][:, rf:], semantic_pred=occupancy[:, rf:].squeeze(2),
                                          hd_map=plain['hdmap'], commands=[carla.command_name(commands[i])], target_points=target)
            else:
                scene = ops_plan.plan_scene(plain['segmentation'], plain['pedestrian'], plain['hdmap'], rf)
                final = model.planning.drive(plain['cam_front'], trajs[:, :, 1:], plain['costvolume'][:, rf:], *scene,
                                             ops_plan.command_codes([carla.command_name(commands[i])], device='cuda'), target)[0]
        final = final.float().cpu().numpy()
        steer, throttle, brake, meta = carla.control_pid(final, np.float32(speed[i]), turn, spd, command=commands[i])
        last_steer = steer
        if brake < 0.05:
            brake = 0.0
        if throttle > brake:
            brake = 0.0
        out.append((final, float(steer), float(throttle), float(brake)))
    return out


@pytest.mark.parametrize('planner', [None, 'drive'], ids=['default', 'drive'])
def test_driver_ticks_equal_the_tick_written_out(planning_model, planner):
    from stp3_amd.carla import ClosedLoopDriver
    model = planning_model
    inputs = _tick_inputs()
    frames, pos, compass, speed, commands, wps = inputs
    want = _written_out_ticks(model, inputs, planner or 'forward')        # the default driver: the agent's own planner statements
    kw = {} if planner is None else {'planner': planner}
    driver = ClosedLoopDriver(model, generator=torch.Generator(device='cuda').manual_seed(SEED), **kw)
    got = []
    for i in range(TICKS):
        source = frames[i].pin_memory() if i % 2 else frames[i].cuda()                  # pinned host memory or the device
        got.append(driver.run_step(source, pos[i], compass[i], speed[i], commands[i], wps[i]))
    for res in got[:4]:                                                                 # the warm-up: zero control, buffering only
        assert (res.steer, res.throttle, res.brake) == (0.0, 0.0, 0.0) and res.metadata is None and res.trajectory is None
    for k, (res, (final, steer, throttle, brake)) in enumerate(zip(got[4:], want)):
        assert res.trajectory.shape == (1, 4, 3) and res.trajectory.dtype == np.float32
        diff = np.abs(res.trajectory.astype(np.float64) - final.astype(np.float64)).max()
        print(f'[carla] tick {k + 5}: largest |driver - written-out| trajectory difference {diff:.3e}; control driver '
              f'({res.steer!r}, {res.throttle!r}, {res.brake!r}) written-out ({steer!r}, {throttle!r}, {brake!r})')
        assert np.array_equal(res.trajectory.view(np.uint32), final.view(np.uint32)), k
        assert (res.steer, res.throttle, res.brake) == (steer, throttle, brake), k
        assert res.metadata['command'] == commands[k + 4] and res.metadata['steer'] == float(np.clip(res.metadata['steer'], -1, 1))
    assert not np.array_equal(got[4].trajectory, got[6].trajectory)
    if planner == 'drive':
        eager = _written_out_ticks(model, inputs, 'forward')
        print('[carla] largest |Planning.drive - model.planning| way point difference over ticks 5-7:',
              max(float(np.abs(a[0].astype(np.float64) - b[0].astype(np.float64)).max()) for a, b in zip(want, eager)))
    # reset() mid-sequence restarts the warm-up: four buffering ticks, then the first planned one equals tick 5 of a fresh run
    # on the same inputs (frames 0..4) except for the sampler's draws, which continue
    driver.reset()
    assert driver.step == -1 and driver.last_steer == 0 and driver.engine.filled == 0 and len(driver.gps) == 0
    again = [driver.run_step(frames[i].cuda(), pos[i], compass[i], speed[i], commands[i], wps[i]) for i in range(5)]
    assert all(r.trajectory is None and (r.steer, r.throttle, r.brake) == (0.0, 0.0, 0.0) for r in again[:4])
    assert again[4].trajectory is not None and again[4].metadata['speed'] == float(np.float32(speed[4]))


def test_driver_rejects_other_frames(planning_model):
    from stp3_amd.carla import ClosedLoopDriver
    with pytest.raises(ValueError):
        ClosedLoopDriver(planning_model, warm_ticks=1)
    with pytest.raises(ValueError):
        ClosedLoopDriver(planning_model, planner='other')
