"""CPU: depth labels from LiDAR points and from stored maps (stp3_amd.datas.DepthLabeller; csrc/stp3_depth.hip) against the
reference's own NuscenesData.get_depth_from_lidar (:289-300) and the depth branch of get_input_data (:257-267), recorded by
scripts/make_golden_depth.py in tests/golden/depth_labels.npz on the cases of tests/depth_cases.py (the inputs are rebuilt
here; their sha256 is checked before anything else).

How results are compared.  The rounded maps are pinned, EXACTLY: the generator asserts that every non-zero unrounded output of
the reference on a float64 map lies more than 1e-6 from a half-integer (margins in the fixture: 5e-6 .. 9e-2) while the plain
evaluation of the four-tap blend differs from ATen's fused one by <= 3e-14; for the dense float32 map (differences <= 1.6e-5)
the fixture lists the outputs within 1e-3 of a half-integer (at most 0.5 % of the pixels) -- those are compared to +-1, all
others exactly.  The projection (nuScenes devkit, PARITY UNPINNED) is compared with the restatement in tests/depth_cases.py:
pixels and mask exactly (the clouds keep every coordinate 1e-3 off an integer and off the mask's bounds), depths bit for bit
(the same float64 statements, rounded to float32 at the same places).  Class ids: the trainer's statement, exactly."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depth_cases as DC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
KERNELS = ('depth_project_kernel', 'depth_labels_kernel', 'depth_clear_kernel', 'void depth_scatter_kernel<true>', 'void depth_scatter_kernel<false>',
           'void depth_resample_kernel<0>', 'void depth_resample_kernel<1>', 'void depth_resample_kernel<2>',
           'void depth_resample_kernel<3>')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(H.load('depth_labels.npz'))


@functools.lru_cache(maxsize=None)
def built(name):
    """The inputs of a case, after their digests have been compared with the fixture's."""
    lidar = name in DC.LIDAR_CASES
    case = DC.build_lidar(name) if lidar else DC.build_map(name)
    assert DC.digest(case, DC.LIDAR_KEYS if lidar else ('maps',)) == fixture()[f'{name}/sha'].tolist(), f'{name}: the case builder drifted'
    return case


@functools.lru_cache(maxsize=None)
def projected(name):
    return DC.projected(built(name))


def labeller(name):
    from stp3_amd.datas import DepthLabeller
    return DepthLabeller(**DC.geometry(built(name)))


def cloud(name, device='cpu'):
    case = built(name)
    return (torch.from_numpy(case['points']).to(device), torch.from_numpy(case['offsets']).to(device),
            torch.from_numpy(case['steps']).to(device), DC.BEFORE, torch.from_numpy(case['intrinsics']).to(device))


def check_projection(name, pixels, depth, keep, what):
    want_pixels, want_depth, want_keep = projected(name)
    assert np.array_equal(np.asarray(keep), want_keep), f'{what}: keep mask'
    assert np.array_equal(np.asarray(pixels), want_pixels), f'{what}: pixels'
    assert np.asarray(depth).dtype == np.float64 and np.array_equal(np.asarray(depth), want_depth), f'{what}: depths'


def check_depths(name, got, what):
    """``got`` (F, N, Ho, Wo) against the reference's rounded map, as the module text says."""
    g = fixture()
    want = g[f'{name}/depths'].astype(np.float64)
    got = np.asarray(got).astype(np.float64)
    assert got.shape == want.shape, what
    diff = got != want
    if f'{name}/excluded' in g:
        ex = g[f'{name}/excluded']
        loose = np.zeros_like(diff)
        loose[tuple(ex.T)] = True
        print(f'{what}, {name}: {int(diff.sum())} outputs differ, all among the {len(ex)} listed as within 1e-3 of a half-integer')
        assert np.abs(got - want)[loose].max(initial=0.0) <= 1.0
        diff &= ~loose
    assert not diff.any(), f'{what}, {name}: {int(diff.sum())} outputs differ from the reference'


def check_labels(name, got, what):
    got = np.asarray(got)
    assert got.dtype == np.int64 and np.array_equal(got, fixture()[f'{name}/labels']), f'{what}, {name}: class ids'


def test_fixture_holds_data_only_and_has_its_properties():
    g = fixture()
    assert os.path.getsize(os.path.join(H.GOLDEN, 'depth_labels.npz')) <= 1 << 20
    assert sorted({k.split('/')[0] for k in g}) == sorted(list(DC.LIDAR_CASES) + list(DC.MAP_CASES) + ['meta'])
    assert all(v.dtype.kind in 'iufU' for v in g.values())                               # numbers and strings: no objects
    assert 'PARITY UNPINNED' in str(g['meta/projection']) and 'get_input_data' in str(g['meta/map_route'])
    assert g['small/depths'].shape == (2, 2, 24, 48) and g['small/labels'].shape == (2, 2, 3, 6)
    assert g['real/depths'].shape == (1, 6, 224, 480) and g['real/labels'].shape == (1, 6, 28, 60)
    assert g['half/depths'].shape == (1, 3, 32, 64) and DC.LIDAR_CASES['half']['crop'][0] > 0
    assert int(g['small/duplicates']) >= 100                                             # "last wins" is exercised
    assert built('sparse')['offsets'].tolist() == [0, 0, 1, 6] and built('small')['offsets'].tolist() == [0, 1000, 1037]
    assert all(float(g[f'{n}/margin']) > 1e-6 for n in list(DC.LIDAR_CASES) + ['map64'])
    assert len(g['map32/excluded']) <= 0.005 * g['map32/depths'].size
    # the first and the last kept row and column carry points
    for n in ('small', 'half'):
        d = g[f'{n}/depths']
        assert d[..., 0, :].any() and d[..., -1, :].any() and d[..., :, 0].any() and d[..., :, -1].any(), n
    # last wins is visible: with the FIRST point of a pixel instead, the rounded map would differ
    case, (pixels, depth, keep) = built('small'), projected('small')
    first = labeller('small').reference_from_pixels(*(torch.from_numpy(a[::-1].copy()) for a in (pixels[:1000], depth[:1000], keep[:1000])),
                                                    torch.tensor([0, 1000], dtype=torch.int32))
    assert not np.array_equal(first.numpy()[0], g['small/depths'][0].astype(np.float32))


@pytest.mark.parametrize('name', list(DC.LIDAR_CASES))
def test_torch_path_matches_the_reference(name):
    lab = labeller(name)
    pixels, depth, keep = lab.project(*cloud(name))
    check_projection(name, pixels.numpy(), depth.numpy(), keep.numpy(), 'torch path')
    offsets = cloud(name)[1]
    d64 = lab.from_pixels(pixels, depth, keep, offsets, out_dtype=torch.float64)
    d32 = lab.from_lidar(*cloud(name))
    assert d64.dtype == torch.float64 and d32.dtype == torch.float32 and tuple(d32.shape[2:]) == lab.out_hw
    check_depths(name, d64.numpy(), 'torch path, from_pixels')
    check_depths(name, d32.numpy(), 'torch path, from_lidar')
    labels = lab.from_lidar(*cloud(name), labels=True)
    assert tuple(labels.shape[2:]) == lab.label_hw and torch.equal(labels, lab.class_ids(d32))
    check_labels(name, labels.numpy(), 'torch path')


@pytest.mark.parametrize('name', list(DC.MAP_CASES))
def test_torch_path_matches_the_reference_on_stored_maps(name):
    lab = labeller(name)
    maps = torch.from_numpy(built(name)['maps'])
    check_depths(name, lab.from_maps(maps).numpy(), 'torch path, from_maps')
    check_labels(name, lab.from_maps(maps, labels=True).numpy(), 'torch path, from_maps')


def test_class_ids_are_the_trainers_statement():
    """stp3_amd/trainer.py:220-222 (the reference's trainer.py:269-276) on a map that reaches below and above D_BOUND."""
    from stp3_amd.config import perception_cfg
    from stp3_amd.datas import DepthLabeller
    cfg = perception_cfg(**{'LIFT.GT_DEPTH': True})
    lab = DepthLabeller(cfg)
    assert lab.out_hw == (224, 480) and lab.label_hw == (28, 60) and lab.source_hw == (900, 1600)
    depths = torch.from_numpy(np.random.RandomState(3).randint(0, 80, size=(2, 3, 6, 224, 480)).astype(np.float32))
    ds = cfg.MODEL.ENCODER.DOWNSAMPLE
    want = torch.clamp(depths[:, :3, :, ::ds, ::ds], cfg.LIFT.D_BOUND[0], cfg.LIFT.D_BOUND[1] - 1) - cfg.LIFT.D_BOUND[0]
    got = lab.class_ids(depths)
    assert got.dtype == torch.int64 and torch.equal(got, want.long()) and got.min() == 0 and got.max() == 47


def test_frames_drop_into_assemble_sample():
    from stp3_amd.datas import assemble_sample
    lab = labeller('small')
    depths = lab.from_lidar(*cloud('small'))
    frames = [{'image': torch.zeros(1, 2, 3, 24, 48), 'intrinsics': torch.eye(3).expand(1, 2, 3, 3), 'extrinsics': torch.eye(4).expand(1, 2, 4, 4),
               'depths': depths[f:f + 1], 'segmentation': torch.zeros(1, 1, 8, 8, dtype=torch.int64),
               'pedestrian': torch.zeros(1, 1, 8, 8, dtype=torch.int64), 'instance': torch.zeros(1, 8, 8, dtype=torch.int64),
               'future_egomotion': torch.zeros(1, 6), 'hdmap': torch.zeros(1, 2, 8, 8, dtype=torch.int64)} for f in range(2)]
    data = assemble_sample(frames, receptive_field=2, num_instances=0, gt_depth=True)
    assert torch.equal(data['depths'], depths) and data['depths'].shape == (2, 2, 24, 48)


def test_python_entries_validate():
    lab = labeller('small')
    points, offsets, steps, before, k = cloud('small')
    with pytest.raises(ValueError):
        lab.project(points.double(), offsets, steps, before, k)
    with pytest.raises(ValueError):
        lab.project(points, offsets.long(), steps, before, k)
    with pytest.raises(ValueError):
        lab.project(points, torch.tensor([0, 1000, 900], dtype=torch.int32), steps, before, k)          # not ascending
    with pytest.raises(ValueError):
        lab.project(points, torch.tensor([0, 1000, 2000], dtype=torch.int32), steps, before, k)         # beyond the points
    with pytest.raises(ValueError):
        lab.project(points, offsets, steps.float(), before, k)
    with pytest.raises(ValueError):
        lab.project(points, offsets, steps[:1], before, k)
    with pytest.raises(ValueError):
        lab.project(points, offsets, steps, before[:3], k)
    with pytest.raises(ValueError):
        lab.from_maps(torch.zeros(1, 2, 90, 161))
    with pytest.raises(ValueError):
        lab.from_maps(torch.zeros(1, 2, 90, 160, dtype=torch.float16))
    pixels, depth, keep = lab.project(points, offsets, steps, before, k)
    with pytest.raises(ValueError):
        lab.from_pixels(pixels, depth.float(), keep, offsets)
    with pytest.raises(ValueError):
        lab.from_pixels(pixels.long(), depth, keep, offsets)


def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused first
    nbytes, used = ctypes.c_size_t(), ctypes.c_int32()

    def dims(**over):
        d = _lib.DepthDims()
        d.F, d.N, d.n_total, d.out_kind = 2, 2, 100, _lib.DEPTH_OUT_F32
        for axis, (n_out, n_slot, n_src) in ((d.y, (24, 48, 90)), (d.x, (48, 96, 160))):
            axis.tap = axis.weight = axis.slot_src = axis.src_slot = 64
            axis.n_out, axis.n_slot, axis.n_src = n_out, n_slot, n_src
        for k, v in over.items():
            obj, _, field = k.rpartition('.')
            setattr(getattr(d, obj) if obj else d, field, v)
        return d
    assert lib.stp3_depth_workspace_bytes(ctypes.byref(dims()), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 2 * 2 * 48 * 96 * 4 + 100 * 2 * 4        # winner table + a float32 depth per point and camera
    for bad in (dict(F=0), dict(N=0), dict(n_total=-1), dict(out_kind=3), {'y.n_out': 0}, {'x.n_slot': 0}, {'x.n_slot': 97},
                {'y.n_slot': 91, 'y.n_out': 80}, {'y.tap': None}, {'x.weight': None}, {'x.src_slot': None}):
        assert lib.stp3_depth_workspace_bytes(ctypes.byref(dims(**bad)), ctypes.byref(nbytes)) == -10001, bad
        assert lib.stp3_depth_from_lidar(ctypes.byref(dims(**bad)), fake, fake, fake, 12, fake, fake, 1 << 30, fake, None) == -10001, bad
        assert lib.stp3_depth_from_maps(ctypes.byref(dims(**bad)), fake, 1, fake, None) == -10001, bad
    d = dims()
    assert lib.stp3_depth_workspace_bytes(None, ctypes.byref(nbytes)) == -10001
    assert lib.stp3_depth_from_lidar(ctypes.byref(d), fake, fake, fake, 12, fake, fake, 16, fake, None) == -10003   # workspace too small
    assert lib.stp3_depth_from_lidar(ctypes.byref(d), fake, fake, fake, 16, fake, fake, 1 << 30, fake, None) == -10001   # 5th step flag
    assert lib.stp3_depth_from_lidar(ctypes.byref(d), None, fake, fake, 12, fake, fake, 1 << 30, fake, None) == -10001
    assert lib.stp3_depth_from_lidar(ctypes.byref(d), fake, None, fake, 12, fake, fake, 1 << 30, fake, None) == -10001
    assert lib.stp3_depth_from_pixels(ctypes.byref(d), fake, fake, fake, fake, fake, 16, fake, None) == -10003
    assert lib.stp3_depth_from_pixels(ctypes.byref(d), fake, fake, None, fake, fake, 1 << 30, fake, None) == -10001
    assert lib.stp3_depth_from_maps(ctypes.byref(d), fake, 2, fake, None) == -10001                                # labels are no map dtype
    assert lib.stp3_depth_from_maps(ctypes.byref(d), None, 1, fake, None) == -10001
    assert lib.stp3_depth_project(2, 2, 100, 90, 160, fake, fake, fake, 12, fake, fake, fake, None, None) == -10001
    assert lib.stp3_depth_project(0, 2, 100, 90, 160, fake, fake, fake, 12, fake, fake, fake, fake, None) == -10001
    assert lib.stp3_depth_project(2, 2, 100, 2, 160, fake, fake, fake, 12, fake, fake, fake, fake, None) == -10001
    # the labels-only kernel takes label dims only, and needs a label row's slots to fit in LDS
    assert lib.stp3_depth_labels_from_lidar(ctypes.byref(d), fake, fake, fake, 12, fake, 0, fake, None) == -10001
    lab = dims(out_kind=_lib.DEPTH_OUT_LABELS)
    assert lib.stp3_depth_labels_from_lidar(ctypes.byref(lab), fake, fake, fake, 12, fake, -1, fake, None) == -10001
    assert lib.stp3_depth_labels_bands(ctypes.byref(lab), 0, ctypes.byref(used)) == 0 and used.value == 1
    assert lib.stp3_depth_labels_bands(ctypes.byref(lab), 5, ctypes.byref(used)) == 0 and used.value == 5      # 24 rows: 5 each
    tall = dims(out_kind=_lib.DEPTH_OUT_LABELS, **{'y.n_out': 224, 'y.n_slot': 448, 'y.n_src': 900, 'x.n_out': 480, 'x.n_slot': 960,
                                                   'x.n_src': 1600})
    assert lib.stp3_depth_labels_bands(ctypes.byref(tall), 0, ctypes.byref(used)) == 0 and used.value == 28    # 8 rows of 2 x 960 words
    wide = dims(out_kind=_lib.DEPTH_OUT_LABELS, **{'x.n_out': 5000, 'x.n_slot': 9000, 'x.n_src': 20000})
    assert lib.stp3_depth_labels_bands(ctypes.byref(wide), 0, ctypes.byref(used)) == -10002
    assert lib.stp3_depth_labels_from_lidar(ctypes.byref(wide), fake, fake, fake, 12, fake, 0, fake, None) == -10002


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
def run_host(tmp, lib, order, *extra):
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if order:
        env['HIPCPU_ORDER'] = order
    path = str(tmp / f'out_{order or "plain"}{"_".join(extra)}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_depth.py'), lib, path, *extra], env=env, capture_output=True,
                         text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(path))


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_depth')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_depth.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    return request.param or 'plain', run_host(*host_lib, request.param)


def check_host_case(name, out, what):
    check_projection(name, out[f'{name}/pixels'], out[f'{name}/depth'], out[f'{name}/keep'], what)
    assert out[f'{name}/from_pixels'].dtype == np.float64 and out[f'{name}/from_lidar'].dtype == np.float32
    check_depths(name, out[f'{name}/from_pixels'], f'{what}, from_pixels')
    check_depths(name, out[f'{name}/from_lidar'], f'{what}, from_lidar')
    lab = labeller(name)
    torch_path = lab.from_lidar(*cloud(name))
    assert np.array_equal(out[f'{name}/from_lidar'], torch_path.numpy()), f'{what}: kernels != torch path'
    full_route = lab.class_ids(torch.from_numpy(out[f'{name}/from_lidar'])).numpy()
    for k in ('labels', 'labels_banded', 'labels_table'):
        check_labels(name, out[f'{name}/{k}'], f'{what}, {k}')
        assert np.array_equal(out[f'{name}/{k}'], full_route), f'{what}: {k} != class ids of the full route'


@pytest.mark.parametrize('name', [n for n in DC.LIDAR_CASES if n != 'real'])
def test_kernels_on_host_match_the_reference(host_kernel, name):
    order, out = host_kernel
    check_host_case(name, out, f'kernels on the host ({order} order)')


@pytest.mark.parametrize('name', list(DC.MAP_CASES))
def test_kernels_on_host_match_the_reference_on_stored_maps(host_kernel, name):
    order, out = host_kernel
    what = f'kernels on the host ({order} order)'
    check_depths(name, out[f'{name}/depths'], what)
    check_labels(name, out[f'{name}/labels'], what)
    lab = labeller(name)
    maps = torch.from_numpy(built(name)['maps'])
    assert np.array_equal(out[f'{name}/depths'], lab.reference_from_maps(maps, out_dtype=torch.float64).numpy())   # bit for bit, no list


def test_kernels_on_host_match_the_reference_at_the_real_geometry(host_lib):
    """900 x 1600 -> 224 x 480 -> 28 x 60, 6 cameras, 35 000 points."""
    check_host_case('real', run_host(*host_lib, 'random', 'real'), 'kernels on the host (random order), real geometry')


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_depth_kernels_keep_their_register_budget():
    """No spills, no scratch; every kernel of the file stays within 64 registers (8 waves per SIMD: they are latency-bound
    gathers and a float64 transform), the labels kernel -- 1024 threads per workgroup -- with it."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources
    rows = {k['kernel']: k for k in kernel_resources.kernels_of(os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_depth.hip'))}
    print(json.dumps(rows, indent=1))
    assert sorted(rows) == sorted(KERNELS)
    for name in KERNELS:
        k = rows[name]
        assert k['vgpr_spills'] == 0 and k['sgpr_spills'] == 0 and k['scratch'] == 0, k
        assert k['vgpr'] + k['agpr'] <= 64, k
        assert k['lds_static'] == 0, k
