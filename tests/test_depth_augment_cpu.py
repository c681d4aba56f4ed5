"""CPU: depth labels under the per-image augmentation of the camera images (stp3_amd.datas.DepthLabeller with ``params``;
csrc/stp3_depth_augment.hip) against the chain of the reference's own statements recorded by
scripts/make_golden_depth_augment.py in tests/golden/depth_augment.npz on the cases of tests/depth_augment_cases.py (the inputs
are rebuilt here; their sha256 is checked before anything else).

How results are compared.  The maps hold integers (torch.round precedes the crop, the flip and the rotation, which only move
values), so they are pinned EXACTLY: on the float64 routes the generator asserts that every non-zero unrounded output of the
reference lies more than 1e-6 from a half-integer (margins in the fixture: 4e-5 .. 1e-3) while the plain evaluation of the
four-tap blend differs from ATen's by <= 3e-14 (tests/test_depth_cpu.py); for the dense float32 map the fixture lists the
outputs within 1e-3 of a half-integer (at most 0.5 % of the case's outputs) -- those are compared to +-1, all others exactly."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import depth_augment_cases as DA
from tests import depth_cases as DC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
SOURCE_FILE = os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_depth_augment.hip')
ORDERS = ('', 'reverse', 'random')
KERNELS = ('depth_augment_clear_kernel', 'depth_augment_scatter_kernel', 'void depth_augment_output_kernel<0>',
           'void depth_augment_output_kernel<1>', 'void depth_augment_output_kernel<2>')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(H.load('depth_augment.npz'))


@functools.lru_cache(maxsize=None)
def built(name, seed_offset=0):
    """The inputs of a case; the first build of a case is compared with the fixture's digest."""
    case = DA.build(name, seed_offset)
    if not seed_offset:
        assert DA.digest(*(case[k] for k in DA.input_keys(name))) == str(fixture()[f'{name}/sha']), f'{name}: the case builder drifted'
    return case


def inputs(name, device='cpu', seed_offset=0):
    """(cloud arguments or None, maps or None) as tensors."""
    case = built(name, seed_offset)
    if 'maps' in case:
        return None, torch.from_numpy(case['maps']).to(device)
    return (torch.from_numpy(case['points']).to(device), torch.from_numpy(case['offsets']).to(device),
            torch.from_numpy(case['steps']).to(device), DC.BEFORE, torch.from_numpy(case['intrinsics']).to(device)), None


def call(lab, cloud, maps, reference=False, **kw):
    if cloud is None:
        return (lab.reference_from_maps if reference else lab.from_maps)(maps, **kw)
    return (lab.reference_from_lidar if reference else lab.from_lidar)(*cloud, **kw)


def check_depths(name, got, what):
    """``got`` (F, N, Ho, Wo) against the fixture, as the module text says."""
    g = fixture()
    got = np.asarray(got).astype(np.float64)
    if f'{name}/depths/sha' in g:
        as_int = got.astype(np.int16)
        assert np.array_equal(as_int, got) and got.shape == tuple(g[f'{name}/depths/shape']), what
        assert np.array_equal(AC.strided(as_int), g[f'{name}/depths/sample']), f'{what}, {name}: strided sample'
        assert AC.digest(as_int) == str(g[f'{name}/depths/sha']), f'{what}, {name}: digest'
        return
    want = g[f'{name}/depths'].astype(np.float64)
    assert got.shape == want.shape, what
    diff = got != want
    if f'{name}/excluded' in g:
        ex = g[f'{name}/excluded']
        loose = np.zeros_like(diff)
        loose[tuple(ex.T)] = True
        print(f'{what}, {name}: {int(diff.sum())} outputs differ; {len(ex)} are listed as within 1e-3 of a half-integer')
        assert np.abs(got - want)[loose].max(initial=0.0) <= 1.0
        diff &= ~loose
    assert not diff.any(), f'{what}, {name}: {int(diff.sum())} outputs differ from the reference'


def check_labels(name, got, what):
    got = np.asarray(got)
    want = fixture()[f'{name}/labels']
    assert got.dtype == np.int64 and got.shape == want.shape, what
    if f'{name}/excluded' in fixture():                    # (a listed output that is a label may be one class off)
        ex = fixture()[f'{name}/excluded']
        ex = ex[(ex[:, 2] % DA.DOWNSAMPLE == 0) & (ex[:, 3] % DA.DOWNSAMPLE == 0)]
        loose = np.zeros(want.shape, bool)
        loose[ex[:, 0], ex[:, 1], ex[:, 2] // DA.DOWNSAMPLE, ex[:, 3] // DA.DOWNSAMPLE] = True
        assert np.abs(got - want)[loose].max(initial=0) <= 1
        got = np.where(loose, want, got)
    assert np.array_equal(got, want), f'{what}, {name}: class ids'


def test_fixture_holds_data_only_and_has_its_properties():
    g = fixture()
    assert os.path.getsize(os.path.join(H.GOLDEN, 'depth_augment.npz')) <= 1 << 20
    assert sorted({k.split('/')[0] for k in g}) == sorted(list(DA.CASES) + ['meta'])
    assert all(v.dtype.kind in 'iufUb' for v in g.values())                              # numbers and strings: no objects
    assert 'img_transform' in str(g['meta/chain'])
    assert g['l24/depths'].shape == (3, 2, 24, 40) and g['l24/labels'].shape == (3, 2, 3, 5)
    assert g['l17/depths'].shape == (3, 2, 17, 23) and g['l17/labels'].shape == (3, 2, 3, 3)       # partial last label row / column
    assert tuple(g['real/depths/shape']) == (1, 6, 224, 480) and g['real/labels'].shape == (1, 6, 28, 60)
    for n in ('l24', 'l17', 'real'):
        assert g[f'{n}/nonzero'].min() >= DA.MIN_NONZERO, n
    assert built('e24')['offsets'].tolist() == [0, 0, 1, 3001]
    assert all(float(g[f'{n}/margin']) > 1e-6 for n in DA.CASES if n != 'm32')
    assert len(g['m32/excluded']) <= 0.005 * g['m32/depths'].size
    for n in DA.CASES:                                                                   # the inputs are what the generator saw
        built(n)
    # the cases hold what the issue lists: an up-scale, crops leaving the map on every side, flips, the six angles
    p = DA.params('l24')
    assert sorted({q['resize'] for q in p}) == [0.3, 0.55, 1.4] and {q['flip'] for q in p} == {False, True}
    assert [q['rotate'] for q in p] == [0.0, 0.3, -5.4, 17.25, 90.0, 180.0]
    assert p[0]['crop'][0] < 0 and p[5]['crop'][1] < 0 and p[1]['crop'][2] > p[1]['resize_dims'][0] and p[2]['crop'][3] > p[2]['resize_dims'][1]


@pytest.mark.parametrize('name', list(DA.CASES))
def test_torch_statements_match_the_reference(name):
    lab, params = DA.labeller(name), DA.params(name)
    cloud, maps = inputs(name)
    d64 = call(lab, cloud, maps, params=params, out_dtype=torch.float64)
    d32 = call(lab, cloud, maps, reference=True, params=params)
    ho, wo = DA.CASES[name]['final']
    assert d64.dtype == torch.float64 and d32.dtype == torch.float32 and tuple(d32.shape) == DA.FRAMES_CAMERAS[name] + (ho, wo)
    check_depths(name, d64.numpy(), 'torch statements')
    assert torch.equal(d32.double(), d64)
    labels = call(lab, cloud, maps, params=params, labels=True)
    assert tuple(labels.shape[2:]) == (-(-ho // DA.DOWNSAMPLE), -(-wo // DA.DOWNSAMPLE)) and torch.equal(labels, lab.class_ids(d32))
    check_labels(name, labels.numpy(), 'torch statements')


def test_the_two_reference_branches_take_their_taps_differently():
    """NuscenesData.py:295 recomputes the scale factor (taps from n_src / n_out), :262 hands it on (taps from 1 / resize):
    ``depth_resample_axis(step=)`` follows ATen in both, checked against F.interpolate itself on a dense random map."""
    import torch.nn.functional as F
    from stp3_amd.datas import DepthLabeller, depth_resample_axis
    m = torch.from_numpy(np.random.RandomState(5).uniform(0, 70, size=(1, 1, 90, 160)))
    differ = 0
    for scale in (0.3, 0.5, 0.2003, 0.55, 0.2188, 1.4):
        hr, wr = int(np.floor(90 * scale)), int(np.floor(160 * scale))
        for recompute in (True, False):
            want = F.interpolate(m, scale_factor=scale, mode='bilinear', align_corners=False,
                                 **({'recompute_scale_factor': True} if recompute else {}))
            ay = depth_resample_axis(90, scale, np.arange(hr), step=90.0 / hr if recompute else None)
            ax = depth_resample_axis(160, scale, np.arange(wr), step=160.0 / wr if recompute else None)
            ay, ax = ({k: torch.from_numpy(v) for k, v in t.items()} for t in (ay, ax))
            tab = m[0, 0][ay['slot_src'].long(), :][:, ax['slot_src'].long()]
            ty, tx, hy, wx = ay['tap'].long(), ax['tap'].long(), ay['weight'], ax['weight']
            got = (hy[:, 0:1] * (wx[:, 0] * tab[ty[:, 0]][:, tx[:, 0]] + wx[:, 1] * tab[ty[:, 0]][:, tx[:, 1]]) +
                   hy[:, 1:2] * (wx[:, 0] * tab[ty[:, 1]][:, tx[:, 0]] + wx[:, 1] * tab[ty[:, 1]][:, tx[:, 1]]))
            assert tuple(want.shape[2:]) == (hr, wr) and (got - want[0, 0]).abs().max() < 1e-11, (scale, recompute)
            assert torch.equal(DepthLabeller._blend(tab, ay, ax, torch.float64), torch.round(got))
        a = depth_resample_axis(90, scale, np.arange(hr), step=90.0 / hr)
        b = depth_resample_axis(90, scale, np.arange(hr))
        differ += not (np.array_equal(a['weight'], b['weight']) and np.array_equal(a['slot_src'], b['slot_src']))
    assert differ >= 3                                     # (identical at 0.3 and 0.5: the plain from_lidar's 1 / scale coincides)


def eval_setup():
    """A small stand-in configuration whose crop lies inside the resized map: depth_cases' SMALL geometry."""
    from stp3_amd.datas import DepthLabeller, ImageAugmenter
    geo = DC.SMALL
    h, w = geo['source_hw']
    left, top, right, bottom = geo['crop']
    aug = ImageAugmenter(source_hw=(h, w), final_dim=(bottom - top, right - left),
                         eval_params={'resize': geo['scale'], 'resize_dims': (int(w * geo['scale']), int(h * geo['scale'])), 'crop': geo['crop']})
    return DepthLabeller(**geo), aug


def eval_inputs(device='cpu'):
    case = DC.build_lidar('small')
    cloud = (torch.from_numpy(case['points']).to(device), torch.from_numpy(case['offsets']).to(device),
             torch.from_numpy(case['steps']).to(device), DC.BEFORE, torch.from_numpy(case['intrinsics']).to(device))
    maps = {n: torch.from_numpy(DC.build_map(n)['maps']).to(device) for n in DC.MAP_CASES}
    return cloud, maps


def check_eval_parameters_equal_the_plain_call(device):
    lab, aug = eval_setup()
    cloud, maps = eval_inputs(device)
    params = aug.sample(4, train=False)
    for kw in (dict(), dict(out_dtype=torch.float64), dict(labels=True)):
        plain, got = lab.from_lidar(*cloud, **kw), lab.from_lidar(*cloud, params=params, **kw)
        assert got.dtype == plain.dtype and torch.equal(got, plain), kw
        assert plain.bool().any()
    for n, m in maps.items():
        p = aug.sample(m.shape[0] * m.shape[1], train=False)
        for kw in (dict(), dict(out_dtype=torch.float64), dict(labels=True)):
            plain, got = lab.from_maps(m, **kw), lab.from_maps(m, params=p, **kw)
            assert got.dtype == plain.dtype and torch.equal(got, plain), (n, kw)


def test_eval_parameters_equal_the_plain_labeller():
    check_eval_parameters_equal_the_plain_call('cpu')


def test_geometry_agrees_with_the_augmenters_intrinsics():
    """A single LiDAR point per image (identity steps and intrinsics: the point (u z, v z, z) lands at (u, v)): every non-zero
    output pixel centre lies within 1.5 max(resize, 1) + 1 pixels of post_rot (u, v) + post_tran of ImageAugmenter -- truncation
    plus the bilinear reach in resized pixels (1.5 source pixels times the scale, at least the output's own 1.5), plus the
    nearest rotation's rounding.  A wrong flip or rotation sign is off by the window's size."""
    from stp3_amd.datas import ImageAugmenter
    lab, params = DA.labeller('l24'), AC.CASES['s90']['params']
    assert params == DA.params('l24')
    aug = ImageAugmenter(source_hw=DA.SOURCE, final_dim=(24, 40))
    rot, tran = aug.post_homography(params)
    steps = torch.zeros(6, 1, 4, 12, dtype=torch.float64)
    steps[..., 0] = steps[..., 4] = steps[..., 8] = 1.0
    k = torch.eye(3, dtype=torch.float64).expand(6, 1, 3, 3).contiguous()
    offsets = torch.arange(7, dtype=torch.int32)
    seen, worst = np.zeros(6, int), np.zeros(6)
    for v in np.arange(2.5, 88, 6.0):
        for u in np.arange(2.5, 158, 6.0):
            points = torch.tensor([[u * 32.0, v * 32.0, 32.0]], dtype=torch.float32).expand(6, 3).contiguous()
            # six frames of one camera: image i takes parameter set i
            out = lab.from_lidar(points, offsets, steps, (False,) * 4, k, params=params)
            for i in range(6):
                ys, xs = np.nonzero(out[i, 0].numpy())
                if len(ys):
                    want = rot[i].double() @ torch.tensor([u, v]) + tran[i].double()
                    dist = np.hypot(xs + 0.5 - float(want[0]), ys + 0.5 - float(want[1]))
                    seen[i] += 1
                    worst[i] = max(worst[i], dist.max())
    bounds = np.array([1.5 * max(p['resize'], 1.0) + 1.0 for p in params])
    print('points seen per parameter set', seen.tolist(), 'worst distance', worst.round(2).tolist(), 'bounds', bounds.tolist())
    assert (seen >= 3).all() and (worst <= bounds).all()


def test_python_entries_validate():
    lab, params = DA.labeller('l24'), DA.params('l24')
    cloud, _ = inputs('l24')
    _, maps = inputs('m64')
    with pytest.raises(ValueError):
        lab.from_lidar(*cloud, params=params[:5])                                                  # not F N sets
    with pytest.raises(ValueError):
        lab.from_maps(maps, params=params + params[:1])
    with pytest.raises(ValueError):
        lab.from_lidar(*cloud, params=params, labels=True, fused=True)                             # the LDS kernel is not extended
    two = [dict(p) for p in params]
    two[3]['crop'] = (2, 1, 43, 25)
    with pytest.raises(ValueError):
        lab.from_lidar(*cloud, params=two)                                                         # crops of two sizes
    with pytest.raises(ValueError):
        lab.from_maps(maps, params=[dict(p, crop=(3, 1, 3, 25)) for p in params])                  # an empty crop
    with pytest.raises(ValueError):
        lab.from_maps(maps, params=[dict(p, resize=0.001, resize_dims=(0, 0)) for p in params])    # an empty resized map
    with pytest.raises(ValueError):
        lab.from_maps(maps, params=[dict(params[0], resize_dims=(49, 27))] + params[1:])           # not floor(source * resize)
    with pytest.raises(ValueError):
        lab.from_maps(maps, params=[dict(p, crop=(0, 0, 8193, 24)) for p in params])               # Pillow's rotation overflows
    with pytest.raises(ValueError):
        lab.augment_plan(params, 'cpu', maps=torch.float16)
    # a plan rewritten in place: the same images and window; a plan of label rows and columns takes no rotation
    still = [dict(p, rotate=0.0) for p in params]
    plan = lab.augment_plan(still, 'cpu', labels=True)
    assert plan.separable and lab.augment_plan(still[::-1], 'cpu', like=plan) is plan
    with pytest.raises(ValueError):
        lab.augment_plan(params, 'cpu', like=plan)
    roomy = lab.augment_plan(still, 'cpu', labels=True, rotate=True)
    assert not roomy.separable and lab.augment_plan(params, 'cpu', like=roomy) is roomy
    with pytest.raises(ValueError):
        lab.augment_plan(params[:4], 'cpu', like=roomy)
    with pytest.raises(ValueError):
        lab.augment_plan(DA.params('l17'), 'cpu', like=roomy)


def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused first
    nbytes = ctypes.c_size_t()

    def dims(**over):
        d = _lib.AugmentDepthDims()
        d.F, d.N, d.n_total, d.out_kind = 3, 2, 100, _lib.DEPTH_OUT_F32
        d.H, d.W, d.Ho, d.Wo, d.stride, d.separable, d.records = 90, 160, 24, 40, 1, 0, 64
        for axis, n in ((d.y, 24), (d.x, 40)):
            axis.tap = axis.weight = axis.slot_src = 64
            axis.entries, axis.slots = 6 * n, 12 * n
        for k, v in over.items():
            obj, _, field = k.rpartition('.')
            setattr(getattr(d, obj) if obj else d, field, v)
        return d
    assert lib.stp3_augment_depth_workspace_bytes(ctypes.byref(dims()), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 6 * 48 * 80 * 4 + 100 * 2 * 4             # winner tables + a float32 depth per point and camera
    labels = dims(stride=8, separable=1, out_kind=_lib.DEPTH_OUT_LABELS)
    assert lib.stp3_augment_depth_workspace_bytes(ctypes.byref(labels), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 6 * 6 * 10 * 4 + 100 * 2 * 4              # 3 x 5 label rows and columns
    for bad in (dict(F=0), dict(N=0), dict(n_total=-1), dict(out_kind=3), dict(H=2), dict(Ho=0), dict(Wo=8193), dict(stride=0),
                dict(separable=2), dict(records=None), {'y.tap': None}, {'x.weight': None}, {'x.slot_src': None}, {'y.entries': 23},
                {'x.slots': -1}):
        assert lib.stp3_augment_depth_workspace_bytes(ctypes.byref(dims(**bad)), ctypes.byref(nbytes)) == -10001, bad
        assert lib.stp3_augment_depth_from_lidar(ctypes.byref(dims(**bad)), fake, fake, fake, 12, fake, fake, 1 << 30, fake, None) == -10001, bad
        assert lib.stp3_augment_depth_from_maps(ctypes.byref(dims(**bad)), fake, 1, fake, None) == -10001, bad
    d = dims()
    assert lib.stp3_augment_depth_workspace_bytes(None, ctypes.byref(nbytes)) == -10001
    assert lib.stp3_augment_depth_workspace_bytes(ctypes.byref(d), None) == -10001
    assert lib.stp3_augment_depth_from_lidar(ctypes.byref(d), fake, fake, fake, 12, fake, fake, 16, fake, None) == -10003     # workspace too small
    assert lib.stp3_augment_depth_from_lidar(ctypes.byref(d), fake, fake, fake, 16, fake, fake, 1 << 30, fake, None) == -10001   # 5th step flag
    assert lib.stp3_augment_depth_from_lidar(ctypes.byref(d), None, fake, fake, 12, fake, fake, 1 << 30, fake, None) == -10001
    assert lib.stp3_augment_depth_from_lidar(ctypes.byref(d), fake, None, fake, 12, fake, fake, 1 << 30, fake, None) == -10001
    assert lib.stp3_augment_depth_from_lidar(ctypes.byref(d), fake, fake, fake, 12, fake, None, 1 << 30, fake, None) == -10001
    assert lib.stp3_augment_depth_from_maps(ctypes.byref(d), fake, 2, fake, None) == -10001                                   # labels are no map dtype
    assert lib.stp3_augment_depth_from_maps(ctypes.byref(d), None, 1, fake, None) == -10001
    assert lib.stp3_augment_depth_from_maps(ctypes.byref(d), fake, 1, None, None) == -10001


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
def run_host(tmp, lib, order, *extra):
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if order:
        env['HIPCPU_ORDER'] = order
    path = str(tmp / f'out_{order or "plain"}{"_".join(extra)}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_depth_augment.py'), lib, path, *extra], env=env,
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(path))


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_depth_augment')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[SOURCE_FILE])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    return request.param or 'plain', run_host(*host_lib, request.param)


@functools.lru_cache(maxsize=None)
def torch_statements(name, variant):
    """The torch statements for a variant of a case's parameters, computed once (float64 map, then what follows from it)."""
    lab, params = DA.labeller(name), DA.params(name)
    cloud, maps = inputs(name, seed_offset=1 if variant == 'replay' else 0)
    if variant == 'norot':
        params = [dict(p, rotate=0.0) for p in params]
    elif variant == 'replay':
        params = DA.replay_params(name)
    return call(lab, cloud, maps, reference=True, params=params, out_dtype=torch.float64)


@pytest.mark.parametrize('name', DA.SMALL)
def test_kernels_on_host_match_the_reference(host_kernel, name):
    order, out = host_kernel
    what = f'kernels on the host ({order} order)'
    lab = DA.labeller(name)
    assert out[f'{name}/full'].dtype == np.float64 and out[f'{name}/full32'].dtype == np.float32
    check_depths(name, out[f'{name}/full'], what)
    check_depths(name, out[f'{name}/full32'], what)
    check_labels(name, out[f'{name}/labels'], what)
    # bit for bit with the torch statements, no list of exclusions: the same roundings in the same order
    assert np.array_equal(out[f'{name}/full'], torch_statements(name, 'plain').numpy()), f'{what}: kernels != torch statements'
    assert np.array_equal(out[f'{name}/labels'], lab.class_ids(torch.from_numpy(out[f'{name}/full32'])).numpy())
    # without rotation the labels come from the label rows' and columns' tables alone
    still = torch_statements(name, 'norot')
    assert np.array_equal(out[f'{name}/full_norot'], still.float().numpy())
    assert np.array_equal(out[f'{name}/labels_norot'], lab.class_ids(still.float()).numpy())
    assert np.array_equal(out[f'{name}/replay'], torch_statements(name, 'replay').float().numpy()), f'{what}: rewritten plan'


def test_a_corrupted_record_stays_inside_the_buffers(host_lib):
    """Host stand-in only.  The third image's record holds impossible values (everything at the int32 limits, the rotation's
    integers at the limits, table offsets past the end, absurd list lengths), or its table entries do: the call returns
    STP3_OK, the other images equal the fixture and the canaries around the output and the workspace are intact."""
    out = run_host(*host_lib, '', 'corrupt')
    bad = (1, 0)                                                     # image 2 of 3 frames x 2 cameras
    seen = 0
    for name in ('l24', 'l17', 'm64', 'm32'):
        for damage in ('max', 'min', 'rotation', 'offsets', 'lengths', 'entries'):
            got = out[f'{name}/{damage}/out']
            assert int(out[f'{name}/{damage}/rc']) == 0 and bool(out[f'{name}/{damage}/canaries']), (name, damage)
            if damage not in ('rotation', 'entries'):
                assert not got[bad].any(), (name, damage)           # an impossible value zeroes the image's pixels
            assert np.isfinite(got).all()
            fixed = got.copy()
            fixed[bad] = torch_statements(name, 'plain').numpy()[bad]
            check_depths(name, fixed, f'corrupted record ({damage})')
            seen += 1
    assert seen == 24


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_depth_augment_kernels_keep_their_register_budget():
    """No spills, no scratch, no static LDS; within 64 registers like the kernels of stp3_depth.hip (8 waves per SIMD: they are
    latency-bound gathers and a float64 transform)."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources
    rows = {k['kernel']: k for k in kernel_resources.kernels_of(SOURCE_FILE)}
    print(json.dumps(rows, indent=1))
    assert sorted(rows) == sorted(KERNELS)
    for k in rows.values():
        assert k['vgpr_spills'] == 0 and k['sgpr_spills'] == 0 and k['scratch'] == 0 and k['lds_static'] == 0, k
        assert k['vgpr'] + k['agpr'] <= 64, k
