"""CPU: the training video (stp3_amd/visualisation.py, csrc/stp3_vis.hip) against the reference's own visualise_output
(stp3/utils/visualisation.py:208-322), recorded by scripts/make_golden_visualisation.py in tests/golden/visualisation.npz on the
cases of tests/visualisation_cases.py.

How results are compared: ``visualisation_cases.compare`` -- every byte equal to the reference's, except the bytes of the two
flow-type rows that an angle +-2 ulp away would change (they may differ by 1; under 2 % of a panel) and the planning row, which
is this project's own integer drawing and is compared with the statement ``visualisation_cases.planning_expected``."""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import host_trace
from tests import visualisation_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
PKG = os.path.join(ROOT, 'st-p3_amd', 'stp3_amd')
ORDERS = ('', 'reverse', 'random')
CASE_SAMPLES = [(n, s) for n, c in VC.CASES.items() for s in c['samples']]


def test_fixture_holds_data_only_and_has_its_properties():
    g = VC.fixture()
    assert os.path.getsize(VC.GOLDEN) <= 1 << 20
    assert sorted({k.split('/')[0] for k in g}) == sorted(list(VC.CASES) + ['meta'])
    assert all(v.dtype.kind in 'iuf' for v in g.values())                                  # numbers: no objects
    full = VC.CASES['full']
    assert g['full/video'].shape == (2, 1, 3, 3, 7 * 24, 2 * 22) and full['W'] % 4 != 0 and full['H'] != full['W']
    assert g['off/video'].shape == (1, 1, 2, 3, 168, 44) and g['t1/video'].shape == (1, 1, 1, 3, 70, 18)
    ids = g['full/labels/instance']
    assert 74 in ids and not (ids[0, 2] == 0).any() and ids[0, 2].min() == 1                # the modulo; a frame without background
    assert np.ptp(g['full/labels/centerness'][0, 1]) == 0                                  # a constant centre map
    assert not any(k.startswith('off/') and k.split('/')[-1] in ('instance', 'flow', 'pedestrian', 'instance_flow') for k in g)
    assert all(float(g[f'{n}/fragile_share']) < VC.FRAGILE_SHARE for n in VC.CASES)
    for name in VC.CASES:                                                                  # the planning row was never drawn
        hh = VC.CASES[name]['H']
        assert not g[f'{name}/video'][..., 6 * hh:, :].any()
    # disabled panels are zero, enabled ones carry a black border around something that is not black
    off = g['off/video'][0]
    for row in ('instance', 'flow', 'centerness', 'offset', 'pedestrian'):
        assert not VC.panel(off, 0, row, 0, 24, 22).any() and not VC.panel(off, 1, row, 1, 24, 22).any()
    seg = VC.panel(off, 0, 'segmentation', 1, 24, 22)
    assert not seg[:, 0].any() and not seg[:, :, -1].any() and seg[:, 1:-1, 1:-1].any()
    # the case builder still gives the stored inputs
    for name in VC.CASES:
        labels, output, _ = VC.stored(name)
        built = VC.build(name)
        assert all(torch.equal(v, built[0][k]) for k, v in labels.items()) and all(torch.equal(v, built[1][k]) for k, v in output.items())


def test_tables_are_the_references():
    from stp3_amd import visualisation as V
    g = VC.fixture()
    assert V.INSTANCE_COLOURS.shape == (70, 3) and np.array_equal(V.INSTANCE_COLOURS, g['meta/palette'])
    assert V.JET_BYTES.shape == (256, 3) and np.array_equal(V.JET_BYTES, g['meta/jet'])
    wheel = V.make_color_wheel()
    assert wheel.shape == (55, 3) and wheel.dtype == np.float64 and np.array_equal(wheel, np.floor(wheel))
    corners = {0: (255, 0, 0), 15: (255, 255, 0), 21: (0, 255, 0), 25: (0, 255, 255), 36: (0, 0, 255), 49: (255, 0, 255)}
    assert all(tuple(wheel[k]) == v for k, v in corners.items())
    assert tuple(wheel[1]) == (255, 17, 0) and tuple(wheel[54]) == (255, 0, 43)


def test_jet_bytes_are_matplotlibs():
    matplotlib = pytest.importorskip('matplotlib')
    from stp3_amd import visualisation as V
    jet = matplotlib.colormaps['jet']
    assert np.array_equal(V.JET_BYTES, np.uint8(jet(np.arange(256))[:, :3] * 255))
    x = np.random.RandomState(0).rand(40, 50).astype(np.float32)
    x[0, :3] = (0.0, 1.0, 0.5)
    assert np.array_equal(V.heatmap_image(x, autoscale=False), np.uint8(jet(x)[:, :, :3] * 255))
    assert np.array_equal(V.heatmap_image(x), V.heatmap_image(x, cmap=jet))


@pytest.mark.parametrize('name,sample', CASE_SAMPLES)
def test_cpu_route_matches_the_reference(name, sample):
    from stp3_amd import visualisation as V
    labels, output, consistent = VC.stored(name)
    before = {k: v.clone() for k, v in {**labels, **output}.items()}
    video = V.visualise_output(labels, output, VC.cfg_of(name), sample=sample)
    assert video.dtype == torch.uint8 and video.device.type == 'cpu'
    share = VC.compare(name, video.numpy(), sample, labels, output, 'CPU route')
    print(f'{name} sample {sample}: at most {share:.3%} of a flow panel fragile')
    assert all(torch.equal(v, before[k]) for k, v in {**labels, **output}.items()), 'an input was written to'
    if consistent is not None:                                       # the default post-processing gives the reference's ids
        given = V.visualise_output(labels, output, VC.cfg_of(name), sample=sample, consistent_instance_seg=consistent)
        assert torch.equal(given, video)
    bf16 = VC.stored(name, head_dtype=torch.bfloat16)
    assert torch.equal(V.visualise_output(bf16[0], bf16[1], VC.cfg_of(name), sample=sample), video)
    out = torch.zeros_like(video)
    assert V.visualise_output(labels, output, VC.cfg_of(name), sample=sample, out=out) is out and torch.equal(out, video)


def test_pieces_under_the_references_names():
    from stp3_amd import visualisation as V
    labels, output, _ = VC.stored('full')
    want = VC.golden_video('full', 0)
    flow = labels['flow'][0, 0].numpy().copy()
    keep = flow.copy()
    image = V.flow_to_image(torch.from_numpy(flow))
    assert image.shape == (24, 22, 3) and image.dtype == np.uint8 and np.array_equal(flow, keep)
    assert np.array_equal(image, VC.flow_bytes(flow[0], flow[1]))
    nan = flow.copy()
    nan[0, 2, 3] = np.nan
    assert not V.flow_to_image(nan)[2, 3].any() and np.isnan(nan[0, 2, 3])
    centre = V.make_contour(V.heatmap_image(labels['centerness'][0, 0, 0].numpy())[::-1, ::-1])
    assert np.array_equal(centre.transpose(2, 0, 1), VC.panel(want, 0, 'centerness', 0, 24, 22))
    constant = V.heatmap_image(np.full((5, 6), 0.5, dtype=np.float32))                    # delta = 0: the map's first colour
    assert (constant == V.JET_BYTES[0]).all()
    with pytest.raises(ValueError):
        V.heatmap_image(np.zeros((4, 4), dtype=np.int64))
    ids = labels['instance'][0, 2]
    shown = np.unique(ids.numpy())[1:]
    inst = V.make_contour(V.plot_instance_map(ids, dict(zip(shown, shown)))[::-1, ::-1])
    assert np.array_equal(inst.transpose(2, 0, 1), VC.panel(want, 2, 'instance', 0, 24, 22))
    colours = V.generate_instance_colours({5: 74, 6: 140})
    assert tuple(colours[5]) == tuple(V.INSTANCE_COLOURS[4]) and tuple(colours[6]) == tuple(V.INSTANCE_COLOURS[0])
    double = V.make_contour(np.full((6, 7, 3), 9, dtype=np.uint8), colour=[1, 2, 3], double_line=True)
    assert (double[1, 1] == (1, 2, 3)).all() and (double[2:4, 2:5] == 9).all() and (double[:, -2] == (1, 2, 3)).all()


def test_planning_panel_is_the_stated_drawing():
    from stp3_amd import visualisation as V
    labels, output, _ = VC.stored('full')
    cfg = VC.cfg_of('full')
    for sample in (0, 1):
        got = V.make_contour(V.plot_planning(labels['hdmap'][sample], labels['gt_trajectory'][sample], cfg))
        want = VC.planning_panels(labels, output, sample, cfg)[0]
        assert np.array_equal(got.transpose(2, 0, 1), want)
    # every colour of the drawing is there, the clipped last point included (cell (23, 0) is shown at pixel (0, 21): border)
    flat = {tuple(p) for p in want.reshape(3, -1).T}
    assert {(255, 255, 255), (255, 230, 220), (230, 216, 227), (118, 185, 0), (31, 119, 180), (0, 0, 0)} <= flat
    assert V.line_cells(2, 3, 2, 3) == [(2, 3)] and V.line_cells(0, 0, 2, 5) == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]
    assert V.line_cells(4, 1, 0, 0) == [(4, 1), (3, 1), (2, 1), (1, 0), (0, 0)]
    steps = np.diff(np.array(V.line_cells(3, 9, 11, 2)), axis=0)
    assert (np.abs(steps).max(axis=1) == 1).all()                                          # 8-connected, one cell a step


def test_python_entry_validates():
    from stp3_amd import visualisation as V
    labels, output, _ = VC.stored('full')
    cfg = VC.cfg_of('full')
    with pytest.raises(ValueError):
        V.visualise_output(labels, output, cfg, sample=2)
    with pytest.raises(ValueError):
        V.visualise_output(labels, {**output, 'segmentation': output['segmentation'][:, :, :1]}, cfg)
    with pytest.raises(ValueError):
        V.visualise_output(labels, {**output, 'instance_center': output['instance_center'].double()}, cfg)
    with pytest.raises(ValueError):
        V.visualise_output({**labels, 'pedestrian': labels['pedestrian'].float()}, output, cfg)
    with pytest.raises(ValueError):
        V.visualise_output({**labels, 'hdmap': labels['hdmap'][:, :1]}, output, cfg)


def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = 64                                                      # never dereferenced: every call below is refused first
    nbytes = ctypes.c_size_t()

    def desc(**over):
        d = _lib.VisDesc()
        d.T, d.H, d.W, d.panels = 3, 24, 22, 31
        for field in ('seg', 'ped', 'inst', 'center', 'offset', 'flow'):
            for side in range(2):
                m = getattr(d, field)[side]
                m.ptr = fake
                ids = field == 'inst' or (side == 0 and field in ('seg', 'ped'))
                m.dtype = _lib.VIS_DTYPE_I64 if ids else _lib.DTYPE_F32
        for side in range(2):
            d.plan[side].hdmap, d.plan[side].traj, d.plan[side].n_points = fake, fake, 5
            d.plan[side].hd_dtype = _lib.VIS_DTYPE_I64 if side == 0 else _lib.DTYPE_BF16
        d.ego_cells, d.palette, d.jet, d.wheel, d.n_ego = fake, fake, fake, fake, 32
        for k, v in over.items():
            obj = d
            *path, field = k.split('.')
            for p in path:
                obj = getattr(obj, p[:-1])[int(p[-1])] if p[-1].isdigit() else getattr(obj, p)
            setattr(obj, field, v)
        return d
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc()), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 3 * 32 + ctypes.sizeof(_lib.VisDesc)     # 32 bytes of scalars per frame, then the descriptor's copy
    for bad in (dict(T=0), dict(H=2), dict(W=2), dict(panels=32), dict(n_ego=-1), {'seg0.ptr': None}, {'seg1.ptr': None},
                {'seg0.dtype': 0}, {'seg1.dtype': 2}, {'ped1.ptr': None}, {'inst1.dtype': 0}, {'center0.dtype': 2},
                {'offset1.ptr': None}, {'flow0.ptr': None}, {'flow1.dtype': 7}, dict(palette=None), dict(jet=None), dict(wheel=None),
                {'plan0.hdmap': None}, {'plan1.traj': None}, {'plan1.n_points': -1}, {'plan0.hd_dtype': 3}, dict(ego_cells=None)):
        assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc(**bad)), ctypes.byref(nbytes)) == -10001, bad
        assert lib.stp3_vis_render(ctypes.byref(desc(**bad)), fake, fake, None) == -10001, bad
    # what a disabled panel would read is not asked for
    quiet = desc(panels=0, **{'ped0.ptr': None, 'inst0.ptr': None, 'flow1.ptr': None, 'plan0.hdmap': None, 'palette': None})
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(quiet), ctypes.byref(nbytes)) == 0
    assert lib.stp3_vis_workspace_bytes(None, ctypes.byref(nbytes)) == -10001
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc()), None) == -10001
    assert lib.stp3_vis_render(ctypes.byref(desc()), None, fake, None) == -10001
    assert lib.stp3_vis_render(ctypes.byref(desc()), fake, None, None) == -10001
    assert lib.stp3_vis_render(ctypes.byref(desc()), fake, 68, None) == -10001                 # workspace not 8-byte aligned
    # 2 W * 7 H * 3 * T reaches 2^31: 2 * 4096 * 7 * 4096 * 3 * 4 = 2^31 * 1.3; just below passes
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc(T=4, H=4096, W=4096)), ctypes.byref(nbytes)) == -10002
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc(T=3, H=4096, W=4096)), ctypes.byref(nbytes)) == 0
    assert lib.stp3_vis_workspace_bytes(ctypes.byref(desc(T=9363, H=3, W=3)), ctypes.byref(nbytes)) == -10002      # 7 T > 65535


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_vis')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_vis.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_vis.py'), lib, path], env=env, capture_output=True, text=True,
                         timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return request.param or 'plain', dict(np.load(path))


@pytest.mark.parametrize('name,sample', CASE_SAMPLES)
def test_kernels_on_host_match_the_reference(host_kernel, name, sample):
    sys.path.insert(0, HIPCPU)
    import run_vis
    order, out = host_kernel
    c = VC.CASES[name]
    shape = (1, c['T'], 3, 7 * c['H'], 2 * c['W'])
    n = int(np.prod(shape))
    labels, output, _ = VC.stored(name)
    for tag in ('f32', 'bf16'):
        buf = out[f'{name}/{sample}/{tag}']
        assert buf.shape == (n + run_vis.GUARD,) and (buf[n:] == run_vis.FILL).all(), f'{tag}: the guard band was written to'
        VC.compare(name, buf[:n].reshape(shape), sample, labels, output, f'kernels on the host ({order} order, {tag})')
    assert np.array_equal(out[f'{name}/{sample}/bf16'], out[f'{name}/{sample}/f32'])
    if (name, sample) == ('full', 0):
        buf = out['full/0/unaligned']
        assert buf[0] == run_vis.FILL and (buf[1 + n:] == run_vis.FILL).all() and np.array_equal(buf[1:1 + n], out['full/0/f32'][:n])


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_vis_kernels_keep_their_register_budget():
    """No spills of any kind, no scratch; at most 64 registers (8 waves per SIMD: the painter is a latency-bound gather)."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources
    rows = {k['kernel']: k for k in kernel_resources.kernels_of(os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_vis.hip'))}
    print(json.dumps(rows, indent=1))
    assert sorted(rows) == ['vis_paint_kernel', 'vis_prepare_kernel']
    for k in rows.values():
        assert k['vgpr_spills'] == 0 and k['sgpr_spills'] == 0 and k['scratch'] == 0, k
        assert k['vgpr'] + k['agpr'] <= 64, k


# ---- the trainer's hook ----------------------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.calls = []

    def add_video(self, name, video, global_step=None, fps=None):
        self.calls.append((name, video, global_step, fps))


@pytest.mark.parametrize('prefix,name', [('train', 'train_outputs'), ('val', 'val_outputs_3')])
def test_visualise_hands_the_video_to_the_logger(prefix, name):
    from stp3_amd import visualisation as V
    from stp3_amd.trainer import TrainingModule
    labels, output, _ = VC.stored('t1')
    writer = _Writer()
    module = types.SimpleNamespace(cfg=VC.cfg_of('t1'), logger=types.SimpleNamespace(experiment=writer), training_step_count=7)
    video = TrainingModule.visualise(module, labels, output, 3, prefix=prefix)
    assert len(writer.calls) == 1
    got_name, got_video, step, fps = writer.calls[0]
    assert (got_name, step, fps) == (name, 7, 2) and got_video is video
    assert torch.equal(video, V.visualise_output(labels, output, VC.cfg_of('t1')))
    module.logger = None                                             # without a logger the video is only returned
    assert torch.equal(TrainingModule.visualise(module, labels, output, 3, prefix=prefix), video) and len(writer.calls) == 1


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs gcc for the recording library')
def test_training_step_renders_only_with_a_logger(tmp_path):
    """A dry training step (tests/visualisation_trace.py) without a logger makes no call of the video's entries -- the step's
    C-ABI trace is what it was before the hook existed -- and the same step with a logger makes the same calls, in the same
    order, followed by the instance post-processing and ONE stp3_vis_render."""
    recorder = host_trace.build_recorder(str(tmp_path / 'libstp3hip_recorder.so'))
    log = tmp_path / 'trace.log'
    env = {k: v for k, v in os.environ.items() if not k.startswith('STP3_')}
    env.update(STP3_HOST_DRYRUN='1', STP3_TRACE_LOG=str(log), STP3_REAL_LIB=os.path.join(PKG, 'libstp3hip.so'))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'visualisation_trace.py'), recorder], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = log.read_text().splitlines()
    plain_at, logged_at = lines.index('# plain'), lines.index('# logged')
    names = lambda part: [l.split(' ', 1)[0] for l in part if l.startswith('stp3_')]
    plain, logged = names(lines[plain_at:logged_at]), names(lines[logged_at:])
    assert len(plain) > 100 and not [n for n in plain if n.startswith('stp3_vis_')]
    assert logged[:len(plain)] == plain
    extra = logged[len(plain):]
    assert extra[-2:] == ['stp3_vis_workspace_bytes', 'stp3_vis_render'] and extra.count('stp3_vis_render') == 1
    assert all(n.startswith('stp3_instance_') for n in extra[:-2]), extra
    videos = json.loads(lines[-1][len('# videos '):])
    assert len(videos) == 1 and videos[0]['name'] == 'train_outputs' and videos[0]['global_step'] == 3 and videos[0]['fps'] == 2
    assert videos[0]['shape'] == [1, 3, 3, 7 * 64, 2 * 64] and videos[0]['dtype'] == 'torch.uint8'
