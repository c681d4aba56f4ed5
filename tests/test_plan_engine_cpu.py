"""CPU: the planner tail of an inference call -- ``ops_plan.plan_scene`` / ``plan_drive`` / ``Planning.drive`` (csrc/stp3_plan.hip:
stp3_plan_scene, stp3_plan_drive) -- against the reference and against this project's own torch statements.

The real kernel sources run on the host (tests/hipcpu/run_plan_engine.py); the torch restatements run as they are.
  * tests/golden/planning.npz ``planner/eval/traj``: 1e-4, the tolerance ``Planning.forward`` is held to against that array
    (tests/test_planning_cpu.check_planner as tests/test_planning_gpu.test_planner_float32 calls it);
  * tests/golden/plan_engine.npz (scripts/make_golden_plan_engine.py: the unmodified reference on B = 4, the commands RIGHT / LANE /
    LEFT / FORWARD, with and without a target): refined trajectory 1e-4, occupancy and the selected ROW exact (rows, not
    indices: the reference's triplicated set has three indices per row); the fixture's own margin between the best and the
    second-best distinct total is asserted to be beyond COST_TOL;
  * the scene kernel against the torch statements on continuous random logits: occupancy exact (hand-made argmax ties included),
    mask values within 1e-6, threshold decisions equal wherever the probability is further than 1e-6 from 0.5, those cells
    being fewer than 0.1 % (the hand-made cells AT 0.5 are checked apart: lane zeroed, drivable kept);
  * selection on N = 1 800, T = 6, B = 4: the float64 total (the module's torch statements) of the kernel's pick within COST_TOL of
    the minimum over the command's range; an exact tie gives the lower index;
  * arguments: both C entry points without a GPU, the Python entries, ``command_codes``."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import plan_engine_cases as PC
from tests.test_planning_cpu import COST_TOL, PLANNING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
TRAJ_TOL = dict(rtol=1e-4, atol=1e-4)
EINVAL, EUNSUP = -10001, -10002


def cfg(**over):
    from stp3_amd.config import perception_cfg
    return perception_cfg(**{**PLANNING, **over})


@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_plan_engine')
    lib = hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'))
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_plan_engine.py'), lib, str(tmp / 'out.npz')], env=env,
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(str(tmp / 'out.npz')))


def torch_path(planner, ins, scene):
    """``plan_scene`` + ``Planning.drive`` on CPU tensors: the torch restatements."""
    from stp3_amd import ops_plan
    with torch.no_grad():
        occupancy, lane, drivable = ops_plan.plan_scene(*scene)
        trajs = ins['trajs'] if 'segmentation' in ins else ins['sample_trajs']
        final, selected, index = planner.drive(ins['cam_front'], trajs, ins['cost_volume'], occupancy, lane, drivable,
                                               ops_plan.command_codes(ins['commands']), ins['target'])
    return {'final': final.numpy(), 'selected': selected.numpy(), 'index': index.numpy(), 'occupancy': occupancy.numpy(),
            'lane': lane.numpy(), 'drivable': drivable.numpy()}


# ---- 1. tests/golden/planning.npz ----
def test_torch_statements_match_planning_fixture():
    planner, ins = PC.golden_planner(cfg())
    got = torch_path(planner, ins, (PC.logits_of(ins['occupancy']), None, ins['hdmap_logits'], 0))
    want = H.load('planning.npz')['planner/eval/traj']
    print('[plan engine] torch statements vs planner/eval/traj:', np.abs(got['final'] - want).max())
    np.testing.assert_allclose(got['final'], want, **TRAJ_TOL)
    assert np.array_equal(got['occupancy'], ins['occupancy'].float().numpy())
    assert got['index'].dtype == np.int32 and np.array_equal(got['selected'], ins['sample_trajs'].numpy()[[0, 1], got['index']])


def test_kernel_on_host_matches_planning_fixture(host_kernel):
    want = H.load('planning.npz')['planner/eval/traj']
    ins = H.planning_inputs(cfg())
    print('[plan engine] kernel on the host vs planner/eval/traj:', np.abs(host_kernel['golden/final'] - want).max())
    np.testing.assert_allclose(host_kernel['golden/final'], want, **TRAJ_TOL)
    assert np.array_equal(host_kernel['golden/occupancy'], ins['occupancy'].float().numpy())
    index = host_kernel['golden/index']
    assert index.dtype == np.int32 and 0 <= index[0] < 20 <= index[1] < 40            # LEFT, FORWARD of 60 rows
    assert np.array_equal(host_kernel['golden/selected'], ins['sample_trajs'].numpy()[[0, 1], index])
    assert (host_kernel['golden/final'][..., 2] == 0).all()


# ---- 2. tests/golden/plan_engine.npz ----
def test_fixture_holds_data_only_and_no_near_tie():
    g = H.load('plan_engine.npz')
    assert os.path.getsize(os.path.join(H.GOLDEN, 'plan_engine.npz')) <= 16 << 10
    assert sorted(g.files) == sorted(['commands', 'occupancy'] + [f'{c}/{k}' for c in ('target', 'zero')
                                                                  for k in ('traj', 'selected', 'best', 'second')])
    assert list(g['commands']) == PC.COMMANDS and g['occupancy'].dtype == np.uint8
    for case in ('target', 'zero'):
        best, second = g[f'{case}/best'].astype(np.float64), g[f'{case}/second'].astype(np.float64)
        assert best.shape == (4,) and (second - best > COST_TOL['atol'] + COST_TOL['rtol'] * np.abs(second)).all(), (best, second)
    assert not np.array_equal(g['target/best'], g['zero/best']) and not np.array_equal(g['target/traj'], g['zero/traj'])   # the goal term counts


def fixture_occupancy(g, T=4):
    return np.unpackbits(g['occupancy']).reshape(PC.BATCH, T, 200, 200).astype(np.float32)


def check_against_fixture(got, case, what):
    g = H.load('plan_engine.npz')
    ins = PC.inputs(cfg(), zero_target=case == 'zero')
    err = np.abs(got['final'] - g[f'{case}/traj']).max()
    print(f'[plan engine] {what}, case {case}: refined trajectory within {err:.3e} of the reference (bound 1e-4), rows', got['index'])
    np.testing.assert_allclose(got['final'], g[f'{case}/traj'], **TRAJ_TOL)
    assert np.array_equal(got['occupancy'], fixture_occupancy(g))
    assert np.array_equal(got['selected'], g[f'{case}/selected'])
    assert np.array_equal(got['selected'], ins['trajs'].numpy()[np.arange(PC.BATCH), got['index']])
    for b, command in enumerate(PC.COMMANDS):
        lo, hi = PC.command_range(command, ins['trajs'].shape[1])
        assert lo <= got['index'][b] < hi, (b, command, got['index'][b])


@pytest.mark.parametrize('case', ['target', 'zero'])
def test_torch_statements_match_reference_fixture(case):
    from stp3_amd.models.planning_model import Planning
    c = cfg()
    ins = PC.inputs(c, zero_target=case == 'zero')
    got = torch_path(PC.planner(c, Planning), ins, (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']))
    check_against_fixture(got, case, 'torch statements')


@pytest.mark.parametrize('case', ['target', 'zero'])
def test_kernel_on_host_matches_reference_fixture(host_kernel, case):
    got = {k: host_kernel[f'{case}/{k}'] for k in ('final', 'selected', 'index', 'occupancy')}
    check_against_fixture(got, case, 'kernel on the host')


# ---- 3. the scene kernel against the torch statements ----
@pytest.mark.parametrize('name,dtype', [('scene_f32', torch.float32), ('scene_bf16', torch.bfloat16), ('scene_cl', torch.float32)])
def test_scene_kernel_on_host_against_torch_statements(host_kernel, name, dtype):
    from stp3_amd.ops_plan import plan_scene_reference
    from stp3_amd.utils import hp
    seg, ped, hd, n_present, ties = PC.scene_case(dtype)
    occupancy, lane, drivable = plan_scene_reference(seg, ped, hd, n_present)
    assert np.array_equal(host_kernel[f'{name}/occupancy'], occupancy.numpy())
    assert 0.05 < occupancy.mean() < 0.95
    for row in ties['free']:
        assert (host_kernel[f'{name}/occupancy'][:, :, row] == 0).all(), row
    for row in ties['occupied']:
        assert (host_kernel[f'{name}/occupancy'][:, :, row] == 1).all(), row
    excluded = 0
    for key, want, pair, keep_half in (('lane', lane, hd[:, 0:2], False), ('drivable', drivable, hd[:, 2:4], True)):
        got = host_kernel[f'{name}/{key}']
        prob = torch.softmax(hp(pair).double(), dim=1)[:, 1].numpy()
        exact_half = (hp(pair)[:, 0] == hp(pair)[:, 1]).numpy()                       # the hand-made cells: probability exactly 0.5
        band = (np.abs(prob - 0.5) <= 1e-6) & ~exact_half
        excluded += int(band.sum())
        clear = ~band
        assert np.array_equal((got != 0)[clear], (want.numpy() != 0)[clear]), key
        assert np.abs(got - want.numpy())[clear].max() <= 1e-6, key
        assert exact_half.sum() >= 16 and ((got[exact_half] == 0.5).all() if keep_half else (got[exact_half] == 0).all()), key
    share = excluded / (2 * lane.numel())
    print(f'[plan engine] {name}: {excluded} cells within 1e-6 of the threshold ({share:.2e} of all; bound 1e-3)')
    assert share < 1e-3


def test_scene_kernel_without_pedestrian_head(host_kernel):
    from stp3_amd.ops_plan import plan_scene_reference
    seg, _, hd, n_present, _ = PC.scene_case()
    assert np.array_equal(host_kernel['scene_noped/occupancy'], plan_scene_reference(seg, None, hd, n_present)[0].numpy())
    assert not np.array_equal(host_kernel['scene_noped/occupancy'], host_kernel['scene_f32/occupancy'])


def test_scene_layouts_agree_bitwise(host_kernel):
    for k in ('occupancy', 'lane', 'drivable'):
        assert np.array_equal(host_kernel[f'scene_cl/{k}'].view(np.uint32), host_kernel[f'scene_f32/{k}'].view(np.uint32)), k


# ---- 4. selection ----
def totals_float64(c, ins, lane, drivable, occupancy, trajs):
    from stp3_amd.cost import Cost_Function
    cf = Cost_Function(c).double()
    with torch.no_grad():
        fc, fo = cf(ins['cost_volume'].double(), trajs[..., :2].double(), torch.from_numpy(occupancy).double(),
                    torch.from_numpy(lane).double()[:, None], torch.from_numpy(drivable).double()[:, None], ins['target'].double())
    return (fc + fo.sum(dim=-1)).numpy()


def test_selection_is_the_cheapest_of_the_command_range(host_kernel):
    c = cfg(**{'N_FUTURE_FRAMES': 6, 'PLANNING.SAMPLE_NUM': 1800})
    ins = PC.selection_case(c)
    assert tuple(ins['trajs'].shape) == (4, 1800, 6, 3) and not ins['trajs'].is_contiguous()
    lane, drivable, occupancy = (host_kernel[f'select/{k}'] for k in ('lane', 'drivable', 'occupancy'))
    total = totals_float64(c, ins, lane, drivable, occupancy, ins['trajs'])
    index = host_kernel['select/index']
    for b, command in enumerate(PC.COMMANDS):
        lo, hi = PC.command_range(command, 1800)
        assert lo <= index[b] < hi
        got, best = total[b, index[b]], total[b, lo:hi].min()
        print(f'[plan engine] sample {b} ({command}): row {index[b]}, float64 total {got:.6f}, minimum of the range {best:.6f}')
        assert got - best <= COST_TOL['atol'] + COST_TOL['rtol'] * abs(best), (b, got, best)
    assert np.array_equal(host_kernel['select/selected'], ins['trajs'].numpy()[np.arange(4), index])
    assert np.isfinite(host_kernel['select/final']).all()
    # an exact tie: the winner's row copied over a neighbour -- the lower of the two indices is returned
    other = host_kernel['tie/other']
    assert (other != index).all() and (np.abs(other - index) == 1).all()
    assert np.array_equal(host_kernel['tie/index'], np.minimum(index, other))
    assert (other < index).any()
    assert np.array_equal(host_kernel['tie/selected'], host_kernel['select/selected'])
    assert np.array_equal(host_kernel['tie/final'].view(np.uint32), host_kernel['select/final'].view(np.uint32))


def test_torch_statements_break_an_exact_tie_towards_the_lower_index():
    from stp3_amd.models.planning_model import Planning
    c = cfg()
    ins = PC.inputs(c)
    planner = PC.planner(c, Planning)
    scene = (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present'])
    first = torch_path(planner, ins, scene)
    ins['trajs'] = ins['trajs'].clone()
    other = []
    for b, command in enumerate(PC.COMMANDS):
        lo, _ = PC.command_range(command, 60)
        win = int(first['index'][b])
        other.append(win - 1 if win > lo else win + 1)
        ins['trajs'][b, other[-1]] = ins['trajs'][b, win]
    again = torch_path(planner, ins, scene)
    assert np.array_equal(again['index'], np.minimum(first['index'], np.array(other)))
    assert np.array_equal(again['final'], first['final'])


# ---- 5. arguments ----
def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused first

    def scene(d, **null):
        a = dict(seg=fake, ped=fake, hd=fake, occ=fake, lane=fake, drv=fake)
        a.update(null)
        return lib.stp3_plan_scene(ctypes.byref(d) if d is not None else None, a['seg'], a['ped'], a['hd'], a['occ'], a['lane'],
                                   a['drv'], None)

    def scene_dims(**over):
        d = _lib.SceneDims()
        d.B, d.S, d.T, d.H, d.W, d.Cs, d.Cp, d.first = 1, 7, 4, 200, 200, 2, 2, 3
        for k, v in over.items():
            setattr(d, k, v)
        return d
    assert scene(None) == EINVAL
    for null in ('seg', 'ped', 'hd', 'occ', 'lane', 'drv'):
        assert scene(scene_dims(), **{null: None}) == EINVAL, null
    for over in (dict(B=0), dict(T=0), dict(H=0), dict(W=-1), dict(Cs=0), dict(Cp=-1), dict(first=-1), dict(first=4), dict(S=6)):
        assert scene(scene_dims(**over)) == EINVAL, over
    for over in (dict(seg_dtype=2), dict(ped_dtype=7), dict(hd_dtype=-1), dict(B=65536, H=4, W=4)):
        assert scene(scene_dims(**over)) == EUNSUP, over

    names = ('trajs', 'cv', 'occ', 'drv', 'lane', 'target', 'command', 'fp0', 'fpl', 'h0', 'final', 'selected', 'index')

    def plan_dims(**over):
        d = _lib.PlanDims()
        d.B, d.N, d.T, d.H, d.W, d.K0, d.KL = 1, 1800, 6, 200, 200, 32, 192
        d.dx0 = d.dx1 = 0.5
        d.lr_dist = 1.0
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def drive_dims(**over):
        q = _lib.DriveDims()
        q.Hs, q.traj_cols, q.traj_batch_stride, q.traj_row_stride, q.traj_point_stride, q.cv_batch_stride = 256, 3, 1800 * 21, 21, 3, 240000
        q.weights = 64
        for k, v in over.items():
            setattr(q, k, v)
        return q

    def drive(d, q, **null):
        a = {k: fake for k in names}
        a.update(null)
        return lib.stp3_plan_drive(ctypes.byref(d) if d is not None else None, ctypes.byref(q) if q is not None else None,
                                   *[a[k] for k in names], None)
    assert drive(None, drive_dims()) == EINVAL and drive(plan_dims(), None) == EINVAL
    for null in names:
        assert drive(plan_dims(), drive_dims(), **{null: None}) == EINVAL, null
    assert drive(plan_dims(), drive_dims(weights=None)) == EINVAL
    assert drive(plan_dims(), drive_dims(traj_batch_stride=1 << 31)) == EUNSUP
    for over in (dict(N=1801), dict(N=1799), dict(B=0), dict(T=0), dict(dx0=0.0)):
        assert drive(plan_dims(**over), drive_dims()) == EINVAL, over
    for over in (dict(Hs=0), dict(Hs=-64), dict(traj_cols=1), dict(traj_point_stride=2), dict(traj_row_stride=-1)):
        assert drive(plan_dims(), drive_dims(**over)) == EINVAL, over
    for over in (dict(Hs=100), dict(Hs=576), dict(Hs=1024), dict(Hs=32), dict(cv_dtype=2), dict(h0_dtype=-1)):
        assert drive(plan_dims(), drive_dims(**over)) == EUNSUP, over
    assert drive(plan_dims(N=6000), drive_dims()) == EUNSUP                            # 4 (N (T + 1) + ...) bytes > 160 KB of LDS
    assert drive(plan_dims(T=342, N=3), drive_dims()) == EUNSUP
    assert ctypes.sizeof(_lib.SceneDims) == 160 and ctypes.sizeof(_lib.DriveDims) == 56


def test_command_codes():
    from stp3_amd.ops_plan import command_codes
    codes = command_codes(['LEFT', 'FORWARD', 'RIGHT', 'LANE', 'left', '', 'LANEFOLLOW'])
    assert codes.dtype == torch.int32 and codes.tolist() == [0, 1, 2, 3, 3, 3, 3]
    for bad in ('LEFT', [0, 1], [None]):
        with pytest.raises(ValueError):
            command_codes(bad)


def test_python_entries_validate():
    from stp3_amd import ops_plan
    from stp3_amd.models.planning_model import Planning
    c = cfg()
    ins = PC.inputs(c)
    seg, ped, hd, n_present = ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']
    for args in ((seg[:, :, :, :100], ped, hd, n_present), (seg, ped[:, :3], hd, n_present), (seg, ped, hd[:, :2], n_present),
                 (seg, ped, hd, 7), (seg, ped, hd, -1), (seg[0], ped, hd, n_present), (seg.double(), ped, hd, n_present),
                 (seg, ped, hd.half(), n_present), (seg.long(), ped, hd, n_present)):
        with pytest.raises(ValueError):
            ops_plan.plan_scene(*args)
    planner = PC.planner(c, Planning)
    occupancy, lane, drivable = ops_plan.plan_scene(seg, ped, hd, n_present)
    codes = ops_plan.command_codes(ins['commands'])
    h0 = torch.zeros(4, c.PLANNING.GRU_STATE_SIZE)
    good = dict(trajs=ins['trajs'], cost_volume=ins['cost_volume'], occupancy=occupancy, lane=lane, drivable=drivable, codes=codes,
                target=ins['target'], h0=h0)
    for bad in (dict(trajs=ins['trajs'][:, :59]), dict(trajs=ins['trajs'][..., :1]), dict(trajs=ins['trajs'].double()),
                dict(cost_volume=ins['cost_volume'][:, :3]), dict(cost_volume=ins['cost_volume'].long()), dict(occupancy=occupancy[:, :3]),
                dict(lane=lane[:, :100]), dict(drivable=drivable[:2]), dict(codes=codes.long()), dict(codes=codes[:3]),
                dict(target=ins['target'][:, :1]), dict(h0=h0[:2]), dict(h0=h0[0])):
        with pytest.raises(ValueError):
            ops_plan.plan_drive(planner, **{**good, **bad})
    final, selected, index = ops_plan.plan_drive(planner, **good)
    assert tuple(final.shape) == (4, 4, 3) and tuple(selected.shape) == (4, 4, 3) and index.dtype == torch.int32


def test_drive_weights_follow_a_load_state_dict():
    """The transposed copies keep their addresses and follow the parameters' versions."""
    from stp3_amd.models.planning_model import Planning
    planner = PC.planner(cfg(), Planning)
    w = planner.drive_weights('cpu')
    assert planner.drive_weights('cpu') is w and w.current()
    assert torch.equal(w.buffers['w_hh_t'], planner.GRU.weight_hh.detach().t()) and w.buffers['w_hh_t'].is_contiguous()
    ptrs = {k: v.data_ptr() for k, v in w.buffers.items()}
    sd = {k: v * 1.5 for k, v in planner.state_dict().items() if k.startswith(('GRU.', 'decoder.'))}
    planner.load_state_dict(sd, strict=False)
    assert not w.current()
    assert planner.drive_weights('cpu') is w and w.current()
    assert torch.equal(w.buffers['w1_t'], planner.decoder[0].weight.detach().t()) and torch.equal(w.buffers['b2'], planner.decoder[2].bias)
    assert ptrs == {k: v.data_ptr() for k, v in w.buffers.items()}
