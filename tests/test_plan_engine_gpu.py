"""GPU: the planner tail on the MI355X -- ``ops_plan.plan_scene`` + ``Planning.drive`` (stp3_plan_scene / stp3_plan_drive) against the
reference fixtures and against the eager chain it replaces (evaluate.py:96-132: argmax, logical_or, ``model.planning``).

FIXTURES: float32 ``Planning.drive`` within 1e-4 of tests/golden/planning.npz ``planner/eval/traj`` and of both cases of
tests/golden/plan_engine.npz (occupancy and selected row exact); under bf16 autocast (bf16 only inside ``reduce_channel``) within
5e-2 absolute of ``planner/eval/traj``, the bound of tests/test_planning_gpu.test_planner_bf16_autocast.
EAGER CHAIN, on the outputs of a planning model's forward under bf16 autocast (bf16 heads in the layouts the decoder leaves):
``occupancy`` bit-equal to the argmax / logical_or statements; ``selected_traj`` equal to what ``Planning.select`` picks (the eager
totals' best and second-best distinct candidates further apart than COST_TOL: asserted); ``final_traj``: its error against a
float64 evaluation of the same GRU and decoder from the same h0 and selected trajectory at most 4 x the error of the eager
``Planning.forward`` against that truth (measured: 2.5e-7 .. 3.7e-7 against 3.1e-3 .. 5.1e-3 -- under autocast the eager GRU
and decoder run in bf16, the kernel always in float32); a second batch with other commands and targets; two calls bit-equal;
new planner weights are followed (``Planning.drive_weights``).
(The same tail captured into ``InferenceEngine``'s graph passed these checks too, but was no faster per tick than the eager
chain -- profiles/plan_engine_timing.txt -- and is not part of the engine.)"""
import copy

import numpy as np
import pytest
import torch

from stp3_amd import synthetic
from tests import helpers as H
from tests import plan_engine_cases as PC
from tests.test_inference_gpu import _plain
from tests.test_planning_cpu import COST_TOL, PLANNING, cfg

pytestmark = pytest.mark.gpu
TRAJ_TOL = dict(rtol=1e-4, atol=1e-4)
BATCH, SEED = 2, 7
COMMANDS = (['LEFT', 'LANE'], ['RIGHT', 'FORWARD'])


def cuda(ins):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in ins.items()}


def drive(planner, ins, scene, trajs, autocast=False):
    from stp3_amd import ops_plan
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        occupancy, lane, drivable = ops_plan.plan_scene(*scene)
        final, selected, index = planner.drive(ins['cam_front'], trajs, ins['cost_volume'], occupancy, lane, drivable,
                                               ops_plan.command_codes(ins['commands'], device='cuda'), ins['target'])
    assert final.dtype == torch.float32 and index.dtype == torch.int32
    return {'final': final.cpu().numpy(), 'selected': selected.cpu().numpy(), 'index': index.cpu().numpy(),
            'occupancy': occupancy.cpu().numpy()}


# ---- 7. the fixtures on the device ----
@pytest.mark.parametrize('autocast', [False, True])
def test_drive_matches_planning_fixture(autocast):
    planner, ins = PC.golden_planner(cfg())
    planner, ins = planner.cuda(), cuda(ins)
    got = drive(planner, ins, (PC.logits_of(ins['occupancy']), None, ins['hdmap_logits'], 0), ins['sample_trajs'], autocast)
    want = H.load('planning.npz')['planner/eval/traj']
    err = np.abs(got['final'] - want).max()
    print(f'[plan engine] Planning.drive (bf16 autocast: {autocast}) vs planner/eval/traj: {err:.3e}')
    if autocast:
        assert err <= 5e-2
    else:
        np.testing.assert_allclose(got['final'], want, **TRAJ_TOL)
    assert np.array_equal(got['occupancy'], ins['occupancy'].float().cpu().numpy())
    assert np.array_equal(got['selected'], ins['sample_trajs'].cpu().numpy()[[0, 1], got['index']])


@pytest.mark.parametrize('case', ['target', 'zero'])
def test_drive_matches_reference_fixture(case):
    from stp3_amd.models.planning_model import Planning
    from tests.test_plan_engine_cpu import check_against_fixture
    c = cfg()
    ins = cuda(PC.inputs(c, zero_target=case == 'zero'))
    planner = PC.planner(c, Planning).cuda()
    got = drive(planner, ins, (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']), ins['trajs'])
    check_against_fixture(got, case, 'Planning.drive on the GPU')
    again = drive(planner, ins, (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']), ins['trajs'])
    assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got)      # bit-reproducible


# ---- 8. the engine against the eager chain ----
@torch.no_grad()
def eager_chain(model, batch, commands):
    """What a caller runs today (evaluate.py:88-132) under bf16 autocast, plus the quantities the checks need."""
    plain = _plain(model, batch)
    rf = model.receptive_field
    seg = torch.argmax(plain['segmentation'], dim=2, keepdim=True)
    ped = torch.argmax(plain['pedestrian'], dim=2, keepdim=True)
    occupancy = torch.logical_or(seg, ped)
    trajs, target = batch['sample_trajectory'].cuda()[:, :, 1:], batch['target_point'].cuda()
    planning = model.planning
    args = (plain['costvolume'][:, rf:], occupancy[:, rf:].squeeze(2), plain['hdmap'][:, 0:2], plain['hdmap'][:, 2:4], target)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        _, final = planning(plain['cam_front'], trajs, None, args[0], args[1], plain['hdmap'], commands, target)
        samples = planning.command_samples(trajs, commands)
        selected = planning.select(samples, *args)
        fc, fo = planning._costs(trajs, *args)
        h0 = planning.reduce_channel(plain['cam_front']).flatten(start_dim=1).float()
    total = fc + fo.sum(dim=-1)
    # float64 truth of the refinement from the same h0 and selected trajectory
    gru, dec = copy.deepcopy(planning.GRU).double(), copy.deepcopy(planning.decoder).double()
    h, point, truth = h0.double(), torch.zeros(len(h0), 2, device='cuda', dtype=torch.float64), []
    for i in range(selected.shape[1]):
        h = gru(torch.cat([point, selected[:, i, :2].double(), target.double()], dim=-1), h)
        point = dec(h)
        truth.append(point)
    return {'plain': plain, 'occupancy': occupancy[:, rf:].squeeze(2).float(), 'selected': selected, 'final': final.float(),
            'total': total, 'truth': torch.stack(truth, dim=1)}


def assert_no_near_tie(total, commands):
    for b, command in enumerate(commands):
        lo, hi = PC.command_range(command, total.shape[1])
        two = torch.sort(total[b, lo:hi].double()).values[:2]
        gap, bound = float(two[1] - two[0]), COST_TOL['atol'] + COST_TOL['rtol'] * abs(float(two[1]))
        print(f'[plan engine] sample {b} ({command}): best {float(two[0]):.6f}, second {float(two[1]):.6f}, gap {gap:.3e} (COST_TOL {bound:.1e})')
        assert gap > bound, 'the eager totals have a near-tie: change SEED'


@torch.no_grad()
def drive_chain(model, plain, batch, commands):
    """``plan_scene`` + ``Planning.drive`` on the forward's outputs, as a caller of the new API writes it."""
    from stp3_amd import ops_plan
    rf = model.receptive_field
    with torch.autocast('cuda', dtype=torch.bfloat16):
        occupancy, lane, drivable = ops_plan.plan_scene(plain['segmentation'], plain['pedestrian'], plain['hdmap'], rf)
        final, selected, index = model.planning.drive(plain['cam_front'], batch['sample_trajectory'].cuda()[:, :, 1:],
                                                      plain['costvolume'][:, rf:], occupancy, lane, drivable,
                                                      ops_plan.command_codes(commands, device='cuda'), batch['target_point'].cuda())
    return {'final_traj': final, 'selected_traj': selected, 'selected_index': index, 'occupancy': occupancy}


def check_call(out, eager, commands, what):
    assert out['occupancy'].dtype == torch.float32 and torch.equal(out['occupancy'], eager['occupancy'])
    assert_no_near_tie(eager['total'], commands)
    assert torch.equal(out['selected_traj'], eager['selected'])
    index = out['selected_index'].long()
    for b, command in enumerate(commands):
        lo, hi = PC.command_range(command, eager['total'].shape[1])
        assert lo <= int(index[b]) < hi
    assert out['final_traj'].dtype == torch.float32 and (out['final_traj'][..., 2] == 0).all()
    err_drive = float((out['final_traj'][..., :2].double() - eager['truth']).abs().max())
    err_eager = float((eager['final'][..., :2].double() - eager['truth']).abs().max())
    print(f'[plan engine] {what}: final_traj error against the float64 refinement: Planning.drive {err_drive:.3e}, eager '
          f'Planning.forward {err_eager:.3e} (bound: 4 x the eager error)')
    assert err_drive <= 4.0 * err_eager, (err_drive, err_eager)


@pytest.fixture(scope='module')
def planning_model():
    from stp3_amd.cost import Cost_Function
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    c = cfg()
    model = H.fill_deterministic(STP3(c))
    # (the cost function's parameters are grid constants -- dx, bx, the safety weights -- not weights to randomise)
    model.planning.cost_function.load_state_dict(Cost_Function(c).state_dict())
    model = to_channels_last(model.eval().cuda())
    batch = synthetic.make_batch(batch=BATCH, seq=7, seed=SEED, planning=(c.N_FUTURE_FRAMES, c.PLANNING.SAMPLE_NUM))
    return model, batch


def test_drive_equals_the_eager_chain(planning_model):
    model, batch = planning_model
    eager = eager_chain(model, batch, COMMANDS[0])
    assert eager['plain']['segmentation'].dtype in (torch.bfloat16, torch.float32)   # the kernels read the heads as they are
    out = drive_chain(model, eager['plain'], batch, COMMANDS[0])
    assert tuple(out['final_traj'].shape) == (BATCH, 4, 3)
    check_call(out, eager, COMMANDS[0], 'first batch')
    other = synthetic.make_batch(batch=BATCH, seq=7, seed=SEED + 4, planning=(4, 60))
    eager2 = eager_chain(model, other, COMMANDS[1])
    out2 = drive_chain(model, eager2['plain'], other, COMMANDS[1])
    check_call(out2, eager2, COMMANDS[1], 'second batch')
    assert not torch.equal(out2['final_traj'], out['final_traj']) and not torch.equal(out2['selected_traj'], out['selected_traj'])
    again = drive_chain(model, eager2['plain'], other, COMMANDS[1])
    assert all(torch.equal(again[k], out2[k]) for k in out2)                          # bit-reproducible


def test_drive_follows_new_planner_weights(planning_model):
    """The transposed weight copies follow a ``load_state_dict`` in place."""
    model, batch = planning_model
    eager = eager_chain(model, batch, COMMANDS[0])
    out = drive_chain(model, eager['plain'], batch, COMMANDS[0])
    planning = model.planning
    weights = planning.drive_weights(torch.device('cuda', torch.cuda.current_device()))
    ptr = weights.buffer.data_ptr()
    original = {k: v.clone() for k, v in planning.state_dict().items()}
    g = torch.Generator(device='cuda').manual_seed(9)
    changed = {k: (v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g, device=v.device)
                   if v.is_floating_point() and k.startswith(('GRU.', 'decoder.')) else v) for k, v in original.items()}
    try:
        planning.load_state_dict(changed)
        fresh = drive_chain(model, eager['plain'], batch, COMMANDS[0])
        assert not torch.equal(fresh['final_traj'], out['final_traj'])
        check_call(fresh, eager_chain(model, batch, COMMANDS[0]), COMMANDS[0], 'after load_state_dict')
    finally:
        planning.load_state_dict(original)
    back = drive_chain(model, eager['plain'], batch, COMMANDS[0])
    assert all(torch.equal(back[k], out[k]) for k in out)
    assert sum(w.buffer.data_ptr() == ptr for w in planning.__dict__['_drive_weights'].values()) == 1
