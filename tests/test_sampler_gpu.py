"""GPU: csrc/stp3_sampler.hip on the MI355X -- the planner's candidate set against the reference's own sampler as recorded
in tests/golden/sampler.npz (checks and bounds: tests/test_sampler_cpu.py), batched and repeated launches bit for bit, a
captured launch replayed on new draws, drawn samples, and the sampled set through Planning.forward."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_planning_cpu import PLANNING
from tests.test_sampler_cpu import CASES, case, check_one_spacing, check_rows, check_sorting

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('i', CASES)
def test_kernel_matches_the_reference_rows(i):
    from stp3_amd.ops_plan import sample_trajectories, sample_trajectories_reference
    g = H.load('sampler.npz')
    v0, kappa, nf, m, draws = case(g, i, 'cuda')
    unsorted_rows = sample_trajectories(v0, kappa, nf, m, draws=draws, sort=False)
    assert unsorted_rows.is_cuda and unsorted_rows.dtype == torch.float32 and tuple(unsorted_rows.shape) == (1, m, nf + 1, 3)
    check_rows(unsorted_rows[0].cpu().numpy(), g[f'c{i}_rows'], f'kernel, case {i}')
    rows, order = sample_trajectories(v0, kappa, nf, m, draws=draws, return_order=True)
    check_sorting(rows[0].cpu().numpy(), order[0].cpu().numpy(), unsorted_rows[0].cpu().numpy(), g[f'c{i}_keys'], f'kernel, case {i}')
    # the same method in torch float64 on the host
    ref, ref_order = sample_trajectories_reference(v0.cpu(), kappa.cpu(), nf, m, draws=draws.cpu(), sort=False, return_order=True)
    check_one_spacing(unsorted_rows[0].cpu().numpy(), ref[0].numpy(), f'kernel against the torch path, case {i}')
    again, order2 = sample_trajectories(v0, kappa, nf, m, draws=draws, return_order=True)
    assert torch.equal(again, rows) and torch.equal(order2, order)
    assert torch.equal(sample_trajectories(v0, kappa, nf, m, draws=draws), rows)              # without the order output


def test_batch_equals_single_launches():
    from stp3_amd.ops_plan import sample_trajectories
    g = H.load('sampler.npz')
    same = [i for i in CASES if tuple(g[f'c{i}_params'][2:]) == (1800, 6)]
    assert len(same) == 3
    singles = [sample_trajectories(*case(g, i, 'cuda')[:4], draws=case(g, i, 'cuda')[4], return_order=True) for i in same]
    p = np.stack([g[f'c{i}_params'] for i in same])
    draws = torch.from_numpy(np.stack([g[f'c{i}_draws'] for i in same])).cuda()
    rows, order = sample_trajectories(torch.from_numpy(p[:, 0].copy()).cuda(), torch.from_numpy(p[:, 1].copy()).cuda(), 6, 1800,
                                      draws=draws, return_order=True)
    for n, (r, o) in enumerate(singles):
        assert torch.equal(rows[n], r[0]) and torch.equal(order[n], o[0])


def test_captured_launch_replays_on_new_draws():
    from stp3_amd.ops_plan import sample_trajectories
    g = H.load('sampler.npz')
    v0, kappa, nf, m, draws1 = case(g, 1, 'cuda')
    draws2 = case(g, 0, 'cuda')[4]
    buf = draws1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample_trajectories(v0, kappa, nf, m, draws=buf)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sample_trajectories(v0, kappa, nf, m, draws=buf)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, sample_trajectories(v0, kappa, nf, m, draws=draws1))
    buf.copy_(draws2)
    graph.replay()
    torch.cuda.synchronize()
    eager = sample_trajectories(v0, kappa, nf, m, draws=draws2)
    assert torch.equal(out, eager) and not torch.equal(eager, sample_trajectories(v0, kappa, nf, m, draws=draws1))


def test_drawn_samples_have_the_structure_the_planner_relies_on():
    from stp3_amd.ops_plan import sample_trajectories
    v0 = torch.tensor([5.0, 8.3, 0.0, 12.0], device='cuda')
    kappa = torch.tensor([0.0, 0.05, -0.3, 0.004], device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(7)
    rows, order = sample_trajectories(v0, kappa, 6, 1800, generator=gen, return_order=True)
    assert tuple(rows.shape) == (4, 1800, 7, 3) and rows.dtype == torch.float32 and torch.isfinite(rows).all()
    keys = rows[:, :, -1, 0]
    assert (keys.diff(dim=1) >= 0).all()
    assert torch.equal(order.long().sort(dim=1).values, torch.arange(1800, device='cuda').expand(4, 1800))
    tied = keys.diff(dim=1) == 0
    assert (order.diff(dim=1)[tied] > 0).all()
    # every trajectory starts at the ego pose (an arc about a negative curvature at radius * sin(pi) ~ 1e-14, as the reference)
    assert rows[:, :, 0].abs().max() <= 1e-12
    # Planning.command_samples cuts LEFT / FORWARD / RIGHT thirds out of the ordered set
    assert (keys[:, :600].median(dim=1).values < 0).all() and (keys[:, 1200:].median(dim=1).values > 0).all()
    gen2 = torch.Generator(device='cuda').manual_seed(7)
    assert torch.equal(sample_trajectories(v0, kappa, 6, 1800, generator=gen2), rows)


def test_sampled_set_through_the_planner():
    """datas.trajectory_sampling -> Planning.forward in evaluation mode (nuscenes/Planning.yml sizes: 1 800 samples, 6 steps):
    a finite plan, and Planning.select returns a row of the sampled set."""
    from stp3_amd import datas
    from stp3_amd.config import perception_cfg
    from stp3_amd.models.planning_model import Planning
    c = perception_cfg(**{**PLANNING, 'N_FUTURE_FRAMES': 6, 'PLANNING.SAMPLE_NUM': 1800})
    ins = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in H.planning_inputs(c).items()}
    speed, steering = torch.tensor([6.5, 3.0], device='cuda'), torch.tensor([0.04, -0.2], device='cuda')
    sampled = datas.trajectory_sampling(speed, steering, c.N_FUTURE_FRAMES, c.PLANNING.SAMPLE_NUM, left_hand_traffic=False,
                                        generator=torch.Generator(device='cuda').manual_seed(5))
    assert tuple(sampled.shape) == (2, 1800, 7, 3) and sampled.is_cuda
    pl = Planning(c, 64, 6, gru_state_size=c.PLANNING.GRU_STATE_SIZE)
    for sub in (pl.reduce_channel, pl.GRU, pl.decoder):
        H.fill_deterministic(sub)
    pl = pl.cuda().eval()
    trajs = sampled[:, :, 1:]                                                                 # as the trainer hands them over
    with torch.no_grad():
        loss, plan = pl(ins['cam_front'], trajs, ins['gt_trajs'], ins['cost_volume'], ins['occupancy'], ins['hdmap_logits'],
                        ins['commands'], ins['target'])
        samples = pl.command_samples(trajs, ins['commands'])
        lane, drivable = ins['hdmap_logits'][:, 0:2], ins['hdmap_logits'][:, 2:4]
        chosen = pl.select(samples, ins['cost_volume'], ins['occupancy'], lane, drivable, ins['target'])
    assert loss == 0 and tuple(plan.shape) == (2, 6, 3) and torch.isfinite(plan).all()
    assert tuple(chosen.shape) == (2, 6, 3)
    for b in range(2):
        assert (trajs[b] == chosen[b]).flatten(1).all(dim=1).any(), b
