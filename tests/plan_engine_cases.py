"""TEST INFRASTRUCTURE -- the inputs of tests/golden/plan_engine.npz, built by scripts/make_golden_plan_engine.py (reference side)
and tests/test_plan_engine_*.py / tests/hipcpu/run_plan_engine.py (this project's side) from ``helpers.det_tensor``: exact integer
arithmetic, bit-identical everywhere.  The fixture stores expected outputs only."""
import torch

from tests import helpers as H

BATCH = 4
COMMANDS = ['RIGHT', 'LANE', 'LEFT', 'FORWARD']            # 'LANE': none of the three thirds -- all candidates
TARGETS = [[-3.0, 20.0], [2.0, 25.0], [4.0, 18.0], [0.0, 30.0]]
SEED = 400                                                  # (changed until no sample's selection rests on a near-tie)


def planner(cfg, cls):
    """``cls`` (this project's Planning or the reference's) with the deterministic weights, in eval mode."""
    pl = cls(cfg, 64, 6, gru_state_size=cfg.PLANNING.GRU_STATE_SIZE)
    for sub in (pl.reduce_channel, pl.GRU, pl.decoder):
        H.fill_deterministic(sub)
    return pl.eval()


def inputs(cfg, zero_target=False):
    """Decoder-head logits with a sparse foreground (an obstacle ahead, speckles elsewhere, pedestrians in other cells), hd-map
    logits with two dividers and a drivable corridor, candidates as ``helpers.planning_inputs`` builds them."""
    B, N, T, S = BATCH, cfg.PLANNING.SAMPLE_NUM, cfg.N_FUTURE_FRAMES, cfg.TIME_RECEPTIVE_FIELD + cfg.N_FUTURE_FRAMES
    step_y = H.det_tensor((B, N, T), SEED + 1).abs() * 6.0
    step_x = H.det_tensor((B, N, T), SEED + 2, 1.5)
    scale = torch.where(torch.arange(N) % 11 == 10, 4.0, 1.0).view(1, N, 1)
    trajs = torch.stack([torch.cumsum(step_x, dim=2) * scale, torch.cumsum(step_y, dim=2) * scale,
                         H.det_tensor((B, N, T), SEED + 3)], dim=-1)
    seg = H.det_tensor((B, S, 2, 200, 200), SEED + 4)
    seg[:, :, 0] += 1.8
    seg[:, :, 1, 112:118, 96:104] += 4.0                   # an obstacle 6-9 m ahead
    ped = H.det_tensor((B, S, 2, 200, 200), SEED + 5)
    ped[:, :, 0] += 1.9
    ped[:, :, 1, 130:133, 90:93] += 4.0
    hd = H.det_tensor((B, 4, 200, 200), SEED + 6)
    hd[:, 1, :, 92] += 3.0
    hd[:, 1, :, 108] += 3.0
    hd[:, 3, :, 85:116] += 3.0
    hd[:, 2, :, :85] += 3.0
    hd[:, 2, :, 116:] += 3.0
    hd[1, 3, 120:, :] -= 6.0                               # sample 1: the road ends 10 m ahead
    target = torch.zeros(B, 2) if zero_target else torch.tensor(TARGETS)
    return {'trajs': trajs, 'segmentation': seg, 'pedestrian': ped, 'hdmap': hd,
            'cost_volume': H.det_tensor((B, T, 200, 200), SEED + 7, 2.0), 'cam_front': H.det_tensor((B, 64, 28, 60), SEED + 8),
            'target': target, 'commands': list(COMMANDS), 'n_present': cfg.TIME_RECEPTIVE_FIELD}


def golden_planner(cfg):
    """This project's Planning as tests/test_planning_cpu.planner_case leaves it for its eval call (deterministic weights, then
    ONE training forward, which moves the BatchNorm statistics of ``reduce_channel``), and the inputs of that call."""
    from stp3_amd.models.planning_model import Planning
    ins = H.planning_inputs(cfg)
    pl = Planning(cfg, 64, 6, gru_state_size=cfg.PLANNING.GRU_STATE_SIZE)
    for sub in (pl.reduce_channel, pl.GRU, pl.decoder):
        H.fill_deterministic(sub)
    pl.train()                                             # (no dropout or drop-connect in the planner: nothing to neutralise)
    pl(ins['cam_front'].clone(), ins['sample_trajs'].clone(), ins['gt_trajs'].clone(), ins['cost_volume'].clone(), ins['occupancy'],
       ins['hdmap_labels'], ins['commands'], ins['target'])
    return pl.eval(), ins


def logits_of(occupancy):
    """(B, T, 2, H, W) float32 logits whose argmax is the boolean ``occupancy`` (B, T, H, W)."""
    on = occupancy.float() * 2.0 - 1.0
    return torch.stack([torch.zeros_like(on), on], dim=2)


def scene_case(dtype=torch.float32, seed=5):
    """Continuous random logits for the scene kernel: three vehicle classes, two pedestrian classes, five frames of which the
    last three are used, and cells with hand-made ties.  Returns (segmentation, pedestrian, hdmap, n_present, the rows of the ties)."""
    g = torch.Generator().manual_seed(seed)
    B, S, H_, W_ = 2, 5, 40, 56
    seg = torch.randn(B, S, 3, H_, W_, generator=g)
    ped = torch.randn(B, S, 2, H_, W_, generator=g) - 0.5
    hd = torch.randn(B, 4, H_, W_, generator=g) * 2.0
    ped[:, :, 1, :4] = -9.0                                # no pedestrian in the rows of the ties
    seg[:, :, :, 0] = torch.tensor([5.0, 5.0, 1.0]).view(1, 1, 3, 1)      # classes 0 and 1 tie: class 0 -- free
    seg[:, :, :, 1] = torch.tensor([1.0, 5.0, 5.0]).view(1, 1, 3, 1)      # classes 1 and 2 tie: class 1 -- occupied
    seg[:, :, :, 2] = torch.tensor([5.0, 5.0, 5.0]).view(1, 1, 3, 1)      # all tie: class 0 -- free
    seg[:, :, :, 3] = torch.tensor([1.0, 0.5, 1.0]).view(1, 1, 3, 1)      # classes 0 and 2 tie: class 0 -- free
    hd[:, :, 0, :8] = 0.25                                 # equal logits: probability exactly 0.5 -- lane zeroed, drivable kept
    return seg.to(dtype), ped.to(dtype), hd.to(dtype), 2, {'free': (0, 2, 3), 'occupied': (1,)}


def selection_case(cfg, seed=3):
    """N = 1 800, T = 6, B = 4 candidates from ``synthetic.make_planning_inputs`` over the scene of ``inputs``."""
    from stp3_amd import synthetic
    ins = inputs(cfg)
    plan = synthetic.make_planning_inputs(BATCH, cfg.N_FUTURE_FRAMES, cfg.PLANNING.SAMPLE_NUM, seed=seed)
    ins['sample_trajectory'] = plan['sample_trajectory']
    ins['trajs'] = plan['sample_trajectory'][:, :, 1:]
    return ins


def command_range(command, n):
    k = {'LEFT': 0, 'FORWARD': 1, 'RIGHT': 2}.get(command)
    return (0, n) if k is None else (k * (n // 3), (k + 1) * (n // 3))
