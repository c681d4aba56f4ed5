"""TEST INFRASTRUCTURE -- the deterministic inputs of the evaluation-scorer tests (stp3_amd.evaluation; csrc/stp3_eval.hip)
and the runs that tests/test_eval_cpu.py (CPU route), tests/hipcpu/run_eval.py (the kernel source on the host) and
tests/test_eval_gpu.py (the MI355X) share: ``run_semantic`` / ``run_planning`` / ``run_panoptic`` drive an ``EvalScorer`` on
``device`` and return what it holds as numpy arrays; the checks are in tests/test_eval_cpu.py."""
import numpy as np
import torch

from tests import helpers as H
from tests import instance_cases as IC

# name: (H, W, segmentation classes, dtype, channels-last).  37 x 53 is no multiple of a wave or a tile; 200 x 200 needs 20
# workgroups per plane.  Three segmentation classes with n_classes = 2: predictions outside [0, n)
SEMANTIC = {
    's_f32': (37, 53, 2, torch.float32, False), 's_f32_cl': (37, 53, 2, torch.float32, True),
    's_bf16': (37, 53, 2, torch.bfloat16, False), 's_bf16_cl': (37, 53, 2, torch.bfloat16, True),
    's_c3_cl': (37, 53, 3, torch.float32, True), 's_c3_bf16': (37, 53, 3, torch.bfloat16, False),
    'b_f32': (200, 200, 2, torch.float32, False), 'b_bf16_cl': (200, 200, 2, torch.bfloat16, True),
    'b_c3': (200, 200, 3, torch.float32, False),
}
SEM_B, SEM_S, SEM_RF = 2, 3, 2                    # first scored frame: receptive field - 1 = 1


def semantic_cfg():
    from stp3_amd.config import perception_cfg
    return perception_cfg(**{'TIME_RECEPTIVE_FIELD': SEM_RF, 'N_FUTURE_FRAMES': SEM_S - SEM_RF, 'SEMANTIC_SEG.PEDESTRIAN.ENABLED': True,
                             'SEMANTIC_SEG.HDMAP.ENABLED': True, 'INSTANCE_SEG.ENABLED': False, 'INSTANCE_FLOW.ENABLED': False,
                             'PLANNING.ENABLED': False})


def _logits(rs, shape):
    """Random logits, a quarter of them quantised (exact ties between classes), with planted NaNs and infinities at fixed pixels of
    every plane: class axis = -3."""
    x = rs.standard_normal(shape).astype(np.float32)
    q = rs.uniform(size=shape[:-3] + (1,) + shape[-2:]) < 0.25
    x = np.where(q, np.rint(x * 2.0) / 2.0, x).astype(np.float32)
    x[..., :, 0, 0:3] = 0.75                      # all classes equal: class 0 wins
    x[..., 0, 1, 0], x[..., 1, 1, 1], x[..., :, 1, 2] = np.nan, np.nan, np.nan      # NaN in class 0, in class 1, in all
    x[..., 0, 2, 0], x[..., 1, 2, 1], x[..., :, 2, 2] = np.inf, np.inf, np.inf
    x[..., 0, 3, 0], x[..., 1, 3, 1], x[..., :, 3, 2] = -np.inf, -np.inf, -np.inf
    x[..., 0, 4, 0], x[..., 1, 4, 0] = np.nan, np.inf                               # a NaN beats +inf
    x[..., 0, 4, 1], x[..., 1, 4, 1] = np.inf, np.nan
    return x


def _labels(rs, shape, n):
    y = rs.randint(0, n, size=shape).astype(np.int64)
    y[rs.uniform(size=shape) < 0.03] = 255        # the ignore value: no class of its own
    y[..., 0:5, 0:3] = rs.randint(0, n, size=shape[:-2] + (5, 3))
    y[..., 5, 0:2] = 255
    return y


def _layout(x, dtype, channels_last, device):
    t = torch.from_numpy(x).to(dtype)
    if channels_last:                             # the class axis (-3) innermost in memory, the same logical shape
        t = t.movedim(-3, -1).contiguous().movedim(-1, -3)
        assert not t.is_contiguous()
    return t.to(device)


def semantic_inputs(name, update, device='cpu'):
    """(output, labels) of update 0 or 1 of a SEMANTIC case."""
    h, w, cs, dtype, cl = SEMANTIC[name]
    rs = np.random.RandomState(1000 + 10 * sorted(SEMANTIC).index(name) + update)
    out = {'segmentation': _layout(_logits(rs, (SEM_B, SEM_S, cs, h, w)), dtype, cl, device),
           'pedestrian': _layout(_logits(rs, (SEM_B, SEM_S, 2, h, w)), dtype, cl, device),
           'hdmap': _layout(_logits(rs, (SEM_B, 2, 2, h, w)).reshape(SEM_B, 4, h, w), dtype, cl, device)}
    labels = {'segmentation': torch.from_numpy(_labels(rs, (SEM_B, SEM_S, 1, h, w), 2)).to(device),
              'pedestrian': torch.from_numpy(_labels(rs, (SEM_B, SEM_S, 1, h, w), 2)).to(device),
              'hdmap': torch.from_numpy(_labels(rs, (SEM_B, 2, h, w), 2)).to(device)}
    return out, labels


def semantic_expected(output, labels):
    """int64 (4, 2, 4): the states of four IntersectionOverUnion objects fed with torch.argmax, as evaluate.py:95-112 does."""
    from stp3_amd.metrics import IntersectionOverUnion
    rf = SEM_RF
    ms = [IntersectionOverUnion(2) for _ in range(4)]
    ms[0](torch.argmax(output['segmentation'].float(), dim=2, keepdim=True)[:, rf - 1:], labels['segmentation'][:, rf - 1:])
    ms[1](torch.argmax(output['pedestrian'].float(), dim=2, keepdim=True)[:, rf - 1:], labels['pedestrian'][:, rf - 1:])
    for i in range(2):
        ms[2 + i](torch.argmax(output['hdmap'][:, 2 * i:2 * i + 2].float(), dim=1, keepdim=True), labels['hdmap'][:, i:i + 1])
    return np.stack([np.stack([getattr(m, k).numpy() for k in ('true_positive', 'false_positive', 'false_negative', 'support')], axis=1)
                     for m in ms]).astype(np.int64)


def run_semantic(device, names=tuple(SEMANTIC)):
    from stp3_amd.evaluation import EvalScorer
    out = {}
    for name in names:
        scorer = EvalScorer(semantic_cfg(), device)
        scorer.update(*semantic_inputs(name, 0, device))
        out[f'sem/{name}/one'] = scorer.states()['semantic']
        scorer.update(*semantic_inputs(name, 1, device))
        out[f'sem/{name}/two'] = scorer.states()['semantic']
        scorer.reset()
        out[f'sem/{name}/reset'] = scorer.states()['semantic']
    return out


# ---- planning: the inputs of test_planning_cpu.test_planning_metric_matches_the_reference, the occupancy as label maps ----
def planning_cfg():
    from tests.test_planning_cpu import cfg
    return cfg()


def planning_inputs(device='cpu'):
    """([(trajs, gt_trajectory), (trajs, gt_trajectory)], labels): the two updates of the fixture.  The occupancy of
    helpers.planning_inputs is split between the segmentation and the pedestrian label (their OR is the occupancy; 255 is as
    occupied as 1); the frames before the first future frame are all ones -- a wrong frame index collides everywhere."""
    c = planning_cfg()
    rf, T = int(c.TIME_RECEPTIVE_FIELD), int(c.N_FUTURE_FRAMES)
    ins = H.planning_inputs(c)
    occ = ins['occupancy']
    B = occ.shape[0]
    rows = torch.arange(200).view(1, 1, 200, 1)
    to_seg = (rows % 3 != 0).expand_as(occ)
    seg = torch.ones(B, rf + T, 1, 200, 200, dtype=torch.int64)
    ped = torch.ones(B, rf + T, 1, 200, 200, dtype=torch.int64)
    seg[:, rf:, 0] = (occ & to_seg).long() * torch.where(rows % 2 == 0, 255, 1)
    ped[:, rf:, 0] = (occ & ~to_seg).long()
    assert torch.equal(seg[:, rf:, 0].bool() | ped[:, rf:, 0].bool(), occ) and (occ & to_seg).any() and (occ & ~to_seg).any()

    def with_origin(t):                           # labels['gt_trajectory'] holds the origin in front
        return torch.cat([torch.zeros_like(t[:, :1]), t], dim=1).to(device)
    plan2, expert2 = H.planning_metric_trajs(c)
    updates = [(ins['sample_trajs'][:, 7].clone().to(device), with_origin(ins['gt_trajs'].clone())),
               (plan2.to(device), with_origin(expert2))]
    return updates, {'segmentation': seg.to(device), 'pedestrian': ped.to(device)}


def run_planning(device):
    from stp3_amd.evaluation import EvalScorer
    scorer = EvalScorer(planning_cfg(), device)
    updates, labels = planning_inputs(device)
    for trajs, gt in updates:
        scorer._update_planning(trajs, {**labels, 'gt_trajectory': gt})
    s = scorer.states()
    out = {f'plan/{k}': np.asarray(s[k]) for k in ('obj_col', 'obj_box_col', 'L2', 'total')}
    for k, v in scorer.compute().items():
        if k.startswith('plan_'):
            out[f'plan/compute/{k}'] = v.numpy()
    return out


# ---- panoptic: tests/golden/instance.npz ----
def panoptic_cfg():
    from stp3_amd.config import perception_cfg
    return perception_cfg(**{'TIME_RECEPTIVE_FIELD': 1, 'INSTANCE_SEG.ENABLED': True, 'SEMANTIC_SEG.PEDESTRIAN.ENABLED': False,
                             'SEMANTIC_SEG.HDMAP.ENABLED': False, 'PLANNING.ENABLED': False})


def panoptic_error_inputs():
    """[(pred, gt, the error words expected)]: each breaks one clause of stp3_eval_panoptic's contract."""
    base_gt = np.zeros((1, 2, 40, 40), np.int64)
    base_gt[:, :, 5:9, 5:9] = 1
    pred = base_gt.copy()
    big = pred.copy()
    big[0, 1, 6, 6] = 1 << 20
    negative = base_gt.copy()
    negative[0, 0, 20, 20] = -1
    full = np.full_like(base_gt, 3)
    many = np.zeros_like(base_gt)
    many[0, 1].reshape(-1)[100:1400] = np.arange(1, 1301)             # 1300 distinct ids against background
    return [(big, base_gt, [1, 0, 0, 0]), (pred, negative, [1, 0, 0, 0]), (pred, full, [0, 1, 0, 0]), (pred, many, [0, 0, 1, 0]),
            (many, base_gt, [0, 0, 1, 0]), (pred, base_gt, [0, 0, 0, 0])]


def run_panoptic(device, names=tuple(IC.CASES), fixture=None, errors=True, build=IC.build):
    """Per case: per-frame rows, the state after one update of a fresh scorer, compute(), the state on the renamed ids, the
    state without the consistency rule; 'clean' in two updates; the error words."""
    from stp3_amd.evaluation import EvalScorer
    g = fixture if fixture is not None else dict(H.load('instance.npz'))
    cfg = panoptic_cfg()
    out = {}

    def scored(pred, gt, **kw):
        scorer = EvalScorer(cfg, device, **kw)
        for p, t in zip(pred, gt):
            scorer._update_panoptic(torch.from_numpy(p).to(device), {'instance': torch.from_numpy(t).to(device)})
        return scorer
    for name in names:
        gt = build(name)['gt_instance']
        tracked = g[f'{name}/tracked']
        scorer = scored([tracked.astype(np.int64)], [gt])
        if scorer._workspace is not None:
            out[f'pan/{name}/frames'] = scorer.panoptic_frames()
        out[f'pan/{name}/err'] = scorer.err.cpu().numpy()
        out[f'pan/{name}/state'] = scorer.states()['panoptic']
        comp = scorer.compute()
        out[f'pan/{name}/compute'] = np.stack([comp[f'vehicle_{k}'].numpy() for k in ('pq', 'sq', 'rq')])
        out[f'pan/{name}/renamed'] = scored([g[f'{name}/renamed'].astype(np.int32)], [gt.astype(np.int32)]).states()['panoptic']
        out[f'pan/{name}/loose'] = scored([tracked.astype(np.int64)], [gt], temporally_consistent=False).states()['panoptic']
        if name == 'clean':
            t = tracked.astype(np.int64)
            out['pan/clean/split'] = scored([t[:2], t[2:]], [gt[:2], gt[2:]]).states()['panoptic']
    if errors:                                    # (the torch route raises instead: PanopticMetric.overlap_table)
        out['pan/errors'] = np.stack([scored([pred], [gt]).err.cpu().numpy() for pred, gt, _ in panoptic_error_inputs()])
    return out
