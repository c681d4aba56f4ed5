"""GPU: csrc/stp3_eval.hip on the MI355X through stp3_amd.evaluation -- the semantic, planning and panoptic checks of
tests/test_eval_cpu.py (where the references and bounds are explained) on device tensors, a second call bit for bit, a whole
``EvalScorer.update`` captured into a graph and replayed onto other inputs (it could not be if anything inside waited for the
device), and ``evaluate()`` on a Prediction.yml-shaped model with and without an ``InferenceEngine``."""
import numpy as np
import pytest
import torch

from tests import eval_cases as EC
from tests import helpers as H
from tests.test_eval_cpu import bits, built, by_hand, check_panoptic, check_planning, check_semantic, fixture
from tests.test_prediction_cpu import PREDICTION

pytestmark = pytest.mark.gpu


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f'a second call differs: {k}'


def test_semantic_kernel():
    out = EC.run_semantic('cuda')
    check_semantic(out)
    same(out, EC.run_semantic('cuda'))


def test_planning_kernel():
    out = EC.run_planning('cuda')
    check_planning(out)
    same(out, EC.run_planning('cuda'))


def test_panoptic_kernel():
    out = EC.run_panoptic('cuda', fixture=fixture(), build=built)
    check_panoptic(out)
    same(out, EC.run_panoptic('cuda', fixture=fixture(), build=built))


def full_inputs(k):
    """Update k (0 / 1) of a scorer with every metric on: B 2, S 7, receptive field 3, 200 x 200."""
    updates, labels = EC.planning_inputs('cuda')
    rs = np.random.RandomState(500 + k)
    output = {'segmentation': torch.from_numpy(EC._logits(rs, (2, 7, 2, 200, 200))).cuda(),
              'pedestrian': torch.from_numpy(EC._logits(rs, (2, 7, 2, 200, 200))).cuda().to(torch.bfloat16),
              'hdmap': torch.from_numpy(EC._logits(rs, (2, 4, 200, 200))).cuda()}
    labels['hdmap'] = torch.from_numpy(EC._labels(rs, (2, 2, 200, 200), 2)).cuda()
    labels['instance'] = torch.from_numpy(built('clean')['gt_instance'][2 * k:2 * k + 2]).cuda()
    trajs, labels['gt_trajectory'] = updates[k]
    instance = torch.from_numpy(fixture()['clean/tracked'][2 * k:2 * k + 2].astype(np.int64)).cuda()
    return output, labels, trajs.contiguous(), instance


def test_captured_update_replays_on_other_inputs():
    from stp3_amd.config import perception_cfg
    from stp3_amd.evaluation import EvalScorer
    from tests.test_planning_cpu import PLANNING
    cfg = perception_cfg(**{**PLANNING, 'INSTANCE_SEG.ENABLED': True})
    assert cfg.TIME_RECEPTIVE_FIELD == 3 and cfg.N_FUTURE_FRAMES == 4
    first, second = full_inputs(0), full_inputs(1)
    eager = EvalScorer(cfg, 'cuda')
    eager.update(*first)
    eager.update(*second)
    want = eager.states()
    assert want['semantic'][:, 1].min() > 0 and want['obj_box_col'].sum() > 0 and want['panoptic'][1, 1] > 0 and want['total'] == 4

    clone = lambda x: {k: v.clone() for k, v in x.items()} if isinstance(x, dict) else x.clone()
    buf = tuple(clone(x) for x in first)
    scorer = EvalScorer(cfg, 'cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scorer.update(*buf)                       # warm-up outside the capture
        scorer.reset()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scorer.update(*buf)
    graph.replay()
    for dst, src in zip(buf, second):
        if isinstance(dst, dict):
            for k in dst:
                dst[k].copy_(src[k])
        else:
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = scorer.states()
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


class Recorder:
    """Calls the forward and keeps copies of what it returned: the heads evaluate() scored."""

    def __init__(self, forward):
        self.forward, self.outputs = forward, []

    def __call__(self, *inputs):
        out = self.forward(*inputs)
        self.outputs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()})
        return out


@pytest.fixture(scope='module')
def prediction_module():
    from stp3_amd import synthetic
    from stp3_amd.config import perception_cfg
    from stp3_amd.trainer import TrainingModule
    from stp3_amd.utils import to_channels_last
    tm = to_channels_last(TrainingModule(perception_cfg(**PREDICTION).convert_to_dict()).cuda())
    tm.eval()
    loader = [synthetic.make_batch(batch=1, seq=7, seed=3 + k, instance=True) for k in range(2)]
    return tm, loader


@pytest.mark.parametrize('with_engine', [False, True])
def test_evaluate_prediction_config(prediction_module, with_engine):
    from stp3_amd.evaluation import _to_device, evaluate
    from stp3_amd.inference import InferenceEngine
    tm, loader = prediction_module
    rf = tm.model.receptive_field
    if with_engine:
        rec = Recorder(InferenceEngine(tm.model, loader[0], autocast_dtype=torch.bfloat16))
        got = evaluate(tm, loader, engine=rec)
    else:
        rec = Recorder(tm.model.forward)
        tm.model.forward = rec
        try:
            got = evaluate(tm, loader)
        finally:
            del tm.model.forward
    assert len(rec.outputs) == 2
    assert set(got) == {'vehicle_iou', 'vehicle_pq', 'vehicle_sq', 'vehicle_rq'}
    assert all(np.isfinite(float(v)) for v in got.values())
    with torch.no_grad():
        labels = [tm.prepare_future_labels(_to_device(b, 'cuda')) for b in loader]
        want = by_hand(tm.cfg, rec.outputs, labels, rf)
    for k in want:
        assert np.array_equal(bits(got[k].numpy()), bits(want[k].numpy())), (k, float(got[k]), float(want[k]))


def test_evaluate_planning_config():
    """Planning.yml shape (pedestrian and hd-map heads, the planner), two batches of one sample: the IoUs and, per horizon, the
    planning scores of evaluate() against the metric classes driven over the same heads and the same planned trajectories
    (``plan_scene`` + ``Planning.drive`` are bit-reproducible)."""
    from stp3_amd import ops_plan, synthetic
    from stp3_amd.evaluation import _to_device, evaluate
    from stp3_amd.metrics import PlanningMetric
    from stp3_amd.trainer import TrainingModule
    from stp3_amd.utils import to_channels_last
    c = EC.planning_cfg()
    tm = to_channels_last(TrainingModule(c.convert_to_dict()).cuda())
    tm.eval()
    loader = [synthetic.make_batch(batch=1, seq=7, seed=3 + k, planning=(c.N_FUTURE_FRAMES, c.PLANNING.SAMPLE_NUM)) for k in range(2)]
    rec = Recorder(tm.model.forward)
    tm.model.forward = rec
    try:
        got = evaluate(tm, loader)
    finally:
        del tm.model.forward
    rf, T = tm.model.receptive_field, c.N_FUTURE_FRAMES
    plan_keys = {f'plan_{k}_{i + 1}s' for k in ('obj_col', 'obj_box_col', 'L2') for i in range(T // 2)}
    assert set(got) == {'vehicle_iou', 'pedestrian_iou', 'lane_divider_iou', 'drivable_area_iou'} | plan_keys
    assert all(np.isfinite(float(v)) for v in got.values())
    metrics = [PlanningMetric(c, 2 * (i + 1)).cuda() for i in range(T // 2)]
    labels = []
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        for batch, o in zip(loader, rec.outputs):
            batch = _to_device(batch, 'cuda')
            l = tm.prepare_future_labels(batch)
            labels.append(l)
            occupancy, lane, drivable = ops_plan.plan_scene(o['segmentation'], o['pedestrian'], o['hdmap'], rf)
            final_traj, _, _ = tm.model.planning.drive(o['cam_front'], batch['sample_trajectory'][:, :, 1:].float(), o['costvolume'][:, rf:],
                                                       occupancy, lane, drivable, ops_plan.command_codes(batch['command'], 'cuda'),
                                                       batch['target_point'])
            truth = l['segmentation'][:, rf:].squeeze(2).bool() | l['pedestrian'][:, rf:].squeeze(2).bool()
            for i, m in enumerate(metrics):
                t = 2 * (i + 1)
                m(final_traj[:, :t], l['gt_trajectory'][:, 1:t + 1], truth[:, :t])
        want = by_hand(c, rec.outputs, labels, rf)
    for k in want:
        assert np.array_equal(bits(got[k].numpy()), bits(want[k].numpy())), (k, float(got[k]), float(want[k]))
    for i, m in enumerate(metrics):
        for key, value in m.compute().items():
            name = f'plan_{key}_{i + 1}s'
            np.testing.assert_allclose(got[name].numpy(), value.mean().cpu().numpy(), rtol=1e-6, err_msg=name)
    assert float(got['plan_L2_1s']) > 0
