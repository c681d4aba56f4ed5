"""GPU: csrc/stp3_instance.hip on the MI355X -- every case of tests/golden/instance.npz through
stp3_amd.instance.predict_instance_segmentation_and_trajectories on device tensors (checks and their reasons:
tests/test_instance_cpu.py), repeated calls bit for bit, the call captured into a graph and replayed onto other inputs (there
is no host synchronisation inside), the kernels against the torch path on random heads, PanopticMetric on device tensors, and
the evaluation step of a Prediction.yml-shaped model."""
import sys

import numpy as np
import pytest
import torch

from tests import instance_cases as IC
from tests.test_instance_cpu import HIPCPU, built, check_case, fixture, heads, metric_state, run_case
from tests.test_prediction_cpu import PREDICTION

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(IC.CASES))
def test_kernels_match_the_reference(name):
    raw, centers, counts, tracked, mc = run_case(name, 'cuda', check=True)
    assert raw.is_cuda and tracked.is_cuda and raw.dtype == torch.int32
    check_case(name, raw.cpu().numpy(), centers.cpu().numpy(), counts.cpu().numpy(), tracked.cpu().numpy(), mc, 'kernels')
    again = run_case(name, 'cuda', check=True)
    assert all(torch.equal(a, b) for a, b in zip((raw, centers, counts, tracked), again[:4])), 'a second call differs'


def test_prediction_shape_is_in_the_fixture():
    assert tuple(fixture()['clean/raw'].shape) == (4, 7, 200, 200)


def test_captured_call_replays_on_other_inputs():
    """The whole call (compute_matched_centers=False) captured on one stream: it could not be if anything inside waited for
    the device.  Replayed on the clean case and then on the same case with its samples rotated."""
    from stp3_amd.instance import predict_instance_segmentation_and_trajectories
    want = torch.from_numpy(fixture()['clean/renamed'].astype(np.int64))
    first = heads(built('clean'), 'cuda')
    second = {k: v.roll(1, dims=0) for k, v in first.items()}
    buf = {k: v.clone() for k, v in first.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        predict_instance_segmentation_and_trajectories(buf)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = predict_instance_segmentation_and_trajectories(buf)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    for k in buf:
        buf[k].copy_(second[k])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want.roll(1, dims=0)) and not torch.equal(want, want.roll(1, dims=0))


def test_kernels_equal_the_torch_path_on_random_heads():
    sys.path.insert(0, HIPCPU)
    from run_instance import random_heads
    from stp3_amd import instance as I
    center, offset, fg = (torch.from_numpy(a) for a in random_heads(5))
    want = I.segment_frames_reference(center, offset, fg)
    got = I.segment_frames(center.cuda(), offset.cuda(), fg.cuda())
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    flow = torch.from_numpy((2.0 * np.random.RandomState(6).standard_normal((2, 3, 2, 24, 40))).astype(np.float32))
    tracked, err = I.track_frames(got[0].view(2, 3, 24, 40), flow.cuda(), check=True)
    assert tracked.dtype == torch.int32 and not err.any()
    assert torch.equal(tracked.cpu().long(), I.track_frames_reference(want[0].view(2, 3, 24, 40), flow))
    bad = got[0].view(2, 3, 24, 40).clone()
    bad[0, 1][bad[0, 1] == 1] = 101                                                           # breaks the tracker's contract
    with pytest.raises(I.InstanceError):
        I.track_frames(bad, flow.cuda(), check=True)


def test_panoptic_metric_on_device_equals_the_host():
    from stp3_amd.metrics import PanopticMetric
    g = fixture()
    for name in ('clean', 'crowded', 'deg_all_foreground'):
        pred, gt = torch.from_numpy(g[f'{name}/tracked'].astype(np.int64)), torch.from_numpy(built(name)['gt_instance'])
        host, dev = PanopticMetric(2), PanopticMetric(2).cuda()
        host(pred, gt)
        dev(pred.cuda(), gt.cuda())
        assert dev.iou.is_cuda and np.array_equal(metric_state(dev).view(np.uint32), metric_state(host).view(np.uint32)), name
        assert np.array_equal(metric_state(dev).view(np.uint32), g[f'{name}/metric_state'].view(np.uint32)), name


def test_prediction_config_evaluation_step_scores_instances():
    """nuscenes/Prediction.yml shape (7 output frames, 200 x 200), batch 2: the evaluation branch post-processes the heads
    of the (untrained) model on the device and the panoptic metric comes out finite."""
    from stp3_amd import synthetic
    from stp3_amd.config import perception_cfg
    from stp3_amd.trainer import TrainingModule
    from stp3_amd.utils import to_channels_last
    tm = to_channels_last(TrainingModule(perception_cfg(**PREDICTION).convert_to_dict()).cuda())
    tm.eval()
    batch = synthetic.make_batch(batch=2, seq=7, seed=3, instance=True)
    batch = {k: (v.cuda() if torch.is_tensor(v) and k not in ('intrinsics', 'extrinsics', 'future_egomotion') else v)
             for k, v in batch.items()}
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        output, labels, _ = tm.shared_step(batch, False)
    assert output['instance_center'].shape[:2] == (2, 7)
    state = metric_state(tm.metric_panoptic_val)
    assert state[1:].sum() > 0 and np.isfinite(state).all()             # (the labels hold vehicles: each is matched or missed)
    comp = tm.metric_panoptic_val.compute()
    assert all(tuple(comp[k].shape) == (2,) and torch.isfinite(comp[k]).all() for k in ('pq', 'sq', 'rq'))
