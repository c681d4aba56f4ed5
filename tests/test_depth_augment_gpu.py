"""GPU: csrc/stp3_depth_augment.hip on the MI355X -- every case of tests/golden/depth_augment.npz through
stp3_amd.datas.DepthLabeller with ``params`` on device tensors, exactly (checks and their reasons:
tests/test_depth_augment_cpu.py) and bit for bit against the torch statements run on the same device tensors; the
parameters of ``sample(train=False)`` against the plain entries; a call captured into a graph with a plan and replayed after
the plan was rewritten in place for a second parameter set and another cloud (there is no host synchronisation inside)."""
import pytest
import torch

from tests import depth_augment_cases as DA
from tests.test_depth_augment_cpu import (call, check_depths, check_eval_parameters_equal_the_plain_call, check_labels, inputs,
                                          torch_statements)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', DA.SMALL)
def test_kernels_match_the_reference(name):
    lab, params = DA.labeller(name), DA.params(name)
    cloud, maps = inputs(name, 'cuda')
    d64 = call(lab, cloud, maps, params=params, out_dtype=torch.float64)
    d32 = call(lab, cloud, maps, params=params)
    labels = call(lab, cloud, maps, params=params, labels=True)
    assert d64.is_cuda and d64.dtype == torch.float64 and d32.dtype == torch.float32 and labels.dtype == torch.int64
    check_depths(name, d64.cpu().numpy(), 'kernels')
    check_depths(name, d32.cpu().numpy(), 'kernels')
    check_labels(name, labels.cpu().numpy(), 'kernels')
    # the torch statements on the same tensors, and on the CPU: bit for bit, no list of exclusions
    assert torch.equal(d64, call(lab, cloud, maps, reference=True, params=params, out_dtype=torch.float64))
    assert torch.equal(d64.cpu(), torch_statements(name, 'plain'))
    assert torch.equal(labels, lab.class_ids(d32))
    assert torch.equal(labels, call(lab, cloud, maps, reference=True, params=params, labels=True))
    # without rotation the labels come from the tables of the label rows and columns alone
    still = [dict(p, rotate=0.0) for p in params]
    assert torch.equal(call(lab, cloud, maps, params=still, labels=True).cpu(), lab.class_ids(torch_statements(name, 'norot').float()))
    # a second run, bit for bit
    assert torch.equal(call(lab, cloud, maps, params=params, out_dtype=torch.float64), d64)


def test_kernels_match_the_reference_at_the_real_geometry():
    """6 x 900 x 1600 -> 224 x 480 -> 28 x 60, 35 000 points, parameters inside the limits of the Lift-Splat draw."""
    lab, params = DA.labeller('real'), DA.params('real')
    cloud, _ = inputs('real', 'cuda')
    d32 = lab.from_lidar(*cloud, params=params)
    check_depths('real', d32.cpu().numpy(), 'kernels, real geometry')
    labels = lab.from_lidar(*cloud, params=params, labels=True)
    check_labels('real', labels.cpu().numpy(), 'kernels, real geometry')
    assert torch.equal(labels, lab.class_ids(d32))


def test_eval_parameters_equal_the_plain_entries():
    check_eval_parameters_equal_the_plain_call('cuda')


@pytest.mark.parametrize('name', DA.SMALL)
def test_captured_and_replayed_with_new_parameters(name):
    """Captured on one stream (it could not be if anything inside waited for the device or allocated); replayed after the
    plan's tables and the inputs in their static buffers were rewritten."""
    lab, params, second = DA.labeller(name), DA.params(name), DA.replay_params(name)
    cloud, maps = inputs(name, 'cuda')
    cloud2, maps2 = inputs(name, 'cuda', 1)
    static = maps.clone() if cloud is None else tuple(t.clone() if torch.is_tensor(t) else t for t in cloud)
    if cloud is None:
        plan = lab.augment_plan(params, 'cuda', maps=maps.dtype)
    else:
        plan = lab.augment_plan(params, 'cuda', points=cloud[0].shape[0] * cloud[2].shape[1])   # (point, camera) pairs

    def run():
        return lab.from_maps(static, plan=plan) if cloud is None else lab.from_lidar(*static, plan=plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch_statements(name, 'plain').float())
    if cloud is None:
        static.copy_(maps2)
    else:
        assert cloud2[0].shape == cloud[0].shape
        for dst, src in zip(static, cloud2):
            if torch.is_tensor(dst):
                dst.copy_(src)
    assert lab.augment_plan(second, 'cuda', like=plan) is plan
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch_statements(name, 'replay').float())
    assert not torch.equal(torch_statements(name, 'plain'), torch_statements(name, 'replay'))
