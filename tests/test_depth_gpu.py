"""GPU: csrc/stp3_depth.hip on the MI355X -- every case of tests/golden/depth_labels.npz through
stp3_amd.datas.DepthLabeller on device tensors, exactly (checks and their reasons: tests/test_depth_cpu.py), repeated calls
bit for bit, the kernel routes against the torch statements run on the GPU on a random cloud, and from_lidar captured into a
graph and replayed onto other points through the same buffers (there is no host synchronisation inside)."""
import numpy as np
import pytest
import torch

from tests import depth_cases as DC
from tests.test_depth_cpu import built, check_depths, check_labels, check_projection, cloud, labeller

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(DC.LIDAR_CASES))
def test_kernels_match_the_reference(name):
    lab = labeller(name)
    args = cloud(name, 'cuda')
    pixels, depth, keep = lab.project(*args, check=True)
    assert pixels.is_cuda and keep.dtype == torch.bool
    check_projection(name, pixels.cpu().numpy(), depth.cpu().numpy(), keep.cpu().numpy(), 'kernels')
    d64 = lab.from_pixels(pixels, depth, keep, args[1], out_dtype=torch.float64)
    d32 = lab.from_lidar(*args)
    assert d64.is_cuda and d64.dtype == torch.float64 and d32.dtype == torch.float32
    check_depths(name, d64.cpu().numpy(), 'kernels, from_pixels')
    check_depths(name, d32.cpu().numpy(), 'kernels, from_lidar')
    want = lab.class_ids(d32)
    fused = lab.from_lidar(*args, labels=True, fused=True)
    lab.label_bands = 3
    banded = lab.from_lidar(*args, labels=True, fused=True)
    table = lab.from_lidar(*args, labels=True)
    check_labels(name, fused.cpu().numpy(), 'kernels, labels only')
    assert torch.equal(fused, want) and torch.equal(banded, want) and torch.equal(table, want)
    assert torch.equal(lab.from_pixels(pixels, depth, keep, args[1], labels=True), want)
    # a second run, bit for bit
    assert torch.equal(lab.from_lidar(*args), d32) and torch.equal(lab.from_lidar(*args, labels=True), want)
    assert torch.equal(lab.from_pixels(pixels, depth, keep, args[1], out_dtype=torch.float64), d64)


@pytest.mark.parametrize('name', list(DC.MAP_CASES))
def test_kernels_match_the_reference_on_stored_maps(name):
    lab = labeller(name)
    maps = torch.from_numpy(built(name)['maps']).cuda()
    got = lab.from_maps(maps, out_dtype=torch.float64)
    check_depths(name, got.cpu().numpy(), 'kernels, from_maps')
    check_labels(name, lab.from_maps(maps, labels=True).cpu().numpy(), 'kernels, from_maps')
    assert torch.equal(got, lab.reference_from_maps(maps, out_dtype=torch.float64))           # the torch statements on the GPU
    assert torch.equal(got, lab.from_maps(maps, out_dtype=torch.float64))


def random_cloud(seed, n=5000, device='cuda'):
    """3 frames (the middle one empty) x 4 cameras -- the two frames' rigs of the 'small' case side by side -- and points
    all round the sensor (most of them outside any one camera, many behind it), unfiltered: coordinates may fall anywhere,
    which is fair where both sides evaluate the same statements."""
    rs = np.random.RandomState(seed)
    case = built('small')
    steps = np.concatenate([case['steps'], case['steps'][::-1]], axis=1)[[0, 1, 0]]                     # (3, 4, 4, 12)
    k = np.concatenate([case['intrinsics'], case['intrinsics'][::-1]], axis=1)[[0, 1, 0]]
    points = (rs.standard_normal((n, 3)) * [12.0, 12.0, 2.0]).astype(np.float32)
    offsets = np.array([0, n // 2, n // 2, n], np.int32)
    return (torch.from_numpy(points).to(device), torch.from_numpy(offsets).to(device), torch.from_numpy(steps.copy()).to(device),
            DC.BEFORE, torch.from_numpy(k.copy()).to(device))


def test_kernel_routes_equal_the_torch_path_on_a_random_cloud():
    lab = labeller('small')
    args = random_cloud(7)
    want_p = lab.reference_project(*args)
    got_p = lab.project(*args)
    assert all(torch.equal(g, w) for g, w in zip(got_p, want_p)) and int(want_p[2].sum()) > 200
    want = lab.reference_from_lidar(*args, out_dtype=torch.float64)
    assert int((want > 0).sum()) > 100
    assert torch.equal(lab.from_lidar(*args, out_dtype=torch.float64), want)
    assert torch.equal(lab.from_pixels(*got_p, args[1], out_dtype=torch.float64), want)
    assert torch.equal(lab.from_lidar(*args, labels=True), lab.class_ids(want.float()))
    assert torch.equal(lab.from_lidar(*args, labels=True, fused=True), lab.class_ids(want.float()))


def test_captured_call_replays_on_other_points():
    """from_lidar, full map and labels (both routes), captured on one stream: it could not be if anything inside waited for the device.
    Replayed on the 'small' cloud and then on the same cloud with its two frames' cameras exchanged and the frame boundary moved."""
    lab = labeller('small')
    first = cloud('small', 'cuda')
    points, offsets, steps, before, k = first
    second = (points.flip(0).contiguous(), torch.tensor([0, 300, 1037], dtype=torch.int32, device='cuda'), steps.flip(1).contiguous(),
              before, k.flip(1).contiguous())
    want = [(lab.reference_from_lidar(*a), lab.reference_from_lidar(*a, labels=True)) for a in (first, second)]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][1], want[1][1])
    buf = tuple(t.clone() if torch.is_tensor(t) else t for t in first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lab.from_lidar(*buf), lab.from_lidar(*buf, labels=True), lab.from_lidar(*buf, labels=True, fused=True)   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        full, labels, fused = lab.from_lidar(*buf), lab.from_lidar(*buf, labels=True), lab.from_lidar(*buf, labels=True, fused=True)
    for i, (inputs, (want_full, want_labels)) in enumerate(zip((first, second), want)):
        for dst, src in zip(buf, inputs):
            if torch.is_tensor(dst):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(labels, want_labels) and torch.equal(fused, want_labels), f'replay {i}: labels'
        assert torch.equal(full, want_full), f'replay {i}: full map, {int((full != want_full).sum())} outputs differ'
    assert torch.equal(lab.from_lidar(*buf), want[1][0])                                        # and the same call outside the graph
