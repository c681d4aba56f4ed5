"""GPU: the training video painted by csrc/stp3_vis.hip (stp3_amd.visualisation.visualise_output on GPU tensors) against the
reference's videos of tests/golden/visualisation.npz and against the CPU route, under the comparison rule of
tests/visualisation_cases.py (every byte equal; the flow-type bytes that an angle +-2 ulp away would change may differ by 1; the
planning row against the integer statement ``planning_expected``)."""
import numpy as np
import pytest
import torch

from tests import visualisation_cases as VC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(n, s, d) for n, c in VC.CASES.items() for s in c['samples'] for d in (torch.float32, torch.bfloat16)]


@pytest.mark.parametrize('name,sample,dtype', CASES, ids=[f'{n}-{s}-{str(d).split(".")[1]}' for n, s, d in CASES])
def test_kernels_match_the_reference(name, sample, dtype):
    """Every fixture case with the DEFAULT instance post-processing (the GPU kernels of stp3_amd.instance)."""
    from stp3_amd import visualisation as V
    labels, output, _ = VC.stored(name, device=DEV, head_dtype=dtype)
    before = {k: v.clone() for k, v in {**labels, **output}.items()}
    video = V.visualise_output(labels, output, VC.cfg_of(name), sample=sample)
    assert video.dtype == torch.uint8 and video.device == torch.device(DEV) and video.is_contiguous()
    host = VC.stored(name)
    share = VC.compare(name, video.cpu().numpy(), sample, host[0], host[1], f'kernels ({dtype})')
    print(f'{name} sample {sample} {dtype}: at most {share:.3%} of a flow panel fragile')
    assert all(torch.equal(v, before[k]) for k, v in {**labels, **output}.items()), 'an input was written to'


@pytest.fixture(scope='module')
def large():
    """200 x 200 cells, T = 3, B = 2: (labels, output, ids, cfg) on the GPU and the CPU route's videos of both samples."""
    from stp3_amd import visualisation as V
    labels, output, ids, cfg = VC.random_case(2, 3, 200, 200, seed=21)
    want = [V.visualise_output_reference(labels, output, cfg, sample=s, consistent_instance_seg=ids).numpy() for s in range(2)]
    to = lambda d: {k: v.to(DEV) for k, v in d.items()}
    return (labels, output), (to(labels), to(output), ids.to(DEV)), cfg, want


def test_large_maps_match_the_cpu_route(large):
    from stp3_amd import visualisation as V
    (labels, output), (dl, do, dids), cfg, want = large
    video = V.visualise_output(dl, do, cfg, sample=1, consistent_instance_seg=dids)
    assert tuple(video.shape) == (1, 3, 3, 1400, 400)
    share = VC.compare_videos(video.cpu().numpy(), want[1], VC.flow_sources(labels, output, 1), VC.planning_panels(labels, output, 1, cfg),
                              'kernels, 200 x 200')
    print(f'200 x 200: at most {share:.3%} of a flow panel fragile')
    # strided sources (channels-last head outputs, a sliced label map) are read in place
    do2 = {k: (v.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) if v.ndim == 5 else v) for k, v in do.items()}
    wide = torch.zeros(2, 3, 1, 200, 216, dtype=torch.int64, device=DEV)
    wide[..., 8:208] = dl['segmentation']
    dl2 = {**dl, 'segmentation': wide[..., 8:208]}
    assert not do2['instance_offset'].is_contiguous() and not dl2['segmentation'].is_contiguous()
    assert torch.equal(V.visualise_output(dl2, do2, cfg, sample=1, consistent_instance_seg=dids), video)


def test_out_is_painted_in_place_and_reused(large):
    from stp3_amd import visualisation as V
    _, (dl, do, dids), cfg, _ = large
    fresh = [V.visualise_output(dl, do, cfg, sample=s, consistent_instance_seg=dids) for s in range(2)]
    assert not torch.equal(fresh[0], fresh[1])
    out = torch.full((1, 3, 3, 1400, 400), 7, dtype=torch.uint8, device=DEV)
    for s in (0, 1, 0):
        assert V.visualise_output(dl, do, cfg, sample=s, consistent_instance_seg=dids, out=out) is out
        assert torch.equal(out, fresh[s])
    with pytest.raises(ValueError):
        V.visualise_output(dl, do, cfg, consistent_instance_seg=dids, out=out[:, :2])
    with pytest.raises(ValueError):
        V.visualise_output(dl, do, cfg, consistent_instance_seg=dids, out=out.cpu())
    # a video that does not start on a word boundary takes the byte stores: same bytes, nothing outside them
    n = out.numel()
    buf = torch.full((n + 65,), 0xA5, dtype=torch.uint8, device=DEV)
    V.visualise_output(dl, do, cfg, sample=1, consistent_instance_seg=dids, out=buf[1:1 + n].view(out.shape))
    assert torch.equal(buf[1:1 + n].view(out.shape), fresh[1]) and int(buf[0]) == 0xA5 and bool((buf[1 + n:] == 0xA5).all())


def test_render_is_capturable_and_replays_on_changed_inputs():
    """One single-stream capture of the render (after an eager call, which uploads the colour tables); the inputs are then
    overwritten in place and the replay must equal an eager call on them."""
    from stp3_amd import visualisation as V
    cfg = VC.cfg_of('full')
    labels, output, consistent = VC.stored('full', device=DEV)
    take = lambda d, b: {k: v[b:b + 1].clone() for k, v in d.items()}
    static_l, static_o, static_ids = take(labels, 0), take(output, 0), consistent[:1].clone()
    out = torch.zeros(1, 3, 3, 168, 44, dtype=torch.uint8, device=DEV)
    V.visualise_output(static_l, static_o, cfg, consistent_instance_seg=static_ids, out=out)
    first = out.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        V.visualise_output(static_l, static_o, cfg, consistent_instance_seg=static_ids, out=out)
    out.zero_()
    graph.replay()
    assert torch.equal(out, first)
    for static, source in ((static_l, labels), (static_o, output)):
        for k, v in static.items():
            v.copy_(source[k][1:2])
    static_ids.copy_(consistent[1:2])
    graph.replay()
    eager = V.visualise_output(static_l, static_o, cfg, consistent_instance_seg=static_ids)
    assert torch.equal(out, eager) and not torch.equal(out, first)
    host = VC.stored('full')
    VC.compare('full', out.cpu().numpy(), 1, host[0], host[1], 'replayed graph')


def test_render_does_not_synchronise_with_the_host(monkeypatch):
    """With the instance ids given, nothing inside visualise_output waits for the device or pulls a tensor to the host."""
    from stp3_amd import visualisation as V
    cfg = VC.cfg_of('full')
    labels, output, consistent = VC.stored('full', device=DEV)
    want = V.visualise_output(labels, output, cfg, consistent_instance_seg=consistent).cpu()       # (uploads the tables, once)
    counts = {}

    def counting(owner, attr):
        inner = getattr(owner, attr)

        def wrapped(*args, **kwargs):
            counts[attr] = counts.get(attr, 0) + 1
            return inner(*args, **kwargs)
        monkeypatch.setattr(owner, attr, wrapped)
    counting(torch.cuda, 'synchronize')
    for attr in ('cpu', 'item', 'tolist', 'numpy'):
        counting(torch.Tensor, attr)
    video = V.visualise_output(labels, output, cfg, sample=0, consistent_instance_seg=consistent)
    seen = dict(counts)
    monkeypatch.undo()
    assert seen == {}, seen
    assert torch.equal(video.cpu(), want)
