"""CPU: vehicle instance post-processing (stp3_amd.instance; csrc/stp3_instance.hip) and PanopticMetric
(stp3_amd.metrics) against the reference's own stp3/utils/instance.py:80-330 and stp3/metrics.py:74-261, recorded by
scripts/make_golden_instance.py in tests/golden/instance.npz on the cases of tests/instance_cases.py (the head outputs are
rebuilt here; their sha256 is checked before anything else).

How results are compared.  Maps before tracking, centres, counts and frame 0 after tracking: exactly the reference's.  Frames
t >= 1 after tracking: the reference hands fresh ids out in the iteration order of a Python set, this project in ascending
order of the old id (stp3_amd/instance.py), so the result must equal the reference's after ONE renaming per sample -- a
bijection on the non-zero ids, the same for all frames, the identity on every id of frame 0, that only exchanges ids created
at the same step -- which ``check_tracked`` derives from the two maps and checks; the number of fresh ids per step must be
the reference's; and the result must equal ``renamed`` (the reference's maps with that renaming applied, computed by the
generator from the raw and tracked maps alone) exactly.  Nothing is masked or left out.

Bounds.  ``matched_centers``: 1e-5 absolute (a float32 mean of at most a few thousand coordinates < 1024: the reference sums
in float32, this project exactly).  PanopticMetric: counts exact; ``iou`` bit-equal for one update on a fresh metric (same
float32 operations in the same order), and within n * 2^-24 relative (n = matches summed: the worst case of re-ordering a
float32 sum of n positive terms) where updates are split.  Assignment: total cost within 1e-9 relative of scipy's (two
float64 sums of at most 100 terms in different orders), pairs equal where the costs are continuous random (a unique optimum)."""
import ctypes
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import instance_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
HEADS = ('segmentation', 'instance_center', 'instance_offset', 'instance_flow')
ORDERS = ('', 'reverse', 'random')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(H.load('instance.npz'))


@functools.lru_cache(maxsize=None)
def built(name):
    """The inputs of a case, after their digests have been compared with the fixture's."""
    case = IC.build(name)
    sha = IC.digest(case)
    assert [sha[k] for k in IC.INPUT_KEYS] == fixture()[f'{name}/sha'].tolist(), f'{name}: the case builder drifted'
    return case


def heads(case, device='cpu'):
    return {k: None if case[k] is None else torch.from_numpy(case[k]).to(device) for k in HEADS}


def check_tracked(got, name, what):
    """``got`` (B, S, H, W) integer numpy against the fixture, as the module text says."""
    g = fixture()
    raw, ref, renamed, fresh = (g[f'{name}/{k}'].astype(np.int64) for k in ('raw', 'tracked', 'renamed', 'fresh'))
    got = np.asarray(got).astype(np.int64)
    assert got.shape == ref.shape
    n_swapped = 0
    for b in range(len(ref)):
        assert np.array_equal(got[b, 0], ref[b, 0]), f'{what}: frame 0 of sample {b}'
        pairs = np.unique(np.stack([ref[b].reshape(-1), got[b].reshape(-1)], axis=1), axis=0)
        assert len(set(pairs[:, 0])) == len(pairs) == len(set(pairs[:, 1])), f'{what}: sample {b}: not a bijection of ids'
        assert (pairs[:, 0] == 0).sum() == 1 and [0, 0] in pairs.tolist(), f'{what}: sample {b}: background renamed'
        edges = int(ref[b, 0].max()) + np.concatenate([[0], np.cumsum(fresh[b])])      # ids created at step t: (edges[t-1], edges[t]]
        step_of = lambda ids: np.searchsorted(edges, ids, side='left')
        assert np.array_equal(step_of(pairs[:, 0]), step_of(pairs[:, 1])), f'{what}: sample {b}: ids of different steps exchanged'
        first = pairs[pairs[:, 0] <= edges[0]]
        assert np.array_equal(first[:, 0], first[:, 1]), f'{what}: sample {b}: an id of frame 0 renamed'
        n_swapped += int((pairs[:, 0] != pairs[:, 1]).sum())
        if name != 'deg_not_consistent':
            assert IC.renaming(raw[b], got[b])[1] == fresh[b].tolist(), f'{what}: sample {b}: fresh ids per step'
    assert np.array_equal(got, renamed), f'{what}: != the reference renamed to ascending fresh ids'
    print(f'{what}, {name}: equal to the reference up to {n_swapped} renamed ids, equal to its ascending renaming exactly')
    return n_swapped


def check_matched_centers(got, name, what):
    g = fixture()
    keys = g[f'{name}/mc_keys'].tolist()
    assert sorted(int(k) for k in got) == keys
    worst = 0.0
    for k in keys:
        want = g[f'{name}/mc_{k}']
        assert got[k].dtype == np.float32 and got[k].shape == want.shape
        worst = max(worst, float(np.abs(got[k] - want).max()))
    print(f'{what}: matched_centers of {len(keys)} ids within {worst:.2e} (bound 1e-5)')
    assert worst <= 1e-5


def run_case(name, device='cpu', check=False):
    """(raw, centres, counts, tracked, matched centres or None) of stp3_amd.instance on a fixture case."""
    from stp3_amd import instance as I
    case = built(name)
    o = heads(case, device)
    b, s, _, h, w = o['segmentation'].shape
    fg = torch.argmax(o['segmentation'], dim=2) == 1
    raw, centers, counts = I.segment_frames(o['instance_center'].reshape(b * s, h, w), o['instance_offset'].reshape(b * s, 2, h, w),
                                            fg.reshape(b * s, h, w))
    before = {k: v for k, v in o.items()}
    res = I.predict_instance_segmentation_and_trajectories(o, compute_matched_centers=case['matched'],
                                                           make_consistent=case['make_consistent'], check=check)
    assert all(o[k] is before[k] for k in o), 'the output dictionary was written to'
    tracked, mc = res if case['matched'] else (res, None)
    assert tracked.dtype == torch.int64 and tracked.shape == (b, s, h, w)
    return raw.view(b, s, h, w), centers, counts, tracked, mc


def check_case(name, raw, centers, counts, tracked, mc, what):
    g = fixture()
    assert np.array_equal(np.asarray(raw), g[f'{name}/raw']), f'{what}: maps before tracking'
    assert np.array_equal(np.asarray(centers), g[f'{name}/centers']) and np.array_equal(np.asarray(counts), g[f'{name}/counts']), \
        f'{what}: centres'
    swapped = check_tracked(np.asarray(tracked), name, what)
    if mc is not None:
        check_matched_centers(mc, name, what)
    return swapped


def test_fixture_holds_data_only_and_has_its_properties():
    g = fixture()
    assert os.path.getsize(os.path.join(H.GOLDEN, 'instance.npz')) <= 1 << 20
    assert sorted({k.split('/')[0] for k in g}) == sorted(IC.CASES)
    assert all(v.dtype.kind in 'iufU' for v in g.values())
    for name in IC.NON_INTEGER:
        assert g[f'{name}/gap'] > 5e-7, name
    assert g['integer/ties'] > 0
    assert all(g[f'{name}/match_margin'] > 1e-3 for name in IC.CASES)
    assert g['crowded/counts'].max() == 100 and (g['clean/fresh'] >= 2).any()
    tp, fp, fn = g['clean/metric_state'][1:, 1]
    assert tp >= 50 and fp >= 5 and fn >= 5 and g['clean/penalties'] >= 3


@pytest.mark.parametrize('name', list(IC.CASES))
def test_torch_path_matches_the_reference(name):
    raw, centers, counts, tracked, mc = run_case(name)
    assert raw.dtype == torch.int32 and centers.dtype == torch.int32 and tuple(centers.shape[1:]) == (100, 2)
    check_case(name, raw.numpy(), centers.numpy(), counts.numpy(), tracked.numpy(), mc, 'torch path')


def test_some_case_needs_the_renaming():
    """The reference's set order is not ascending somewhere in the fixture -- otherwise the renaming rule would be untested."""
    g = fixture()
    assert any(not np.array_equal(g[f'{n}/tracked'], g[f'{n}/renamed']) for n in IC.CASES)


def test_single_frame_functions_keep_the_reference_surface():
    from stp3_amd import instance as I
    case, g = built('nonsquare'), fixture()
    o = heads(case)
    fg = torch.argmax(o['segmentation'], dim=2) == 1
    seg, centers = I.get_instance_segmentation_and_centers(o['instance_center'][0, 1], o['instance_offset'][0, 1], fg[0, 1])
    n = int(g['nonsquare/counts'][1])
    assert seg.dtype == torch.int64 and tuple(seg.shape) == (1, 48, 72) and np.array_equal(seg[0].numpy(), g['nonsquare/raw'][0, 1])
    assert centers.dtype == torch.int64 and np.array_equal(centers.numpy(), g['nonsquare/centers'][1, :n])
    assert torch.equal(I.find_instance_centers(o['instance_center'][0, 1]), centers)
    ids = I.group_pixels(centers, o['instance_offset'][0, 1])
    assert tuple(ids.shape) == (1, 48, 72) and int(ids.min()) == 1 and int(ids.max()) == n
    sparse = torch.tensor([[0, 7, 7], [3, 0, 9]])
    assert I.make_instance_seg_consecutive(sparse).tolist() == [[0, 2, 2], [1, 0, 3]]
    assert I.update_instance_ids(sparse, torch.tensor([7, 9]), torch.tensor([1, 2])).tolist() == [[0, 1, 1], [3, 0, 2]]
    both = I.make_instance_id_temporally_consistent(torch.from_numpy(g['nonsquare/raw'].astype(np.int64)), o['instance_flow'])
    assert both.dtype == torch.int64 and np.array_equal(both.numpy(), g['nonsquare/renamed'])
    seg0, c0 = I.get_instance_segmentation_and_centers(o['instance_center'][0, 1] * 0, o['instance_offset'][0, 1], fg[0, 1])
    assert int(seg0.abs().max()) == 0 and tuple(c0.shape) == (0, 2)


def test_tracker_refuses_what_breaks_its_contract():
    from stp3_amd import instance as I
    raw = torch.zeros(1, 2, 8, 8, dtype=torch.int64)
    raw[:, :, 1, 1], raw[:, :, 5, 5] = 1, 2
    flow = torch.zeros(1, 2, 2, 8, 8)
    assert I.track_frames(raw, flow)[0].tolist() == raw.tolist()
    gap = raw.clone()
    gap[0, 1, 5, 5] = 3
    with pytest.raises(I.InstanceError):
        I.track_frames(gap, flow)
    full = raw.clone()
    full[0, 0] = 1
    with pytest.raises(I.InstanceError):
        I.track_frames(full, flow)
    inf = flow.clone()
    inf[0, 0, 0, 1, 1] = float('inf')
    with pytest.raises(I.InstanceError):
        I.track_frames(raw, inf)
    inf[0, 0, 0, 1, 1], inf[0, 0, 0, 0, 0] = 0.0, float('inf')                # a background pixel's flow is never read
    assert I.track_frames(raw, inf)[0].tolist() == raw.tolist()


# ---- the assignment ----
def lsap_matrices():
    rs = np.random.RandomState(7)
    shapes = [(1, 1), (1, 100), (100, 1), (100, 100), (2, 3), (3, 2), (64, 65), (65, 64), (37, 91), (91, 37), (99, 100), (100, 99)]
    shapes += [tuple(int(v) for v in rs.randint(1, 101, size=2)) for _ in range(20)]
    for k, shape in enumerate(shapes):
        yield rs.uniform(0.0, 50.0, size=shape).astype(np.float32), True
        if k % 3 == 0:
            yield rs.randint(0, 4, size=shape).astype(np.float32), False      # many equal optima: the total alone is defined


def test_host_solver_agrees_with_scipy():
    scipy_optimize = pytest.importorskip('scipy.optimize')
    from stp3_amd.instance import lsap
    worst = 0.0
    for cost, unique in lsap_matrices():
        r, c = lsap(cost)
        rs, cs = scipy_optimize.linear_sum_assignment(cost.astype(np.float64))
        assert len(r) == min(cost.shape) and len(set(r)) == len(r) and len(set(c)) == len(c) and (np.diff(r) > 0).all()
        mine, theirs = cost[r, c].astype(np.float64).sum(), cost[rs, cs].astype(np.float64).sum()
        worst = max(worst, abs(mine - theirs) / max(theirs, 1.0))
        assert abs(mine - theirs) <= 1e-9 * max(theirs, 1.0), cost.shape
        if unique:
            assert np.array_equal(r, rs) and np.array_equal(c, cs), cost.shape
    print(f'host solver: total cost within {worst:.1e} relative of scipy (bound 1e-9), pairs equal on the continuous matrices')
    with pytest.raises(ValueError):
        lsap(np.array([[1.0, np.nan]]))


# ---- the real kernel source, executed on the host (tests/hipcpu) ----
def run_host(tmp, lib, order, extra=()):
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    if order:
        env['HIPCPU_ORDER'] = order
    path = str(tmp / f'out_{order or "plain"}{"_".join(extra)}.npz')
    if extra:
        np.save(path + '.sizes.npy', LSAP_SCENES)
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_instance.py'), lib, path, *extra], env=env,
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(path))


LSAP_SCENES = np.array([(1, 1, 1), (1, 100, 2), (100, 1, 3), (100, 100, 4), (2, 3, 5), (64, 65, 6), (65, 64, 7), (37, 91, 8),
                        (91, 37, 9), (99, 100, 10), (100, 99, 11), (17, 17, 12)])


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_instance')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'))


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    return request.param or 'plain', run_host(*host_lib, request.param)


@pytest.mark.parametrize('name', IC.HOST_KERNEL_CASES + ['clean0'])
def test_kernels_on_host_match_the_reference(host_kernel, name):
    order, out = host_kernel
    g = fixture()
    what = f'kernels on the host ({order} order)'
    if name != 'clean0':
        mc = None
        check_case(name, out[f'{name}/raw'], out[f'{name}/centers'], out[f'{name}/counts'], out[f'{name}/tracked'], mc, what)
        return
    built('clean')
    assert np.array_equal(out['clean0/raw'], g['clean/raw'][:1]) and np.array_equal(out['clean0/counts'], g['clean/counts'][:7])
    assert np.array_equal(out['clean0/centers'], g['clean/centers'][:7])
    assert np.array_equal(out['clean0/tracked'], g['clean/renamed'][:1])
    assert IC.renaming(g['clean/raw'][0], out['clean0/tracked'][0])[1] == g['clean/fresh'][0].tolist()


def test_kernels_on_host_equal_the_torch_path_on_random_heads(host_kernel):
    """Plateaus, a NaN, an infinity, a frame under the threshold, an all-foreground frame, integer offsets (exact ties)."""
    sys.path.insert(0, HIPCPU)
    from run_instance import random_heads
    from stp3_amd import instance as I
    order, out = host_kernel
    center, offset, fg = random_heads(5)
    raw, centers, counts = I.segment_frames_reference(torch.from_numpy(center), torch.from_numpy(offset), torch.from_numpy(fg))
    assert int(counts[2]) == 0 and int(counts.max()) == 100 and int(raw[4].min()) == 0
    assert np.array_equal(out['random/counts'], counts.numpy()) and np.array_equal(out['random/centers'], centers.numpy())
    assert np.array_equal(out['random/raw'], raw.numpy())
    flow = (2.0 * np.random.RandomState(6).standard_normal((2, 3, 2, 24, 40))).astype(np.float32)
    tracked = I.track_frames_reference(raw.view(2, 3, 24, 40), torch.from_numpy(flow))
    assert not out['random/err'].any() and np.array_equal(out['random/tracked'], tracked.numpy())
    assert out['errors'].tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 0, 1]]


def test_kernel_assignment_agrees_with_scipy_and_the_host_solver(host_lib):
    scipy_optimize = pytest.importorskip('scipy.optimize')
    sys.path.insert(0, HIPCPU)
    from run_instance import point_scene
    from stp3_amd import instance as I
    out = run_host(*host_lib, '', extra=('lsap',))
    worst = 0.0
    for k, (n0, n1, seed) in enumerate(LSAP_SCENES):
        raw, flow = point_scene(np.random.RandomState(int(seed)), int(n0), int(n1))
        got = out[f'p{k}'][0]
        want = I.track_frames_reference(torch.from_numpy(raw), torch.from_numpy(flow), matching_threshold=1e30)[0].numpy()
        assert np.array_equal(got, want), (n0, n1)
        dist = I.step_distances(torch.from_numpy(raw[0, 0]), torch.from_numpy(raw[0, 1]), torch.from_numpy(flow[0, 0]),
                                torch.arange(1, n0 + 1), int(n1))
        assert dist.dtype == np.float32 and dist.shape == (n0, n1)
        pix = raw[0, 1] > 0
        cols, ids = raw[0, 1][pix] - 1, got[1][pix]
        matched = ids <= n0                                             # (threshold 1e30: every assigned pair is kept)
        rows, cols = ids[matched] - 1, cols[matched]
        rs, cs = scipy_optimize.linear_sum_assignment(dist.astype(np.float64))
        assert len(rows) == min(n0, n1) and len(set(rows)) == len(rows)
        mine, theirs = dist[rows, cols].astype(np.float64).sum(), dist[rs, cs].astype(np.float64).sum()
        worst = max(worst, abs(mine - theirs) / max(theirs, 1.0))
        assert abs(mine - theirs) <= 1e-9 * max(theirs, 1.0), (n0, n1)
        order = np.argsort(rows)
        assert np.array_equal(rows[order], rs) and np.array_equal(cols[order], cs), (n0, n1)
    print(f'kernel assignment: total cost within {worst:.1e} relative of scipy (bound 1e-9), the same pairs, on {len(LSAP_SCENES)} scenes')


# ---- PanopticMetric ----
KEYS = ('iou', 'true_positive', 'false_positive', 'false_negative')


def metric_state(m):
    return np.stack([getattr(m, k).cpu().numpy() for k in KEYS])


@pytest.mark.parametrize('name', list(IC.CASES))
def test_panoptic_metric_matches_the_reference(name):
    from stp3_amd.metrics import PanopticMetric
    g = fixture()
    pred, gt = torch.from_numpy(g[f'{name}/tracked'].astype(np.int64)), torch.from_numpy(built(name)['gt_instance'])
    m = PanopticMetric(n_classes=2)
    frames = m.frame_results(m.overlap_table(pred, gt), *gt.shape[:2])
    assert np.array_equal(frames[:, 1:], g[f'{name}/metric_frames'][:, 1:]), 'per-frame tp / fp / fn'
    assert np.array_equal(frames[:, 0].view(np.uint32), g[f'{name}/metric_frames'][:, 0].view(np.uint32)), 'per-frame iou bits'
    m(pred, gt)
    assert np.array_equal(metric_state(m).view(np.uint32), g[f'{name}/metric_state'].view(np.uint32))
    comp = m.compute()
    assert sorted(comp) == ['pq', 'rq', 'sq']
    assert np.array_equal(np.stack([comp[k].numpy() for k in ('pq', 'sq', 'rq')]), g[f'{name}/metric_compute'])
    loose = PanopticMetric(n_classes=2, temporally_consistent=False)
    loose(pred, gt)
    assert int(loose.true_positive[1] - m.true_positive[1]) == int(g[f'{name}/penalties'])
    # the renaming of fresh ids is invisible to the metric
    renamed = PanopticMetric(n_classes=2)
    renamed(torch.from_numpy(g[f'{name}/renamed'].astype(np.int64)), gt)
    assert np.array_equal(metric_state(renamed).view(np.uint32), metric_state(m).view(np.uint32))
    m.reset()
    assert not metric_state(m).any() and m.compute()['pq'].tolist() == [0.0, 0.0]


def test_panoptic_metric_two_updates_equal_one():
    from stp3_amd.metrics import PanopticMetric
    g = fixture()
    pred, gt = torch.from_numpy(g['clean/tracked'].astype(np.int64)), torch.from_numpy(built('clean')['gt_instance'])
    one, two = PanopticMetric(2), PanopticMetric(2)
    one(pred, gt)
    two(pred[:2], gt[:2])
    two(pred[2:], gt[2:])
    a, b = metric_state(one).astype(np.float64), metric_state(two).astype(np.float64)
    assert np.array_equal(a[1:], b[1:])
    n = a[1]                                                            # matches summed per class
    bound = n * 2.0 ** -24 * np.abs(a[0])
    print(f'iou of two updates against one: difference {np.abs(a[0] - b[0]).tolist()}, bound {bound.tolist()}')
    assert (np.abs(a[0] - b[0]) <= bound).all()
    assert len(two.state_dict()) == 0


def _sync_worker(rank, world, port, out):
    import torch.distributed as dist
    from stp3_amd.metrics import PanopticMetric
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    g = H.load('instance.npz')
    pred, gt = torch.from_numpy(g['clean/tracked'].astype(np.int64)), torch.from_numpy(IC.build('clean')['gt_instance'])
    m = PanopticMetric(2)
    m(pred[2 * rank:2 * rank + 2], gt[2 * rank:2 * rank + 2])
    local = metric_state(m)
    m.sync()
    out[rank] = (local, metric_state(m))
    dist.destroy_process_group()


def test_panoptic_metric_sync_sums_the_states_over_two_ranks():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_sync_worker, args=(2, port, out), nprocs=2, join=True)
    (l0, s0), (l1, s1) = out[0], out[1]
    assert np.array_equal(s0, s1) and np.array_equal(s0, l0 + l1) and l0[1, 1] > 0 and l1[1, 1] > 0


# ---- arguments ----
def test_c_entries_validate_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused first

    def segment(n=28, h=200, w=200, **null):
        p = {k: fake for k in ('center', 'offset', 'fg', 'seg', 'centers', 'counts')}
        p.update(null)
        return lib.stp3_instance_segment(n, h, w, 0.1, p['center'], p['offset'], p['fg'], p['seg'], p['centers'], p['counts'], None)

    def track(b=4, s=7, h=200, w=200, **null):
        p = {k: fake for k in ('raw', 'flow', 'out', 'err')}
        p.update(null)
        return lib.stp3_instance_track(b, s, h, w, 3.0, p['raw'], p['flow'], p['out'], p['err'], None)
    for bad in (dict(n=0), dict(h=0), dict(w=-1)):
        assert segment(**bad) == -10001, bad
    for null in ('center', 'offset', 'fg', 'seg', 'centers', 'counts'):
        assert segment(**{null: None}) == -10001, null
    assert segment(h=1025) == -10002 and segment(w=4096) == -10002
    for bad in (dict(b=0), dict(s=0), dict(h=0), dict(w=0)):
        assert track(**bad) == -10001, bad
    for null in ('raw', 'out', 'err'):
        assert track(**{null: None}) == -10001, null
    assert track(h=1025) == -10002 and track(w=1 << 20) == -10002


def test_python_entries_validate():
    from stp3_amd import instance as I
    with pytest.raises(AssertionError):
        I.segment_frames(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))          # offset without its 2 planes
    with pytest.raises(AssertionError):
        I.find_instance_centers(torch.zeros(8, 8))
    with pytest.raises(AssertionError):
        I.predict_instance_segmentation_and_trajectories(heads(built('nonsquare')), compute_matched_centers=True)   # B = 2


# ---- trainer ----
def test_validation_step_feeds_the_panoptic_metric(monkeypatch):
    """``shared_step(batch, False)`` with INSTANCE_SEG on: all S frames are post-processed, frames [rf - 1:] scored against
    labels['instance'] (reference trainer.py:222-228).  The network is replaced by heads derived from the batch's own labels
    (the CPU has no kernels to run it); the state-dict keys stay the committed ones."""
    import json
    from stp3_amd import synthetic
    from stp3_amd.config import perception_cfg
    from stp3_amd.metrics import PanopticMetric
    from stp3_amd.trainer import TrainingModule
    cfg = perception_cfg(**{'IMAGE.FINAL_DIM': (64, 96), 'LIFT.GT_DEPTH': True, 'INSTANCE_SEG.ENABLED': True,
                            'INSTANCE_FLOW.ENABLED': True})
    tm = TrainingModule(cfg.convert_to_dict())
    assert isinstance(tm.metric_panoptic_val, PanopticMetric) and not any('panoptic' in k for k in tm.state_dict())
    plain = TrainingModule(perception_cfg(**{'IMAGE.FINAL_DIM': (64, 96)}).convert_to_dict())
    assert not hasattr(plain, 'metric_panoptic_val')
    want = json.load(open(os.path.join(H.GOLDEN, 'state_dict_keys.json')))
    full = TrainingModule(perception_cfg(**{'LIFT.GT_DEPTH': True, 'INSTANCE_SEG.ENABLED': True,
                                            'INSTANCE_FLOW.ENABLED': True}).convert_to_dict())
    assert any(sorted(full.state_dict()) == sorted(v) for v in want.values()), 'state-dict keys changed'
    batch = synthetic.make_batch(batch=2, seq=3, final_dim=(64, 96), seed=4, gt_depth=True, instance=True)
    labels = tm.prepare_future_labels(batch)
    vehicle = labels['instance'] > 0
    seg = torch.stack([(~vehicle).float(), vehicle.float()], dim=2)
    output = {'segmentation': seg, 'instance_center': labels['centerness'], 'instance_offset': labels['offset'],
              'instance_flow': labels['flow'], 'pedestrian': torch.zeros_like(seg), 'hdmap': torch.zeros(2, 4, 200, 200),
              'depth_prediction': None}
    monkeypatch.setattr(tm.model, 'forward', lambda *a, **k: dict(output))
    tm.eval()
    rf = tm.model.receptive_field
    with torch.no_grad():
        out, _, loss = tm.shared_step(batch, False)
    assert loss == {} and out['segmentation'] is seg
    state = metric_state(tm.metric_panoptic_val)
    n_frames = 2 * (3 - rf + 1)
    assert state[1, 0] == n_frames, 'background is matched once per scored frame'
    assert state[1:, 1].sum() > 0, 'no vehicle was scored'
    comp = tm.metric_panoptic_val.compute()
    assert all(torch.isfinite(comp[k]).all() for k in ('pq', 'sq', 'rq'))
