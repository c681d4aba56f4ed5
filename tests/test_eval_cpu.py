"""CPU: the evaluation scorer (stp3_amd.evaluation; csrc/stp3_eval.hip) -- its kernels executed on the host (tests/hipcpu, in
forward, reverse and random fiber order), its torch route on CPU tensors, the C ABI's argument checks through the real
libstp3hip.so, ``sync()`` over two gloo ranks and ``evaluate()`` on a stub module.  Inputs and runs: tests/eval_cases.py.

What the results are compared with, and why the bounds are what they are:
  semantic  the states of ``IntersectionOverUnion`` fed with ``torch.argmax`` of the same tensors: integer counts, exactly.
  planning  tests/golden/planning.npz ``metric/*`` (the reference's PlanningMetric on the same inputs): the counts exactly; L2
            within rtol 1e-6, the bound of test_planning_cpu.test_planning_metric_matches_the_reference (the reference's float32
            running sum of 2 B = 4 terms errs by at most 3 * 2^-24 relative; the scorer sums them in float64).
  panoptic  tests/golden/instance.npz: per-frame counts exactly and IoU by bits, the state after one update by bits; two
            updates against one within n * 2^-24 * iou (n = matches), the bound of
            test_instance_cpu.test_panoptic_metric_two_updates_equal_one."""
import ctypes
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import eval_cases as EC
from tests import helpers as H
from tests import instance_cases as IC
from tests.test_instance_cpu import HIPCPU, ORDERS, built, fixture

from stp3_amd import evaluation as EV


# ---- the checks, shared with tests/test_eval_gpu.py ----
@functools.lru_cache(maxsize=None)
def semantic_want(name, update):
    return EC.semantic_expected(*EC.semantic_inputs(name, update))


def check_semantic(out, names=tuple(EC.SEMANTIC)):
    for name in names:
        one, two = semantic_want(name, 0), semantic_want(name, 1)
        assert one[:, 1].min() > 0 and (one[:, :, 3] > one[:, :, 0]).all(), 'the case exercises every counter'
        assert out[f'sem/{name}/one'].dtype == np.int64 and np.array_equal(out[f'sem/{name}/one'], one), name
        assert np.array_equal(out[f'sem/{name}/two'], one + two), f'{name}: two updates'
        assert not out[f'sem/{name}/reset'].any(), f'{name}: reset()'


def test_semantic_inputs_hold_the_corner_cases():
    out, labels = EC.semantic_inputs('s_c3_cl', 0)
    seg = out['segmentation']
    assert torch.isnan(seg).any() and torch.isinf(seg).any() and (labels['segmentation'] == 255).any()
    assert (seg[:, :, 0] == seg[:, :, 1]).float().mean() > 0.01, 'exact ties'
    assert (torch.argmax(seg, dim=2) == 2).any(), 'predictions outside [0, n_classes)'
    assert seg.stride(2) == 1 and not EC.semantic_inputs('s_f32', 0)[0]['segmentation'].stride(2) == 1


def check_planning(out):
    g = H.load('planning.npz')
    for k in ('obj_col', 'obj_box_col', 'total'):
        assert np.array_equal(out[f'plan/{k}'], g[f'metric/{k}'].astype(np.int64)), k
    assert out['plan/obj_col'].sum() > 0 and out['plan/obj_box_col'].sum() > 0          # the fixture's collisions are still there
    rel = np.abs(out['plan/L2'] - g['metric/L2'].astype(np.float64)) / g['metric/L2']
    print(f'L2 against the reference: relative difference {rel.tolist()} (bound 1e-6)')
    np.testing.assert_allclose(out['plan/L2'], g['metric/L2'], rtol=1e-6)
    # the horizon keys: three PlanningMetric(cfg, 2 k) objects fed the prefixes (evaluate.py:70-73, 135-137, 162-166)
    from stp3_amd.metrics import PlanningMetric
    c = EC.planning_cfg()
    updates, labels = EC.planning_inputs()
    rf = int(c.TIME_RECEPTIVE_FIELD)
    truth = labels['segmentation'][:, rf:].squeeze(2).bool() | labels['pedestrian'][:, rf:].squeeze(2).bool()
    keys = set()
    for i in range(int(c.N_FUTURE_FRAMES) // 2):
        m, t = PlanningMetric(c, 2 * (i + 1)), 2 * (i + 1)
        for trajs, gt in updates:
            m(trajs[:, :t], gt[:, 1:t + 1], truth[:, :t])
        for key, value in m.compute().items():
            name = f'plan_{key}_{i + 1}s'
            keys.add(f'plan/compute/{name}')
            np.testing.assert_allclose(out[f'plan/compute/{name}'], value.mean().numpy(), rtol=1e-6, err_msg=name)
    assert keys == {k for k in out if k.startswith('plan/compute/')} and len(keys) == 3 * (int(c.N_FUTURE_FRAMES) // 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_panoptic(out, names=tuple(IC.CASES), native=True):
    g = fixture()
    for name in names:
        built(name)
        assert not out[f'pan/{name}/err'].any(), f'{name}: an error word on a fixture case'
        if native:
            frames, want = out[f'pan/{name}/frames'], g[f'{name}/metric_frames']
            assert frames.shape == want.shape and np.array_equal(frames[:, 1:], want[:, 1:]), f'{name}: per-frame tp / fp / fn'
            assert np.array_equal(bits(frames[:, 0]), bits(want[:, 0])), f'{name}: per-frame iou bits'
        state = out[f'pan/{name}/state']
        assert np.array_equal(bits(state), bits(g[f'{name}/metric_state'])), f'{name}: state'
        assert np.array_equal(out[f'pan/{name}/compute'], g[f'{name}/metric_compute'][:, 1]), f'{name}: compute()'
        assert np.array_equal(bits(out[f'pan/{name}/renamed']), bits(state)), f'{name}: the renaming of fresh ids is visible'
        assert int(out[f'pan/{name}/loose'][1, 1] - state[1, 1]) == int(g[f'{name}/penalties']), f'{name}: penalties'
    if 'clean' in names:
        a, b = out['pan/clean/state'].astype(np.float64), out['pan/clean/split'].astype(np.float64)
        assert np.array_equal(a[1:], b[1:])
        bound = a[1] * 2.0 ** -24 * np.abs(a[0])
        print(f'iou of two updates against one: difference {np.abs(a[0] - b[0]).tolist()}, bound {bound.tolist()}')
        assert (np.abs(a[0] - b[0]) <= bound).all()
    if native:
        want = [w for _, _, w in EC.panoptic_error_inputs()]
        assert out['pan/errors'].tolist() == want, 'every error word by the input that breaks its clause, and by nothing else'


# ---- the kernel source on the host ----
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_eval')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'))


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    run = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_eval.py'), lib, path], env=env, capture_output=True, text=True,
                         timeout=3000)
    assert run.returncode == 0 and 'RESULT' in run.stdout, run.stderr[-1500:]
    return dict(np.load(path))


def test_semantic_kernel_on_host(host_kernel):
    check_semantic(host_kernel)


def test_planning_kernel_on_host(host_kernel):
    check_planning(host_kernel)


def test_panoptic_kernel_on_host(host_kernel):
    check_panoptic(host_kernel)


# ---- the torch route of the scorer ----
def test_semantic_on_cpu_tensors():
    check_semantic(EC.run_semantic('cpu', ('s_f32', 's_bf16_cl', 's_c3_cl')), ('s_f32', 's_bf16_cl', 's_c3_cl'))


def test_planning_on_cpu_tensors():
    check_planning(EC.run_planning('cpu'))


def test_panoptic_on_cpu_tensors():
    names = ('nonsquare', 'deg_all_foreground', 'crowded', 'clean')
    check_panoptic(EC.run_panoptic('cpu', names, fixture(), errors=False), names, native=False)


def test_error_words_raise():
    scorer = EV.EvalScorer(EC.panoptic_cfg(), 'cpu')
    scorer.err[2] = 1
    with pytest.raises(EV.EvalError, match='distinct'):
        scorer.compute()
    scorer.reset()
    assert set(scorer.compute()) == {'vehicle_iou', 'vehicle_pq', 'vehicle_sq', 'vehicle_rq'}


# ---- the C ABI, without a device ----
def test_argument_validation_without_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUP = -10001, -10002
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def sem(**kw):
        d = _lib.EvalDims()
        d.B, d.S, d.H, d.W, d.Cs, d.Cp, d.E, d.n_classes, d.first = 1, 3, 8, 8, 2, 2, 2, 2, 1
        d.seg_stride[:], d.ped_stride[:], d.hd_stride[:] = (384, 128, 64, 8, 1), (384, 128, 64, 8, 1), (256, 64, 8, 1)
        ptrs = {k: p for k in ('seg', 'ped', 'hd', 'seg_label', 'ped_label', 'hd_label', 'counts')}
        for k, v in kw.items():
            if k in ptrs:
                ptrs[k] = v
            else:
                setattr(d, k, v)
        return lib.stp3_eval_semantic(ctypes.byref(d), *(ptrs[k] for k in ('seg', 'ped', 'hd', 'seg_label', 'ped_label', 'hd_label',
                                                                             'counts')), None)
    assert lib.stp3_eval_semantic(None, p, p, p, p, p, p, p, None) == EINVAL
    for k in ('seg', 'ped', 'hd', 'seg_label', 'ped_label', 'hd_label', 'counts'):
        assert sem(**{k: None}) == EINVAL, k
    for k in ('B', 'S', 'H', 'W', 'Cs', 'n_classes'):
        assert sem(**{k: 0}) == EINVAL, k
    assert sem(first=-1) == EINVAL and sem(first=3) == EINVAL
    assert sem(Cs=17) == EUNSUP and sem(Cp=17) == EUNSUP and sem(n_classes=9) == EUNSUP and sem(H=1025) == EUNSUP
    assert sem(seg_dtype=7) == EUNSUP

    def plan(**kw):
        d = _lib.EvalPlanDims()
        d.B, d.T, d.S, d.H, d.W, d.K, d.first_future = 2, 4, 7, 8, 8, 4, 3
        d.dx0, d.dx1, d.bx0, d.bx1 = 0.5, 0.5, -2.0, -2.0
        d.traj_stride[:], d.gt_stride[:] = (12, 3), (12, 3)
        ptrs = {k: p for k in ('trajs', 'gt', 'seg_label', 'ped_label', 'footprint', 'obj_col', 'obj_box_col', 'total', 'l2')}
        for k, v in kw.items():
            if k in ptrs:
                ptrs[k] = v
            else:
                setattr(d, k, v)
        return lib.stp3_eval_planning(ctypes.byref(d), *ptrs.values(), None)
    for k in ('trajs', 'gt', 'seg_label', 'footprint', 'obj_col', 'obj_box_col', 'total', 'l2'):
        assert plan(**{k: None}) == EINVAL, k
    for k in ('B', 'T', 'S', 'H', 'W', 'K'):
        assert plan(**{k: 0}) == EINVAL, k
    assert plan(first_future=-1) == EINVAL and plan(first_future=4) == EINVAL and plan(dx0=0.0) == EINVAL
    assert plan(B=257) == EUNSUP and plan(B=256, T=5, S=9) == EUNSUP and plan(H=1025) == EUNSUP

    need = ctypes.c_size_t()
    assert lib.stp3_eval_panoptic_workspace_bytes(2, 7, 2, ctypes.byref(need)) == 0 and need.value == 2 * 5 * 32 + 8
    assert lib.stp3_eval_panoptic_workspace_bytes(2, 7, 7, ctypes.byref(need)) == EINVAL
    assert lib.stp3_eval_panoptic_workspace_bytes(0, 7, 0, ctypes.byref(need)) == EINVAL
    assert lib.stp3_eval_panoptic_workspace_bytes(2, 7, 0, None) == EINVAL

    def pan(B=1, S=2, H=8, W=8, first=0, pred=p, gt=p, ws=p, ws_bytes=4096, state=p, err=p):
        return lib.stp3_eval_panoptic(B, S, H, W, first, 1, 0, pred, gt, ws, ws_bytes, state, err, None)
    for k in ('pred', 'gt', 'ws', 'state', 'err'):
        assert pan(**{k: None}) == EINVAL, k
    for k in ('B', 'S', 'H', 'W'):
        assert pan(**{k: 0}) == EINVAL, k
    assert pan(first=-1) == EINVAL and pan(first=2) == EINVAL
    assert pan(H=1025) == EUNSUP and pan(W=1025) == EUNSUP
    assert pan(ws_bytes=8) == -10003


# ---- sync() ----
def _sync_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from stp3_amd.config import perception_cfg
    cfg = perception_cfg(**{'TIME_RECEPTIVE_FIELD': EC.SEM_RF, 'INSTANCE_SEG.ENABLED': True, 'SEMANTIC_SEG.PEDESTRIAN.ENABLED': True,
                            'SEMANTIC_SEG.HDMAP.ENABLED': True, 'PLANNING.ENABLED': False})
    scorer = EV.EvalScorer(cfg, 'cpu')
    output, labels = EC.semantic_inputs('s_f32', rank)
    case = IC.build('nonsquare')
    g = H.load('instance.npz')
    labels['instance'] = torch.from_numpy(case['gt_instance'][rank:rank + 1, :3])
    scorer.update({k: v[rank:rank + 1] for k, v in output.items()}, {k: v[rank:rank + 1] if k != 'instance' else v for k, v in labels.items()},
                  instance=torch.from_numpy(g['nonsquare/tracked'][rank:rank + 1, :3].astype(np.int64)))
    scorer.counts[0, 0, 0] += 5 + rank           # (the scorer's own buffers are reduced too)
    local = scorer.states()
    scorer.sync()
    out[rank] = (local, scorer.states())
    dist.destroy_process_group()


def test_sync_sums_the_states_over_two_ranks():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_sync_worker, args=(2, port, out), nprocs=2, join=True)
    (l0, s0), (l1, s1) = out[0], out[1]
    assert l0['semantic'].sum() > 0 and l0['panoptic'][1:].sum() > 0 and not np.array_equal(l0['semantic'], l1['semantic'])
    for k in ('semantic', 'panoptic'):
        assert np.array_equal(s0[k], l0[k] + l1[k]) and np.array_equal(s1[k], s0[k]), k
    assert l1['semantic'][0, 0, 0] - l0['semantic'][0, 0, 0] != 0


# ---- evaluate() ----
class StubModel(torch.nn.Module):
    """Returns canned heads: batch k of the loader gets sample k of the 'nonsquare' instance case plus random semantic heads."""
    receptive_field = 2

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls = outputs, 0

    def forward(self, image, intrinsics, extrinsics, future_egomotion):
        self.calls += 1
        return self.outputs[int(image[0])]


class StubModule(torch.nn.Module):
    def __init__(self, cfg, outputs, labels):
        super().__init__()
        self.cfg, self.model, self.labels = cfg, StubModel(outputs), labels

    def prepare_future_labels(self, batch):
        return self.labels[int(batch['image'][0])]


def stub_case():
    from stp3_amd.config import perception_cfg
    cfg = perception_cfg(**{'TIME_RECEPTIVE_FIELD': 2, 'INSTANCE_SEG.ENABLED': True, 'SEMANTIC_SEG.PEDESTRIAN.ENABLED': True,
                            'SEMANTIC_SEG.HDMAP.ENABLED': True, 'PLANNING.ENABLED': False})
    case = built('nonsquare')
    rs = np.random.RandomState(77)
    outputs, labels = [], []
    for k in range(2):
        o = {key: torch.from_numpy(case[key][k:k + 1]) for key in ('segmentation', 'instance_center', 'instance_offset', 'instance_flow')}
        s, (h, w) = o['segmentation'].shape[1], o['segmentation'].shape[-2:]
        o['pedestrian'] = torch.from_numpy(rs.standard_normal((1, s, 2, h, w)).astype(np.float32))
        o['hdmap'] = torch.from_numpy(rs.standard_normal((1, 4, h, w)).astype(np.float32))
        gt = torch.from_numpy(case['gt_instance'][k:k + 1])
        outputs.append(o)
        labels.append({'segmentation': (gt > 0).long().unsqueeze(2), 'pedestrian': torch.from_numpy(rs.randint(0, 2, (1, s, 1, h, w))),
                       'hdmap': torch.from_numpy(rs.randint(0, 2, (1, 2, h, w))), 'instance': gt})
    loader = [{'image': torch.tensor([k]), 'intrinsics': None, 'extrinsics': None, 'future_egomotion': None} for k in range(2)]
    return cfg, outputs, labels, loader


def by_hand(cfg, outputs, labels, rf):
    """The existing metric classes driven as evaluate.py:95-119, 143-160 drives them."""
    from stp3_amd.instance import predict_instance_segmentation_and_trajectories
    from stp3_amd.metrics import IntersectionOverUnion, PanopticMetric
    dev = outputs[0]['segmentation'].device
    seg = cfg.SEMANTIC_SEG
    veh, ped = IntersectionOverUnion(2).to(dev), IntersectionOverUnion(2).to(dev)
    hd = [IntersectionOverUnion(2, absent_score=1).to(dev) for _ in range(2)]
    pan = PanopticMetric(2).to(dev)
    for o, l in zip(outputs, labels):
        veh(torch.argmax(o['segmentation'], dim=2, keepdim=True)[:, rf - 1:], l['segmentation'][:, rf - 1:])
        if seg.PEDESTRIAN.ENABLED:
            ped(torch.argmax(o['pedestrian'], dim=2, keepdim=True)[:, rf - 1:], l['pedestrian'][:, rf - 1:])
        if seg.HDMAP.ENABLED:
            for i in range(2):
                hd[i](torch.argmax(o['hdmap'][:, 2 * i:2 * i + 2], dim=1, keepdim=True), l['hdmap'][:, i:i + 1])
        if cfg.INSTANCE_SEG.ENABLED:
            pan(predict_instance_segmentation_and_trajectories(o, compute_matched_centers=False)[:, rf - 1:], l['instance'][:, rf - 1:])
    want = {'vehicle_iou': veh.compute()[1]}
    if seg.PEDESTRIAN.ENABLED:
        want['pedestrian_iou'] = ped.compute()[1]
    if seg.HDMAP.ENABLED:
        for i, name in enumerate(seg.HDMAP.ELEMENTS):
            want[name + '_iou'] = hd[i].compute()[1]
    if cfg.INSTANCE_SEG.ENABLED:
        for k, v in pan.compute().items():
            want['vehicle_' + k] = v[1]
    return {k: v.cpu() for k, v in want.items()}


def test_evaluate_on_a_stub_module():
    cfg, outputs, labels, loader = stub_case()
    module = StubModule(cfg, outputs, labels)
    got = EV.evaluate(module, loader, device='cpu')
    want = by_hand(cfg, outputs, labels, 2)
    assert module.model.calls == 2 and not module.training
    assert set(got) == set(want) == {'vehicle_iou', 'pedestrian_iou', 'lane_divider_iou', 'drivable_area_iou', 'vehicle_pq',
                                     'vehicle_sq', 'vehicle_rq'}
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].dim() == 0 and np.array_equal(bits(got[k].numpy()), bits(want[k].numpy())), k
    assert 0 < float(got['vehicle_iou']) < 1 and float(got['vehicle_pq']) > 0
