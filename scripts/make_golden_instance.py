"""Writes tests/golden/instance.npz: the reference's instance post-processing (stp3/utils/instance.py:80-330) and its
PanopticMetric (stp3/metrics.py:74-261), both unmodified and loaded from the reference tree, on the cases of
tests/instance_cases.py, for tests/test_instance_cpu.py / test_instance_gpu.py.

    python scripts/make_golden_instance.py [--time]

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, scipy and torch.  The head outputs are not stored (16 MB a
case): the tests rebuild them with the same builder and check the sha256 stored here first.

Per case ``<name>/``:
  sha           the builder's digests, one hex string per input (instance_cases.INPUT_KEYS order)
  raw           int16 (B, S, H, W): the per-frame maps before tracking (make_consistent=False)
  centers, counts   int16 (B * S, 100, 2) (row, column; zero beyond the count), int16 (B * S): the centres kept per frame
  tracked       int16 (B, S, H, W): predict_instance_segmentation_and_trajectories with the case's options
  renamed       ``tracked`` with the ids created at each step renamed to ascend with the raw id (instance_cases.renaming: from
                the two maps alone) -- what this project's rule gives; ``fresh``: int16 (B, S) fresh ids per step
  gap           float64: the smallest relative gap between the two nearest centres over all foreground pixels, in float64
                (integer case: ``ties``, the number of foreground pixels whose two nearest centres are EXACTLY equally far)
  match_margin  float64: the smallest |distance - matching_threshold| over all assigned pairs
  mc_keys, mc_<id>   matched_centers of the cases that ask for them
  metric_frames float32 (B * S, 4, 2): iou / true_positive / false_positive / false_negative of every frame in update
                order, ``metric_state`` (4, 2) their accumulation, ``metric_compute`` (3, 2) pq / sq / rq, ``penalties``: the
                number of inconsistent-id penalties (true positives gained by temporally_consistent=False)
The properties the fixture is meant to have are asserted below; ``--time`` also prints the reference's time per call on this
CPU for batch 4 x 7 frames x 200 x 200, clean and crowded.
"""
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_stubs  # noqa: E402
from tests import instance_cases as IC  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'instance.npz')
GAP_MIN, MATCH_MARGIN_MIN, THRESHOLD = 5e-7, 1e-3, 3.0
KEYS = ('iou', 'true_positive', 'false_positive', 'false_negative')


def load_reference():
    """ref_stubs.install() plus the Lightning stand-ins that stp3/metrics.py imports (the idea of
    oracle/make_golden_train.install_trainer_stubs: metric states are plain buffers)."""
    ref_stubs.install()

    class Metric(nn.Module):
        def __init__(self, compute_on_step=False, **kwargs):
            super().__init__()

        def add_state(self, name, default, dist_reduce_fx=None):
            self.register_buffer(name, default, persistent=False)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    mod('pytorch_lightning', LightningModule=nn.Module)
    mod('pytorch_lightning.metrics')
    mod('pytorch_lightning.metrics.metric', Metric=Metric)
    mod('pytorch_lightning.metrics.functional')
    mod('pytorch_lightning.metrics.functional.classification', stat_scores_multiple_classes=None)
    mod('pytorch_lightning.metrics.functional.reduction', reduce=None)
    import stp3.metrics as ref_metrics
    import stp3.utils.instance as ref_instance
    return ref_instance, ref_metrics


def tensors(case, dtype=torch.float32):
    return {k: None if case[k] is None else torch.from_numpy(case[k]).to(dtype)
            for k in ('segmentation', 'instance_center', 'instance_offset', 'instance_flow')}


def run_reference(ref, case, dtype=torch.float32):
    """(raw (B,S,H,W), centres per frame, tracked, matched_centers or None, assigned distances)."""
    out = tensors(case, dtype)
    b, s = out['segmentation'].shape[:2]
    fg = torch.argmax(out['segmentation'], dim=2) == 1
    centers = [ref.get_instance_segmentation_and_centers(out['instance_center'][i, t], out['instance_offset'][i, t], fg[i, t])[1]
               for i in range(b) for t in range(s)]
    raw = ref.predict_instance_segmentation_and_trajectories(dict(out), make_consistent=False)
    assigned = []
    keep = ref.linear_sum_assignment

    def recording(d):
        r, c = keep(d)
        assigned.extend(d[r, c].tolist())
        return r, c
    ref.linear_sum_assignment = recording                     # (the module's global, for this call: the file is untouched)
    try:
        res = ref.predict_instance_segmentation_and_trajectories(dict(out), compute_matched_centers=case['matched'],
                                                                 make_consistent=case['make_consistent'])
    finally:
        ref.linear_sum_assignment = keep
    tracked, mc = res if case['matched'] else (res, None)
    return raw, centers, tracked, mc, np.array(assigned)


def nearest_gap(case, centers_per_frame):
    """(smallest relative gap between the two nearest centres over the foreground pixels, number of exact ties), float64."""
    seg, off = case['segmentation'], case['instance_offset'].astype(np.float64)
    b, s, _, h, w = seg.shape
    gap, ties = np.inf, 0
    for i in range(b):
        for t in range(s):
            c = centers_per_frame[i * s + t].numpy().astype(np.float64)
            if len(c) < 2:
                continue
            fg = seg[i, t, 1] > seg[i, t, 0]
            rr, cc = np.nonzero(fg)
            loc = np.stack([rr + off[i, t, 0][fg], cc + off[i, t, 1][fg]], axis=1)
            d = np.sqrt(((c[None] - loc[:, None]) ** 2).sum(-1))
            d.sort(axis=1)
            ties += int((d[:, 0] == d[:, 1]).sum())
            rel = (d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-300)
            gap = min(gap, float(rel.min())) if len(rel) else gap
    return gap, ties


def run_metric(ref_metrics, pred, gt, consistent=True):
    metric = ref_metrics.PanopticMetric(n_classes=2, temporally_consistent=consistent)
    frames = []
    inner = metric.panoptic_metrics

    def recording(*args):
        r = inner(*args)
        frames.append(np.stack([r[k].numpy().copy() for k in KEYS]))
        return r
    metric.panoptic_metrics = recording
    metric.update(pred, gt)
    state = np.stack([getattr(metric, k).numpy() for k in KEYS])
    comp = metric.compute()
    return np.stack(frames).astype(np.float32), state.astype(np.float32), np.stack([comp[k].numpy() for k in ('pq', 'sq', 'rq')])


def main():
    ref, ref_metrics = load_reference()
    out = {}
    totals = np.zeros((4, 2))
    penalties_total = 0
    for name in IC.CASES:
        case = IC.build(name)
        raw, centers, tracked, mc, assigned = run_reference(ref, case)
        raw64, _, tracked64, _, _ = run_reference(ref, case, torch.float64)
        assert torch.equal(raw, raw64) and torch.equal(tracked, tracked64), f'{name}: float64 inputs change the maps'
        b, s, h, w = raw.shape
        assert int(raw.max()) <= 100 and int(tracked.max()) < 32768
        gap, ties = nearest_gap(case, centers)
        margin = float(np.abs(assigned - THRESHOLD).min()) if len(assigned) else np.inf
        assert margin > MATCH_MARGIN_MIN, (name, margin)
        if IC.CASES[name].get('integer'):
            assert ties > 0, f'{name}: no exact tie between two centres'
            out[f'{name}/ties'] = np.array(ties)
        else:
            assert gap > GAP_MIN, (name, gap)
        pre = f'{name}/'
        sha = IC.digest(case)
        out[pre + 'sha'] = np.array([sha[k] for k in IC.INPUT_KEYS])
        out[pre + 'raw'] = raw.numpy().astype(np.int16)
        cen = np.zeros((b * s, 100, 2), np.int16)
        for i, c in enumerate(centers):
            cen[i, :len(c)] = c.numpy()
        out[pre + 'centers'], out[pre + 'counts'] = cen, np.array([len(c) for c in centers], np.int16)
        out[pre + 'tracked'] = tracked.numpy().astype(np.int16)
        renamed, fresh = zip(*[IC.renaming(raw[i].numpy(), tracked[i].numpy()) for i in range(b)]) if case['make_consistent'] \
            else ((tracked[i].numpy() for i in range(b)), [[0] * s] * b)
        out[pre + 'renamed'] = np.stack(list(renamed)).astype(np.int16)
        out[pre + 'fresh'] = np.array(fresh, np.int16)
        out[pre + 'gap'], out[pre + 'match_margin'] = np.array(gap), np.array(margin)
        if mc is not None:
            out[pre + 'mc_keys'] = np.array(sorted(int(k) for k in mc), np.int64)
            for k, v in mc.items():
                assert v.dtype == np.float32
                out[pre + f'mc_{int(k)}'] = np.ascontiguousarray(v)
        gt = torch.from_numpy(case['gt_instance'])
        frames, state, comp = run_metric(ref_metrics, tracked, gt)
        _, loose, _ = run_metric(ref_metrics, tracked, gt, consistent=False)
        penalties = int(loose[1, 1] - state[1, 1])
        out[pre + 'metric_frames'], out[pre + 'metric_state'], out[pre + 'metric_compute'] = frames, state, comp
        out[pre + 'penalties'] = np.array(penalties)
        totals += state
        penalties_total += penalties
        n_per_frame = [len(c) for c in centers]
        print(f'{name}: centres per frame {min(n_per_frame)}..{max(n_per_frame)}, ids up to {int(tracked.max())}, fresh per step '
              f'{np.array(fresh).tolist()}, gap {gap:.2e}, ties {ties}, match margin {margin:.2e}, vehicle tp/fp/fn '
              f'{state[1:, 1].tolist()}, penalties {penalties}, pq/sq/rq {comp[:, 1].tolist()}')
        # the properties each case exists for
        if name == 'clean':
            assert 10 <= min(n_per_frame) and max(n_per_frame) <= 20
            assert (np.array(fresh) >= 2).any(), 'no step creates two or more ids'
            assert state[1, 1] >= 50 and state[2, 1] >= 5 and state[3, 1] >= 5 and penalties >= 3, (state, penalties)
        if name == 'crowded':
            cm = ref.find_instance_centers(torch.from_numpy(case['instance_center'][0, 0]))
            assert len(cm) > 100 and max(n_per_frame) == 100
        if name == 'deg_mid_empty':
            assert n_per_frame[2] == 0 and n_per_frame[1] > 0 and n_per_frame[3] > 0
        if name == 'deg_first_empty':
            assert n_per_frame[0] == 0 and n_per_frame[1] > 0
        if name == 'deg_all_foreground':
            assert int(raw[0, 1].min()) == 0 and (case['segmentation'][0, 1, 1] > case['segmentation'][0, 1, 0]).all()
        if name == 'nonsquare':
            assert h != w and 200 not in (h, w)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes; vehicle totals tp/fp/fn', totals[1:, 1].tolist(), 'penalties', penalties_total)
    assert os.path.getsize(OUT) <= 1 << 20
    if '--time' in sys.argv:
        cpu = [l.split(':', 1)[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')][:1]
        for name in ('clean', 'crowded'):
            o = tensors(IC.build(name, B=4, S=7))
            ref.predict_instance_segmentation_and_trajectories(dict(o))
            t = time.perf_counter()
            for _ in range(3):
                ref.predict_instance_segmentation_and_trajectories(dict(o))
            print(f'reference predict_instance_segmentation_and_trajectories, {name}, 4 x 7 x 200 x 200: '
                  f'{(time.perf_counter() - t) / 3 * 1e3:.0f} ms per call (torch CPU, {torch.get_num_threads()} threads) on {cpu}')


if __name__ == '__main__':
    main()
