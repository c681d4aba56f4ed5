"""The evaluation loop of the reference (``evaluate.py:76-169``) with its scoring on the device.

``EvalScorer`` holds the states of every metric ``evaluate.py`` prints -- the IoU of the vehicle, pedestrian and hd-map heads,
the panoptic quality of the vehicle instances, L2 and collision rates of the planned trajectory at every horizon -- and
``update`` adds one batch to them.  On GPU tensors an update is three or four launches of csrc/stp3_eval.hip
(``stp3_eval_semantic``, ``stp3_eval_planning``, ``stp3_eval_panoptic`` and its finishing launch, include/stp3_hip.h) and
nothing else: no ``argmax`` / ``logical_or`` tensors, no boolean indexing, ``bincount`` or ``unique``, no copy to the host --
nothing in it waits for the device, so the whole call can be captured by ``torch.cuda.graph``.  ``compute`` is the one
device-to-host copy.  On CPU tensors, and for configurations the kernels do not cover (more than 8 classes, a panoptic
metric that is not (n_classes 2, vehicles_id 1), shapes beyond the kernels' limits), an update runs the arithmetic of
``metrics.IntersectionOverUnion`` / ``PlanningMetric`` / ``PanopticMetric`` on objects the scorer owns; both kinds of state
add, and ``compute`` / ``states`` / ``sync`` see their sum.

One deliberate difference: the kernels count in int64 (and sum L2 in float64), where the reference and the three metric
classes accumulate in float32 and stop being exact above 2^24 -- about 420 frames of 200 x 200 for ``support``.  The results
are equal while the totals stay below that.

``evaluate(module, loader)`` is the loop itself, without the plotting, and returns the dict ``evaluate.py`` prints."""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib, ops, ops_plan
from ._lib import check as _check
from .metrics import IntersectionOverUnion, PanopticMetric, PlanningMetric

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}
MAX_LOGITS, MAX_CLASSES, MAX_SIDE, MAX_PLAN_POINTS, MAX_PLANES = 16, 8, 1024, 1024, 65535
PANOPTIC_PAIRS = 1024                       # STP3_EVAL_PANOPTIC_PAIRS
PANOPTIC_ERRORS = ('an instance id lies outside [0, 2^20)',
                   'no ground-truth pixel of an update is background (id 0 of gt_instance must be background)',
                   f'a frame has more than {PANOPTIC_PAIRS - 1} distinct (ground-truth id, predicted id) pairs, or a sample matched more '
                   f'than {PANOPTIC_PAIRS} ground-truth ids',
                   'reserved')
IOU_KEYS = ('true_positive', 'false_positive', 'false_negative', 'support')


class EvalError(RuntimeError):
    pass


def _dense(t, dtype=torch.int64):
    return t if t.dtype == dtype and t.is_contiguous() else t.to(dtype).contiguous()


def _strides_fit(t):
    return all(0 <= s < 2 ** 31 for s in t.stride())


class EvalScorer:
    """See the module docstring.  ``cfg``: the configuration node (``TrainingModule.cfg``); ``device``: where the states live."""

    def __init__(self, cfg, device, temporally_consistent=True, vehicles_id=1):
        self.cfg, self.device = cfg, torch.device(device)
        seg = cfg.SEMANTIC_SEG
        self.n_classes = len(seg.VEHICLE.WEIGHTS)
        self.pedestrian = bool(seg.PEDESTRIAN.ENABLED)
        self.elements = list(seg.HDMAP.ELEMENTS) if seg.HDMAP.ENABLED else []
        self.instance = bool(cfg.INSTANCE_SEG.ENABLED)
        self.planning = bool(cfg.PLANNING.ENABLED)
        self.receptive_field = int(cfg.TIME_RECEPTIVE_FIELD)
        self.n_future = int(cfg.N_FUTURE_FRAMES)
        self.temporally_consistent, self.vehicles_id = bool(temporally_consistent), int(vehicles_id)
        E, n, T = len(self.elements), self.n_classes, self.n_future
        # one buffer, so that compute() is ONE copy: int64 counts [2 + E][n][4], int64 obj_col [T], obj_box_col [T], total [1],
        # float64 L2 [T], float32 panoptic [4][2] (8 floats), int32 err [4]
        n_counts = (2 + E) * n * 4
        self._packed = torch.zeros(8 * (n_counts + 2 * T + 1 + T) + 4 * 8 + 4 * 4, dtype=torch.uint8, device=self.device)
        at = 0

        def take(count, dtype, size):
            nonlocal at
            view = self._packed[at:at + count * size].view(dtype)
            at += count * size
            return view
        self.counts = take(n_counts, torch.int64, 8).view(2 + E, n, 4)
        self.obj_col, self.obj_box_col, self.total = take(T, torch.int64, 8), take(T, torch.int64, 8), take(1, torch.int64, 8)
        self.L2 = take(T, torch.float64, 8)
        self.panoptic = take(8, torch.float32, 4).view(4, 2)
        self.err = take(4, torch.int32, 4)
        self._n_int = n_counts + 2 * T + 1
        self._workspace = None
        self._footprint = None
        self._host = {}                          # the metric objects of the torch route, made when first needed

    # ---- the torch route: the existing classes ----
    def _host_metric(self, key):
        if key not in self._host:
            if key == 'planning':
                m = PlanningMetric(self.cfg, self.n_future)
            elif key == 'panoptic':
                m = PanopticMetric(self.n_classes, self.temporally_consistent, self.vehicles_id)
            else:
                m = IntersectionOverUnion(2 if key.startswith('hdmap') else self.n_classes,
                                          absent_score=1 if key.startswith('hdmap') else 0)
            self._host[key] = m.to(self.device)
        return self._host[key]

    def reset(self):
        self._packed.zero_()
        for m in self._host.values():
            m.reset()

    # ---- semantic ----
    def _semantic_native(self, seg, ped, hd):
        if not seg.is_cuda or self.n_classes > MAX_CLASSES:
            return False
        B, S, Cs, H, W = seg.shape
        planes = B * (S - self.receptive_field + 1) * (2 if ped is not None else 1) + B * len(self.elements)
        heads = [t for t in (seg, ped, hd) if t is not None]
        return (Cs <= MAX_LOGITS and (ped is None or ped.shape[2] <= MAX_LOGITS) and H <= MAX_SIDE and W <= MAX_SIDE and
                planes <= MAX_PLANES and all(t.dtype in _DTYPES and _strides_fit(t) for t in heads))

    def _update_semantic(self, output, labels):
        rf = self.receptive_field
        seg = output['segmentation'].detach()
        ped = output['pedestrian'].detach() if self.pedestrian else None
        hd = output['hdmap'].detach() if self.elements else None
        if not self._semantic_native(seg, ped, hd):
            self._host_metric('vehicle')(torch.argmax(seg, dim=2, keepdim=True)[:, rf - 1:], labels['segmentation'][:, rf - 1:])
            if ped is not None:
                self._host_metric('pedestrian')(torch.argmax(ped, dim=2, keepdim=True)[:, rf - 1:], labels['pedestrian'][:, rf - 1:])
            for i in range(len(self.elements)):
                self._host_metric(f'hdmap{i}')(torch.argmax(hd[:, 2 * i:2 * (i + 1)], dim=1, keepdim=True), labels['hdmap'][:, i:i + 1])
            return
        B, S, Cs, H, W = seg.shape
        d = _lib.EvalDims()
        d.B, d.S, d.H, d.W, d.Cs, d.n_classes, d.first = B, S, H, W, Cs, self.n_classes, rf - 1
        d.Cp = 0 if ped is None else ped.shape[2]
        d.E = len(self.elements)
        d.seg_dtype = _DTYPES[seg.dtype]
        d.seg_stride[:] = seg.stride()
        seg_label = _dense(labels['segmentation'])
        ped_label = hd_label = None
        assert tuple(seg_label.shape) == (B, S, 1, H, W), (tuple(seg_label.shape), tuple(seg.shape))
        if ped is not None:
            d.ped_dtype = _DTYPES[ped.dtype]
            d.ped_stride[:] = ped.stride()
            ped_label = _dense(labels['pedestrian'])
            assert tuple(ped.shape[:2]) + tuple(ped.shape[3:]) == (B, S, H, W) and ped_label.shape == seg_label.shape
        if hd is not None:
            d.hd_dtype = _DTYPES[hd.dtype]
            d.hd_stride[:] = hd.stride()
            hd_label = _dense(labels['hdmap'])
            assert tuple(hd.shape) == (B, 2 * d.E, H, W) and tuple(hd_label.shape) == (B, d.E, H, W)
        _check(_lib.lib().stp3_eval_semantic(ctypes.byref(d), ops._ptr(seg), ops._ptr(ped) if ped is not None else None,
                                             ops._ptr(hd) if hd is not None else None, ops._ptr(seg_label),
                                             ops._ptr(ped_label) if ped is not None else None,
                                             ops._ptr(hd_label) if hd is not None else None, ops._ptr(self.counts), ops._stream()),
               'stp3_eval_semantic')

    # ---- planning ----
    def _update_planning(self, final_traj, labels):
        rf, T = self.receptive_field, self.n_future
        gt = labels['gt_trajectory'][:, 1:]
        seg_label = labels['segmentation']
        ped_label = labels.get('pedestrian')
        B, S = seg_label.shape[:2]
        H, W = seg_label.shape[-2:]
        assert tuple(final_traj.shape[:2]) == (B, T) and tuple(gt.shape[:2]) == (B, T) and S >= rf + T
        host = self._host_metric('planning')     # (also the owner of the grid constants and the footprint)
        native = (final_traj.is_cuda and B * T <= MAX_PLAN_POINTS and H <= MAX_SIDE and W <= MAX_SIDE and
                  [H, W] == list(host.bev_dimension[:2]))
        if not native:
            truth = seg_label[:, rf:].squeeze(2).bool()
            if ped_label is not None:
                truth = truth | ped_label[:, rf:].squeeze(2).bool()
            host(final_traj.detach().float(), gt.float(), truth)
            return
        trajs, gt = final_traj.detach(), gt.detach()
        if trajs.dtype != torch.float32 or trajs.stride(-1) != 1:
            trajs = trajs.float().contiguous()
        if gt.dtype != torch.float32 or gt.stride(-1) != 1:
            gt = gt.float().contiguous()
        if self._footprint is None:
            self._footprint = host.footprint.to(device=trajs.device, dtype=torch.int32).contiguous()
            self._grid = [float(v) for v in host.dx.detach().cpu()[:2]] + [float(v) for v in host.bx.detach().cpu()[:2]]
        d = _lib.EvalPlanDims()
        d.B, d.T, d.S, d.H, d.W, d.K, d.first_future = B, T, S, H, W, self._footprint.shape[0], rf
        d.dx0, d.dx1, d.bx0, d.bx1 = self._grid
        d.traj_stride[:] = trajs.stride()[:2]
        d.gt_stride[:] = gt.stride()[:2]
        seg_label = _dense(seg_label)
        ped_label = _dense(ped_label) if ped_label is not None else None
        _check(_lib.lib().stp3_eval_planning(ctypes.byref(d), ops._ptr(trajs), ops._ptr(gt), ops._ptr(seg_label),
                                             ops._ptr(ped_label) if ped_label is not None else None, ops._ptr(self._footprint),
                                             ops._ptr(self.obj_col), ops._ptr(self.obj_box_col), ops._ptr(self.total),
                                             ops._ptr(self.L2), ops._stream()), 'stp3_eval_planning')

    # ---- panoptic ----
    def _update_panoptic(self, instance, labels):
        rf = self.receptive_field
        gt = labels['instance']
        assert instance.shape == gt.shape and gt.dim() == 4
        B, S, H, W = gt.shape
        native = (instance.is_cuda and self.n_classes == 2 and self.vehicles_id == 1 and H <= MAX_SIDE and W <= MAX_SIDE and
                  H * W < 2 ** 24 and B <= MAX_PLANES)
        if not native:
            self._host_metric('panoptic')(instance[:, rf - 1:], gt[:, rf - 1:])
            return
        wide = instance.dtype != torch.int32 or gt.dtype != torch.int32
        dtype = torch.int64 if wide else torch.int32
        pred, gt = _dense(instance.detach(), dtype), _dense(gt, dtype)
        need = ctypes.c_size_t()
        _check(_lib.lib().stp3_eval_panoptic_workspace_bytes(B, S, rf - 1, ctypes.byref(need)), 'stp3_eval_panoptic_workspace_bytes')
        if self._workspace is None or self._workspace.numel() * 4 < need.value:
            self._workspace = torch.empty((need.value + 3) // 4, dtype=torch.float32, device=pred.device)
        self.frames_shape = (B * (S - rf + 1), 4, 2)
        _check(_lib.lib().stp3_eval_panoptic(B, S, H, W, rf - 1, int(self.temporally_consistent), int(wide), ops._ptr(pred),
                                             ops._ptr(gt), ops._ptr(self._workspace), self._workspace.numel() * 4,
                                             ops._ptr(self.panoptic), ops._ptr(self.err), ops._stream()), 'stp3_eval_panoptic')

    def panoptic_frames(self):
        """float32 numpy (B (S - receptive_field + 1), 4, 2): the per-frame results of the last native panoptic update."""
        n = int(np.prod(self.frames_shape))
        return self._workspace[:n].cpu().numpy().reshape(self.frames_shape)

    @torch.no_grad()
    def update(self, output, labels, final_traj=None, instance=None):
        """``output``: the model's (or the ``InferenceEngine``'s) dict; ``labels``: ``TrainingModule.prepare_future_labels``;
        ``final_traj`` (B, N_FUTURE_FRAMES, >= 2): the planned trajectory (PLANNING.ENABLED); ``instance`` (B, S, H, W): the
        consistent ids of ``predict_instance_segmentation_and_trajectories`` (INSTANCE_SEG.ENABLED)."""
        self._update_semantic(output, labels)
        if self.instance:
            if instance is None:
                raise ValueError('INSTANCE_SEG.ENABLED: update() needs the consistent instance ids')
            self._update_panoptic(instance, labels)
        if self.planning:
            if final_traj is None:
                raise ValueError('PLANNING.ENABLED: update() needs the planned trajectory')
            self._update_planning(final_traj, labels)

    # ---- results ----
    def sync(self, group=None):
        """Sum the states over the process group (``dist_reduce_fx='sum'``), as the metric classes do."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        n = self._n_int
        ints = torch.cat([self._packed[:8 * n].view(torch.int64), self.err.to(torch.int64)])
        dist.all_reduce(ints, group=group)
        self._packed[:8 * n].view(torch.int64).copy_(ints[:n])
        self.err.copy_(ints[n:].clamp(max=1).to(torch.int32))
        floats = torch.cat([self.L2, self.panoptic.reshape(-1).double()])
        dist.all_reduce(floats, group=group)
        self.L2.copy_(floats[:self.n_future])
        self.panoptic.copy_(floats[self.n_future:].float().view(4, 2))
        for key in sorted(self._host):
            self._host[key].sync(group)

    def states(self):
        """The raw states as numpy arrays after ONE device-to-host copy of the scorer's buffer (the objects of the torch route add
        theirs): 'semantic' int64 (2 + E, n_classes, 4) -- tp, fp, fn, support of vehicle, pedestrian, hd-map elements --,
        'obj_col', 'obj_box_col' int64 (T,), 'total' int64, 'L2' float64 (T,), 'panoptic' float32 (4, n_classes) -- iou, tp, fp,
        fn --, 'err' int32 (4,).  Raises ``EvalError`` on a set error word."""
        host = self._packed.cpu()
        E, n, T = len(self.elements), self.n_classes, self.n_future
        n_counts = (2 + E) * n * 4
        ints = host[:8 * self._n_int].view(torch.int64).numpy().copy()
        at = 8 * self._n_int
        l2 = host[at:at + 8 * T].view(torch.float64).numpy().copy()
        pan = host[at + 8 * T:at + 8 * T + 32].view(torch.float32).numpy().copy().reshape(4, 2)
        err = host[at + 8 * T + 32:].view(torch.int32).numpy().copy()
        if err.any():
            raise EvalError('stp3_eval_panoptic: ' + '; '.join(PANOPTIC_ERRORS[k] for k in range(4) if err[k]))
        out = {'semantic': ints[:n_counts].reshape(2 + E, n, 4), 'obj_col': ints[n_counts:n_counts + T],
               'obj_box_col': ints[n_counts + T:n_counts + 2 * T], 'total': ints[n_counts + 2 * T], 'L2': l2, 'err': err}
        panoptic = np.zeros((4, n), np.float32)
        if n == 2:
            panoptic += pan
        for key, m in self._host.items():
            if key == 'planning':
                out['obj_col'] = out['obj_col'] + m.obj_col.cpu().numpy().round().astype(np.int64)
                out['obj_box_col'] = out['obj_box_col'] + m.obj_box_col.cpu().numpy().round().astype(np.int64)
                out['total'] = out['total'] + int(m.total)
                out['L2'] = out['L2'] + m.L2.cpu().numpy().astype(np.float64)
            elif key == 'panoptic':
                panoptic = panoptic + np.stack([getattr(m, k).cpu().numpy() for k in PanopticMetric.KEYS])
            else:
                head = {'vehicle': 0, 'pedestrian': 1}.get(key)
                head = 2 + int(key[5:]) if head is None else head
                state = np.stack([getattr(m, k).cpu().numpy() for k in IOU_KEYS], axis=1).round().astype(np.int64)
                out['semantic'][head, :state.shape[0]] += state
        out['panoptic'] = panoptic
        return out

    @staticmethod
    def _iou(counts, absent_score):
        """IntersectionOverUnion.compute of class 1, in its float32 arithmetic."""
        tp, fp, fn, sup = (torch.tensor(float(v), dtype=torch.float32) for v in counts)
        if float(sup + tp + fp) == 0:
            return torch.tensor(float(absent_score), dtype=torch.float32)
        return (tp / (tp + fp + fn).clamp(min=1)).float()

    def compute(self):
        """The dict ``evaluate.py:143-169`` prints: 0-dim float32 CPU tensors by its keys."""
        s = self.states()
        results = {'vehicle_iou': self._iou(s['semantic'][0, 1], 0)}
        if self.pedestrian:
            results['pedestrian_iou'] = self._iou(s['semantic'][1, 1], 0)
        for i, name in enumerate(self.elements):
            results[name + '_iou'] = self._iou(s['semantic'][2 + i, 1], 1)
        if self.instance:
            iou, tp, fp, fn = (torch.from_numpy(s['panoptic'][k].copy()) for k in range(4))
            ones = torch.ones_like(tp)
            denominator = torch.maximum(tp + fp / 2 + fn / 2, ones)
            for key, value in (('pq', iou / denominator), ('sq', iou / torch.maximum(tp, ones)), ('rq', tp / denominator)):
                results['vehicle_' + key] = value[1]
        if self.planning:
            total = torch.tensor(int(s['total']))
            per_step = {'obj_col': torch.from_numpy(s['obj_col']).float() / total,
                        'obj_box_col': torch.from_numpy(s['obj_box_col']).float() / total,
                        'L2': (torch.from_numpy(s['L2']) / total).float()}
            for i in range(self.n_future // 2):                  # evaluate.py:70-73: PlanningMetric(cfg, 2 (i + 1))
                for key, value in per_step.items():
                    results[f'plan_{key}_{i + 1}s'] = value[:2 * (i + 1)].mean()
        return results


def _to_device(batch, device):
    """evaluate.py's ``preprocess_batch``, except that the camera poses stay where they are: the lift builds its geometry
    constants from them on the host."""
    return {k: (v.to(device) if torch.is_tensor(v) and k not in ('intrinsics', 'extrinsics', 'future_egomotion') else v)
            for k, v in batch.items()}


def evaluate(module, loader, engine=None, device=None):
    """The loop of ``evaluate.py:76-169`` without the plotting.  ``module``: a ``TrainingModule`` (its ``cfg``, ``model`` and
    ``prepare_future_labels``); ``loader``: an iterable of batch dicts; ``engine``: an ``InferenceEngine`` of ``module.model`` to
    run the forward through (else ``module.model`` under ``no_grad`` and bf16 autocast).  Returns ``EvalScorer.compute()``."""
    from .instance import predict_instance_segmentation_and_trajectories
    cfg, model = module.cfg, module.model
    device = torch.device(device) if device is not None else next(model.parameters()).device
    scorer = EvalScorer(cfg, device)
    rf = model.receptive_field
    module.eval()
    for batch in loader:
        batch = _to_device(batch, device)
        labels = module.prepare_future_labels(batch)
        inputs = (batch['image'], batch['intrinsics'], batch['extrinsics'], batch['future_egomotion'])
        auto = torch.autocast('cuda', dtype=torch.bfloat16) if device.type == 'cuda' else contextlib.nullcontext()
        with torch.no_grad(), auto:
            output = engine(*inputs) if engine is not None else model(*inputs)
            instance = final_traj = None
            if cfg.INSTANCE_SEG.ENABLED:
                instance = predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False)
            if cfg.PLANNING.ENABLED:
                pedestrian = output['pedestrian'] if cfg.SEMANTIC_SEG.PEDESTRIAN.ENABLED else None
                occupancy, lane, drivable = ops_plan.plan_scene(output['segmentation'], pedestrian, output['hdmap'], rf)
                codes = ops_plan.command_codes(batch['command'], device)
                final_traj, _, _ = model.planning.drive(output['cam_front'], batch['sample_trajectory'][:, :, 1:].float(),
                                                        output['costvolume'][:, rf:], occupancy, lane, drivable, codes,
                                                        batch['target_point'])
            scorer.update(output, labels, final_traj, instance)
    return scorer.compute()
