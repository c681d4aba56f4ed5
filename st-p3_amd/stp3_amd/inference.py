"""Inference: the eval forward of ``STP3`` as ONE hipGraph of fused kernels.

What the reference runs per validation sample (evaluate.py:76-91, batch 1 over the 6 019 samples) and per simulator tick
(carla_agent.py:445) is ``model(image, intrinsics, extrinsics, future_egomotion)`` in eval mode.  Launched eagerly that forward
is ~500 kernel launches whose GPU time at batch 1 is a fraction of the host time it takes to issue them, and every
conv -> BatchNorm -> activation layer makes two full passes over its tensor.  ``InferenceEngine`` removes both:

    engine = InferenceEngine(model, example_batch, autocast_dtype=torch.bfloat16)     # model: STP3, eval mode, on the GPU
    out = engine(image, intrinsics, extrinsics, future_egomotion)                     # the dict STP3.forward returns

* construction allocates static input buffers (the example images are COPIED: the engine never writes the caller's tensor),
  prepares the voxel-pool plan (``STP3.prepare_plan``: host pose mathematics + the index kernels), runs a few warm-up forwards under ``torch.no_grad()`` and autocast and captures ONE single-stream graph
  of the forward (as ``graph.GraphedTrainStep`` does for the training step; with a prepared plan the forward forks no stream);
* ``engine(...)`` copies the images into the static buffer (skipped when the caller hands that buffer, ``engine.image``, back),
  rebuilds the plan and the ego-motion vector IN PLACE, replays, and returns the static output tensors.  THE OUTPUTS ARE
  OVERWRITTEN BY THE NEXT CALL; ``clone=True`` returns copies;
* inside the engine (its warm-up and capture, ``layers.fused.eval_fusion``) a layer whose BatchNorm runs on its running
  statistics takes the fused eval operators -- ``ops.conv2d_affine`` / ``ops.depthwise_conv2d_affine`` / ``ops.small_linear_affine``: the BatchNorm, the
  activation and the skip in the convolution's epilogue, constants from ``EvalCoefficients`` -- which keep the rounding points
  of the two operators they replace: the engine's outputs are BIT-EQUAL to ``model.eval()(...)`` under the same autocast
  (tests/test_inference_gpu.py).  Outside the engine nothing changes.  Without bf16 autocast (a float32 engine) the plain
  operators are captured as they are;
* ``refresh()`` after the caller changed parameters or running statistics (``load_state_dict`` of another checkpoint): the bf16
  weight shadows, the merged gate weights of the GRU cells (``ops_pred.EngineGateWeights``: buffers the engine owns) and the
  coefficient arena are rewritten in place -- the graph is not captured again;
* a shape other than the captured one, a model in training mode and a model on the CPU raise ``Stp3HipError``.

STREAMING.  The simulator tick is a sliding window (carla_agent.py:408-432): the newest camera frame joins a buffer and the model
is handed all T = ``receptive_field`` frames again, T - 1 of which it encoded on the tick before.  In eval mode the image encoder
couples no two images (BatchNorm on running statistics, squeeze-excite and the ASPP pooling per image, drop-connect off), while
everything behind it depends on the whole window (past frames are re-aligned to the new present pose every tick).
``StreamingEngine`` therefore caches exactly the encoder's two outputs, in the pixel-major float32 layout the voxel pool reads:

    engine = StreamingEngine(model, example_batch, autocast_dtype=torch.bfloat16)     # example: the shapes of InferenceEngine's
    out = engine.step(image_new, intrinsics, extrinsics, future_egomotion)            # (B, N, 3, H, W) + the WINDOW's poses

* ``step`` copies the B * N newest images (a third of the window's), rebuilds the plan and the ego-motion vector in place and
  replays ONE single-stream graph: the encoder on B * N images, ``ops.window_push`` (one launch: both caches advance by a frame
  in place), the voxel pool on the caches, then ``STP3.forward_from_bev`` -- the plain forward's own tail;
* it returns None while fewer than T frames were pushed since construction or ``reset()`` (the reference agent only buffers
  during its first ticks as well), then the static output dict (``clone=True``: copies).  ``depth_prediction`` is a view of the
  float32 logits cache (the plain forward returns the autocast dtype; equal after ``.float()``);
* the encoder's kernels size their grids and partial sums from the problem, so B * N images and B * T * N images may round
  differently: the outputs are BIT-EQUAL to ``model.eval()(...)`` with the encoder called per frame (B * N images at a time),
  not to the full-window forward (tests/test_streaming_gpu.py prints the difference to the latter);
* ``reset()`` zero-fills the caches and starts a new sequence, ``refresh()`` is ``InferenceEngine.refresh``; neither captures again.

Any configuration whose eval forward is free of host synchronisation can be captured: Perception.yml (N_FUTURE_FRAMES = 0) and
the prediction stage (eval mode samples with zero noise, models/stp3.py ``distribution_forward``).  The planner call that
follows the forward stays with the caller, as in evaluate.py:121-132 (or ``ops_plan.plan_scene`` + ``Planning.drive``): captured behind
the forward it measured no faster per tick than issued eagerly while the replay runs (profiles/plan_engine_timing.txt).
"""
import contextlib

import torch
import torch.nn as nn

from . import _lib, capture, ops, ops_pred
from ._lib import Stp3HipError
from .layers import fused


def _pad8(c):
    return (int(c) + 7) // 8 * 8


class EvalCoefficients:
    """The arena of per-channel constants of every eval BatchNorm of ``model``: [scale | shift][lanes] float32 per layer,
    lanes = channels rounded up to 8 (zeros beyond the channels), written by ONE launch of stp3_bn_eval_coefs from the
    running statistics / weight / bias as they are in device memory -- at construction and in ``refresh()``, never per forward.
    The addresses are static: a captured graph reads the arena."""

    def __init__(self, model, device):
        self.device = torch.device(device)
        self.layers = [m for m in model.modules()
                       if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats and self._takes(m)]
        self.offsets, total = {}, 0
        for m in self.layers:
            self.offsets[id(m)] = total
            total += 2 * _pad8(m.num_features)
        self.arena = torch.zeros(max(total, 1), dtype=torch.float32, device=self.device)
        self.table, self.rows, self.total_blocks, self.pointers = None, 0, 0, None
        self.refresh()

    def _takes(self, m):
        tensors = [m.running_mean, m.running_var] + [t for t in (m.weight, m.bias) if t is not None]
        return all(t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device for t in tensors)

    def _pointers(self):
        return tuple((m.running_mean.data_ptr(), m.running_var.data_ptr(), 0 if m.weight is None else m.weight.data_ptr(),
                      0 if m.bias is None else m.bias.data_ptr()) for m in self.layers)

    def _build_table(self):
        arr = (_lib.BnCoefEntry * max(len(self.layers), 1))()
        block = 0
        for rec, m, ptrs in zip(arr, self.layers, self._pointers()):
            rec.running_mean, rec.running_var, rec.gamma, rec.beta = (p or None for p in ptrs)
            rec.out = self.arena.data_ptr() + 4 * self.offsets[id(m)]
            rec.first_block = block
            rec.channels, rec.lanes, rec.eps = m.num_features, _pad8(m.num_features), float(m.eps)
            block += (_pad8(m.num_features) + 255) // 256
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.rows, self.total_blocks, self.pointers = len(self.layers), block, self._pointers()

    def refresh(self):
        """Rewrite the arena from the BatchNorm buffers and parameters: one launch."""
        if not self.layers:
            return
        if not all(self._takes(m) for m in self.layers):
            raise Stp3HipError('EvalCoefficients.refresh: a BatchNorm layer changed its dtype / device since the engine was built')
        if self.pointers != self._pointers():          # (a buffer was replaced, not overwritten: the arena's addresses stay)
            self._build_table()
        guard = torch.cuda.device(self.device) if self.device.type == 'cuda' else contextlib.nullcontext()
        with guard:
            ops.bn_eval_coefs(self.table, self.rows, self.total_blocks)

    def lookup(self, bn):
        """[scale | shift][lanes] of ``bn`` (a view of the arena), or None for a layer the arena does not hold."""
        off = self.offsets.get(id(bn))
        if off is None:
            return None
        return self.arena[off:off + 2 * _pad8(bn.num_features)]

    def scope(self):
        return fused.eval_fusion(self)


_INPUTS = ('image', 'intrinsics', 'extrinsics', 'future_egomotion')


class InferenceEngine:
    """See the module docstring.  ``example_batch``: a dict with 'image', 'intrinsics', 'extrinsics', 'future_egomotion' (or
    those four in a tuple) of the shapes every later call will have."""

    def __init__(self, model, example_batch, autocast_dtype=torch.bfloat16, warmup=3):
        if isinstance(example_batch, dict):
            example_batch = tuple(example_batch[k] for k in _INPUTS)
        image, intrinsics, extrinsics, ego = example_batch
        self._check_model(model)
        dev = next(model.parameters()).device
        self.model, self.device, self.autocast_dtype = model, dev, autocast_dtype
        # static inputs: the images on the device; the camera poses stay on the host (ops.lift_matrices builds the bit-exact
        # geometry constants there, and with a prepared plan the forward only slices them); the ego-motion vectors, which the
        # temporal model reads, in a device buffer refreshed per call
        # (always a buffer of the engine's own: every later call overwrites it, and the caller's example is the caller's)
        self.image = image.to(dev, copy=True)
        self.poses = (intrinsics, extrinsics)
        self.ego = ego.detach().float().to(dev)
        self._ego_upload = ops.PinnedUpload(self.ego)
        self.shapes = tuple(tuple(t.shape) for t in example_batch)
        self.plan = model.prepare_plan(intrinsics, extrinsics, ego, dev)
        model.prebuilt_plan = None
        # the fused eval operators serve the bf16 path; a float32 engine captures the plain operators
        self.coefs = EvalCoefficients(model, dev) if autocast_dtype == torch.bfloat16 else None
        # the merged gate weights of the prediction stage's GRU cells (bf16 path only): buffers refresh() rewrites in place
        self.gates = ops_pred.EngineGateWeights()
        self.stream = capture.warm_up(self._forward, dev, warmup)
        self.graph, self.outputs = capture.capture(self._forward, self.stream, dev)
        self.replays = 0

    @staticmethod
    def _check_model(model, deep=True):
        param = next(model.parameters(), None)
        if param is None or param.device.type != 'cuda':
            raise Stp3HipError('InferenceEngine: the model is on the CPU (the engine captures a hipGraph of the GPU forward)')
        if model.training or (deep and any(m.training for m in model.modules())):
            raise Stp3HipError('InferenceEngine: the model is in training mode (call model.eval() first)')

    def _forward(self):
        model = self.model
        model.prebuilt_plan = self.plan                        # the forward pools with the prepared plan: no host work
        auto = (torch.autocast('cuda', dtype=self.autocast_dtype) if self.autocast_dtype is not None
                else contextlib.nullcontext())
        scope = fused.eval_fusion(self.coefs, self.gates) if self.coefs is not None else contextlib.nullcontext()
        try:
            with torch.no_grad(), auto, scope:
                return model(self.image, self.poses[0], self.poses[1], self.ego)
        finally:
            model.prebuilt_plan = None

    def refresh(self):
        """Call after the parameters or running statistics changed (e.g. ``load_state_dict``): rewrites the bf16 weight shadows,
        the merged gate weights of the GRU cells (cut from those shadows) and the coefficient arena in place.  The graph is
        not captured again."""
        self._check_model(self.model)
        with torch.cuda.device(self.device):
            ops.invalidate_weight_cache()
            self.gates.refresh()
            if self.coefs is not None:
                self.coefs.refresh()

    def __call__(self, image, intrinsics, extrinsics, future_egomotion, clone=False):
        """One forward.  Returns the dict ``STP3.forward`` returns; its tensors are the engine's static outputs, OVERWRITTEN BY
        THE NEXT CALL -- ``clone=True`` returns copies."""
        self._check_model(self.model, deep=False)
        shapes = tuple(tuple(t.shape) for t in (image, intrinsics, extrinsics, future_egomotion))
        if shapes != self.shapes:
            raise Stp3HipError(f'InferenceEngine: input shapes {shapes} differ from the captured {self.shapes}')
        if image is not self.image:
            self.image.copy_(image, non_blocking=True)
        self.poses = (intrinsics, extrinsics)
        self.plan = self.model.prepare_plan(intrinsics, extrinsics, future_egomotion, self.device, out=self.plan)
        self.model.prebuilt_plan = None
        self._ego_upload(future_egomotion.detach().float().cpu())
        self.graph.replay()
        self.replays += 1
        if clone:
            return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.outputs.items()}
        return self.outputs


def streaming_tick(model, image, feat_window, logits_window, plan, ego):
    """What ``StreamingEngine`` captures: the encoder on the newest frame's images (B, N, 3, H, W) -> ``ops.window_push`` -> the
    voxel pool on the caches -> the plain forward's tail.  The caller provides ``torch.no_grad()``, the autocast and the
    fused-eval scope."""
    d = plan.dims
    feat, depth = model.encoder(image.view(d.B * d.N, *image.shape[2:]))
    ops.window_push([(feat, feat_window), (depth, logits_window)])
    bev = ops.lift_splat_pm(feat_window, logits_window, plan, model.discount, model.bev_channels_last, model._bev_dtype())
    # the two outputs the plain forward takes from the encoder's tensors: the present frame's front camera, and the depth
    # logits of the whole window -- (B, T, N, D, fH, fW) over the cache's [B][T][N][fH][fW][D] memory
    cam_front = model._cam_front(feat.view(d.B, 1, d.N, *feat.shape[1:]))
    depth = logits_window.view(d.B, d.T, d.N, d.fH, d.fW, d.D).permute(0, 1, 2, 5, 3, 4)
    return model.forward_from_bev(bev, depth, cam_front, ego)


class StreamingEngine:
    """See the module docstring (STREAMING).  ``example_batch`` as for ``InferenceEngine``: its image has at least
    ``model.receptive_field`` frames, of which the engine takes B, N and the image size; its poses have the shapes every later
    ``step`` hands in."""

    def __init__(self, model, example_batch, autocast_dtype=torch.bfloat16, warmup=3):
        if isinstance(example_batch, dict):
            example_batch = tuple(example_batch[k] for k in _INPUTS)
        image, intrinsics, extrinsics, ego = example_batch
        self._check_model(model)
        dev = next(model.parameters()).device
        self.model, self.device, self.autocast_dtype = model, dev, autocast_dtype
        t = self.frames = int(model.receptive_field)
        if image.dim() != 6 or image.shape[1] < t:
            raise Stp3HipError(f'StreamingEngine: the example image has shape {tuple(image.shape)}; (B, S >= {t}, N, 3, H, W) expected')
        b, _, n, c, h, w = image.shape
        # static inputs: the NEWEST frame's images on the device (a buffer of the engine's own); the window's camera poses stay
        # on the host, its ego-motion vectors go to a device buffer refreshed per step -- as in InferenceEngine
        self.image = torch.empty((b, n, c, h, w), dtype=image.dtype, device=dev)
        self.image.copy_(image[:, t - 1])
        self.ego = ego.detach().float().to(dev)
        self._ego_upload = ops.PinnedUpload(self.ego)
        self.pose_shapes = tuple(tuple(p.shape) for p in (intrinsics, extrinsics, ego))
        self.plan = model.prepare_plan(intrinsics, extrinsics, ego, dev)
        model.prebuilt_plan = None
        # the window caches: what stp3_lift_splat_fwd reads, [B][T][N fH fW][C | D] float32
        d = self.plan.dims
        self.feat_window = torch.zeros((b, t, d.NPIX, d.C), dtype=torch.float32, device=dev)
        self.logits_window = torch.zeros((b, t, d.NPIX, d.D), dtype=torch.float32, device=dev)
        self.coefs = EvalCoefficients(model, dev) if autocast_dtype == torch.bfloat16 else None
        self.gates = ops_pred.EngineGateWeights()
        self.stream = capture.warm_up(self._tick, dev, warmup)
        self.graph, self.outputs = capture.capture(self._tick, self.stream, dev)
        self.replays = 0
        self.filled = 0
        self.reset()                                           # (the warm-up ticks pushed the example frame)

    def _tick(self):
        auto = (torch.autocast('cuda', dtype=self.autocast_dtype) if self.autocast_dtype is not None
                else contextlib.nullcontext())
        scope = fused.eval_fusion(self.coefs, self.gates) if self.coefs is not None else contextlib.nullcontext()
        with torch.no_grad(), auto, scope:
            return streaming_tick(self.model, self.image, self.feat_window, self.logits_window, self.plan, self.ego)

    def reset(self):
        """Start a new sequence: zero-fill the caches; the next T - 1 steps return None.  The graph is not captured again."""
        self.feat_window.zero_()
        self.logits_window.zero_()
        self.filled = 0

    _check_model = staticmethod(InferenceEngine._check_model)
    refresh = InferenceEngine.refresh                          # (reads self.model / device / gates / coefs: the same fields)

    def step(self, image_new, intrinsics, extrinsics, future_egomotion, clone=False):
        """One tick.  ``image_new``: the newest frame, (B, N, 3, H, W) or (B, 1, N, 3, H, W); the three pose tensors describe the
        WHOLE current window (shapes of the example).  Returns None until T frames have been pushed, then the dict
        ``STP3.forward`` returns: the engine's static outputs, OVERWRITTEN BY THE NEXT STEP -- ``clone=True`` returns copies."""
        self._check_model(self.model, deep=False)
        if image_new is not self.image:
            shape = tuple(image_new.shape)
            if shape != tuple(self.image.shape) and shape != (self.image.shape[0], 1) + tuple(self.image.shape[1:]):
                raise Stp3HipError(f'StreamingEngine: image shape {shape} differs from the captured {tuple(self.image.shape)}')
        shapes = tuple(tuple(p.shape) for p in (intrinsics, extrinsics, future_egomotion))
        if shapes != self.pose_shapes:
            raise Stp3HipError(f'StreamingEngine: pose shapes {shapes} differ from the captured {self.pose_shapes}')
        if image_new is not self.image:
            self.image.copy_(image_new.reshape(self.image.shape), non_blocking=True)
        self.plan = self.model.prepare_plan(intrinsics, extrinsics, future_egomotion, self.device, out=self.plan)
        self.model.prebuilt_plan = None
        self._ego_upload(future_egomotion.detach().float().cpu())
        self.graph.replay()
        self.replays += 1
        self.filled = min(self.filled + 1, self.frames)
        if self.filled < self.frames:
            return None
        if clone:
            return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.outputs.items()}
        return self.outputs
