"""GPU: ``stp3_amd.inference.StreamingEngine`` -- one new frame per tick, the encoder outputs of the older frames cached -- and its
kernel ``stp3_window_push`` (CPU side: tests/test_streaming_cpu.py).

KERNEL: ``ops.window_push`` against a torch roll-and-append (clone, shift, cast), EXACTLY: T in {1, 2, 3} x B in {1, 2} on frames of
(N, fH, fW, C) = (2, 3, 5, 12) (fewer vectors than one workgroup, an odd pixel count); (6, 28, 60, 64) and (6, 28, 60, 48) at B = 4,
T = 3 in one launch (more than one round of the grid); sources in bf16 and float32, NCHW and channels-last memory; three successive
pushes (shifted data is shifted again); a guard band behind every window stays untouched.

ENGINE.  THE ORACLE IS PARENT CODE: the plain ``model.eval()(window, ...)`` under bf16 autocast with ``model.encoder`` wrapped in
a shim that calls the real encoder once per frame -- T groups of B * N images, index order (b, t, n) -- and reassembles both
outputs.  The encoder's kernels size their grids and partial sums from the problem, so that is the plain forward at the shapes
the streaming tick runs; every non-None output of ``StreamingEngine.step`` must equal it BIT FOR BIT (``depth_prediction`` after
``.float()``: the engine returns a view of its float32 cache).  Equality with the full-window forward is NOT asserted: the
largest absolute difference to the full-window ``InferenceEngine`` is printed.
Perception.yml at B = 1, T = 3 over a 6-frame sequence with poses per window (ticks 1-2 return None, ticks 3-6 equal the oracle on
windows [0..2] .. [3..5]; three replays with the static image handed back are identical; the caller's image is never written);
the same at B = 2 for 4 ticks (the sample stride of the caches); a Prediction.yml-shaped model at the size
tests/test_prediction_gpu.py uses, two full windows; ``reset()`` in the middle of a sequence (the next T - 1 steps return None, the
step after equals the oracle on the new frames alone); ``load_state_dict`` of perturbed weights and running statistics (stale
until ``refresh()``, equal after it); wrong shapes, a model in training mode and a model on the CPU raise ``Stp3HipError``."""
import contextlib

import pytest
import torch
import torch.nn as nn

from stp3_amd import synthetic
from stp3_amd.config import perception_cfg
from tests import helpers as H
from tests import test_inference_gpu as TI

pytestmark = pytest.mark.gpu
POSES = TI.POSES


# ---- the kernel ----
def _roll_and_append(window, new):
    """clone, shift, cast: window (B,T,NPIX,C) float32, new (B*N,C,fH,fW) -> the window one frame later."""
    b, t, npix, c = window.shape
    frame = new.float().reshape(b, -1, c, new.shape[2] * new.shape[3]).permute(0, 1, 3, 2).reshape(b, 1, npix, c)
    out = window.clone()
    out[:, :-1] = window[:, 1:]
    out[:, -1:] = frame
    return out


def _source(shape, dtype, layout, gen):
    v = torch.randn(shape, generator=gen, device='cuda').to(dtype)
    return v.contiguous(memory_format=torch.channels_last) if layout == 'nhwc' else v.contiguous()


GUARD = 256


def _push_case(b, t, n, fh, fw, channels, dtype, layout, seed):
    from stp3_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(seed)
    npix = n * fh * fw
    bufs, windows, wants = [], [], []
    for c in channels:
        size = b * t * npix * c
        buf = torch.cat([torch.randn(size, generator=gen, device='cuda'), torch.full((GUARD,), -7.5, device='cuda')])
        bufs.append(buf)
        windows.append(buf[:size].view(b, t, npix, c))
        wants.append(windows[-1].clone())
    for k in range(3):
        news = [_source((b * n, c, fh, fw), dtype, layout, gen) for c in channels]
        assert all(new.stride(1) == (1 if layout == 'nhwc' else fh * fw) for new in news)
        ops.window_push(list(zip(news, windows)))
        wants = [_roll_and_append(want, new) for want, new in zip(wants, news)]
        for j, (buf, window, want) in enumerate(zip(bufs, windows, wants)):
            assert torch.equal(window.view(torch.int32), want.view(torch.int32)), (b, t, channels[j], k)
            assert bool((buf[window.numel():] == -7.5).all()), (b, t, channels[j], k)      # the guard band is untouched


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_window_push_small_frames(dtype, layout):
    for b in (1, 2):
        for t in (1, 2, 3):
            _push_case(b, t, 2, 3, 5, (12,), dtype, layout, seed=10 * b + t)
            _push_case(b, t, 2, 3, 5, (12, 8), dtype, layout, seed=100 + 10 * b + t)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_window_push_more_than_one_grid_round(dtype, layout):
    """B = 4, T = 3, both caches of Perception.yml in one launch: 645 120 + 483 840 vectors on a grid of 2 x 1 024 workgroups."""
    _push_case(4, 3, 6, 28, 60, (64, 48), dtype, layout, seed=5)


def test_window_push_rejects_what_the_kernel_does_not_take():
    from stp3_amd import ops
    from stp3_amd._lib import Stp3HipError
    window = torch.zeros(1, 3, 30, 12, device='cuda')
    with pytest.raises(Stp3HipError):
        ops.window_push([(torch.zeros(2, 10, 3, 5, device='cuda'), torch.zeros(1, 3, 30, 10, device='cuda'))])    # channels % 4
    with pytest.raises(Stp3HipError):
        ops.window_push([(torch.zeros(2, 12, 3, 5, device='cuda', dtype=torch.float16), window)])
    with pytest.raises(Stp3HipError):
        ops.window_push([(torch.zeros(2, 12, 3, 4, device='cuda'), window)])                                          # another frame size
    with pytest.raises(Stp3HipError):
        ops.window_push([(torch.zeros(2, 12, 15, device='cuda'), window)])                                            # a frame of another rank
    with pytest.raises(Stp3HipError):
        ops.window_push([(torch.zeros(2, 12, 3, 5), window)])                                                         # a CPU tensor
    assert not window.any()


# ---- the engine ----
@contextlib.contextmanager
def per_frame_encoder(model, b, n):
    """``model.encoder`` split per frame: the (B*T*N, 3, H, W) input in T groups of B*N images -- index order (b, t, n) -- through the
    real encoder, both outputs reassembled in the original order."""
    real = model.encoder

    class Shim(nn.Module):
        def forward(self, x):
            t = x.shape[0] // (b * n)
            frames = x.view(b, t, n, *x.shape[1:])
            feats, depths = [], []
            for k in range(t):
                feat, depth = real(frames[:, k].reshape(b * n, *x.shape[1:]))
                feats.append(feat.view(b, n, *feat.shape[1:]))
                depths.append(depth.view(b, n, *depth.shape[1:]))
            feat, depth = torch.stack(feats, dim=1), torch.stack(depths, dim=1)
            return feat.reshape(b * t * n, *feat.shape[3:]), depth.reshape(b * t * n, *depth.shape[3:])

    model.encoder = Shim()
    try:
        yield
    finally:
        model.encoder = real


def _oracle(model, window):
    b, _, n = window['image'].shape[:3]
    with per_frame_encoder(model, b, n):
        return TI._plain(model, window)


def _mismatches(got, want):
    """tests/test_inference_gpu._mismatches with ``depth_prediction`` widened on both sides."""
    assert got is not None
    wide = lambda out: {k: (v.float() if k == 'depth_prediction' and v is not None else v) for k, v in out.items()}   # noqa: E731
    return TI._mismatches(wide(got), wide(want))


def _sequence(batch, frames, seq=3, first_seed=40, **kw):
    """(images (B, frames, N, 3, H, W) on the host, one pose dict per window of 3 frames): synthetic.make_batch frames, every
    window with camera and ego poses of its own (past frames are re-aligned to the new present pose on every tick)."""
    parts = [synthetic.make_batch(batch=batch, seq=3, seed=first_seed + i, with_labels=False)['image'] for i in range((frames + 2) // 3)]
    images = torch.cat(parts, dim=1)[:, :frames].contiguous()
    poses = []
    for k in range(frames - 2):
        rig = synthetic.make_batch(batch=batch, seq=seq, seed=first_seed + 50 + k, with_images=False, with_labels=False, **kw)
        poses.append({key: rig[key] for key in POSES})
    assert not torch.equal(poses[0]['extrinsics'], poses[-1]['extrinsics']) or frames == 3
    return images, poses


def _window(images, poses, k):
    return {'image': images[:, k:k + 3], **poses[k]}


def _run(engine, images, poses, ticks):
    """Push frames 0 .. ticks-1; per tick the (cloned) outputs or None."""
    outs = []
    for i in range(ticks):
        k = max(i - 2, 0)
        outs.append(engine.step(images[:, i].cuda(), *[poses[k][key] for key in POSES], clone=True))
    return outs


@pytest.fixture(scope='module')
def model():
    return TI._perception_model()


@pytest.fixture(scope='module')
def perception_b1(model):
    """Perception.yml, B = 1, T = 3, a 6-frame sequence: (images, poses, oracle outputs of windows 0..3, engine, outputs of ticks
    1..6)."""
    from stp3_amd.inference import StreamingEngine
    images, poses = _sequence(1, 6)
    oracle = [_oracle(model, _window(images, poses, k)) for k in range(4)]
    example = _window(images, poses, 0)
    example['image'] = example['image'].cuda()
    kept = example['image'].clone()
    engine = StreamingEngine(model, example, autocast_dtype=torch.bfloat16)
    assert engine.filled == 0 and torch.equal(example['image'], kept)
    ticks = _run(engine, images, poses, 6)
    return images, poses, oracle, engine, ticks


def test_perception_b1_ticks_equal_the_per_frame_oracle(model, perception_b1):
    from stp3_amd.inference import InferenceEngine
    images, poses, oracle, engine, ticks = perception_b1
    assert ticks[0] is None and ticks[1] is None                                        # the window is not full yet
    assert engine.filled == 3 and engine.replays == 6
    for k in range(4):
        bad = _mismatches(ticks[k + 2], oracle[k])
        print(f'[streaming] Perception B=1, tick {k + 3} (window {k}..{k + 2}): mismatching elements', bad)
        assert not bad, (k, bad)
    assert _mismatches(ticks[3], ticks[2]), 'two windows gave the same outputs'
    got = ticks[5]
    assert got['depth_prediction'].shape == oracle[3]['depth_prediction'].shape
    # against the FULL-WINDOW engine: printed, not asserted (B N and B T N images may round differently in the encoder)
    last = _window(images, poses, 3)
    full = InferenceEngine(model, last, autocast_dtype=torch.bfloat16)(*TI._inputs(last), clone=True)
    for key in sorted(got):
        if got[key] is not None:
            diff = (got[key].float() - full[key].float()).abs().max().item()
            print(f'[streaming] {key}: largest |streaming - full-window engine| = {diff:.3e} '
                  f'(largest |full-window| {full[key].float().abs().max().item():.3e})')


def test_replays_with_the_static_image_are_identical(perception_b1):
    images, poses, oracle, engine, ticks = perception_b1
    pose = [poses[3][key] for key in POSES]
    mine = images[:, 5].cuda()
    kept = mine.clone()
    first = engine.step(mine, *pose, clone=True)
    assert torch.equal(mine, kept) and engine.image.data_ptr() != mine.data_ptr()       # the caller's image is never written
    # the window now holds frames 4, 5, 5: handing the static buffer back pushes frame 5 again -- from the second replay on the
    # window is 5, 5, 5 and the outputs repeat
    engine.step(engine.image, *pose)
    base = engine.step(engine.image, *pose, clone=True)
    for i in range(3):
        again = engine.step(engine.image, *pose)
        assert all(again[k] is engine.outputs[k] for k in again)                       # the static tensors
        bad = _mismatches(again, base)
        assert not bad, (i, bad)
    assert _mismatches(base, first)
    assert torch.equal(engine.image, kept.view(engine.image.shape)) and torch.equal(mine, kept)
    # (B, 1, N, 3, H, W) is taken as well
    assert not _mismatches(engine.step(mine[:, None], *pose), base)


def test_perception_b2_covers_the_sample_stride(model):
    from stp3_amd.inference import StreamingEngine
    images, poses = _sequence(2, 4, first_seed=60)
    oracle = [_oracle(model, _window(images, poses, k)) for k in range(2)]
    engine = StreamingEngine(model, _window(images, poses, 0), autocast_dtype=torch.bfloat16)
    ticks = _run(engine, images, poses, 4)
    assert ticks[0] is None and ticks[1] is None
    for k in range(2):
        bad = _mismatches(ticks[k + 2], oracle[k])
        print(f'[streaming] Perception B=2, tick {k + 3}: mismatching elements', bad)
        assert not bad, (k, bad)
    # the samples differ: a cache indexed with the wrong sample stride could not have passed
    assert not torch.equal(ticks[3]['segmentation'][0], ticks[3]['segmentation'][1])


def test_reset_in_the_middle_of_a_sequence(model, perception_b1):
    images, poses, oracle, engine, ticks = perception_b1
    assert engine.filled == 3
    graph = engine.graph
    engine.reset()
    assert engine.filled == 0 and not engine.feat_window.any() and not engine.logits_window.any()
    # frames 1, 2, 3 alone: window 1 of the sequence
    outs = [engine.step(images[:, i].cuda(), *[poses[1][key] for key in POSES], clone=True) for i in (1, 2, 3)]
    assert outs[0] is None and outs[1] is None and engine.filled == 3
    bad = _mismatches(outs[2], oracle[1])
    print('[streaming] after reset(): mismatching elements', bad)
    assert not bad, bad
    assert engine.graph is graph                                                        # not captured again


def test_refresh_after_load_state_dict(model, perception_b1):
    """As tests/test_inference_gpu._check_refresh: the oracle on the changed weights runs LAST (an eager forward rewrites the bf16
    shadows by itself and would hide a ``refresh()`` that forgot them)."""
    images, poses, oracle, engine, ticks = perception_b1
    window = _window(images, poses, 2)

    def run():
        engine.reset()
        return _run(engine, images[:, 2:5], [poses[2]], 3)[2]

    assert not _mismatches(run(), oracle[2])
    original = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator(device='cuda').manual_seed(5)
    changed = {}
    for k, v in original.items():
        if not v.is_floating_point():
            changed[k] = v
        elif k.endswith('running_var'):
            changed[k] = v * (1.0 + 0.2 * torch.rand(v.shape, generator=g, device=v.device))
        else:
            changed[k] = v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g, device=v.device)
    try:
        model.load_state_dict(changed)
        stale = run()                                                                   # no eager forward yet
        engine.refresh()
        fresh = run()
        want = _oracle(model, window)
        stale_bad = _mismatches(stale, want)
        print('[streaming] without refresh(): entries that differ from the oracle', sorted(stale_bad))
        assert stale_bad, 'the engine followed a weight change without refresh()'
        bad = _mismatches(fresh, want)
        print('[streaming] after refresh(): mismatching elements', bad)
        assert not bad, bad
        assert _mismatches(fresh, oracle[2]), 'perturbed weights gave the original outputs'
    finally:
        model.load_state_dict(original)
        engine.refresh()
    assert not _mismatches(run(), oracle[2])


def test_error_paths(model, perception_b1):
    from stp3_amd._lib import Stp3HipError
    from stp3_amd.inference import StreamingEngine
    from stp3_amd.models.stp3 import STP3
    images, poses, oracle, engine, ticks = perception_b1
    pose = [poses[0][key] for key in POSES]
    filled = engine.filled
    with pytest.raises(Stp3HipError, match='shape'):
        engine.step(images[:, :3].cuda(), *pose)                                        # a whole window instead of the newest frame
    with pytest.raises(Stp3HipError, match='shape'):
        engine.step(images[:, 0, :, :, :-8].cuda(), *pose)
    two = synthetic.make_batch(batch=2, seq=3, seed=7, with_images=False, with_labels=False)
    with pytest.raises(Stp3HipError, match='shape'):
        engine.step(images[:, 0].cuda(), *[two[key] for key in POSES])
    assert engine.filled == filled                                                      # a rejected step pushes nothing
    example = _window(images, poses, 0)
    model.train()
    try:
        with pytest.raises(Stp3HipError, match='training'):
            engine.step(images[:, 0].cuda(), *pose)
        with pytest.raises(Stp3HipError, match='training'):
            StreamingEngine(model, example)
    finally:
        model.eval()
    with pytest.raises(Stp3HipError, match='CPU'):
        StreamingEngine(STP3(perception_cfg()).eval(), example)
    with pytest.raises(Stp3HipError, match='shape'):
        StreamingEngine(model, {**example, 'image': example['image'][:, :2]})           # fewer frames than the receptive field
    # the engine is unharmed
    engine.reset()
    assert not _mismatches(_run(engine, images, poses, 3)[2], oracle[0])


def test_prediction_two_windows_equal_the_oracle():
    """A Prediction.yml-shaped model (N_FUTURE_FRAMES = 4, GAUSSIAN present distribution) at the size
    tests/test_prediction_gpu.py uses, B = 1: the poses carry 7 frames as ``InferenceEngine``'s example does."""
    from stp3_amd.inference import StreamingEngine
    from stp3_amd.models.stp3 import STP3
    from stp3_amd.utils import to_channels_last
    from tests.test_prediction_cpu import PREDICTION
    model = to_channels_last(H.fill_deterministic(STP3(perception_cfg(**PREDICTION))).eval().cuda())
    images, poses = _sequence(1, 4, seq=7, first_seed=80)
    oracle = [_oracle(model, _window(images, poses, k)) for k in range(2)]
    engine = StreamingEngine(model, _window(images, poses, 0), autocast_dtype=torch.bfloat16)
    ticks = _run(engine, images, poses, 4)
    assert ticks[0] is None and ticks[1] is None
    assert ticks[2]['segmentation'].shape[:2] == (1, 7)
    for k in range(2):
        bad = _mismatches(ticks[k + 2], oracle[k])
        print(f'[streaming] Prediction B=1, tick {k + 3}: entries', sorted(key for key, v in ticks[k + 2].items() if v is not None),
              'mismatching elements', bad)
        assert not bad, (k, bad)
    assert engine.gates.entries, 'the GRU cells of the prediction stage did not take the engine\'s gate weights'
