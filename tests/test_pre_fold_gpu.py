"""GPU: conv -> BatchNorm -> ReLU -> 1x1 conv chains with the BatchNorm apply pass folded into the 1x1 layer's operand load
(ops_fused.PRE_FOLD, ``_ConvBnActConv1x1``) against the same modules with the switch off (the separate operators).

The fold evaluates the same expressions at the same rounding points on the same kernels' tiles, so everything is compared with
``torch.equal``: every output, the input gradient, every parameter gradient (the flat gradient buckets: the direct-bucket,
deferred-partials and assembled-weight routes of the weight gradients are all in play) and every buffer (the BatchNorm
running statistics and batch counters), over two passes with a parameter update in between.

  decoder heads   Decoder at b = 1, s = 2, 64 channels, 16 x 16, every head enabled: the merged 3x3 -> BatchNorm -> ReLU ->
                  block-diagonal 1x1 and the hd-map head on the present frame
  hd-map alone    the same decoder with only the hd-map head enabled: no merge, both heads through ``run_fused``
  DeepLabHead     (16, 8, hidden 16) at N = 2, 40 x 40 (dilations 12 / 24 / 36 < 40: the one-buffer ASPP route): four branches
                  -> one table -> projection, and the 3x3 -> BatchNorm -> ReLU -> 1x1 tail"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

ALL = {'perceive_hdmap': True, 'predict_pedestrian': True, 'predict_instance': True, 'predict_future_flow': True, 'planning': True}
HDMAP = {'perceive_hdmap': True, 'predict_pedestrian': False, 'predict_instance': False, 'predict_future_flow': False,
         'planning': False}


def _decoder(gate):
    from stp3_amd.models.decoder import Decoder
    return Decoder(64, 2, 2, 2, gate), (1, 2, 64, 16, 16)


def _deeplab():
    from stp3_amd.layers.convolutions import DeepLabHead
    return DeepLabHead(16, 8, hidden_channel=16), (2, 16, 40, 40)        # (4-D: fed in bf16, as the layer in front of it would)


def _outputs(y):
    if isinstance(y, dict):
        return {k: v for k, v in y.items() if v is not None}
    return {'y': y}


def _run(monkeypatch, lib, make, on, min_elements=0):
    from stp3_amd import _lib, ops, ops_fused
    from stp3_amd.layers import fused
    from stp3_amd.parallel import GradientBuckets
    from stp3_amd.utils import to_channels_last
    calls = {}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in ('stp3_conv2d_fwd_pre', 'stp3_conv2d_wgrad_pre', 'stp3_conv2d_wgrad_partials', 'stp3_bn_apply_fwd'):
                return fn

            def wrapped(*a):
                key = name + ('+pre' if name == 'stp3_conv2d_wgrad_partials' and a[3] else '')
                calls[key] = calls.get(key, 0) + 1
                return fn(*a)
            return wrapped

    monkeypatch.setattr(_lib, 'lib', lambda: Counting())
    monkeypatch.setattr(ops_fused, 'PRE_FOLD', on)
    if min_elements is not None:                 # (these shapes are far below the size from which the fold pays)
        monkeypatch.setattr(ops_fused, 'PRE_FOLD_MIN_ELEMENTS', min_elements)
    ops.invalidate_weight_cache()
    torch.manual_seed(11)
    module, shape = make()
    model = to_channels_last(module).cuda().train()
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    buckets = GradientBuckets(model)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(*shape, generator=g).cuda()
    if x0.dim() == 4:                   # (the one-buffer ASPP route, like the model's, takes bf16 activations)
        x0 = x0.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    passes = []
    for _ in range(2):
        buckets.zero_grad()
        x = x0.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            outs = _outputs(model(x))
        loss = sum(v.float().square().mean() for v in outs.values())
        loss.backward()
        buckets.finish()
        fused.flush_batch_counters()
        passes.append(({k: v.detach().clone() for k, v in outs.items()}, x.grad.clone(),
                       torch.cat([f.clone() for f, _ in buckets.buckets]),
                       {k: v.detach().clone() for k, v in model.named_buffers()}))
        with torch.no_grad():
            for fp in buckets.flat_params:
                fp.mul_(0.97)
        ops.invalidate_weight_cache()
    torch.cuda.synchronize()
    return passes, calls


@pytest.mark.parametrize('make', [lambda: _decoder(ALL), lambda: _decoder(HDMAP), _deeplab],
                         ids=['decoder-all-heads', 'decoder-hdmap-alone', 'deeplab-head'])
def test_fold_is_bit_equal_to_the_separate_operators(monkeypatch, make):
    from stp3_amd import _lib
    lib = _lib.lib()                                     # (the library itself: each run counts through a wrapper of its own)
    off, calls_off = _run(monkeypatch, lib, make, False)
    on, calls_on = _run(monkeypatch, lib, make, True)
    # the switch does what it says: no folded launch with it off; with it on the 1x1 consumers and their weight gradients run
    # folded and their producers' apply passes are gone
    assert not any('pre' in k for k in calls_off), calls_off
    assert calls_on.get('stp3_conv2d_fwd_pre', 0) >= 4, calls_on
    assert calls_on.get('stp3_conv2d_wgrad_pre', 0) + calls_on.get('stp3_conv2d_wgrad_partials+pre', 0) == calls_on['stp3_conv2d_fwd_pre']
    assert calls_on.get('stp3_bn_apply_fwd', 0) < calls_off['stp3_bn_apply_fwd'], (calls_on, calls_off)
    for (o_out, o_dx, o_flat, o_buf), (f_out, f_dx, f_flat, f_buf) in zip(off, on):
        assert o_out.keys() == f_out.keys()
        for k in o_out:
            assert float(o_out[k].float().abs().max()) > 0 and torch.equal(o_out[k], f_out[k]), k
        assert float(o_dx.abs().max()) > 0 and torch.equal(o_dx, f_dx)
        assert float(o_flat.abs().max()) > 0 and torch.equal(o_flat, f_flat), float((o_flat - f_flat).abs().max())
        assert o_buf.keys() == f_buf.keys() and any('running_var' in k for k in o_buf)
        for k in o_buf:
            assert torch.equal(o_buf[k], f_buf[k]), k


def test_small_layers_keep_the_separate_operators(monkeypatch):
    """Below ``ops_fused.PRE_FOLD_MIN_ELEMENTS`` (the measured size from which the fold pays) nothing is folded."""
    from stp3_amd import _lib
    _, calls = _run(monkeypatch, _lib.lib(), _deeplab, True, min_elements=None)
    assert not any('pre' in k for k in calls) and calls['stp3_bn_apply_fwd'] > 0, calls
