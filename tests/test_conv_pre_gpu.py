"""GPU: BatchNorm (+ ReLU) in the operand load of a 1x1 convolution (csrc/stp3_conv.hip, PRE) against the unfused pair.

stp3_conv2d_fwd_pre, stp3_conv2d_wgrad_pre and stp3_conv2d_wgrad_partials (+ stp3_conv2d_wgrad_reduce_batch) read the
convolution output z and the (scale, shift) of stp3_bn_finalize; the reference stores y = act(BN(z)) with stp3_bn_apply_fwd and
runs the plain entry points on it.  The fold is the same arithmetic at the same rounding points, so the comparison is
``torch.equal`` -- no tolerance.  Shapes and constants: tests/conv_pre_cases.py (row tail, K tail, channel-sliced x with
ldx > Cin, Cout tails, pixel splits in the weight gradient, act(shift) > 0 so that unmasked padding would show)."""
import pytest
import torch

from tests import conv_pre_cases as PC

pytestmark = pytest.mark.gpu


def _check(out, min_splits=1):
    assert out['shift_positive'] and out['x_is_slice'], out           # the case is what it claims to be
    assert out['fwd_finite'] and out['fwd_nonzero'], out
    assert out['fwd_equal'], out
    if 'wgrad_equal' in out:
        assert out['wgrad_nonzero'] and out['splits'] >= min_splits, out
        assert out['wgrad_equal'] and out['wgrad_batched_equal'], out


@pytest.mark.parametrize('name,kw', PC.case_list(), ids=[n for n, _ in PC.case_list()])
def test_fold_equals_apply_then_plain(name, kw):
    from stp3_amd import ops
    out = PC.run_case(ops, 'cuda', **kw)
    torch.cuda.synchronize()
    # 645 pixels = 11 steps of 64: the weight gradient splits them over >= 2 workgroups (partials + reduction)
    _check(out, min_splits=2 if name.startswith('m645') else 1)


@pytest.mark.parametrize('act', [PC.ACT_NONE, PC.ACT_RELU])
def test_fold_on_the_wide_forward_tile(act):
    """Cin = 136 (three K steps), Cout = 136, 257 pixel tiles: the forward takes its 128 x 128 tile, the weight gradient the
    128 x 128 tile with 2 x 2 blocks, the last ones mostly beyond the tensor."""
    from stp3_amd import ops
    w = PC.WIDE
    out = PC.run_case(ops, 'cuda', shape=w['shape'], cin=w['cin'], ldx=w['ldx'], cout=w['cout'], act=act, with_bias=bool(act), seed=7)
    torch.cuda.synchronize()
    _check(out, min_splits=2)
