"""GPU: the loss and label-warp kernels (csrc/stp3_loss.hip) through ``stp3_amd.ops_loss`` / ``stp3_amd.losses`` against the
float64 references of tests/loss_cases.py -- values AND gradients (stp3_ce_topk_bwd, stp3_reg_loss_bwd), at the selection
kernel's edges (rows shorter than a wave, 1023 / 1024 / 1025 pixels around its 1024 threads, 40 960 / 41 000 around what it keeps
in registers, k = 1, k = P - 1, the sum route, exact ties at the threshold, rows with fewer than k live pixels, losses over many
exponents), the regression kernel's masks and grid-stride loop, and the warp on maps whose every pixel is a distinct number
(exact power-of-two cases with ties at every pixel; a general case checked away from half-integer coordinates).

What is pinned, with the bounds of tests/loss_cases.py (from the arithmetic, not from these observations):
  values                  |got - ref| <= 1e-5 |ref|
  float32 gradients       relative to the reference's largest entry: 2e-6 (C <= 4), 1e-5 (C = 48)
  bf16 gradients          per element |got - ref| <= 2^-7 |ref| + 1e-6 max|ref|
  exact zeros             bit zeros: ignored / masked pixels, pixels below the threshold, pred == target under L1
  determinism             every operator run twice, value and gradient ``torch.equal``
  accumulate              stp3_ce_topk_fwd with accumulate = 1 on a preset out: preset + value, one float32 addition
  warp                    ``torch.equal`` to the closed form (exact cases); no mismatch away from unsure pixels (general case)

Largest errors observed on the MI355X (``pytest -m gpu -s`` prints every figure):
  values                  7.6e-8 (cross-entropy, k-edges-k1), 4.7e-8 (regression, reg-l1-f32-c1)      bound 1e-5
  float32 gradients       2.2e-7 (C <= 4, selT-edges-p1023), 8.5e-8 (regression, reg-none-ignored)     bound 2e-6
                          1.8e-7 (C = 48, depth)                                                       bound 1e-5
  bf16 gradients          0.48 of the per-element bound (base-bf16-nhwc), 0.49 (reg-l2-bf16)           bound 1
  warp                    0 mismatching pixels in every case, the 0.39 % unsure pixels of the general case included
  smallest gap of a top-k case without deliberate ties: 2.4e-5 (cached-edge-p40960)                    needs >= 1e-5
The bounds are not tightened to these figures."""
import json

import pytest
import torch

from tests import loss_cases as LC

pytestmark = pytest.mark.gpu
CASES = LC.case_list()


def check(name, out):
    kind = out['kind']
    if kind == 'warp':
        assert out['distinct_sources'], (name, out)
        assert out['mismatches_sure'] == 0, (name, out)
        if out['mode'] == 'exact':
            assert out['equal'], (name, out)
        assert out['repeat_equal'] is True, (name, out)
        return
    assert out['value_err'] <= LC.VALUE_RTOL, (name, out)
    if kind == 'accumulate':
        assert out['accumulated_equal'], (name, out)
        return
    assert out['finite'], (name, out)
    if out['grad_dtype'] == 'torch.bfloat16':
        assert out['grad_ulp_excess'] <= LC.GRAD_ULP_EXCESS, (name, out)
    else:
        assert out['grad_err'] <= (LC.GRAD_RTOL_F32_C48 if out.get('classes') == 48 else LC.GRAD_RTOL_F32), (name, out)
    assert out['zeros_are_bit_zero'], (name, out)
    assert out['repeat_equal'] is True, (name, out)
    if kind == 'ce':
        assert out['ignored_are_bit_zero'] and out['grad_layout_kept'], (name, out)
    elif kind == 'hdmap':
        assert out['module_equal'], (name, out)
    else:
        assert out['masked_are_bit_zero'] and out['pad_zero'], (name, out)


@pytest.mark.parametrize('name,kw', CASES, ids=[n for n, _ in CASES])
def test_kernels_equal_float64_reference(name, kw):
    from stp3_amd import ops
    out = LC.run_case(ops, 'cuda', **kw)
    torch.cuda.synchronize()
    print('FIGURES', name, json.dumps(out))
    check(name, out)


def test_on_a_side_stream():
    """One cross-entropy case and the exact warp cases on a stream set with ``torch.cuda.stream``: launches, workspace and the
    backward pass follow the current stream."""
    from stp3_amd import ops
    cases = dict(CASES)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = {name: LC.run_case(ops, 'cuda', **cases[name]) for name in ('base', 'warp-exact-16x16', 'warp-exact-8x32')}
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for name, out in outs.items():
        check(name, out)
