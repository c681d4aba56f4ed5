"""GPU: every C entry point of csrc/stp3_dwconv.hip through ``stp3_amd._lib`` against the float64 references of
tests/dwconv_cases.py, at the smallest shapes at which each mechanism of the kernels is live: the tails of the 4-column register
tile, the 2 x 2 quads of the stride-2 data gradient at leading pad 0 / 1 / 2, channel-vector counts that do not divide 256, the
second block column (more than 256 channel vectors), more than one grid round of the persistent kernels, all 256 lanes on pixels,
the 32-bit byte offsets at their largest (a 4 292 870 400-byte tensor) and the ``uint64_t`` instantiations (4 303 360 000 bytes).

What is pinned:
  exact pass (integer data)   ``torch.equal`` to the reference for fwd, fwd_bias, bwd_data, bwd_weight, bwd_weight_oihw (also the
                              transposed tap-major result bit for bit), the y and sums of fwd_stats and of fwd_stats_bn (the same
                              bits), the coef and running statistics of fwd_stats_bn against fwd_stats + stp3_bn_finalize (the
                              same bits); every entry run twice; canary rows around y, dx, dw, sums and coef unchanged; one bf16
                              case with integers wide enough that a third of the outputs are rounded to bf16
  real pass (N(0, 1) data)    per element, the bounds derived in tests/dwconv_cases.py (``*_excess`` = error / bound <= 1)
  fwd_affine                  act none / relu / swish on an exactly known bf16(y)
  large tensors               zero everywhere but in integer patches at the origin, the last rows and columns and around byte
                              offsets 2^31 and 2^32: float64 crops, and ``count_nonzero`` of the whole of y and dx
  argument checks             the return codes of every entry (on the GPU library)

Largest real-pass figures observed on the MI355X (``pytest -m gpu -s`` prints every figure), as error / bound (bound = 1):
  float32 y, y + bias, dx   0.44, 0.45, 0.37  (rounds-k3-s2-f32, second-column-c1032-f32; largest error 5.4e-6, k7-c64-f32)
  bf16 y, y + bias, dx      0.996 each        (rounds-k3-s2-bf16: a rounding to bf16 uses its half ulp fully; error 0.031)
  dw                        0.64 float32 (one-pixel-k5-f32, a single product), 0.30 bf16; largest error 1.7e-4 (narrow-c8-bf16)
  sums                      0.34 (one-pixel-k5-f32); largest relative error 3.1e-7
  coef mean                 0.92 (second-column-c1032-f32: two roundings against gamma_2)
  coef invstd, scale, shift 0.020, 0.023, 0.021 (largest relative error of invstd 1.6e-7 against 7.8e-6)
  running mean, variance    0.38, 0.007
  fwd_affine                none 0.993, relu 0.993, swish 0.995 (bf16 half ulp; largest error 0.0625)
Every exact-pass flag was true in every case, and both tensors around 4 GiB ran (they were not skipped).
The bounds are not tightened to these figures."""
import json

import pytest
import torch

from tests import dwconv_cases as DC

pytestmark = pytest.mark.gpu
CASES = DC.case_list()


def check(name, out):
    """The asserts on the figures of one case: every flag true, every error / bound ratio <= 1."""
    if out['kind'] == 'large':
        assert 'skipped' not in out, (name, out)
        for key in ('fwd', 'fwd_stats_y', 'fwd_stats_sums', 'bwd_data', 'bwd_weight', 'canaries_intact'):
            assert out[key] is True, (name, key, out)
        return
    for part in ('exact', 'affine'):
        for key, v in out.get(part, {}).items():
            if isinstance(v, bool):
                assert v is True, (name, part, key, out[part])
    for part in ('real', 'affine'):
        for key, v in out.get(part, {}).items():
            if key.endswith('_excess'):
                assert v <= 1.0, (name, part, key, v, out[part])
    assert out['real']['canaries_intact'] is True and out['real']['finite'] is True, (name, out['real'])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from stp3_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('name,kw', CASES, ids=[n for n, _ in CASES])
def test_depthwise_entries_equal_float64_reference(name, kw):
    out = DC.run_case(_lib(), 'cuda', _stream, **kw)
    torch.cuda.synchronize()
    print('FIGURES', name, json.dumps(out))
    if 'skipped' in out:
        pytest.skip(out['skipped'])
    check(name, out)


def test_depthwise_entries_on_a_side_stream():
    """One stride-1 and one stride-2 case on a stream set with ``torch.cuda.stream``: every launch of every entry, the partial
    rows in the workspace and their reductions follow the stream the caller hands over."""
    cases = dict(CASES)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = {name: DC.run_case(_lib(), 'cuda', _stream, **cases[name]) for name in ('tile-wo13-k3-bf16', 's2-pad1-k5-f32')}
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for name, out in outs.items():
        check(name, out)


def test_depthwise_argument_checks():
    res = DC.abi(_lib(), 'cuda')
    assert len(res) >= 140
    for name, rc, want in res:
        assert rc == want, (name, rc, want)
