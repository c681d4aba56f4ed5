"""TEST INFRASTRUCTURE -- run the inference kernels (stp3_conv2d_fwd_affine, stp3_dwconv2d_fwd_affine, stp3_linear_fwd_affine,
stp3_bn_eval_coefs) on CPU
tensors through libstp3hip_cpu.so (tests/hipcpu/build.py), next to the two operators they replace, and store both results.

    python tests/hipcpu/run_inference.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_inference_cpu.py (which holds the checks).  Per case ``<name>/fused`` and ``<name>/plain`` (bf16 bit
patterns as uint16): the fused operator, and ``ops.conv2d`` / ``ops.depthwise_conv2d`` followed by the eval ``ops.bn_act``;
``coefs/<k>/arena`` with the BatchNorm tensors it was computed from."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2
RES_NONE, RES_BEFORE_ACT, RES_AFTER_ACT = 0, 1, 2

# name: (N, Cin, H, W, channels, k, stride, padding, dilation, act, res_mode, conv bias, slot lanes (0: own tensor), slot offset)
CONV_CASES = {
    # pointwise: the whole-row streaming kernel (Cout = 144), the direct one (Cout = 96), the tiled one (Cin > 128)
    'pw_rows_swish': (2, 24, 9, 13, 144, 1, 1, 0, 1, ACT_SWISH, RES_NONE, False, 0, 0),
    'pw_direct_relu': (2, 32, 9, 13, 96, 1, 1, 0, 1, ACT_RELU, RES_NONE, False, 0, 0),
    'pw_lines_none_res_after': (2, 64, 9, 13, 128, 1, 1, 0, 1, ACT_NONE, RES_AFTER_ACT, False, 0, 0),
    'pw_direct_none_res_after': (2, 144, 7, 11, 24, 1, 1, 0, 1, ACT_NONE, RES_AFTER_ACT, False, 0, 0),
    'pw_tiled_relu': (1, 256, 9, 13, 64, 1, 1, 0, 1, ACT_RELU, RES_NONE, False, 0, 0),
    # 3x3: plain, with the skip before / after the activation, with a convolution bias, into a channel slice (ldy > Cout)
    'c3_relu': (2, 16, 11, 14, 64, 3, 1, 1, 1, ACT_RELU, RES_NONE, False, 0, 0),
    'c3_relu_res_before': (2, 64, 11, 14, 64, 3, 1, 1, 1, ACT_RELU, RES_BEFORE_ACT, False, 0, 0),
    'c3_none_res_after': (2, 64, 11, 14, 64, 3, 1, 1, 1, ACT_NONE, RES_AFTER_ACT, False, 0, 0),
    'c3_swish_bias': (1, 32, 11, 14, 40, 3, 1, 1, 1, ACT_SWISH, RES_NONE, True, 0, 0),
    'c3_relu_slot': (2, 16, 11, 14, 32, 3, 1, 1, 1, ACT_RELU, RES_NONE, False, 96, 32),
    'c3_wide_tile': (1, 24, 128, 256, 256, 3, 1, 1, 1, ACT_RELU, RES_NONE, False, 0, 0),
    'c3_stride2_swish': (2, 8, 15, 21, 48, 3, 2, 0, 1, ACT_SWISH, RES_NONE, False, 0, 0),
    # dilated 3x3 (ASPP), 7x7 stride 2 (decoder stem)
    'c3_dilated_relu': (1, 32, 30, 34, 64, 3, 1, 12, 12, ACT_RELU, RES_NONE, False, 0, 0),
    'c7_stride2_relu': (1, 64, 20, 24, 64, 7, 2, 3, 1, ACT_RELU, RES_NONE, False, 0, 0),
    # zero-padded channel lanes: 35 channels in 40 lanes (the temporal model), alone, into a slot, with a skip
    'lanes35_relu': (3, 40, 10, 12, 35, 3, 1, 1, 1, ACT_RELU, RES_NONE, False, 0, 0),
    'lanes35_relu_slot': (3, 40, 10, 12, 35, 3, 1, 1, 1, ACT_RELU, RES_NONE, False, 120, 40),
    'lanes35_none_res_after': (3, 40, 10, 12, 35, 1, 1, 0, 1, ACT_NONE, RES_AFTER_ACT, False, 0, 0),
    'lanes68_pw_swish': (2, 16, 9, 13, 68, 1, 1, 0, 1, ACT_SWISH, RES_BEFORE_ACT, False, 0, 0),
    # a per-sample bias in front of the BatchNorm (names ending in _sbias): the ASPP projection (1x1 over 256 channels: the
    # tiled kernel), a 3x3 with zero-padded lanes and a skip
    'pw_tiled_relu_sbias': (3, 256, 9, 13, 64, 1, 1, 0, 1, ACT_RELU, RES_NONE, False, 0, 0),
    'lanes35_c3_res_after_sbias': (3, 40, 10, 12, 35, 3, 1, 1, 1, ACT_RELU, RES_AFTER_ACT, False, 0, 0),
}

# name: (rows, K, N, act): the 1x1 convolution of a pooled descriptor + its eval BatchNorm (stp3_linear_fwd_affine)
LINEAR_CASES = {
    'lin_relu': (12, 160, 64, ACT_RELU),
    'lin_none_lanes21': (5, 70, 21, ACT_NONE),
}

# name: (N, C, H, W, k, stride): odd planes under the "same" padding FROZEN for a canonical 16 x 16 input (StaticSamePadConv2d
# applies the canonical padding to whatever it is given): asymmetric at stride 2 -- (0, 1) for 3x3, (1, 2) for 5x5
DW_CASES = {
    'dw3_s1': (2, 48, 13, 17, 3, 1),
    'dw3_s2': (2, 48, 13, 17, 3, 2),
    'dw5_s1': (2, 40, 13, 17, 5, 1),
    'dw5_s2': (2, 40, 13, 17, 5, 2),
}


CANONICAL = 16


def setup(lib_path):
    """As tests/hipcpu/run_sampler.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)
    return ops


def make_bn(g, channels, eps):
    bn = nn.BatchNorm2d(channels, eps=eps)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(channels, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(channels, generator=g) * 2 + 0.05)
        bn.weight.copy_(torch.randn(channels, generator=g) * 0.7 + 1.0)
        bn.bias.copy_(torch.randn(channels, generator=g) * 0.3)
    return bn.eval()


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def same_pad(size, k, s):
    """The frozen TF-"same" padding of models.efficientnet.StaticSamePadConv2d for an input of ``size``: (before, after)."""
    out = -(-size // s)
    pad = max((out - 1) * s + (k - 1) + 1 - size, 0)
    return pad // 2, pad - pad // 2


def main(lib_path, out_path):
    ops = setup(lib_path)
    from stp3_amd import inference
    out = {}
    cl = torch.channels_last
    bns = {}
    g = torch.Generator().manual_seed(7)
    for name, c in CONV_CASES.items():
        bns[name] = make_bn(g, c[4], 1e-3 if 'swish' in name else 1e-5)
    for name, c in DW_CASES.items():
        bns[name] = make_bn(g, c[1], 1e-3)
    for name, c in LINEAR_CASES.items():
        bns[name] = make_bn(g, c[2], 1e-5)
    coefs = inference.EvalCoefficients(nn.ModuleDict(bns), torch.device('cpu'))
    for k, (name, bn) in enumerate(bns.items()):
        out[f'coefs/{name}/arena'] = coefs.lookup(bn).numpy().copy()
        for key in ('running_mean', 'running_var', 'weight', 'bias'):
            out[f'coefs/{name}/{key}'] = getattr(bn, key).detach().numpy().copy()
        out[f'coefs/{name}/eps'] = np.float32(bn.eps)

    with torch.no_grad():
        for name, (n, cin, h, w, ch, k, s, p, d, act, res_mode, has_bias, slot, c0) in CONV_CASES.items():
            bn = bns[name]
            lanes = (ch + 7) // 8 * 8
            x = (torch.randn(n, cin, h, w, generator=g)).to(torch.bfloat16).contiguous(memory_format=cl)
            wgt = torch.randn(lanes, cin, k, k, generator=g) * (1.5 / (cin * k * k) ** 0.5)
            wgt[ch:] = 0                                      # zero-padded output lanes
            cbias = torch.randn(lanes, generator=g) if has_bias else None
            if cbias is not None:
                cbias[ch:] = 0
            y0 = ops.conv2d(x, wgt, cbias, s, p, d)
            res = None
            if res_mode != RES_NONE:
                res = torch.randn(y0.shape, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
            slots = [None, None]
            if slot:
                # two buffers filled with a pattern: what lies outside the slot must stay untouched
                slots = [(torch.full((n, slot, *y0.shape[2:]), 3.0, dtype=torch.bfloat16).contiguous(memory_format=cl), c0)
                         for _ in range(2)]
            sb = torch.randn(n, ch, generator=g) if name.endswith('_sbias') else None
            plain = ops.bn_act(y0, bn.weight, bn.bias, bn.running_mean, bn.running_var, False, 0.1, bn.eps, act=act, res=res,
                               res_mode=res_mode, sbias=sb, group=False, channels=ch if lanes != ch else None, out_slot=slots[0])
            assert ops.conv2d_affine_supported(x, wgt, s, ch, res, slots[1], sb, p, cbias), name
            fusedy = ops.conv2d_affine(x, wgt, cbias, s, p, d, coefs.lookup(bn), ch, act, res, res_mode, out_slot=slots[1], sbias=sb)
            assert fusedy.shape == plain.shape
            if slot:
                plain, fusedy = slots[0][0], slots[1][0]      # the whole buffers
            out[f'{name}/plain'], out[f'{name}/fused'] = bits(plain), bits(fusedy)
            out[f'{name}/conv'] = bits(y0)
        for name, (n, c, h, w, k, s) in DW_CASES.items():
            bn = bns[name]
            x = torch.randn(n, c, h, w, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
            wgt = torch.randn(c, 1, k, k, generator=g) * (1.5 / k)
            (top, bottom), (left, right) = same_pad(CANONICAL, k, s), same_pad(CANONICAL, k, s)
            pad = (left, right, top, bottom)
            y0 = ops.depthwise_conv2d(x, wgt, s, pad)
            plain = ops.bn_act(y0, bn.weight, bn.bias, bn.running_mean, bn.running_var, False, 0.1, bn.eps, act=ACT_SWISH, group=False)
            assert ops.depthwise_affine_supported(x, wgt, s), name
            fusedy = ops.depthwise_conv2d_affine(x, wgt, s, pad, coefs.lookup(bn), ACT_SWISH)
            out[f'{name}/plain'], out[f'{name}/fused'], out[f'{name}/pad'] = bits(plain), bits(fusedy), np.array(pad)
        # a layer the streaming pointwise kernels run takes no per-sample bias: the host keeps it on two operators
        xs = torch.zeros(2, 32, 9, 13, dtype=torch.bfloat16).contiguous(memory_format=cl)
        out['sbias_pointwise_supported'] = np.array(ops.conv2d_affine_supported(xs, torch.zeros(96, 32, 1, 1), 1, 96, None, None,
                                                                                 torch.zeros(2, 96), 0, None))
        for name, (m, k, n, act) in LINEAR_CASES.items():
            bn = bns[name]
            x = torch.randn(m, k, generator=g)
            w = torch.randn(n, k, generator=g) * (1.5 / k ** 0.5)
            y0 = ops.small_linear(x, w)
            plain = ops.bn_act(y0.view(m, n, 1, 1), bn.weight, bn.bias, bn.running_mean, bn.running_var, False, 0.1, bn.eps, act=act,
                               group=False)
            coef = coefs.lookup(bn)
            fusedy = ops.small_linear_affine(x, w, None, coef, coef.numel() // 2, act)
            out[f'{name}/plain'], out[f'{name}/fused'] = plain.reshape(m, n).numpy().copy(), fusedy.numpy().copy()
            out[f'{name}/linear'] = y0.numpy().copy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
