"""Cases of the operand-side BatchNorm (+ ReLU) of the 1x1 convolutions (csrc/stp3_conv.hip, PRE): stp3_conv2d_fwd_pre and
stp3_conv2d_wgrad_pre / stp3_conv2d_wgrad_partials against the UNFUSED pair -- stp3_bn_apply_fwd into a tensor, then the plain
entry point on that tensor -- bit for bit.  Shared by tests/test_conv_pre_gpu.py (MI355X) and tests/hipcpu/run_conv_pre.py (the
kernel sources executed on CPU threads, checked by tests/test_conv_pre_cpu.py).

Shapes: M = N*H*W = 70 (a row tail inside one 128-pixel tile) and 645 = 64 * 10 + 5 (several tiles, and enough 64-pixel steps
for the weight gradient to split its pixels: partial sums + reduction); Cin = 72 (two K steps of 64 with a tail; more than one
64-channel block of the weight gradient's X tile, the last one partly beyond Cin); Cout = 8, 24 (one 64-channel tile with a
tail) and 136 (three of them); x is a channel slice (offset 8) of a wider buffer (ldx = 96 > Cin).  beta >= 1 keeps
act(shift) > 0 on every channel (asserted): padding that met the matrix cores as act(shift) instead of zero would show."""
import ctypes

import torch

ACT_NONE, ACT_RELU = 0, 1
SHAPES = {'m70': (2, 5, 7), 'm645': (3, 5, 43)}
CIN, LDX, OFF = 72, 96, 8
COUTS = (8, 24, 136)
# the 128 x 128 tile of the forward kernel: more than two K steps, more than 64 output channels, >= 512 workgroups
WIDE = dict(shape=(1, 128, 257), cin=136, ldx=152, cout=136)
EPS, MOMENTUM = 1e-5, 0.1


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def make_inputs(dev, shape, cin, ldx, cout, seed):
    """x: channel slice [OFF, OFF + cin) of a (N, ldx, H, W) bf16 channels-last buffer; w, bias, dy, gamma, beta."""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    wide = _cl((torch.randn(n, ldx, h, w, generator=g) * 1.5 + 0.25).to(torch.bfloat16)).to(dev)
    x = wide[:, OFF:OFF + cin]
    wgt = _cl((torch.randn(cout, cin, 1, 1, generator=g) * 0.2).to(torch.bfloat16)).to(dev)
    bias = torch.randn(cout, generator=g).to(dev)
    dy = _cl(torch.randn(n, cout, h, w, generator=g).to(torch.bfloat16)).to(dev)
    gamma = (0.5 + torch.rand(cin, generator=g)).to(dev)
    beta = (1.0 + torch.rand(cin, generator=g)).to(dev)
    return x, wgt, bias, dy, gamma, beta


def bn_constants(ops, x, gamma, beta):
    """(sums [2][C], coef [scale | shift | mean | invstd][C], count) of x through stp3_bn_stats and stp3_bn_finalize."""
    from stp3_amd import _lib
    lib = _lib.lib()
    n, c, h, w = x.shape
    xv, ld = ops._rows_view(x)
    dims = _lib.BnDims(n, h * w, c, ld, ld, ld, _lib.DTYPE_BF16, 0, 0, 0, 0, 0)
    ws, ws_bytes = ops._bn_workspace(n, c, x.device)
    sums = torch.empty(2 * c, dtype=torch.float32, device=x.device)
    _lib.check(lib.stp3_bn_stats(ctypes.byref(dims), xv.data_ptr(), None, ws.data_ptr(), ws_bytes, sums.data_ptr(),
                                 ops._stream_handle()), 'stp3_bn_stats')
    coef = torch.empty(4 * c, dtype=torch.float32, device=x.device)
    count = float(n * h * w)
    _lib.check(lib.stp3_bn_finalize(sums.data_ptr(), c, count, gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, None, None,
                                    coef.data_ptr(), ops._stream_handle()), 'stp3_bn_finalize')
    return sums, coef, count


def bn_apply(ops, x, sums, count, gamma, beta, act):
    """y = act(BN(x)) through stp3_bn_apply_fwd (training mode, no skip, no per-sample terms): the tensor the fold never stores."""
    from stp3_amd import _lib
    n, c, h, w = x.shape
    xv, ld = ops._rows_view(x)
    y = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    dims = _lib.BnDims(n, h * w, c, ld, c, c, _lib.DTYPE_BF16, act, 0, 0, 0, 0)
    save = torch.empty(2 * c, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().stp3_bn_apply_fwd(ctypes.byref(dims), xv.data_ptr(), None, None, None, sums.data_ptr(), count,
                                            gamma.data_ptr(), beta.data_ptr(), EPS, MOMENTUM, None, None, save.data_ptr(),
                                            save.data_ptr() + 4 * c, y.data_ptr(), ops._stream_handle()), 'stp3_bn_apply_fwd')
    return y


def _conv_dims(x, cout, ldx, ldy, has_bias):
    from stp3_amd import _lib
    n, cin, h, w = x.shape
    return _lib.ConvDims(n, h, w, cin, h, w, cout, 1, 1, 1, 0, 0, 1, 1, ldx, ldy, _lib.DTYPE_BF16, int(has_bias))


def forward_pair(ops, x, y, wgt, bias, coef, act):
    """(stp3_conv2d_fwd on the stored y, stp3_conv2d_fwd_pre on x)."""
    from stp3_amd import _lib
    lib = _lib.lib()
    n, cin, h, w = x.shape
    cout = wgt.shape[0]
    xv, ldx = ops._rows_view(x)
    ref = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    got = torch.empty_like(ref)
    b = None if bias is None else bias.data_ptr()
    _lib.check(lib.stp3_conv2d_fwd(ctypes.byref(_conv_dims(y, cout, cin, cout, bias is not None)), y.data_ptr(), wgt.data_ptr(), b,
                                   ref.data_ptr(), None, None, 0, ops._stream_handle()), 'stp3_conv2d_fwd')
    _lib.check(lib.stp3_conv2d_fwd_pre(ctypes.byref(_conv_dims(x, cout, ldx, cout, bias is not None)), xv.data_ptr(), wgt.data_ptr(), b,
                                       coef.data_ptr(), act, got.data_ptr(), ops._stream_handle()), 'stp3_conv2d_fwd_pre')
    return ref, got


def wgrad_triple(ops, x, y, dy, coef, act):
    """(stp3_conv2d_wgrad on the stored y, stp3_conv2d_wgrad_pre on x, stp3_conv2d_wgrad_partials on x + the batched
    reduction, the number of pixel splits)."""
    from stp3_amd import _lib
    lib = _lib.lib()
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    xv, ldx = ops._rows_view(x)
    dev = x.device
    dims_y, dims_x = _conv_dims(y, cout, cin, cout, False), _conv_dims(x, cout, ldx, cout, False)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.stp3_conv2d_wgrad_workspace(ctypes.byref(dims_x), ctypes.byref(nbytes)), 'stp3_conv2d_wgrad_workspace')
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
    ref, got, batched = (torch.empty(cout * cin, dtype=torch.float32, device=dev) for _ in range(3))
    stream = ops._stream_handle()
    _lib.check(lib.stp3_conv2d_wgrad(ctypes.byref(dims_y), dy.data_ptr(), y.data_ptr(), ref.data_ptr(), ws.data_ptr(),
                                     nbytes.value, stream), 'stp3_conv2d_wgrad')
    _lib.check(lib.stp3_conv2d_wgrad_pre(ctypes.byref(dims_x), dy.data_ptr(), xv.data_ptr(), coef.data_ptr(), act, got.data_ptr(),
                                         ws.data_ptr(), nbytes.value, stream), 'stp3_conv2d_wgrad_pre')
    splits = ctypes.c_int32()
    _lib.check(lib.stp3_conv2d_wgrad_partials(ctypes.byref(dims_x), dy.data_ptr(), xv.data_ptr(), coef.data_ptr(), act,
                                              ws.data_ptr(), nbytes.value, ctypes.byref(splits), stream),
               'stp3_conv2d_wgrad_partials')
    job = (_lib.WgradJob * 1)()
    job[0].partials, job[0].dw, job[0].numel, job[0].splits = ws.data_ptr(), batched.data_ptr(), cout * cin, splits.value
    _lib.check(lib.stp3_conv2d_wgrad_reduce_batch(1, job, stream), 'stp3_conv2d_wgrad_reduce_batch')
    return ref, got, batched, splits.value


def run_case(ops, dev, shape, cin, ldx, cout, act, with_bias, seed=0, wgrad=True):
    """One case -> dict of the bit comparisons (and what makes them meaningful)."""
    x, wgt, bias, dy, gamma, beta = make_inputs(dev, shape, cin, ldx, cout, seed)
    sums, coef, count = bn_constants(ops, x, gamma, beta)
    y = bn_apply(ops, x, sums, count, gamma, beta, act)
    ref, got = forward_pair(ops, x, y, wgt, bias if with_bias else None, coef, act)
    out = {'shift_positive': bool((coef[cin:2 * cin] > 0).all()), 'x_is_slice': bool(ops._rows_view(x)[1] == ldx > cin),
           'fwd_equal': bool(torch.equal(ref, got)), 'fwd_finite': bool(torch.isfinite(ref.float()).all()),
           'fwd_nonzero': bool(ref.float().abs().max() > 0)}
    if wgrad:
        wref, wgot, wbat, splits = wgrad_triple(ops, x, y, dy, coef, act)
        out.update(wgrad_equal=bool(torch.equal(wref, wgot)), wgrad_batched_equal=bool(torch.equal(wref, wbat)),
                   wgrad_nonzero=bool(wref.abs().max() > 0), splits=int(splits))
    return out


def case_list():
    """[(name, keyword arguments of ``run_case``)]: every shape x Cout x activation; the bias alternates with the case."""
    cases = []
    for sname, shape in SHAPES.items():
        for cout in COUTS:
            for act in (ACT_NONE, ACT_RELU):
                with_bias = (cout // 8 + act) % 2 == 0
                cases.append((f'{sname}-cout{cout}-{"relu" if act else "none"}-{"bias" if with_bias else "nobias"}',
                              dict(shape=shape, cin=CIN, ldx=LDX, cout=cout, act=act, with_bias=with_bias, seed=cout + act)))
    return cases
