"""Cases of the depthwise kernels (csrc/stp3_dwconv.hip): float64 references written from the definition in include/stp3_hip.h
(the ``stp3_dwconv_dims`` block), the table of shapes at which every C entry point is compared with them, and the return codes of
the argument checks.  Shared by tests/test_dwconv_exact_gpu.py (MI355X) and tests/hipcpu/run_dwconv.py (the kernel sources
executed on CPU threads, checked by tests/test_dwconv_exact_cpu.py).

The entries are called through ``stp3_amd._lib`` (ctypes, ``DwConvDims``), never through ``stp3_amd.ops*``: each entry, its
workspace query and its layouts are what is tested.  Tensors are channels-last [N][H][W][C], weights tap-major [K*K][C] float32.

References (float64, no convolution routine):
  ref_fwd         y[n,ho,wo,c]  = bias[c] + sum_{kh,kw} xp[n, ho*S+kh, wo*S+kw, c] * w[kh*K+kw, c]   (xp: the zero-padded input)
  ref_bwd_data    dxp[n, ho*S+kh, wo*S+kw, c] += dy[n,ho,wo,c] * w[kh*K+kw, c], dx = the unpadded part
  ref_bwd_weight  dw[kh*K+kw, c] = sum_{n,ho,wo} dy[n,ho,wo,c] * xp[n, ho*S+kh, wo*S+kw, c]
  ref_sums        sum and sum of squares per channel of the ROUNDED y (what a statistics pass over the stored tensor reads)
  ref_bn          stp3_bn_finalize: mean = sum / count, var = max(sq / count - mean^2, 0), invstd = 1 / sqrt(var + eps),
                  coef = scale (gamma * invstd) | shift (beta - mean * scale) | mean | invstd, running <- (1 - m) running + m * new
                  (running_var takes the unbiased variance var * count / (count - 1))
  ref_affine      act(bf16(y) * scale + shift), act = none / relu / swish (v * sigmoid(v))

EXACT PASS.  x, w, dy and the bias are small integers, so every product and every partial sum is an integer below 2^24 and float32
arithmetic is exact in ANY order of summation: the kernels must return the reference bit for bit, in float32 and in bf16 (which
holds integers up to 256 exactly and rounds larger ones to nearest-even exactly as ``tensor.to(torch.bfloat16)`` does).  The
precondition -- the sum of the absolute values of the terms of every accumulated quantity (window sum, per-channel sum |y| and
sum y^2, per-tap sum |dy x|) stays below 2^24 -- is asserted ON THE REFERENCE ALONE before a kernel runs.  A seed or a range that
misses it is replaced, never the condition.

REAL PASS.  x, dy ~ N(0, 1), w with full float32 mantissas.  u = 2^-24, gamma_n = n u / (1 - n u), A = the float64 sum of the
absolute values of the terms of the same element.  Every bound below comes from this arithmetic; none is fitted to an observation
(the observed figures are recorded in the docstring of tests/test_dwconv_exact_gpu.py).

  float32 y, dx   |got - ref| <= gamma_n A, n = K^2 + 1: the accumulator starts at the bias (or 0) and takes one fused
                  multiply-add, one rounding, per tap.
  bf16 y, dx      the float32 accumulator acc has |acc - ref| <= gamma_n A; rounding it to bf16 (8 significant bits, nearest)
                  adds at most 2^-9 ... 2^-8 |acc|:  |got - ref| <= 2^-8 |ref| + (1 + 2^-8) gamma_n A.
  dw              gamma_n A with n = N Ho Wo, valid for ANY summation order of n products (fused or rounded); this pins the
                  precision class of the weight gradient only -- its terms are pinned by the exact pass.
  sums            against float64 sums of the y THE KERNEL WROTE: every output pixel enters one chain of float32 additions (sum)
                  or fused multiply-adds (sum of squares), the partial rows are added in double and rounded to float32 once:
                  at most n = N Ho Wo + 1 roundings on any term: gamma_n sum|y|, gamma_n sum y^2.
  coef            against the float64 formula on THE KERNEL'S OWN float32 sums s, q (count = n):
                    ic = fl(1 / n)                                   relative error  <= u
                    mean = fl(s ic)                                                   <= gamma_2
                    e = fl(q ic) <= gamma_2;  m2 = fl(mean^2) <= gamma_5;  var = fl(e - m2), one more rounding (a fused
                    form drops one of these roundings): |var - var*| <= gamma_3 e* + gamma_6 mean*^2 <= gamma_12 E[y^2]
                    (mean^2 <= E[y^2]).  The case asserts var >= 0.05 E[y^2] on the reference; the kernel's sums are within
                    gamma_n of the reference's, which moves the ratio by less than 1e-3 of itself, so the cancellation
                    amplifies by at most 1 / 0.05 * 1.05 = 21:  relative error of var <= 21 gamma_12.
                    invstd = 1 / sqrt(var + eps): the addition (u; eps > 0 only damps the relative error of var), the square
                    root halves the relative error and adds 1 ulp (2 u, HIP's documented bound), the division 1 ulp (2 u):
                    relative error <= 10.5 gamma_12 + 5 u =: INVSTD_REL  (~131 u = 7.8e-6)
                    scale = fl(gamma invstd)                          <= INVSTD_REL + u
                    shift = fl(beta - fl(mean scale)) (or fused):     absolute <= (gamma_2 + INVSTD_REL + 3 u) (|beta| + |mean scale|)
                    running_mean: two products and a sum, <= gamma_2 + 3 u of (|(1 - m) old| + |m mean|); running_var the
                    same with var's relative error and the factor unbias (one more product): 21 gamma_12 + 5 u.
  fwd_affine      integer x and w (so bf16(y) is exactly known), real scale and shift.  t = fma(v, scale, shift) is ONE
                  rounding of the exact value: |t - t*| <= u |t*|.  none / relu: the bf16 rounding adds 2^-8 |t|:
                  |got - ref| <= (2^-8 + 2 u) |ref|.  swish = t * rcp(1 + exp(-t)) with exp(-t) = v_exp_f32(-t log2 e):
                  the product t log2 e is rounded (absolute u |t| log2 e in the exponent = relative u |t| of the power),
                  t's own error gives another u |t|, v_exp_f32 1 ulp (2 u); 1 + e rounds once (u) and never amplifies a
                  relative error of e; v_rcp_f32 1 ulp (2 u); the product with t (u) and t's own error (u):
                  relative (2 |t| + 7) u, then the bf16 rounding: |got - ref| <= (2^-8 + (2 |t| + 8) u) |ref|.  The case asserts
                  |t| <= 60 on the reference (no overflow of exp, no subnormal result).

``run_case`` returns plain numbers and flags; the asserts live in the test files.  An ``*_excess`` figure is the largest
|got - ref| / bound over the elements of a quantity and must stay <= 1."""
import ctypes
import math

import torch

U = 2.0 ** -24
EXACT_LIMIT = float(2 ** 24)
BF16_HALF_ULP = 2.0 ** -8
BN_EPS, BN_MOMENTUM = 1e-3, 0.01              # the EfficientNet trunk's BatchNorm constants
MIN_VAR_SHARE = 0.05                          # real pass: var >= 0.05 E[y^2] on the reference
MAX_AFFINE_T = 60.0
WIDE_SHARE = 0.1                              # wide-integer case: share of reference outputs beyond 256
CANARY = 7777.0                               # fills every output buffer and its guard rows before a call
ACTS = {'none': 0, 'relu': 1, 'swish': 2}
EINVAL, EUNSUP, ENOSPACE = -10001, -10002, -10003


def gamma(n):
    return n * U / (1.0 - n * U)


INVSTD_REL = 10.5 * gamma(12) + 5 * U
VAR_REL = 21 * gamma(12)


# ---- references -----------------------------------------------------------------------------------------------------
def out_size(h, w, k, s, pads):
    l, r, t, b = pads
    return (h + t + b - k) // s + 1, (w + l + r - k) // s + 1


def _padded(x, pads):
    l, r, t, b = pads
    n, h, w, c = x.shape
    xp = x.new_zeros(n, h + t + b, w + l + r, c)
    xp[:, t:t + h, l:l + w] = x
    return xp


def _window(xp, kh, kw, s, ho, wo):
    return xp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]


def ref_fwd(x, w, bias, k, s, pads):
    """x [N][H][W][C], w [K*K][C], bias [C] or None, float64 -> y [N][Ho][Wo][C] float64."""
    n, h, wd, c = x.shape
    ho, wo = out_size(h, wd, k, s, pads)
    xp = _padded(x, pads)
    y = x.new_zeros(n, ho, wo, c)
    if bias is not None:
        y += bias
    for kh in range(k):
        for kw in range(k):
            y += _window(xp, kh, kw, s, ho, wo) * w[kh * k + kw]
    return y


def ref_bwd_data(dy, w, k, s, pads, h, wd):
    l, r, t, b = pads
    n, ho, wo, c = dy.shape
    dxp = dy.new_zeros(n, h + t + b, wd + l + r, c)
    for kh in range(k):
        for kw in range(k):
            _window(dxp, kh, kw, s, ho, wo).add_(dy * w[kh * k + kw])
    return dxp[:, t:t + h, l:l + wd].contiguous()


def ref_bwd_weight(x, dy, k, s, pads):
    n, ho, wo, c = dy.shape
    xp = _padded(x, pads)
    return torch.stack([(dy * _window(xp, kh, kw, s, ho, wo)).sum(dim=(0, 1, 2)) for kh in range(k) for kw in range(k)])


def ref_sums(y_rounded):
    """[2][C] float64: sum and sum of squares over the pixels of the rounded outputs."""
    yd = y_rounded.double()
    return torch.stack([yd.sum(dim=(0, 1, 2)), (yd * yd).sum(dim=(0, 1, 2))])


def ref_bn(sums, count, gamma_, beta, eps, momentum, running_mean, running_var):
    """stp3_bn_finalize in float64 -> coef [4][C], running_mean, running_var, var."""
    s, q = sums[0].double(), sums[1].double()
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma_.double() * invstd
    shift = beta.double() - mean * scale
    unbias = count / (count - 1.0) if count > 1 else 1.0
    rm = (1.0 - momentum) * running_mean.double() + momentum * mean
    rv = (1.0 - momentum) * running_var.double() + momentum * var * unbias
    return torch.stack([scale, shift, mean, invstd]), rm, rv, var


def ref_affine(y_bf16, scale, shift, act):
    t = y_bf16.double() * scale.double() + shift.double()
    if act == 'relu':
        return t.clamp_min(0.0), t
    if act == 'swish':
        return t * torch.sigmoid(t), t
    return t, t


# ---- inputs ---------------------------------------------------------------------------------------------------------
TORCH_DTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}


def _ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def int_inputs(shape, seed, xr=2, wr=2):
    """Integer x, dy in [-xr, xr], w in [-wr, wr], bias in [-2, 2] as float64 CPU tensors."""
    n, c, h, wd, k, s, pads = shape
    ho, wo = out_size(h, wd, k, s, pads)
    g = torch.Generator().manual_seed(seed)
    return (_ints((n, h, wd, c), xr, g), _ints((k * k, c), wr, g), _ints((n, ho, wo, c), xr, g), _ints((c,), 2, g))


def real_inputs(shape, dtype, seed):
    """x, dy ~ N(0, 1) rounded to the case's type, w and bias float32 with full mantissas; CPU tensors in the kernel's types."""
    n, c, h, wd, k, s, pads = shape
    ho, wo = out_size(h, wd, k, s, pads)
    g = torch.Generator().manual_seed(seed + 1000)
    td = TORCH_DTYPE[dtype]
    return (torch.randn(n, h, wd, c, generator=g).to(td), torch.randn(k * k, c, generator=g) * 0.5,
            torch.randn(n, ho, wo, c, generator=g).to(td), torch.randn(c, generator=g))


def bn_inputs(c, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5, torch.randn(c, generator=g) * 0.1,
            torch.rand(c, generator=g) + 0.5)                    # gamma, beta, running_mean, running_var


# ---- calling the entries --------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return bool(a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)))


class Guarded:
    """An output tensor between two canary rows, the whole buffer (the tensor included) preset to CANARY."""

    def __init__(self, shape, dtype, dev, guard):
        self.n = 1
        for v in shape:
            self.n *= int(v)
        assert (guard * torch.empty(0, dtype=dtype).element_size()) % 16 == 0
        self.guard = guard
        self.buf = torch.full((self.n + 2 * guard,), CANARY, dtype=dtype, device=dev)
        self.t = self.buf[guard:guard + self.n].view(shape)
        self.canary = torch.full((), CANARY, dtype=dtype, device=dev)

    def intact(self):
        g = self.guard
        return bool((self.buf[:g] == self.canary).all() and (self.buf[g + self.n:] == self.canary).all())

    def ptr(self):
        return self.t.data_ptr()


def _ptr(t):
    return None if t is None else t.data_ptr()


class Entries:
    """The ten C entry points of csrc/stp3_dwconv.hip (and stp3_bn_finalize) on tensors of one device."""

    def __init__(self, lib, dev, stream, shape, dtype):
        from stp3_amd import _lib
        self.lib, self.dev, self.stream, self._lib = lib, dev, stream, _lib
        n, c, h, wd, k, s, pads = shape
        self.shape, self.dtype, self.td = shape, dtype, TORCH_DTYPE[dtype]
        self.ho, self.wo = out_size(h, wd, k, s, pads)
        self.dims = _lib.DwConvDims(n, h, wd, c, self.ho, self.wo, k, s, pads[2], pads[0],
                                    _lib.DTYPE_BF16 if dtype == 'bf16' else _lib.DTYPE_F32)
        self.count = n * self.ho * self.wo
        need = ctypes.c_size_t()
        self.rc(lib.stp3_dwconv2d_fwd_stats_workspace(ctypes.byref(self.dims), ctypes.byref(need)), 'fwd_stats_workspace')
        self.stats_bytes = need.value
        self.rc(lib.stp3_dwconv2d_bwd_weight_workspace(ctypes.byref(self.dims), ctypes.byref(need)), 'bwd_weight_workspace')
        self.wgrad_bytes = need.value
        self.ws = torch.empty(max(self.stats_bytes, self.wgrad_bytes), dtype=torch.uint8, device=dev)
        self.intact = True

    def rc(self, code, what):
        assert code == 0, f'stp3_dwconv2d_{what} returned {code}'

    def _out(self, shape, dtype, guard):
        return Guarded(shape, dtype, self.dev, guard)

    def _done(self, g):
        self.intact = self.intact and g.intact()
        return g.t

    def _y(self):
        n, c = self.shape[0], self.shape[1]
        return self._out((n, self.ho, self.wo, c), self.td, self.wo * c)

    def fwd(self, x, w, bias=None, with_bias_entry=False):
        y = self._y()
        d = ctypes.byref(self.dims)
        if with_bias_entry:
            self.rc(self.lib.stp3_dwconv2d_fwd_bias(d, x.data_ptr(), w.data_ptr(), _ptr(bias), y.ptr(), self.stream()), 'fwd_bias')
        else:
            self.rc(self.lib.stp3_dwconv2d_fwd(d, x.data_ptr(), w.data_ptr(), y.ptr(), self.stream()), 'fwd')
        return self._done(y)

    def fwd_affine(self, x, w, coef, act):
        y = self._y()
        self.rc(self.lib.stp3_dwconv2d_fwd_affine(ctypes.byref(self.dims), x.data_ptr(), w.data_ptr(), coef.data_ptr(), ACTS[act],
                                                  y.ptr(), self.stream()), 'fwd_affine')
        return self._done(y)

    def bwd_data(self, dy, w):
        n, c, h, wd = self.shape[:4]
        dx = self._out((n, h, wd, c), self.td, wd * c)
        self.rc(self.lib.stp3_dwconv2d_bwd_data(ctypes.byref(self.dims), dy.data_ptr(), w.data_ptr(), dx.ptr(), self.stream()), 'bwd_data')
        return self._done(dx)

    def bwd_weight(self, x, dy, oihw=False):
        c, k = self.shape[1], self.shape[4]
        dw = self._out((c, k * k) if oihw else (k * k, c), torch.float32, c)
        fn = self.lib.stp3_dwconv2d_bwd_weight_oihw if oihw else self.lib.stp3_dwconv2d_bwd_weight
        self.rc(fn(ctypes.byref(self.dims), x.data_ptr(), dy.data_ptr(), dw.ptr(), self.ws.data_ptr(), self.wgrad_bytes, self.stream()),
                'bwd_weight_oihw' if oihw else 'bwd_weight')
        return self._done(dw)

    def fwd_stats(self, x, w):
        c = self.shape[1]
        y, sums = self._y(), self._out((2, c), torch.float32, c)
        self.rc(self.lib.stp3_dwconv2d_fwd_stats(ctypes.byref(self.dims), x.data_ptr(), w.data_ptr(), y.ptr(), sums.ptr(),
                                                 self.ws.data_ptr(), self.stats_bytes, self.stream()), 'fwd_stats')
        return self._done(y), self._done(sums)

    def fwd_stats_bn(self, x, w, bn):
        """bn = (gamma, beta, running_mean, running_var) on the device; the running statistics are copied, not touched."""
        c = self.shape[1]
        y, sums, coef = self._y(), self._out((2, c), torch.float32, c), self._out((4, c), torch.float32, c)
        rm, rv = bn[2].clone(), bn[3].clone()
        self.rc(self.lib.stp3_dwconv2d_fwd_stats_bn(ctypes.byref(self.dims), x.data_ptr(), w.data_ptr(), y.ptr(), sums.ptr(),
                                                    float(self.count), bn[0].data_ptr(), bn[1].data_ptr(), BN_EPS, BN_MOMENTUM,
                                                    rm.data_ptr(), rv.data_ptr(), coef.ptr(), self.ws.data_ptr(), self.stats_bytes,
                                                    self.stream()), 'fwd_stats_bn')
        return self._done(y), self._done(sums), self._done(coef), rm, rv

    def bn_finalize(self, sums, bn):
        c = self.shape[1]
        coef = self._out((4, c), torch.float32, c)
        rm, rv = bn[2].clone(), bn[3].clone()
        code = self.lib.stp3_bn_finalize(sums.data_ptr(), c, float(self.count), bn[0].data_ptr(), bn[1].data_ptr(), BN_EPS, BN_MOMENTUM,
                                         rm.data_ptr(), rv.data_ptr(), coef.ptr(), self.stream())
        assert code == 0, f'stp3_bn_finalize returned {code}'
        return self._done(coef), rm, rv


def _twice(fn):
    """fn() -> tensor or tuple of tensors: the first run's outputs and whether the second run gives the same bits."""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return a, all(same_bits(p, q) for p, q in zip(a, b))


def _excess(got, ref, bound):
    """Largest |got - ref| / bound and largest |got - ref| (bound == 0 admits only got == ref)."""
    diff = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, math.inf), diff))
    return float(ratio.max()), float(diff.max())


# ---- the two passes -------------------------------------------------------------------------------------------------
def exact_pass(lib, dev, stream, shape, dtype, seed, xr=2, wr=2):
    n, c, h, wd, k, s, pads = shape
    td = TORCH_DTYPE[dtype]
    x, w, dy, bias = [t.to(dev) for t in int_inputs(shape, seed, xr, wr)]
    ho, wo = out_size(h, wd, k, s, pads)
    # references and their precondition, before any kernel runs
    y, yb, dx, dw = ref_fwd(x, w, None, k, s, pads), None, ref_bwd_data(dy, w, k, s, pads, h, wd), ref_bwd_weight(x, dy, k, s, pads)
    yb = y + bias
    y_r, yb_r, dx_r = y.to(td), yb.to(td), dx.to(td)
    sums = ref_sums(y_r)
    terms = {'window_y': float(ref_fwd(x.abs(), w.abs(), bias.abs(), k, s, pads).max()),
             'window_dx': float(ref_bwd_data(dy.abs(), w.abs(), k, s, pads, h, wd).max()),
             'sum_abs_y': float(y_r.double().abs().sum(dim=(0, 1, 2)).max()), 'sum_y2': float(sums[1].max()),
             'tap_abs_dw': float(ref_bwd_weight(x.abs(), dy.abs(), k, s, pads).max())}
    assert max(terms.values()) < EXACT_LIMIT, f'exactness precondition missed: {terms}: choose another seed or range'
    assert float(y.abs().max()) > 0 and float(dx.abs().max()) > 0 and float(dw.abs().max()) > 0
    big_y, big_dx = float((y.abs() > 256).double().mean()), float((dx.abs() > 256).double().mean())
    if xr > 2:
        assert dtype == 'bf16' and big_y >= WIDE_SHARE and big_dx >= WIDE_SHARE, f'wide case: shares {big_y:.3f} {big_dx:.3f} < {WIDE_SHARE}'
    sums_f = sums.float()
    assert torch.equal(sums_f.double(), sums)

    e = Entries(lib, dev, stream, shape, dtype)
    xd, dyd, wf, bf = x.to(td), dy.to(td), w.float(), bias.float()
    bn = [t.to(dev) for t in bn_inputs(c, seed)]
    out = {'terms': terms, 'share_beyond_256': [big_y, big_dx]}
    (g,), same = _twice(lambda: e.fwd(xd, wf))
    out['fwd'], out['fwd_repeat'] = bool(torch.equal(g, y_r)), same
    (g,), same = _twice(lambda: e.fwd(xd, wf, bf, True))
    out['fwd_bias'], out['fwd_bias_repeat'] = bool(torch.equal(g, yb_r)), same
    out['fwd_bias_null'] = bool(torch.equal(e.fwd(xd, wf, None, True), y_r))
    (g,), same = _twice(lambda: e.bwd_data(dyd, wf))
    out['bwd_data'], out['bwd_data_repeat'] = bool(torch.equal(g, dx_r)), same
    (gw,), same = _twice(lambda: e.bwd_weight(xd, dyd))
    out['bwd_weight'], out['bwd_weight_repeat'] = bool(torch.equal(gw, dw.float())), same
    (go,), same = _twice(lambda: e.bwd_weight(xd, dyd, True))
    out['bwd_weight_oihw'], out['bwd_weight_oihw_repeat'] = bool(torch.equal(go, dw.float().t().contiguous())), same
    out['oihw_is_transposed_tap_major'] = same_bits(go, gw.t().contiguous())
    (gy, gs), same = _twice(lambda: e.fwd_stats(xd, wf))
    out['fwd_stats_y'], out['fwd_stats_sums'], out['fwd_stats_repeat'] = bool(torch.equal(gy, y_r)), bool(torch.equal(gs, sums_f)), same
    (by, bs, bcoef, brm, brv), same = _twice(lambda: e.fwd_stats_bn(xd, wf, bn))
    out['fwd_stats_bn_y'], out['fwd_stats_bn_sums'], out['fwd_stats_bn_repeat'] = bool(torch.equal(by, y_r)), bool(torch.equal(bs, sums_f)), same
    out['stats_bn_same_bits_as_stats'] = same_bits(by, gy) and same_bits(bs, gs)
    (fcoef, frm, frv), same = _twice(lambda: e.bn_finalize(gs, bn))
    out['bn_same_bits_as_finalize'] = same_bits(bcoef, fcoef) and same_bits(brm, frm) and same_bits(brv, frv)
    out['running_stats_moved'] = not same_bits(brm, bn[2]) and not same_bits(brv, bn[3])
    out['canaries_intact'] = e.intact
    return out


def real_pass(lib, dev, stream, shape, dtype, seed, coef_check=True):
    n, c, h, wd, k, s, pads = shape
    td = TORCH_DTYPE[dtype]
    ho, wo = out_size(h, wd, k, s, pads)
    count = n * ho * wo
    xk, wk, dyk, bk = [t.to(dev) for t in real_inputs(shape, dtype, seed)]
    x, w, dy, bias = xk.double(), wk.double(), dyk.double(), bk.double()
    bn = [t.to(dev) for t in bn_inputs(c, seed)]
    y, yb, dx, dw = ref_fwd(x, w, None, k, s, pads), ref_fwd(x, w, bias, k, s, pads), ref_bwd_data(dy, w, k, s, pads, h, wd), ref_bwd_weight(x, dy, k, s, pads)
    a_y = ref_fwd(x.abs(), w.abs(), None, k, s, pads)
    a_dx, a_dw = ref_bwd_data(dy.abs(), w.abs(), k, s, pads, h, wd), ref_bwd_weight(x.abs(), dy.abs(), k, s, pads)
    rsum = ref_sums(y.to(td))
    _, _, _, rvar = ref_bn(rsum, count, bn[0], bn[1], BN_EPS, BN_MOMENTUM, bn[2], bn[3])
    var_share = float((rvar / (rsum[1] / count).clamp_min(1e-300)).min())
    if coef_check:
        assert var_share >= MIN_VAR_SHARE, f'var / E[y^2] = {var_share:.3f} < {MIN_VAR_SHARE}: choose another seed'
    gk = gamma(k * k + 1)

    def pixel_bound(ref, a):
        return gk * a if dtype == 'f32' else BF16_HALF_ULP * ref.abs() + (1 + BF16_HALF_ULP) * gk * a
    e = Entries(lib, dev, stream, shape, dtype)
    out = {'var_share': var_share}
    out['y_excess'], out['y_err'] = _excess(e.fwd(xk, wk), y, pixel_bound(y, a_y))
    out['yb_excess'], out['yb_err'] = _excess(e.fwd(xk, wk, bk, True), yb, pixel_bound(yb, a_y + bias.abs()))
    out['dx_excess'], out['dx_err'] = _excess(e.bwd_data(dyk, wk), dx, pixel_bound(dx, a_dx))
    out['dw_excess'], out['dw_err'] = _excess(e.bwd_weight(xk, dyk), dw, gamma(count) * a_dw)
    gy, gs, gcoef, grm, grv = e.fwd_stats_bn(xk, wk, bn)
    out['stats_y_excess'], _ = _excess(gy, y, pixel_bound(y, a_y))
    own = ref_sums(gy)
    gn = gamma(count + 1)
    own_abs = torch.stack([gy.double().abs().sum(dim=(0, 1, 2)), own[1]])
    out['sums_excess'], _ = _excess(gs, own, gn * own_abs)
    out['sums_rel_err'] = float(((gs.double() - own).abs() / own_abs.clamp_min(1e-300)).max())
    if coef_check:
        rcoef, rrm, rrv, rv_ = ref_bn(gs, count, bn[0], bn[1], BN_EPS, BN_MOMENTUM, bn[2], bn[3])
        scale, shift, mean, invstd = rcoef
        bounds = torch.stack([(INVSTD_REL + U) * scale.abs(),
                              (gamma(2) + INVSTD_REL + 3 * U) * (bn[1].double().abs() + (mean * scale).abs()),
                              gamma(2) * mean.abs(), INVSTD_REL * invstd.abs()])
        for i, name in enumerate(('scale', 'shift', 'mean', 'invstd')):
            out[f'{name}_excess'], _ = _excess(gcoef[i], rcoef[i], bounds[i])
        out['invstd_rel_err'] = float(((gcoef[3].double() - invstd).abs() / invstd).max())
        m = BN_MOMENTUM
        unbias = count / (count - 1.0) if count > 1 else 1.0
        out['running_mean_excess'], _ = _excess(grm, rrm, (gamma(2) + 3 * U) * ((1 - m) * bn[2].double().abs() + m * mean.abs()))
        out['running_var_excess'], _ = _excess(grv, rrv, (VAR_REL + 5 * U) * ((1 - m) * bn[3].double().abs() + m * rv_ * unbias))
    out['canaries_intact'] = e.intact
    out['finite'] = bool(torch.isfinite(gy.double()).all() and torch.isfinite(gcoef).all())
    return out


def affine_pass(lib, dev, stream, shape, seed):
    """stp3_dwconv2d_fwd_affine (bf16, 3x3 / 5x5): integer x and w, real scale and shift, the three activations."""
    n, c, h, wd, k, s, pads = shape
    x, w, _, _ = [t.to(dev) for t in int_inputs(shape, seed)]
    yb = ref_fwd(x, w, None, k, s, pads).to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 3000)
    coef = torch.stack([torch.randn(c, generator=g) * 0.25, torch.randn(c, generator=g)]).to(dev)
    e = Entries(lib, dev, stream, shape, 'bf16')
    xd, wf = x.to(torch.bfloat16), w.float()
    out = {'affine_conv_matches': bool(torch.equal(e.fwd(xd, wf), yb))}
    for act in ACTS:
        ref, t = ref_affine(yb, coef[0], coef[1], act)
        assert float(t.abs().max()) <= MAX_AFFINE_T
        rel = BF16_HALF_ULP + ((2 * t.abs() + 8) * U if act == 'swish' else 2 * U)
        (got,), same = _twice(lambda: e.fwd_affine(xd, wf, coef, act))
        out[f'affine_{act}_excess'], out[f'affine_{act}_err'] = _excess(got, ref, rel * ref.abs())
        out[f'affine_{act}_repeat'] = same
    out['affine_canaries_intact'] = e.intact
    return out


# ---- the two tensors around 4 GiB (GPU only) ------------------------------------------------------------------------
PATCH = 64


def large_patches(side, c, itemsize):
    """Top-left corners of the 64 x 64 patches: the origin, the last rows and columns, and around the pixels whose byte offset
    is 2^31 and (when the tensor reaches it) 2^32."""
    at = [(0, 0), (side - PATCH, side - PATCH)]
    for off in (2 ** 31, 2 ** 32):
        pixel = off // (c * itemsize)
        if pixel < side * side:
            r, col = divmod(pixel, side)
            at.append((min(max(r - PATCH // 2, 0), side - PATCH), min(max(col - PATCH // 2, 0), side - PATCH)))
    for i, (r0, c0) in enumerate(at):                                # the windows of two patches never touch
        for r1, c1 in at[i + 1:]:
            assert abs(r0 - r1) >= PATCH + 8 or abs(c0 - c1) >= PATCH + 8
    return at


def large_pass(lib, dev, stream, side, uint64_path, seed):
    """N = 1, C = 8, bf16, K = 3, stride 1, pad 1 on a side x side image that is zero outside integer patches.  References are
    float64 crops (patch + 2 pixels on every side, cut at the image border: beyond them every term is zero)."""
    c, k, margin = 8, 3, 2
    shape = (1, c, side, side, k, 1, (1, 1, 1, 1))
    nbytes = side * side * c * 2
    limit = 2 ** 32 - (side + side + 16) * c * 4                     # small_tensors() of csrc/stp3_dwconv.hip
    assert (nbytes >= limit) == uint64_path, (nbytes, limit)
    need = 5 * nbytes + (512 * 9 + 2048 * 2) * c * 4 + (64 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        return {'skipped': f'{free} bytes free on the device, the case needs {need}'}
    g = torch.Generator().manual_seed(seed)
    w = _ints((k * k, c), 2, g)
    at = large_patches(side, c, 2)
    x = torch.zeros(1, side, side, c, dtype=torch.bfloat16, device=dev)
    dy = torch.zeros(1, side, side, c, dtype=torch.bfloat16, device=dev)
    crops = []
    for r0, c0 in at:
        ra, rb, ca, cb = max(r0 - margin, 0), min(r0 + PATCH + margin, side), max(c0 - margin, 0), min(c0 + PATCH + margin, side)
        px, pdy = _ints((PATCH, PATCH, c), 2, g), _ints((PATCH, PATCH, c), 2, g)
        cx, cdy = torch.zeros(1, rb - ra, cb - ca, c, dtype=torch.float64), torch.zeros(1, rb - ra, cb - ca, c, dtype=torch.float64)
        cx[0, r0 - ra:r0 - ra + PATCH, c0 - ca:c0 - ca + PATCH] = px
        cdy[0, r0 - ra:r0 - ra + PATCH, c0 - ca:c0 - ca + PATCH] = pdy
        x[0, r0:r0 + PATCH, c0:c0 + PATCH] = px.to(torch.bfloat16).to(dev)
        dy[0, r0:r0 + PATCH, c0:c0 + PATCH] = pdy.to(torch.bfloat16).to(dev)
        # zero padding of the crop is the truth: outside it x and dy are zero (or beyond the image)
        crops.append(((ra, rb, ca, cb), ref_fwd(cx, w, None, k, 1, (1, 1, 1, 1)), ref_bwd_data(cdy, w, k, 1, (1, 1, 1, 1), rb - ra, cb - ca),
                      ref_bwd_weight(cx, cdy, k, 1, (1, 1, 1, 1)), ref_bwd_weight(cx.abs(), cdy.abs(), k, 1, (1, 1, 1, 1))))
    sums = sum(ref_sums(cr[1]) for cr in crops)
    dw = sum(cr[3] for cr in crops)
    terms = {'sum_abs_y': float(sum(cr[1].abs().sum(dim=(0, 1, 2)) for cr in crops).max()), 'sum_y2': float(sums[1].max()),
             'tap_abs_dw': float(sum(cr[4] for cr in crops).max()), 'window': 9.0 * 4}
    assert max(terms.values()) < EXACT_LIMIT and max(float(cr[1].abs().max()) for cr in crops) <= 256
    e = Entries(lib, dev, stream, shape, 'bf16')
    wf = w.float().to(dev)
    out = {'terms': terms, 'bytes': nbytes, 'patches': len(at), 'canaries_intact': True}

    def compare(got, idx):
        ok = int(torch.count_nonzero(got)) == sum(int(torch.count_nonzero(cr[idx])) for cr in crops)
        for (ra, rb, ca, cb), *refs in crops:
            ok = ok and bool(torch.equal(got[:, ra:rb, ca:cb].cpu().double(), refs[idx - 1]))
        return ok
    got = e.fwd(x, wf)
    out['fwd'] = compare(got, 1)
    del got
    gy, gs = e.fwd_stats(x, wf)
    out['fwd_stats_y'], out['fwd_stats_sums'] = compare(gy, 1), bool(torch.equal(gs.cpu().double(), sums))
    del gy
    got = e.bwd_data(dy, wf)
    out['bwd_data'] = compare(got, 2)
    del got
    out['bwd_weight'] = bool(torch.equal(e.bwd_weight(x, dy).cpu().double(), dw))
    out['canaries_intact'] = e.intact
    return out


# ---- the case table -------------------------------------------------------------------------------------------------
def run_case(lib, device, stream, kind='small', **case):
    """One case on ``device`` through ``stp3_amd._lib`` -> dict of plain numbers and flags.  ``stream``: callable -> handle."""
    if kind == 'large':
        out = large_pass(lib, device, stream, case['side'], case['uint64_path'], case['seed'])
    else:
        shape, dtype, seed = case['shape'], case['dtype'], case['seed']
        out = {'exact': exact_pass(lib, device, stream, shape, dtype, seed, case.get('xr', 2), case.get('wr', 2)),
               'real': real_pass(lib, device, stream, shape, dtype, seed, case.get('coef_check', True))}
        if dtype == 'bf16' and shape[4] != 7:
            out['affine'] = affine_pass(lib, device, stream, shape, seed)
    out['kind'] = kind
    return out


P1, P2, P3 = (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)
SHAPES = [
    # tails of the 4-column register tile: Wo = 13, 6, 4 and 1 (Wo mod 4 = 1, 2, 0; Wo < 4)
    ('tile-wo13-k3', (2, 24, 9, 13, 3, 1, P1), {}),                 # C = 24: 6 / 3 channel vectors, dead threads, pl >= PL
    ('tile-wo6-k5', (3, 40, 7, 6, 5, 1, P2), {}),                   # C = 40: 10 / 5 channel vectors
    ('tile-wo4-k7', (1, 8, 3, 4, 7, 1, P3), {}),                    # the image is smaller than the window
    ('tile-wo7-k3', (1, 8, 6, 7, 3, 1, P1), {}),                    # Wo mod 4 = 3
    ('one-pixel-k5', (1, 16, 1, 1, 5, 1, P2), {'coef_check': False}),   # only the centre tap is in range; count = 1: var = 0
    # stride 2 and the 2 x 2 quads of dwconv_bwd_data_s2_kernel: leading pad 0, 1, 2; odd and even H, W; asymmetric trailing pad
    ('s2-pad0-k3', (1, 8, 5, 7, 3, 2, (0, 1, 0, 1)), {}),
    ('s2-pad1-k3', (2, 16, 6, 7, 3, 2, P1), {}),
    ('s2-pad1-k5', (2, 24, 11, 13, 5, 2, (1, 2, 1, 2)), {}),
    ('s2-pad2-k5', (1, 8, 8, 10, 5, 2, P2), {}),
    ('k7-c64', (2, 64, 20, 19, 7, 1, P3), {}),                      # the 7x7 with bias
    # the second block column (by > 1, blockIdx.y > 0): more than 256 channel vectors
    ('second-column-c1032', (1, 1032, 5, 6, 3, 1, P1), {'only': 'f32'}),                 # 258 vectors
    # 257 vectors.  Four output pixels from overlapping windows in each of 2056 channels: some channel always has nearly equal
    # outputs (the best of 300 seeds reaches var = 0.035 E[y^2]), so the real pass cannot state its coef precondition here; the
    # exact pass still compares coef and running statistics with stp3_bn_finalize bit for bit, and the float32 case above
    # holds the real-pass coef check of the second block column
    ('second-column-c2056', (1, 2056, 4, 5, 5, 2, (1, 2, 1, 2)), {'only': 'bf16', 'coef_check': False}),
    # more than one grid round of the persistent kernels: C = 512 float32 = 128 vectors, two pixel lanes per workgroup
    ('rounds-k5-s1', (2, 512, 96, 96, 5, 1, P2), {}),
    ('rounds-k3-s2', (4, 512, 100, 100, 3, 2, (0, 1, 0, 1)), {}),   # 10 000 quads: beyond one resident round of bwd_data_s2
    ('narrow-c8', (2, 8, 300, 301, 3, 1, P1), {'only': 'bf16'}),    # one channel vector: all 256 lanes on pixels
]
# bf16 with wider integers: x, dy in [-16, 16], w in [-8, 8] at K = 7 -- outputs beyond 256 are rounded to bf16
WIDE = ('wide-int-k7', (1, 16, 10, 9, 7, 1, P3), {'only': 'bf16', 'xr': 16, 'wr': 8})
SEEDS = {}                                     # (name, dtype) -> seed, where seed 0 misses a precondition


def case_list():
    """[(name, keyword arguments of ``run_case``)]: both types wherever C allows (bf16 needs C % 8 == 0)."""
    cases = []
    for name, shape, opt in SHAPES + [WIDE]:
        for dtype in ('f32', 'bf16'):
            if opt.get('only', dtype) != dtype or (dtype == 'bf16' and shape[1] % 8):
                continue
            kw = {a: b for a, b in opt.items() if a != 'only'}
            cases.append((f'{name}-{dtype}', dict(kind='small', shape=shape, dtype=dtype, seed=SEEDS.get((name, dtype), 0), **kw)))
    # bf16, N = 1, C = 8: 16380 x 16380 x 8 x 2 = 4 292 870 400 bytes < small_tensors' limit 2^32 - (W + Wo + 16) C 4
    # = 4 294 967 296 - 32 776 * 32 = 4 293 918 464: the uint32 offsets at their largest.  16400 x 16400 x 8 x 2 = 4 303 360 000
    # bytes >= 2^32 - 32 816 * 32 = 4 293 917 184: the uint64_t instantiations.
    cases.append(('large-uint32-16380', dict(kind='large', side=16380, uint64_path=False, seed=1)))
    cases.append(('large-uint64-16400', dict(kind='large', side=16400, uint64_path=True, seed=2)))
    return cases


def host_names():
    """The table without the two tensors around 4 GiB."""
    return [n for n, kw in case_list() if kw['kind'] != 'large']


# ---- argument checks: every call returns before a launch ----------------------------------------------------------------
def abi(lib, dev='cpu'):
    """[(name, return code, expected code)]: expected from include/stp3_hip.h (STP3_EINVAL: bad dimension / null pointer,
    STP3_EUNSUP: a valid request this build does not support, STP3_ENOSPACE: workspace too small) and ``check()``."""
    from stp3_amd import _lib
    c, k = 16, 3
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    need = ctypes.c_size_t()

    def dims(**kw):
        v = dict(N=1, H=4, W=4, C=c, Ho=4, Wo=4, K=k, stride=1, pad_top=1, pad_left=1, dtype=_lib.DTYPE_BF16)
        v.update(kw)
        return _lib.DwConvDims(*[v[f] for f, _ in _lib.DwConvDims._fields_])
    ok = dims()
    stats_ws = 2048 * 2 * c * 4
    wgrad_ws = 512 * k * k * c * 4
    assert lib.stp3_dwconv2d_fwd_stats_workspace(ctypes.byref(ok), ctypes.byref(need)) == 0 and need.value == stats_ws
    assert lib.stp3_dwconv2d_bwd_weight_workspace(ctypes.byref(ok), ctypes.byref(need)) == 0 and need.value == wgrad_ws
    big = torch.zeros(wgrad_ws, dtype=torch.uint8, device=dev).data_ptr()
    # entry -> (callable(dims pointer, pointer list), number of pointers, names of the pointers that may not be NULL)
    entries = {
        'fwd': (lambda d, a: lib.stp3_dwconv2d_fwd(d, a[0], a[1], a[2], None), ('x', 'w', 'y')),
        'fwd_bias': (lambda d, a: lib.stp3_dwconv2d_fwd_bias(d, a[0], a[1], p, a[2], None), ('x', 'w', 'y')),
        'fwd_affine': (lambda d, a: lib.stp3_dwconv2d_fwd_affine(d, a[0], a[1], a[2], 2, a[3], None), ('x', 'w', 'coef', 'y')),
        'fwd_stats_workspace': (lambda d, a: lib.stp3_dwconv2d_fwd_stats_workspace(d, ctypes.byref(need) if a[0] else None), ('bytes',)),
        'fwd_stats': (lambda d, a: lib.stp3_dwconv2d_fwd_stats(d, a[0], a[1], a[2], a[3], a[4] and big, stats_ws, None),
                      ('x', 'w', 'y', 'sums', 'workspace')),
        'fwd_stats_bn': (lambda d, a: lib.stp3_dwconv2d_fwd_stats_bn(d, a[0], a[1], a[2], a[3], 16.0, p, p, 1e-3, 0.01, p, p, a[4],
                                                                     a[5] and big, stats_ws, None), ('x', 'w', 'y', 'sums', 'coef', 'workspace')),
        'bwd_data': (lambda d, a: lib.stp3_dwconv2d_bwd_data(d, a[0], a[1], a[2], None), ('dy', 'w', 'dx')),
        'bwd_weight_workspace': (lambda d, a: lib.stp3_dwconv2d_bwd_weight_workspace(d, ctypes.byref(need) if a[0] else None), ('bytes',)),
        'bwd_weight': (lambda d, a: lib.stp3_dwconv2d_bwd_weight(d, a[0], a[1], a[2], a[3] and big, wgrad_ws, None), ('x', 'dy', 'dw', 'workspace')),
        'bwd_weight_oihw': (lambda d, a: lib.stp3_dwconv2d_bwd_weight_oihw(d, a[0], a[1], a[2], a[3] and big, wgrad_ws, None),
                            ('x', 'dy', 'dw', 'workspace')),
    }
    res = []
    for name, (fn, ptrs) in entries.items():
        full = [p] * len(ptrs)
        res.append((f'{name}:null-dims', fn(None, full), EINVAL))
        for field in ('N', 'H', 'Ho'):
            res.append((f'{name}:{field}=0', fn(ctypes.byref(dims(**{field: 0})), full), EINVAL))
        for i, pn in enumerate(ptrs):
            res.append((f'{name}:null-{pn}', fn(ctypes.byref(ok), full[:i] + [None] + full[i + 1:]), EINVAL))
        for label, kw in (('K=4', dict(K=4)), ('K=7-stride=2', dict(K=7, stride=2)), ('stride=3', dict(stride=3)), ('dtype=7', dict(dtype=7)),
                          ('bf16-C=12', dict(C=12)), ('f32-C=6', dict(C=6, dtype=_lib.DTYPE_F32))):
            res.append((f'{name}:{label}', fn(ctypes.byref(dims(**kw)), full), EUNSUP))
    d = ctypes.byref(ok)
    res += [
        ('fwd_stats:short-workspace', lib.stp3_dwconv2d_fwd_stats(d, p, p, p, p, big, stats_ws - 1, None), ENOSPACE),
        ('fwd_stats_bn:short-workspace', lib.stp3_dwconv2d_fwd_stats_bn(d, p, p, p, p, 16.0, p, p, 1e-3, 0.01, p, p, p, big, stats_ws - 1, None), ENOSPACE),
        ('bwd_weight:short-workspace', lib.stp3_dwconv2d_bwd_weight(d, p, p, p, big, wgrad_ws - 1, None), ENOSPACE),
        ('bwd_weight_oihw:short-workspace', lib.stp3_dwconv2d_bwd_weight_oihw(d, p, p, p, big, wgrad_ws - 1, None), ENOSPACE),
        ('fwd_affine:f32', lib.stp3_dwconv2d_fwd_affine(ctypes.byref(dims(dtype=_lib.DTYPE_F32)), p, p, p, 2, p, None), EUNSUP),
        ('fwd_affine:K=7', lib.stp3_dwconv2d_fwd_affine(ctypes.byref(dims(K=7, pad_top=3, pad_left=3)), p, p, p, 2, p, None), EUNSUP),
        ('fwd_affine:act=9', lib.stp3_dwconv2d_fwd_affine(d, p, p, p, 9, p, None), EINVAL),
        ('fwd_stats_bn:count=0.5', lib.stp3_dwconv2d_fwd_stats_bn(d, p, p, p, p, 0.5, p, p, 1e-3, 0.01, p, p, p, big, stats_ws, None), EINVAL),
        ('fwd_stats_bn:running_mean-only', lib.stp3_dwconv2d_fwd_stats_bn(d, p, p, p, p, 16.0, p, p, 1e-3, 0.01, p, None, p, big, stats_ws, None), EINVAL),
    ]
    return [(n, int(rc), want) for n, rc, want in res]
