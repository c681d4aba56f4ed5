"""Cases of the loss and label-warp kernels (csrc/stp3_loss.hip): float64 references written from the operations' definitions
and the table of shapes, types and edges at which the kernels are compared with them.  Shared by tests/test_loss_gpu.py
(MI355X), tests/hipcpu/run_loss.py (the kernel sources executed on CPU threads, checked by tests/test_loss_cpu.py) and the
kernel-free comparison of the references with the torch statements of ``stp3_amd.losses`` (tests/test_loss_cpu.py).

The references never call ``stp3_amd.losses`` / ``stp3_amd.ops_loss``:

* ``ref_ce_topk``: per-pixel loss scale[row] * w[y] * (logsumexp(z) - z[y]) (0 at ignored pixels), tau = the k-th largest loss of
  the row, take = 1 above tau, (k - #above) / #ties on the ties, 0 below; value = sum(l * take) / (rows * k); the gradient by
  autograd through l with take held constant.  A pixel ties with tau when |l - tau| <= 1e-9 * tau (float64 logsumexp is not
  shift invariant in its last bit, so exact equality would split ties that float32 arithmetic on a logit grid keeps) or when
  l == tau == 0.  It also returns the GAP, the smallest |l - tau| / tau over the pixels that are no ties: a float32 per-pixel
  loss is good to a few ulp (~5e-7 relative), so a gap >= 1e-5 keeps kernel and reference on the same side of the threshold.
* ``ref_reg_loss``: mask from channel 0 of the target only, sum over channels of |d| or d^2 times the row scale, averaged over
  max(count, 1); sign(0) = 0 in the L1 gradient.
* ``ref_warp_nearest``: the closed form bx = (2 wi + 1) / W - 1, ix = ((gx + 1) W - 1) / 2, rounding half to even, zero outside
  [0, W-1] x [0, H-1] -- what the kernel's comment specifies.  (F.affine_grid builds its base grid as linspace * (W-1)/W,
  ~4e-7 px of noise: at exact ties torch's own answer is arbitrary, so torch is the reference only away from ties.)  It also
  returns the mask of UNSURE pixels, ix or iy within eps of a half-integer (the borders -0.5 and W-0.5 included).

Every case states its precondition and ``run_case`` asserts it ON THE REFERENCE ALONE before any kernel output is looked at:
top-k cases without deliberate ties need C <= 4, a gap >= 1e-5 and the k-th largest loss to be its row's only tie; the tie
case (logits on the grid 0.5 * {-2..2}) needs every non-tie >= 1e-5 away from tau and more ties than tau's own pixel; the
general warp case needs an unsure share <= 1 %.  A seed that misses a precondition is replaced -- never the condition.

``run_case`` returns plain numbers and flags; the bounds live in the test files."""
import ctypes
import math

import torch

IGNORE = 255
DISCOUNT = 0.75            # future discount: its powers are exact in float32, so float32 and float64 row scales are equal
GOUT = 0.75                # incoming gradient of every backward pass (not 1: a dropped factor shows)
TIE_REL = 1e-9
MIN_GAP = 1e-5
WARP_EPS = 1e-3
WEIGHTS = {2: [1.0, 2.0], 3: [1.0, 2.0, 0.5], 4: [1.0, 2.0, 0.5, 1.5]}

# The bounds of the test files -- from the arithmetic, never from an observation (the observed figures are recorded in the
# docstring of tests/test_loss_gpu.py):
# values: rows are accumulated in double, expf / logf are documented at 1 ulp and a few float32 roundings per pixel cannot add up
# to 1e-6 relative -- a margin of at least 10x (and the figure of the older GPU loss test)
VALUE_RTOL = 1e-5
# float32 gradients, relative to the reference's largest entry: ~8 float32 roundings (C <= 4), a 48-term sum (C = 48), margin 4x
GRAD_RTOL_F32, GRAD_RTOL_F32_C48 = 2e-6, 1e-5
# bf16 gradients, per element: |got - ref| <= 2^-7 |ref| + 1e-6 max|ref| (one bf16 ulp) -- ``grad_ulp_excess`` is the ratio, <= 1
GRAD_ULP_EXCESS = 1.0


def _prod(v):
    out = 1
    for x in v:
        out *= int(x)
    return out


# ---- references -----------------------------------------------------------------------------------------------------
def ref_ce_topk(logits, labels, weights, row_scale, k, ignore=IGNORE):
    """logits (rows, C, P), labels (rows, P), weights (C,) or None, row_scale (rows,) or None ->
    dict(value, grad (rows, C, P) float64, gap, n_ties (per row, 0 on the sum route), tau, live (rows, P))."""
    z = logits.detach().double().clone().requires_grad_()
    rows, c, p = z.shape
    y = labels.reshape(rows, p).long()
    live = y != ignore
    ys = torch.where(live, y, torch.zeros_like(y))
    nll = torch.logsumexp(z, dim=1) - z.gather(1, ys[:, None]).squeeze(1)
    if weights is not None:
        nll = nll * weights.double()[ys]
    if row_scale is not None:
        nll = nll * row_scale.double()[:, None]
    loss = torch.where(live, nll, torch.zeros_like(nll))
    ld = loss.detach()
    if k <= 0 or k >= p:
        take, denom = torch.ones_like(ld), rows * p
        gap, n_ties, tau = math.inf, torch.zeros(rows, dtype=torch.long), None
    else:
        tau = ld.topk(k, dim=1).values[:, -1:]
        tie = ((ld - tau).abs() <= TIE_REL * tau) | ((ld == 0) & (tau == 0))
        above = (ld > tau) & ~tie
        n_above, n_ties = above.sum(1, keepdim=True), tie.sum(1, keepdim=True)
        take = above.double() + tie.double() * (k - n_above).double() / n_ties.double()
        rel = torch.where(tau > 0, (ld - tau).abs() / tau.clamp_min(1e-300), torch.full_like(ld, math.inf))
        rel = torch.where(tie, torch.full_like(rel, math.inf), rel)
        gap, n_ties, tau, denom = float(rel.min()), n_ties.squeeze(1), tau.squeeze(1), rows * k
    value = (loss * take).sum() / denom
    grad, = torch.autograd.grad(value, z)
    return {'value': value.detach(), 'grad': grad, 'gap': gap, 'n_ties': n_ties, 'tau': tau, 'live': live}


def ref_reg_loss(pred, target, row_scale, norm, ignore=float(IGNORE)):
    """pred, target (rows..., C, H, W), row_scale (rows,) or None -> dict(value, grad like pred float64, count, mask)."""
    x = pred.detach().double().clone().requires_grad_()
    t = target.detach().double()
    mask = t[..., 0, :, :] != ignore
    d = x - t
    per = (d.abs() if norm == 1 else d * d).sum(dim=-3)
    if row_scale is not None:
        per = per * row_scale.double().view(*per.shape[:-2], 1, 1)
    count = int(mask.sum())
    value = torch.where(mask, per, torch.zeros_like(per)).sum() / max(count, 1)
    grad, = torch.autograd.grad(value, x)
    return {'value': value.detach(), 'grad': grad, 'count': count, 'mask': mask}


def ref_warp_nearest(x, theta, identity=None, eps=WARP_EPS):
    """x (F, C, H, W), theta (F, 2, 3), identity: F flags or None -> (y like x, unsure (F, H, W) bool)."""
    f, c, h, w = x.shape
    th = theta.detach().double().reshape(f, 6)
    wi = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    hi = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    bx, by = (2 * wi + 1) / w - 1, (2 * hi + 1) / h - 1
    co = [th[:, i].view(f, 1, 1) for i in range(6)]
    gx = bx * co[0] + by * co[1] + co[2]
    gy = bx * co[3] + by * co[4] + co[5]
    ix, iy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2
    rx, ry = torch.round(ix), torch.round(iy)                         # half to even
    inside = (rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1)
    src = (ry.clamp(0, h - 1) * w + rx.clamp(0, w - 1)).long()
    unsure = (((ix - 0.5) - torch.round(ix - 0.5)).abs() <= eps) | (((iy - 0.5) - torch.round(iy - 0.5)).abs() <= eps)
    own = torch.arange(h * w).view(1, h, w).expand(f, h, w)
    if identity is not None:
        flag = torch.as_tensor(list(identity)).bool().view(f, 1, 1)
        src = torch.where(flag, own, src)
        inside = inside | flag
        unsure = unsure & ~flag
    y = x.reshape(f, c, h * w).gather(2, src.view(f, 1, h * w).expand(f, c, h * w)).view(f, c, h, w)
    y = torch.where(inside.view(f, 1, h, w), y, torch.zeros_like(y))
    return y, unsure


# ---- inputs ---------------------------------------------------------------------------------------------------------
def row_scale_of(lead, n_present):
    """The future-discount factor of every (sample, frame) row as ``stp3_amd.losses`` builds it: 1 for the first
    ``n_present`` frames, DISCOUNT ** i after; None without a discount."""
    if n_present is None:
        return None
    b, s = (1, lead[0]) if len(lead) == 1 else (_prod(lead[:-1]), lead[-1])
    one = [1.0] * n_present + [DISCOUNT ** i for i in range(1, s - n_present + 1)]
    return torch.tensor(one, dtype=torch.float32).repeat(b)


def ce_inputs(shape, dtype='f32', layout='nchw', mode='randn', ignored='block', label_dtype='i64', seed=0, **_):
    """logits (lead..., C, H, W) in the case's type and memory layout, labels (lead..., H, W); both on the CPU."""
    *lead, c, h, w = shape
    rows, p = _prod(lead), h * w
    g = torch.Generator().manual_seed(seed)
    if mode == 'grid':
        z = torch.randint(-2, 3, (rows, c, h, w), generator=g).float() * 0.5
    else:
        z = torch.randn(rows, c, h, w, generator=g) * 2
        if mode == 'wide':                       # losses over many exponents: radix pass 0 chooses among many bins
            z = z * 0.5 * 10 ** (torch.rand(rows, 1, h, w, generator=g) * 4.5 - 3)
            z = (z * 300).clamp(-1e4, 1e4) if dtype == 'bf16' else z.clamp(-80, 80)
    z = z.to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    if layout == 'nhwc':
        z = z.contiguous(memory_format=torch.channels_last)
    z = z.view(*lead, c, h, w)
    y = (torch.rand(rows, p, generator=g) < 0.2).long() if c == 2 else torch.randint(0, c, (rows, p), generator=g)
    if ignored == 'block':
        y[1 % rows, :max(1, p // 10)] = IGNORE
    elif ignored == 'few-live':                  # row 0: nothing live; row 1: 100 live pixels (fewer than k)
        y[0] = IGNORE
        y[1, 100:] = IGNORE
    y = y.view(*lead, h, w)
    return z, y.to(torch.int32) if label_dtype == 'i32' else y


def reg_inputs(shape, dtype='f32', masked='mixed', equal_set=False, seed=0, **_):
    """pred, target (b, s, C, H, W) on the CPU.  'mixed': rows h < 3 carry 255 in target channel 0 (masked); with C > 1 the
    pixels (h = H-1, w < 4) carry 255 in channel 1 ONLY (not masked; pred is near 255 there so that the difference stays of
    order one); ``equal_set``: pred == target exactly on row h = 5."""
    b, s, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(shape, generator=g)
    tgt = torch.randn(shape, generator=g)
    if masked == 'mixed':
        tgt[:, :, 0, :3] = float(IGNORE)
        if c > 1:
            tgt[:, :, 1, h - 1, :4] = float(IGNORE)
            pred[:, :, 1, h - 1, :4] += float(IGNORE)
    elif masked == 'all':
        tgt[:, :, 0] = float(IGNORE)
    pred = pred.to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    if equal_set:
        tgt[:, :, :, 5] = pred[:, :, :, 5].float()
    return pred, tgt


def exact_warp_inputs(h, w):
    """x: a distinct float32 integer per (frame, channel, pixel); thetas whose every step is exact in float32 at power-of-two
    sizes; identity flags on the last two frames (their thetas must be ignored); per frame: does it tie."""
    frames = [('identity', [1, 0, 0, 0, 1, 0], False), ('shift', [1, 0, 2 / w, 0, 1, 0], False),
              ('half', [1, 0, 1 / w, 0, 1, 1 / h], True), ('half-neg', [1, 0, -1 / w, 0, 1, -3 / h], True),
              ('rot180', [-1, 0, 0, 0, -1, 0], False), ('xflip', [-1, 0, 0, 0, 1, 0], False)]
    if h == w:
        frames.append(('rot90', [0, -1, 0, 1, 0, 0], False))
    frames += [('off-map', [1, 0, 4, 0, 1, 0], False), ('flag-half', [1, 0, 1 / w, 0, 1, 1 / h], False),
               ('flag-off-map', [1, 0, 4, 0, 1, 0], False)]
    f, c = len(frames), 2
    x = (torch.arange(f * c * h * w) + 1).float().view(f, c, h, w)
    theta = torch.tensor([t for _, t, _ in frames], dtype=torch.float32).view(f, 2, 3)
    identity = [int(n.startswith('flag')) for n, _, _ in frames]
    return x, theta, identity, [n for n, _, _ in frames], [t for _, _, t in frames]


def general_warp_inputs(seed):
    f, c, h, w = 6, 3, 50, 47
    g = torch.Generator().manual_seed(seed)
    x = (torch.arange(f * c * h * w) + 1).float().view(f, c, h, w)
    ang = torch.randn(f, generator=g) * 0.3
    tx, ty = torch.randn(f, generator=g) * 0.2, torch.randn(f, generator=g) * 0.2
    theta = torch.stack([torch.cos(ang), -torch.sin(ang), tx, torch.sin(ang), torch.cos(ang), ty], dim=-1).view(f, 2, 3)
    return x, theta


# ---- comparisons ----------------------------------------------------------------------------------------------------
def _bit_zero(t):
    """Elementwise: all bits of the float32 / bf16 value are zero (+0, not -0)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16) == 0


def _compare(value, grad, ref_value, ref_grad, repeat_equal):
    """Plain figures of one operator run against its reference (``grad`` in the kernel's type, on the CPU)."""
    got_v, ref_v = float(value), float(ref_value)
    gd = grad.double()
    diff = (gd - ref_grad).abs()
    gmax = float(ref_grad.abs().max())
    out = {'value': got_v, 'ref_value': ref_v,
           'value_err': abs(got_v - ref_v) / abs(ref_v) if ref_v != 0 else (0.0 if got_v == 0 else math.inf),
           'grad_err': float(diff.max()) / gmax if gmax > 0 else (0.0 if float(gd.abs().max()) == 0 else math.inf),
           # one bf16 ulp per element: |got - ref| / (2^-7 |ref| + 1e-6 max|ref|), must stay <= 1
           'grad_ulp_excess': float((diff / (2.0 ** -7 * ref_grad.abs() + 1e-6 * gmax).clamp_min(1e-300)).max()) if gmax > 0
           else (0.0 if float(gd.abs().max()) == 0 else math.inf),
           'zeros_are_bit_zero': bool(_bit_zero(grad)[ref_grad == 0].all()), 'ref_zero_share': float((ref_grad == 0).double().mean()),
           'finite': bool(math.isfinite(got_v) and torch.isfinite(gd).all()), 'repeat_equal': repeat_equal,
           'grad_dtype': str(grad.dtype), 'grad_max': gmax}
    return out


def _to(t, dev):
    return None if t is None else t.to(dev)


REPEAT = True              # run every operator twice and compare the bits (the host stand-in's driver turns it off: its budget)


def _twice(fn):
    """Run ``fn() -> (value, grad)`` twice: (value, grad) of the first run on the CPU and whether the second run equals it
    (None when ``REPEAT`` is off)."""
    v0, g0 = fn()
    if not REPEAT:
        return v0.cpu(), g0.cpu(), None
    v1, g1 = fn()
    return v0.cpu(), g0.cpu(), bool(torch.equal(v0, v1) and torch.equal(g0, g1))


def _ce_refs(z, y, weights, row_scale, k):
    *lead, c, h, w = z.shape
    rows = _prod(lead)
    return ref_ce_topk(z.reshape(rows, c, h * w), y.reshape(rows, h * w), weights, row_scale, k)


def _assert_ce_precondition(ref, c, k, p, ties):
    """On the reference alone.  Sum route (k <= 0 or k >= P): nothing to select."""
    if k <= 0 or k >= p:
        return
    assert c <= 4, 'top-k cases keep C <= 4: the gap argument counts a few float32 roundings per pixel'
    assert ref['gap'] >= MIN_GAP, f'gap {ref["gap"]:.3g} < {MIN_GAP}: choose another seed'
    positive = ref['tau'] > 0
    if ties:
        assert int(ref['n_ties'][positive].min()) > 1, 'the tie case must tie at the threshold in every row'
    else:                                         # (tau == 0: fewer than k live pixels, the ignored ones tie with it by design)
        assert bool((ref['n_ties'][positive] == 1).all()), 'accidental tie at the threshold: choose another seed'


def run_ce(ops, dev, shape, k, dtype='f32', layout='nchw', mode='randn', ignored='block', label_dtype='i64', weights=True,
           n_present=None, ties=False, seed=0):
    from stp3_amd import ops_loss
    *lead, c, h, w = shape
    z, y = ce_inputs(shape, dtype, layout, mode, ignored, label_dtype, seed)
    cw = torch.tensor(WEIGHTS[c]) if weights else None
    rs = row_scale_of(lead, n_present)
    ref = _ce_refs(z, y, cw, rs, k)
    _assert_ce_precondition(ref, c, k, h * w, ties)
    zd, yd, cwd, rsd = z.to(dev), y.to(dev), _to(cw, dev), _to(rs, dev)

    def once():
        x = zd.detach().clone().requires_grad_()
        assert x.stride() == z.stride()
        v = ops_loss.ce_topk_mean(x, yd, cwd, rsd, k, IGNORE)
        v.backward(torch.tensor(GOUT, device=v.device))
        return v.detach(), x.grad.detach()
    value, grad, same = _twice(once)
    out = _compare(value, grad, ref['value'], ref['grad'].view(z.shape) * GOUT, same)
    dead = ~ref['live'].view(*lead, 1, h, w).expand(z.shape)
    out.update(gap=ref['gap'], classes=c, pixels=h * w, k=k, ignored_share=float(dead.double().mean()),
               ignored_are_bit_zero=bool(_bit_zero(grad)[dead].all()), grad_layout_kept=bool(grad.stride() == z.stride()),
               max_ties=int(ref['n_ties'].max()), min_tau=float(ref['tau'].min()) if ref['tau'] is not None else -1.0)
    return out


HD_WEIGHTS, HD_TRAIN, HD_TOPK, HD_RATIO = [[1.0, 5.0], [1.0, 1.0]], [1.0, 2.0], [True, False], [0.25, 0.25]


def hdmap_inputs(seed):
    b, h, w = 2, 25, 40
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(b, 4, h, w, generator=g) * 2).contiguous(memory_format=torch.channels_last)
    tgt = (torch.rand(b, 2, h, w, generator=g) < 0.3).long()
    tgt[0, :, :2] = IGNORE
    return pred, tgt


def run_hdmap(ops, dev, seed=0):
    """``split(2, dim=1)`` pieces of a 4-channel channels-last map: not dense, so the binding copies them; element 0 takes the
    250 largest of 1000 pixels, element 1 all of them.  Directly and through ``losses.HDmapLoss``."""
    from stp3_amd import losses as L, ops_loss
    pred, tgt = hdmap_inputs(seed)
    b, _, h, w = pred.shape
    ks = [int(HD_RATIO[i] * h * w) if HD_TOPK[i] else 0 for i in range(2)]
    refs = [ref_ce_topk(pred[:, 2 * i:2 * i + 2].reshape(b, 2, h * w), tgt[:, i].reshape(b, h * w), torch.tensor(HD_WEIGHTS[i]),
                        None, ks[i]) for i in range(2)]
    _assert_ce_precondition(refs[0], 2, ks[0], h * w, False)
    ref_value = sum(r['value'] * t for r, t in zip(refs, HD_TRAIN))
    ref_grad = torch.cat([r['grad'].view(b, 2, h, w) * t for r, t in zip(refs, HD_TRAIN)], dim=1) * GOUT
    pd, td = pred.to(dev), tgt.to(dev)
    cw = torch.tensor(HD_WEIGHTS).to(dev)
    module = L.HDmapLoss(torch.tensor(HD_WEIGHTS), HD_TRAIN, HD_TOPK, HD_RATIO).to(dev)

    def direct():
        x = pd.detach().clone().requires_grad_()
        pieces = x.split(2, dim=1)
        assert not pieces[0].is_contiguous() and not ops_loss._dense(pieces[0])
        v = sum(ops_loss.ce_topk_mean(pieces[i], td[:, i], cw[i], None, ks[i], IGNORE) * HD_TRAIN[i] for i in range(2))
        v.backward(torch.tensor(GOUT, device=v.device))
        return v.detach(), x.grad.detach()

    def through_module():
        x = pd.detach().clone().requires_grad_()
        v = module(x, td)
        v.backward(torch.tensor(GOUT, device=v.device))
        return v.detach(), x.grad.detach()
    value, grad, same = _twice(direct)
    mv, mg = through_module()
    out = _compare(value, grad, ref_value, ref_grad, same)
    out.update(gap=refs[0]['gap'], module_equal=bool(torch.equal(mv.cpu(), value) and torch.equal(mg.cpu(), grad)))
    return out


def run_reg(ops, dev, shape, norm, dtype='f32', masked='mixed', n_present=None, equal_set=False, noncontig=False, seed=0):
    from stp3_amd import ops_loss
    b, s, c, h, w = shape
    pred, tgt = reg_inputs(shape, dtype, masked, equal_set, seed)
    rs = row_scale_of((b, s), n_present)
    ref = ref_reg_loss(pred, tgt, rs, norm)
    ref_grad = ref['grad'] * GOUT
    if masked == 'mixed' and c > 1:               # the case is what it claims to be: 255 in channel 1 alone does not mask
        assert bool(ref['mask'][:, :, h - 1, :4].all()) and float(ref_grad[:, :, 1, h - 1, :4].abs().max()) > 0
    if equal_set:
        assert bool((ref_grad[:, :, :, 5] == 0).all()) and bool(ref['mask'][:, :, 5].all())
    assert ref['count'] == {'mixed': b * s * (h - 3) * w, 'none': b * s * h * w, 'all': 0}[masked]
    td, rsd = tgt.to(dev), _to(rs, dev)
    if noncontig:                                 # pred is a column slice of a wider tensor: the binding copies it
        wide = torch.zeros(b, s, c, h, w + 3, dtype=pred.dtype)
        wide[..., :w] = pred
        pd = wide.to(dev)
    else:
        pd = pred.to(dev)

    def once():
        leaf = pd.detach().clone().requires_grad_()
        x = leaf[..., :w] if noncontig else leaf
        assert x.is_contiguous() != noncontig
        v = ops_loss.regression_loss(x, td, rsd, norm, float(IGNORE))
        v.backward(torch.tensor(GOUT, device=v.device))
        return v.detach(), leaf.grad.detach()
    value, grad, same = _twice(once)
    pad_zero = True
    if noncontig:
        pad_zero = bool((grad[..., w:] == 0).all())
        grad = grad[..., :w]
    out = _compare(value, grad, ref['value'], ref_grad, same)
    out.update(count=ref['count'], pixels=b * s * h * w, pad_zero=pad_zero,
               masked_are_bit_zero=bool(_bit_zero(grad)[(~ref['mask'])[:, :, None].expand(shape)].all()))
    return out


def run_warp(ops, dev, mode, h=0, w=0, seed=0):
    from stp3_amd import geometry as geo, ops_loss
    if mode == 'exact':
        x, theta, identity, names, tie = exact_warp_inputs(h, w)
    else:
        x, theta = general_warp_inputs(seed)
        identity, names, tie = None, None, None
    ref, unsure = ref_warp_nearest(x, theta, identity, WARP_EPS)
    unsure_share = float(unsure.double().mean())
    off_share = float((ref[:, 0] == 0).double().mean())
    out = {'mode': mode, 'unsure_share': unsure_share, 'off_map_share': off_share, 'distinct_sources': bool(x.unique().numel() == x.numel())}
    if mode == 'exact':
        # away from ties the closed form is torch's own answer (float32 F.affine_grid + F.grid_sample on the CPU)
        plain = [i for i, (t, fl) in enumerate(zip(tie, identity)) if not t and not fl]
        out['ref_equals_torch_without_ties'] = bool(torch.equal(geo.warp_with_theta(x[plain], theta[plain], 'nearest'), ref[plain]))
        out['off_map_frame_zero'] = bool((ref[names.index('off-map')] == 0).all())
        out['flagged_frames_copied'] = bool(all(torch.equal(ref[i], x[i]) for i, fl in enumerate(identity) if fl))
        out['tie_frames_all_unsure'] = bool(all(bool(unsure[i].all()) for i, t in enumerate(tie) if t))
        assert out['ref_equals_torch_without_ties'] and out['off_map_frame_zero'] and out['flagged_frames_copied']
    else:
        assert unsure_share <= 0.01, f'unsure share {unsure_share:.4f} > 1 %: choose another seed'
        assert off_share >= 0.05, 'the zero branch must be exercised'
    xd, thd = x.to(dev), theta.to(dev)
    got = ops_loss.warp_nearest(xd, thd, identity).cpu()
    # (the second run takes the flags as a device tensor, the first as a list)
    again = ops_loss.warp_nearest(xd, thd, None if identity is None else torch.tensor(identity, dtype=torch.int32).to(dev)).cpu()
    wrong = got != ref
    sure = ~unsure[:, None].expand_as(wrong)
    out.update(equal=bool(torch.equal(got, ref)), mismatches_sure=int((wrong & sure).sum()), mismatches_unsure=int((wrong & ~sure).sum()),
               repeat_equal=bool(torch.equal(got, again)))
    return out


def accumulate_check(ops, dev, seed=0):
    """stp3_ce_topk_fwd through the binding with accumulate = 1 on a preset ``out``: preset + value (one float32 addition)."""
    from stp3_amd import _lib
    rows, c, p, k, preset = 3, 2, 1000, 250, 2.5
    z, y = ce_inputs((rows, c, 25, 40), seed=seed)
    cw, rs = torch.tensor(WEIGHTS[c]), row_scale_of((rows,), 1)
    ref = _ce_refs(z, y, cw, rs, k)
    _assert_ce_precondition(ref, c, k, p, False)
    zd, yd, cwd, rsd = z.to(dev), y.reshape(rows, p).to(dev), cw.to(dev), rs.to(dev)
    lib = _lib.lib()
    dims = _lib.CeDims(rows, p, c, k, IGNORE, _lib.DTYPE_F32, c * p, p, 1)
    need = ctypes.c_size_t()
    _lib.check(lib.stp3_ce_topk_workspace_bytes(ctypes.byref(dims), ctypes.byref(need)), 'stp3_ce_topk_workspace_bytes')
    ws = torch.empty(max(need.value, 64), dtype=torch.uint8, device=dev)
    loss_px = torch.empty(rows, p, dtype=torch.float32, device=dev)
    sel = torch.empty(rows, 2, dtype=torch.float32, device=dev)
    res = []
    for acc in (0, 1):
        out = torch.full((1,), preset, dtype=torch.float32, device=dev)
        _lib.check(lib.stp3_ce_topk_fwd(ctypes.byref(dims), zd.data_ptr(), yd.data_ptr(), cwd.data_ptr(), rsd.data_ptr(),
                                        loss_px.data_ptr(), sel.data_ptr(), 1.0 / (rows * k), acc, out.data_ptr(), ws.data_ptr(),
                                        need.value, ops._stream_handle()), 'stp3_ce_topk_fwd')
        res.append(out.cpu())
    ref_v = float(ref['value'])
    return {'value': float(res[0]), 'accumulated': float(res[1]), 'preset': preset,
            'value_err': abs(float(res[0]) - ref_v) / abs(ref_v),
            'accumulated_equal': bool(torch.equal(res[1], torch.full((1,), preset) + res[0]))}


KINDS = {'ce': run_ce, 'hdmap': run_hdmap, 'reg': run_reg, 'warp': run_warp, 'accumulate': accumulate_check}


def run_case(ops, device, kind, **case):
    """One case on ``device`` through ``stp3_amd.ops_loss`` -> dict of plain numbers and flags (``kind`` added)."""
    out = KINDS[kind](ops, device, **case)
    out['kind'] = kind
    return out


def case_list():
    """[(name, keyword arguments of ``run_case``)].  Rows are kept small; P is what matters."""
    base = dict(kind='ce', shape=(3, 2, 25, 40), k=250, n_present=1, seed=1)
    ce = [
        ('base', dict(base)),
        # bf16, channels-last (stride_c = 1, stride_p = C), as the 5-D (b, s, C, H, W) view the model hands over
        ('base-bf16-nhwc', dict(base, shape=(1, 3, 2, 25, 40), dtype='bf16', layout='nhwc', seed=0)),
        # rows shorter than a wave / than the workgroup: most of the 1024 threads hold only padding
        ('short-p5', dict(kind='ce', shape=(3, 4, 1, 5), k=2, n_present=1, seed=1)),
        ('short-p63', dict(kind='ce', shape=(3, 4, 7, 9), k=16, n_present=1, seed=2)),
        ('k-edges-k1', dict(kind='ce', shape=(2, 2, 25, 41), k=1, seed=3)),
        ('k-edges-kPm1', dict(kind='ce', shape=(2, 2, 25, 41), k=1024, seed=3)),
        ('k-edges-kP', dict(kind='ce', shape=(2, 2, 25, 41), k=1025, seed=3)),               # the sum route
        ('k-edges-k0', dict(kind='ce', shape=(2, 2, 25, 41), k=0, seed=3)),
        # around kSelT = 1024 threads: the last thread's first element, every thread one, the first thread's second
        ('selT-edges-p1023', dict(kind='ce', shape=(2, 3, 31, 33), k=255, n_present=1, seed=4)),
        ('selT-edges-p1024', dict(kind='ce', shape=(2, 3, 32, 32), k=256, n_present=1, seed=5)),
        ('selT-edges-p1025', dict(kind='ce', shape=(2, 3, 25, 41), k=256, n_present=1, seed=6)),
        # kSelOwn * kSelT = 40 960: the last register-cached size, and the kernel that re-reads the row
        ('cached-edge-p40960', dict(kind='ce', shape=(2, 2, 40, 1024), k=10240, seed=7)),
        ('cached-edge-p41000', dict(kind='ce', shape=(2, 2, 41, 1000), k=10250, seed=8)),
        ('ties', dict(base, mode='grid', ties=True, seed=9)),
        ('few-live', dict(base, ignored='few-live', seed=10)),
        ('wide-range-f32', dict(base, mode='wide', seed=11)),
        ('wide-range-bf16', dict(base, mode='wide', dtype='bf16', seed=14)),
        ('depth', dict(kind='ce', shape=(1, 2, 3, 48, 7, 9), k=0, weights=False, ignored='none', seed=13)),
        ('hdmap-split', dict(kind='hdmap', seed=14)),
        ('labels-int32', dict(base, label_dtype='i32', seed=15)),
    ]
    small = (2, 3, 2, 12, 17)
    reg = [
        ('reg-l1-f32', dict(kind='reg', shape=small, norm=1, n_present=1, equal_set=True, seed=20)),
        ('reg-l2-f32', dict(kind='reg', shape=small, norm=2, n_present=1, seed=21)),
        ('reg-l1-bf16', dict(kind='reg', shape=small, norm=1, dtype='bf16', n_present=2, equal_set=True, seed=22)),
        ('reg-l2-bf16', dict(kind='reg', shape=small, norm=2, dtype='bf16', n_present=2, seed=23)),
        ('reg-l1-f32-c1', dict(kind='reg', shape=(2, 3, 1, 12, 17), norm=1, seed=24)),
        ('reg-l2-bf16-c1', dict(kind='reg', shape=(2, 3, 1, 12, 17), norm=2, dtype='bf16', n_present=1, seed=25)),
        ('reg-none-ignored', dict(kind='reg', shape=small, norm=2, masked='none', seed=26)),
        ('reg-all-ignored', dict(kind='reg', shape=small, norm=1, masked='all', n_present=1, seed=27)),
        # rows * P = 6 * 150 * 150 = 135 000 > 512 * 256: the forward's grid-stride loop runs
        ('reg-grid-stride', dict(kind='reg', shape=(2, 3, 1, 150, 150), norm=2, n_present=1, seed=28)),
        ('reg-noncontig', dict(kind='reg', shape=small, norm=1, n_present=1, noncontig=True, seed=29)),
    ]
    warp = [
        ('warp-exact-16x16', dict(kind='warp', mode='exact', h=16, w=16)),
        ('warp-exact-8x32', dict(kind='warp', mode='exact', h=8, w=32)),
        ('warp-general', dict(kind='warp', mode='general', seed=30)),
    ]
    return ce + reg + warp + [('accumulate', dict(kind='accumulate', seed=16))]


# what the host stand-in runs in seconds: every row of at most 1025 pixels, every regression case but the 135 000-pixel one
HOST_SKIP = ('cached-edge-p40960', 'cached-edge-p41000', 'reg-grid-stride')


def host_names():
    return [n for n, _ in case_list() if n not in HOST_SKIP]
