"""Trajectory-cost evaluation of the planner on the HIP library (csrc/stp3_plan.hip): the autograd face of
``stp3_traj_cost_fwd`` / ``_bwd`` (include/stp3_hip.h), i.e. of the reference's ``Cost_Function.forward``
(stp3/cost.py:26-47).  Only the cost volume is differentiable -- trajectories, occupancy, hd map and target are data
(stp3/trainer.py:175-189 passes labels and a detached camera feature).
"""
import ctypes
import math

import torch

from . import _lib, ops
from ._lib import check as _check


def supported(cost_volume, trajs):
    """GPU tensors, float32 or bf16 cost volume (float64 tensors take the torch statements of ``cost.py``)."""
    return cost_volume.is_cuda and trajs.is_cuda and cost_volume.dtype in (torch.float32, torch.bfloat16, torch.float16)


def _dims(params, B, N, T, H, W, K0, KL):
    d = _lib.PlanDims()
    d.B, d.N, d.T, d.H, d.W, d.K0, d.KL = B, N, T, H, W, K0, KL
    for k, v in params.items():
        setattr(d, k, float(v))
    return d


class _TrajCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost_volume, trajs, occupancy, drivable, lane, target, target_sum, fp0, fpl, params):
        B, N, T, _ = trajs.shape
        H, W = cost_volume.shape[-2:]
        d = _dims(params, B, N, T, H, W, fp0.shape[0], fpl.shape[0])
        dev = cost_volume.device
        fc = torch.empty(B, N, device=dev, dtype=torch.float32)
        fo = torch.empty(B, N, T, device=dev, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        cell = torch.empty(B, N, T, device=dev, dtype=torch.int32) if need else None
        scale = torch.empty(B, N, T, device=dev, dtype=torch.float32) if need else None
        _check(_lib.lib().stp3_traj_cost_fwd(ctypes.byref(d), ops._ptr(trajs), ops._ptr(cost_volume), ops._ptr(occupancy), ops._ptr(drivable),
                                            ops._ptr(lane), ops._ptr(target), ops._ptr(target_sum), ops._ptr(fp0), ops._ptr(fpl), ops._ptr(fc),
                                            ops._ptr(fo), ops._ptr(cell) if need else None, ops._ptr(scale) if need else None,
                                            ops._stream()), 'stp3_traj_cost_fwd')
        ctx.dims = d
        ctx.shape = cost_volume.shape
        ctx.mark_non_differentiable(fc)                 # comfort + progress depend on the trajectories only
        if need:
            ctx.save_for_backward(cell, scale)
        return fc, fo

    @staticmethod
    def backward(ctx, _g_fc, g_fo):
        cell, scale = ctx.saved_tensors
        g = torch.empty(ctx.shape, device=g_fo.device, dtype=torch.float32)
        _check(_lib.lib().stp3_traj_cost_bwd(ctypes.byref(ctx.dims), ops._ptr(g_fo.contiguous().float()), ops._ptr(cell), ops._ptr(scale),
                                            ops._ptr(g), ops._stream()), 'stp3_traj_cost_bwd')
        return (g,) + (None,) * 9


def traj_cost(cost_volume, trajs, occupancy, drivable, lane, target, fp0, fpl, params):
    """(cost_fc (B, N), cost_fo (B, N, T)) float32.  ``cost_volume`` (B, T, H, W); ``trajs`` (B, N, T, >= 2) unflipped;
    ``occupancy`` (B, T, H, W) any dtype (0 / 1); ``drivable`` / ``lane`` (B, H, W) preprocessed masks; ``target``
    (B, 2); ``fp0`` / ``fpl`` (K, 2) int32 footprint tables on the device; ``params``: the float fields of
    ``stp3_plan_dims``."""
    cv = cost_volume.float().contiguous()
    tr = trajs[..., :2].float().contiguous()
    tgt = target.float().contiguous()
    fc, fo = _TrajCost.apply(cv, tr, occupancy.float().contiguous(), drivable.float().contiguous(),
                             lane.float().contiguous(), tgt, tgt.sum().reshape(1), fp0, fpl, params)
    # always float32, whatever the cost volume's dtype: the reference indexes a half-precision cost volume and ADDS the
    # float32 terms (stp3/cost.py:36-47: the sum promotes to float32); rounding the costs to bf16 (spacing 0.25 .. 1 at
    # their magnitude of 32 .. 200) would re-rank near-tied trajectories and quantise the max-margin hinge
    return fc, fo


# ------------------------------------------------------------------------------------------------------------------
# The candidate set: the reference's trajectory sampler (stp3/utils/sampler.py:8-146) on csrc/stp3_sampler.hip, and the same
# algorithm in vectorised torch float64 for CPU tensors.

SAMPLER_MAX_M = 8192                        # stp3_traj_sample: the keys of one sample in one workgroup's LDS
FRAME_DT = 0.5                              # seconds between the frames the loaders keep (NuscenesData.py:431-436)
# Fresnel integrals: Maclaurin series below _FRESNEL_SPLIT, above it the auxiliary functions f, g from their Laplace integrals
# (DLMF 7.7.10-11) by the trapezoidal rule on Gaussian-weighted nodes -- the constants of csrc/stp3_sampler.hip
_FRESNEL_SPLIT, _FRESNEL_STEP, _FRESNEL_NODES, _FRESNEL_TERMS = 2.0, 0.3, 21, 22
_PI = 3.141592653589793


def _fresnel_series():
    """Maclaurin coefficients (-1)^n / ((2n)! (4n + 1)) and (-1)^n / ((2n + 1)! (4n + 3)), the factorial as a running float64
    product -- operation by operation what the kernel's workgroups build in LDS."""
    cc, cs = [], []
    for n in range(_FRESNEL_TERMS):
        f = 1.0
        for k in range(2, 2 * n + 1):
            f = f * float(k)
        sign = -1.0 if n & 1 else 1.0
        cc.append(sign / (f * float(4 * n + 1)))
        cs.append(sign / (f * float(2 * n + 1) * float(4 * n + 3)))
    return cc, cs


def fresnel_reference(x):
    """(S(x), C(x)) of a float64 tensor, scipy.special.fresnel's convention (integrals of sin / cos(pi t^2 / 2)); within
    1e-14 on |x| <= 16 (tests/test_sampler_cpu.py holds it to 1e-9 against scipy's values)."""
    x = x.double()
    ax = x.abs()
    t = 0.5 * _PI * ax * ax
    small = ax.clamp(max=_FRESNEL_SPLIT)                       # (the series is evaluated everywhere: keep it finite)
    ts = 0.5 * _PI * small * small
    t2 = ts * ts
    cc, cs = _fresnel_series()
    pc, ps = torch.full_like(ts, cc[-1]), torch.full_like(ts, cs[-1])
    for n in range(_FRESNEL_TERMS - 2, -1, -1):                # Horner
        pc = pc * t2 + cc[n]
        ps = ps * t2 + cs[n]
    c_small, s_small = small * pc, small * (ts * ps)
    inv_a = 1.0 / (ax.clamp(min=_FRESNEL_SPLIT) * math.sqrt(_PI / 2.0))
    f, g = torch.full_like(ax, 0.5), torch.zeros_like(ax)
    for k in range(1, _FRESNEL_NODES + 1):
        u = k * _FRESNEL_STEP
        w = math.exp(-(u * u))
        r = u * inv_a
        s2 = r * r
        d = 1.0 / (1.0 + s2 * s2)
        f = f + w * d
        g = g + w * s2 * d
    scale = math.sqrt(2.0) / _PI * _FRESNEL_STEP * inv_a
    f, g = f * scale, g * scale
    sn, cn = torch.sin(t), torch.cos(t)
    big = ax >= _FRESNEL_SPLIT
    c = torch.where(big, 0.5 + f * sn - g * cn, c_small)
    s = torch.where(big, 0.5 - f * cn - g * sn, s_small)
    neg = x < 0
    return torch.where(neg, -s, s), torch.where(neg, -c, c)


def sampler_counts(sample_num, possibility=(0.4, 0.2, 0.4)):
    """(left, straight, right) = int(M p) as stp3/utils/sampler.py:24-26; ValueError when they do not sum to M (the reference
    itself fails on such an M: its arrays no longer fit together)."""
    m = int(sample_num)
    left, straight, right = int(m * possibility[0]), int(m * possibility[1]), int(m * possibility[2])
    if m < 1 or left + straight + right != m:
        raise ValueError(f'sample_num = {m} with possibility {tuple(possibility)} gives {left} + {straight} + {right} '
                         f'trajectories: the counts must sum to sample_num')
    return left, straight, right


def _wrap(theta):
    return torch.remainder(theta + _PI, 2.0 * _PI) - _PI


def _sampler_inputs(v0, kappa, n_future, sample_num, draws, generator, possibility):
    v0 = torch.as_tensor(v0)
    kappa = torch.as_tensor(kappa, device=v0.device)
    v0, kappa = v0.double().reshape(-1).contiguous(), kappa.double().reshape(-1).contiguous()
    if v0.shape != kappa.shape or v0.numel() < 1:
        raise ValueError(f'v0 and kappa must hold one value per sample: {tuple(v0.shape)} and {tuple(kappa.shape)}')
    if int(n_future) < 1:
        raise ValueError(f'n_future = {n_future}')
    counts = sampler_counts(sample_num, possibility)
    need = 3 * int(sample_num) + 2 * (counts[0] + counts[2])
    if draws is None:
        draws = torch.rand(v0.numel(), need, dtype=torch.float64, device=v0.device, generator=generator)
    else:
        if tuple(draws.shape) != (v0.numel(), need) or draws.device != v0.device:
            raise ValueError(f'draws must be ({v0.numel()}, {need}) on {v0.device}: got {tuple(draws.shape)} on {draws.device}')
        draws = draws.double().contiguous()
    return v0, kappa, draws, counts


def sample_trajectories_reference(v0, kappa, n_future, sample_num, draws=None, generator=None, possibility=(0.4, 0.2, 0.4),
                                  sort=True, return_order=False):
    """``sample_trajectories`` in vectorised torch float64 on the tensors' device: stp3/utils/sampler.py:24-104, :129-144 at the
    n_future + 1 frame times, statement by statement and in its operation order."""
    v0, kappa, draws, (nl, ns, nr) = _sampler_inputs(v0, kappa, n_future, sample_num, draws, generator, possibility)
    M, Mc = int(sample_num), nl + nr
    d_acc, d_vel, d_sel, d_alpha, d_pick = draws.split([M, M, M, Mc, Mc], dim=1)
    tt = FRAME_DT * torch.arange(int(n_future) + 1, dtype=torch.float64, device=v0.device)
    acc = 10.0 * (d_acc - 0.5) + 2.0                                                  # :28
    vel = torch.where(d_sel >= 0.2, 15.0 * d_vel, v0[:, None])                        # :32-34
    L = vel[:, :, None] * tt + acc[:, :, None] * (tt * tt) / 2.0                      # :37
    L_line, L = L[:, :ns], L[:, ns:]
    alpha = ((80.0 - 6.0) * d_alpha + 6.0)[:, :, None]                                # :43
    lines = torch.stack([L_line * 0.0, L_line * 1.0, torch.zeros_like(L_line)], dim=-1)          # :47-49
    kap = kappa[:, None, None]
    kr = torch.where(kap <= 0, kap.clamp(max=-0.01), kap.clamp(min=0.01))             # :53
    radius, cx, pos = (1.0 / kr).abs(), -1.0 / kr, kr >= 0
    q = L / radius
    phi = torch.where(pos, q, _PI - q)
    circles = torch.stack([cx + radius * torch.cos(phi), 0.0 + radius * torch.sin(phi), _wrap(torch.where(pos, q, -q))], dim=-1)
    xi0 = kap.abs() / _PI                                                             # :72
    arg = (xi0 + L) / alpha
    S, C = fresnel_reference(arg)
    n0x = torch.where(kap <= 0, 1.0, -1.0).double()
    px, py = alpha * (C * 0.0 + S * n0x), alpha * (C * 1.0 + S * 0.0)                 # :79
    xs, ys = px - px[:, :, :1], py - py[:, :, :1]
    qk = kap / _PI / alpha
    theta0 = 0.5 * _PI * (qk * qk)                                                    # :84
    sign = torch.sign(kap)
    rs, rc = torch.sin(theta0 * sign), torch.cos(theta0 * sign)
    theta = _wrap((0.5 * _PI * (arg * arg) - theta0) * sign)                          # :95-101
    clothoids = torch.stack([rc * xs + rs * ys, -rs * xs + rc * ys, theta], dim=-1)
    curves = torch.where((d_pick >= 0.2)[:, :, None, None], clothoids, circles)       # :108-112
    first, second = curves[:, :nl], curves[:, nl:]
    mirrored = second * second.new_tensor([-1.0, 1.0, -1.0])                          # :132-134 / :138-140
    rows = torch.where(kappa[:, None, None, None] > 0, torch.cat([first, lines, mirrored], dim=1),
                       torch.cat([mirrored, lines, first], dim=1)).float()            # :129-142
    if sort:                                                                          # :143-144, ties by generation index
        order = torch.sort(rows[:, :, -1, 0], dim=1, stable=True).indices
        rows = torch.gather(rows, 1, order[:, :, None, None].expand_as(rows))
    else:
        order = torch.arange(M, device=rows.device).expand(rows.shape[0], M)
    return (rows, order.to(torch.int32).contiguous()) if return_order else rows


def sample_trajectories(v0, kappa, n_future, sample_num, draws=None, generator=None, possibility=(0.4, 0.2, 0.4), sort=True,
                        return_order=False):
    """The planner's candidate set, (B, sample_num, n_future + 1, 3) float32 (x lateral, y forward, heading): the reference's
    ``sample(v0, Kappa, T0, N0, tt, M)[:, ::10]`` (stp3/utils/sampler.py:8-146 as NuscenesData.get_trajectory_sampling
    :427-437 calls it) for a batch, one launch of ``stp3_traj_sample``.

    ``v0`` / ``kappa`` (B,): speed in m/s, curvature in 1/m (positive: left).  ``draws`` (B, 3 M + 2 Mc) float64 in [0, 1): the
    uniforms in the order the reference consumes its numpy stream (include/stp3_hip.h); None draws them with ``torch.rand`` on
    the inputs' device (``generator``).  ``sort``: rows in ascending lateral position of the last pose, equal (stored,
    float32) positions in ascending generation index; ``return_order`` adds (B, M) int32, the generation index of every row
    ([left | lines | right] before the sort).  CPU tensors and sample_num > SAMPLER_MAX_M take
    ``sample_trajectories_reference``."""
    v0, kappa, draws, (nl, ns, nr) = _sampler_inputs(v0, kappa, n_future, sample_num, draws, generator, possibility)
    if not v0.is_cuda or int(sample_num) > SAMPLER_MAX_M:
        return sample_trajectories_reference(v0, kappa, n_future, sample_num, draws, None, possibility, sort, return_order)
    d = _lib.SamplerDims(v0.numel(), int(sample_num), nl, ns, nr, int(n_future), FRAME_DT, 1 if sort else 0)
    trajs = torch.empty(d.B, d.M, d.n_future + 1, 3, device=v0.device, dtype=torch.float32)
    order = torch.empty(d.B, d.M, device=v0.device, dtype=torch.int32) if return_order else None
    _check(_lib.lib().stp3_traj_sample(ctypes.byref(d), ops._ptr(v0), ops._ptr(kappa), ops._ptr(draws), ops._ptr(trajs),
                                       ops._ptr(order) if return_order else None, ops._stream()), 'stp3_traj_sample')
    return (trajs, order) if return_order else trajs


# ------------------------------------------------------------------------------------------------------------------
# The planner tail of an inference call: stp3_plan_scene / stp3_plan_drive (csrc/stp3_plan.hip) for GPU tensors -- two launches
# with no host dependence -- and the torch statements of the same steps, in the same operation order, for CPU tensors.
# (Captured behind the forward in ``inference.InferenceEngine``'s graph they were no faster per tick than the eager statements
# they replace, DESIGN.md section 4.12: the engine does not hold them.)

COMMAND_CODES = {'LEFT': 0, 'FORWARD': 1, 'RIGHT': 2}
COMMAND_ALL = 3                             # any other command: all N candidates (planning_model.py:114-115)
DRIVE_MAX_STATE = 512
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


def command_codes(commands, device=None):
    """(B,) int32: 0 LEFT, 1 FORWARD, 2 RIGHT, 3 for any other string -- the kernel's table of planning_model.py:103-115."""
    if isinstance(commands, str) or not all(isinstance(c, str) for c in commands):
        raise ValueError(f'commands must be a list of strings: {commands!r}')
    return torch.tensor([COMMAND_CODES.get(c, COMMAND_ALL) for c in commands], dtype=torch.int32, device=device)


def _scene_check(segmentation, pedestrian, hdmap, n_present):
    if segmentation.ndim != 5 or hdmap.ndim != 4 or hdmap.shape[1] != 4:
        raise ValueError(f'segmentation must be (B, S, C, H, W) and hdmap (B, 4, H, W): {tuple(segmentation.shape)}, {tuple(hdmap.shape)}')
    B, S, _, H, W = segmentation.shape
    if tuple(hdmap.shape) != (B, 4, H, W):
        raise ValueError(f'hdmap {tuple(hdmap.shape)} does not fit segmentation {tuple(segmentation.shape)}')
    if pedestrian is not None and (pedestrian.ndim != 5 or tuple(pedestrian.shape[:2]) != (B, S) or
                                   tuple(pedestrian.shape[3:]) != (H, W) or pedestrian.device != segmentation.device):
        raise ValueError(f'pedestrian {tuple(pedestrian.shape)} does not fit segmentation {tuple(segmentation.shape)}')
    if not 0 <= int(n_present) < S:
        raise ValueError(f'n_present = {n_present} with {S} frames')
    if hdmap.device != segmentation.device:
        raise ValueError('segmentation and hdmap are on different devices')


def plan_scene_reference(segmentation, pedestrian, hdmap, n_present):
    """``plan_scene`` as torch statements: evaluate.py:96-106,122 and the mask heads of cost.py (``lane_mask`` / ``drivable_mask``)."""
    from .cost import drivable_mask, lane_mask
    seg = torch.argmax(segmentation, dim=2)
    ped = torch.argmax(pedestrian, dim=2) if pedestrian is not None else torch.zeros_like(seg)
    occupancy = torch.logical_or(seg, ped)[:, int(n_present):]
    return occupancy.float().contiguous(), lane_mask(hdmap[:, 0:2]).float(), drivable_mask(hdmap[:, 2:4]).float()


def plan_scene(segmentation, pedestrian, hdmap, n_present, out=None):
    """The planner's inputs from the decoder's heads: (occupancy (B, T, H, W), lane (B, H, W), drivable (B, H, W)) float32, T = S -
    n_present.  ``segmentation`` (B, S, Cs, H, W), ``pedestrian`` (B, S, Cp, H, W) or None, ``hdmap`` (B, 4, H, W): float32 or bf16
    logits in any layout.  GPU tensors: one launch of ``stp3_plan_scene``, into ``out`` (the three tensors) when given; CPU
    tensors: ``plan_scene_reference``."""
    _scene_check(segmentation, pedestrian, hdmap, n_present)
    heads = [t for t in (segmentation, pedestrian, hdmap) if t is not None]
    for t in heads:
        if t.dtype not in _DTYPES:
            raise ValueError(f'logits must be float32 or bfloat16: {t.dtype}')
    if not segmentation.is_cuda:
        return plan_scene_reference(segmentation, pedestrian, hdmap, n_present)
    B, S, Cs, H, W = segmentation.shape
    T = S - int(n_present)
    d = _lib.SceneDims()
    d.B, d.S, d.T, d.H, d.W, d.Cs, d.first = B, S, T, H, W, Cs, int(n_present)
    d.Cp = 0 if pedestrian is None else pedestrian.shape[2]
    d.seg_dtype, d.hd_dtype = _DTYPES[segmentation.dtype], _DTYPES[hdmap.dtype]
    d.ped_dtype = 0 if pedestrian is None else _DTYPES[pedestrian.dtype]
    d.seg_stride[:] = segmentation.stride()
    d.hd_stride[:] = hdmap.stride()
    if pedestrian is not None:
        d.ped_stride[:] = pedestrian.stride()
    dev = segmentation.device
    if out is None:
        out = (torch.empty(B, T, H, W, device=dev), torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev))
    occupancy, lane, drivable = out
    for t, shape in ((occupancy, (B, T, H, W)), (lane, (B, H, W)), (drivable, (B, H, W))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'out: expected a contiguous float32 {shape} tensor on {dev}, got {tuple(t.shape)} {t.dtype}')
    _check(_lib.lib().stp3_plan_scene(ctypes.byref(d), ops._ptr(segmentation), ops._ptr(pedestrian) if pedestrian is not None else None,
                                      ops._ptr(hdmap), ops._ptr(occupancy), ops._ptr(lane), ops._ptr(drivable), ops._stream()),
           'stp3_plan_scene')
    return occupancy, lane, drivable


class DriveWeights:
    """The copy of the planner's GRU cell and decoder that ``stp3_plan_drive`` reads: ONE float32 buffer (the layout of
    ``stp3_drive_dims.weights``) with ``weight_hh`` and the first decoder layer TRANSPOSED -- consecutive threads read consecutive
    addresses.  The buffer keeps its address (a captured graph could read it); ``refresh()`` rewrites it in place, ``current()`` tells
    whether the parameters still have the versions the copy was cut from."""
    NAMES = ('w_ih', 'b_ih', 'w_hh_t', 'b_hh', 'w1_t', 'b1', 'w2', 'b2')

    def __init__(self, gru, decoder, device):
        self.gru, self.decoder, self.device = gru, decoder, torch.device(device)
        if gru.input_size != 6 or not gru.bias or decoder[0].in_features != gru.hidden_size or decoder[2].out_features != 2:
            raise ValueError('plan_drive: the refinement is a GRUCell(6, Hs) with biases and Linear(Hs, Hs) - ReLU - Linear(Hs, 2)')
        self.Hs = gru.hidden_size
        sources = self._sources()
        self.buffer = torch.empty(sum(v.numel() for v in sources.values()), dtype=torch.float32, device=self.device)
        assert self.buffer.numel() == 4 * self.Hs * self.Hs + 27 * self.Hs + 2
        self.buffers, at = {}, 0                               # views of the buffer, by name
        for k, v in sources.items():
            self.buffers[k] = self.buffer[at:at + v.numel()].view(v.shape)
            at += v.numel()
        self.versions = None
        self.refresh()

    def _params(self):
        g, d = self.gru, self.decoder
        return (g.weight_ih, g.bias_ih, g.weight_hh, g.bias_hh, d[0].weight, d[0].bias, d[2].weight, d[2].bias)

    def _sources(self):
        w_ih, b_ih, w_hh, b_hh, w1, b1, w2, b2 = (p.detach() for p in self._params())
        return dict(zip(self.NAMES, (w_ih, b_ih, w_hh.t(), b_hh, w1.t(), b1, w2, b2)))

    def current(self):
        return self.versions == tuple((p.data_ptr(), p._version) for p in self._params())

    def refresh(self):
        with torch.no_grad():
            for k, v in self._sources().items():
                self.buffers[k].copy_(v)
        self.versions = tuple((p.data_ptr(), p._version) for p in self._params())


def _drive_check(trajs, cost_volume, occupancy, lane, drivable, codes, target, h0):
    if trajs.ndim != 4 or trajs.shape[-1] < 2 or trajs.dtype != torch.float32:
        raise ValueError(f'trajs must be float32 (B, N, T, >= 2): {tuple(trajs.shape)} {trajs.dtype}')
    B, N, T, _ = trajs.shape
    if N % 3 != 0 or N < 3:
        raise ValueError(f'N = {N} candidates: one third per command, N % 3 must be 0')
    if cost_volume.ndim != 4 or tuple(cost_volume.shape[:2]) != (B, T):
        raise ValueError(f'cost_volume must be (B, T, H, W) = ({B}, {T}, H, W): {tuple(cost_volume.shape)}')
    H, W = cost_volume.shape[-2:]
    for name, t, shape in (('occupancy', occupancy, (B, T, H, W)), ('lane', lane, (B, H, W)), ('drivable', drivable, (B, H, W)),
                           ('target', target, (B, 2)), ('command_codes', codes, (B,))):
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must be {shape}: {tuple(t.shape)}')
    if codes.dtype != torch.int32:
        raise ValueError(f'command_codes must be int32 (ops_plan.command_codes): {codes.dtype}')
    if h0.ndim != 2 or h0.shape[0] != B:
        raise ValueError(f'h0 must be (B, Hs): {tuple(h0.shape)}')
    if cost_volume.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f'cost_volume dtype {cost_volume.dtype}')
    return B, N, T, H, W


def plan_drive_reference(planner, trajs, cost_volume, occupancy, lane, drivable, codes, target, h0):
    """``plan_drive`` as torch statements in the kernel's operation order: every row scored by ``planner.cost_function``'s terms
    (stp3_amd/cost.py; the masks enter as one-channel maps), total = cost_fc + sum_t cost_fo, the smallest total of the
    command's range with the lowest index on an exact tie, then the GRUCell / decoder loop of ``Planning.forward``."""
    B, N, T, _ = trajs.shape
    fc, fo = planner.cost_function(cost_volume, trajs[..., :2], occupancy, lane[:, None], drivable[:, None], target)
    total = fc + fo.sum(dim=-1)
    rows = torch.arange(N, device=trajs.device)[None]
    k = codes.long()[:, None]
    third = N // 3
    allowed = torch.where((k >= 0) & (k <= 2), (rows >= k * third) & (rows < (k + 1) * third), torch.ones_like(rows, dtype=torch.bool))
    total = torch.where(allowed, total, torch.full_like(total, float('inf')))
    lowest = total.min(dim=1, keepdim=True).values
    # the first row that attains the minimum (all rows, should no total compare: the range's first row)
    index = torch.where(total == lowest, rows, torch.full_like(rows, N)).min(dim=1).values
    first = torch.where((k[:, 0] >= 0) & (k[:, 0] <= 2), k[:, 0] * third, torch.zeros_like(k[:, 0]))
    index = torch.where(index == N, first, index)
    chosen = trajs[torch.arange(B, device=trajs.device), index]
    h = h0.to(planner.GRU.weight_hh.dtype)
    tgt = target.to(h.dtype)
    point = torch.zeros(B, 2, device=h.device, dtype=h.dtype)
    refined = []
    for i in range(T):
        h = planner.GRU(torch.cat([point, chosen[:, i, :2].to(h.dtype), tgt], dim=-1), h)
        point = planner.decoder(h)
        refined.append(point)
    refined = torch.stack(refined, dim=1)
    final = torch.cat([refined, torch.zeros_like(refined[..., :1])], dim=-1)
    selected = torch.zeros(B, T, 3, device=trajs.device, dtype=trajs.dtype)
    cols = min(3, trajs.shape[-1])
    selected[..., :cols] = chosen[..., :cols]
    return final, selected, index.to(torch.int32)


def plan_drive(planner, trajs, cost_volume, occupancy, lane, drivable, codes, target, h0, weights=None, out=None):
    """Select and refine: (final_traj (B, T, 3), selected_traj (B, T, 3), selected_index (B,) int32).

    ``planner``: the ``Planning`` module (its ``cost_function`` gives the grid constants and footprint tables, ``GRU`` / ``decoder``
    the refinement).  ``trajs`` (B, N, T, >= 2) float32, any strides with a dense last axis; ``cost_volume`` (B, T, H, W);
    ``occupancy`` / ``lane`` / ``drivable``: what ``plan_scene`` returns; ``codes`` (B,) int32 (``command_codes``); ``target``
    (B, 2); ``h0`` (B, Hs).  GPU tensors: one launch of ``stp3_plan_drive`` reading ``weights`` (a ``DriveWeights``; default: the
    planner's own, ``Planning.drive_weights``), results into ``out`` when given; CPU tensors: ``plan_drive_reference``."""
    B, N, T, H, W = _drive_check(trajs, cost_volume, occupancy, lane, drivable, codes, target, h0)
    if not trajs.is_cuda:
        return plan_drive_reference(planner, trajs, cost_volume, occupancy, lane, drivable, codes, target, h0)
    Hs = planner.GRU.hidden_size
    if h0.shape[1] != Hs:
        raise ValueError(f'h0 must be (B, {Hs}): {tuple(h0.shape)}')
    if Hs % 64 != 0 or Hs > DRIVE_MAX_STATE:
        raise _lib.Stp3HipError(f'stp3_plan_drive: GRU state size {Hs} (multiples of 64 up to {DRIVE_MAX_STATE})')
    dev = trajs.device
    weights = weights if weights is not None else planner.drive_weights(dev)
    assert tuple(cost_volume.shape[-2:]) == tuple(int(v) for v in planner.cost_function.safetycost.bev_dimension[:2])
    fp0, fpl, params = planner.cost_function._kernel_inputs(dev)
    if trajs.stride(-1) != 1:
        trajs = trajs.contiguous()
    # bf16 tensors (the heads under autocast) are widened inside the kernel: no conversion launch
    if cost_volume.dtype not in _DTYPES or not cost_volume[0].is_contiguous():
        cost_volume = cost_volume.float().contiguous()
    if h0.dtype not in _DTYPES or not h0.is_contiguous():
        h0 = h0.float().contiguous()
    occupancy, lane, drivable = (t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()
                                 for t in (occupancy, lane, drivable))
    target = target.float().contiguous()
    d = _dims(params, B, N, T, H, W, fp0.shape[0], fpl.shape[0])
    q = _lib.DriveDims()
    q.Hs, q.traj_cols, q.cv_dtype, q.h0_dtype = Hs, trajs.shape[-1], _DTYPES[cost_volume.dtype], _DTYPES[h0.dtype]
    q.traj_batch_stride, q.traj_row_stride, q.traj_point_stride = trajs.stride()[:3]
    q.cv_batch_stride = cost_volume.stride(0)
    q.weights = weights.buffer.data_ptr()
    if out is None:
        out = (torch.empty(B, T, 3, device=dev), torch.empty(B, T, 3, device=dev), torch.empty(B, device=dev, dtype=torch.int32))
    final, selected, index = out
    _check(_lib.lib().stp3_plan_drive(ctypes.byref(d), ctypes.byref(q), ops._ptr(trajs), ops._ptr(cost_volume), ops._ptr(occupancy),
                                      ops._ptr(drivable), ops._ptr(lane), ops._ptr(target), ops._ptr(codes), ops._ptr(fp0), ops._ptr(fpl),
                                      ops._ptr(h0), ops._ptr(final), ops._ptr(selected), ops._ptr(index), ops._stream()),
           f'stp3_plan_drive (B {B}, N {N}, T {T}, grid {H} x {W}, footprints {fp0.shape[0]} / {fpl.shape[0]}, Hs {Hs}, trajs strides '
           f'{tuple(trajs.stride())}, cost volume stride {cost_volume.stride(0)}, cells {params["dx0"]} x {params["dx1"]} m)')
    return final, selected, index
