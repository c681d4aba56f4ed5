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
