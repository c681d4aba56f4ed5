"""CPU: the planner's trajectory sampler (stp3_amd.ops_plan.sample_trajectories; csrc/stp3_sampler.hip) against the
reference's own sampler, stp3/utils/sampler.py:8-146, recorded by scripts/make_golden_sampler.py in tests/golden/sampler.npz:
six (v0, kappa, M, n_future) cases with the uniform stream the reference consumed, its rows in generation order and its
sorted keys, plus scipy's Fresnel integrals on a grid.

Rows are compared by identity (generation order), never row by row after sorting: every 1 800-row case has dozens of
neighbouring keys closer than 1e-4 m, so the sorted position of a row is not stable under rounding; the ordering is checked
by its own properties.

Bounds: positions 1.6e-5 m -- two float32 spacings at 64-128 m, one from each side's rounding of float64 values that agree
to ~1e-9; headings 1e-6 rad of the difference wrapped into (-pi, pi] (float32 spacing at pi: 2.4e-7; a heading at +-pi may
land on either side); Fresnel 1e-9 (x 80, the largest clothoid scale, stays two orders below a float32 spacing); kernel
against the torch path on the same draws: one float32 spacing of each value's magnitude (two float64 results that differ in
their last bits can round to neighbouring float32 values, no further)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
POS_TOL, HEADING_TOL, FRESNEL_TOL = 1.6e-5, 1e-6, 1e-9
CASES = range(6)


def case(g, i, device='cpu'):
    """(v0 (1,), kappa (1,), n_future, M, draws (1, 3 M + 2 Mc)) of fixture case i."""
    v0, kappa, m, nf = g[f'c{i}_params']
    return (torch.tensor([v0], device=device), torch.tensor([kappa], device=device), int(nf), int(m),
            torch.from_numpy(g[f'c{i}_draws'])[None].to(device))


def check_rows(rows, want, what):
    """Generation-order rows (M, T, 3) against the fixture's: every value, nothing masked."""
    rows, want = np.asarray(rows, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert rows.shape == want.shape and np.isfinite(rows).all()
    pos = np.abs(rows[..., :2] - want[..., :2]).max()
    dh = rows[..., 2] - want[..., 2]
    heading = np.abs(-((-dh + math.pi) % (2 * math.pi) - math.pi)).max()            # wrapped into (-pi, pi]
    print(f'{what}: position error {pos:.3e} m (bound {POS_TOL}), heading error {heading:.3e} rad (bound {HEADING_TOL})')
    assert pos <= POS_TOL, (what, pos)
    assert heading <= HEADING_TOL, (what, heading)


def check_sorting(sorted_rows, order, unsorted_rows, want_keys, what):
    sorted_rows, order, unsorted_rows = np.asarray(sorted_rows), np.asarray(order), np.asarray(unsorted_rows)
    m = len(unsorted_rows)
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(m)), f'{what}: order is not a permutation'
    assert np.array_equal(sorted_rows.view(np.uint32), unsorted_rows[order].view(np.uint32)), f'{what}: rows != unsorted[order]'
    keys = sorted_rows[:, -1, 0]
    assert (np.diff(keys) >= 0).all(), f'{what}: keys decrease'
    tied = np.diff(keys) == 0
    assert (np.diff(order)[tied] > 0).all(), f'{what}: equal keys not in ascending generation index'
    key_err = np.abs(keys.astype(np.float64) - want_keys).max()
    print(f'{what}: {int(tied.sum())} tied neighbours, sorted keys within {key_err:.3e} m of the reference (bound {POS_TOL})')
    assert key_err <= POS_TOL, (what, key_err)


def check_one_spacing(a, b, what):
    """Every value of two float32 results within one float32 spacing of its magnitude."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    spacing = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    worst = float((diff / spacing).max())
    print(f'{what}: {int((diff > 0).sum())} of {a.size} values differ, at most {worst:.2f} float32 spacings')
    assert worst <= 1.0, (what, worst)


def test_fixture_holds_data_only():
    g = H.load('sampler.npz')
    assert os.path.getsize(os.path.join(H.GOLDEN, 'sampler.npz')) <= 1 << 20
    assert sorted(g.files) == sorted([f'c{i}_{k}' for i in CASES for k in ('params', 'draws', 'rows', 'keys')] +
                                     ['fresnel_x', 'fresnel_s', 'fresnel_c'])
    assert all(g[k].dtype in (np.float32, np.float64) for k in g.files)
    assert [tuple(g[f'c{i}_params']) for i in CASES] == [(5.0, 0.0, 1800, 6), (8.3, 0.05, 1800, 6), (0.0, -0.3, 1800, 6),
                                                         (12.0, 0.004, 600, 4), (3.0, -0.004, 60, 4), (14.9, 0.9, 600, 6)]


@pytest.mark.parametrize('i', CASES)
def test_torch_path_matches_the_reference_rows(i):
    from stp3_amd.ops_plan import sample_trajectories_reference
    g = H.load('sampler.npz')
    v0, kappa, nf, m, draws = case(g, i)
    rows = sample_trajectories_reference(v0, kappa, nf, m, draws=draws, sort=False)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (1, m, nf + 1, 3)
    check_rows(rows[0].numpy(), g[f'c{i}_rows'], f'torch path, case {i}')


@pytest.mark.parametrize('i', CASES)
def test_torch_path_ordering(i):
    from stp3_amd.ops_plan import sample_trajectories, sample_trajectories_reference
    g = H.load('sampler.npz')
    v0, kappa, nf, m, draws = case(g, i)
    unsorted_rows = sample_trajectories_reference(v0, kappa, nf, m, draws=draws, sort=False)[0]
    rows, order = sample_trajectories(v0, kappa, nf, m, draws=draws, return_order=True)       # CPU tensors: the torch path
    check_sorting(rows[0].numpy(), order[0].numpy(), unsorted_rows.numpy(), g[f'c{i}_keys'], f'torch path, case {i}')
    assert torch.equal(sample_trajectories(v0, kappa, nf, m, draws=draws), rows)


def test_fresnel_helper_against_scipy_grid():
    from stp3_amd.ops_plan import fresnel_reference
    g = H.load('sampler.npz')
    x = torch.from_numpy(g['fresnel_x'])
    assert len(x) == 2049 and float(x[0]) == -16.0 and float(x[-1]) == 16.0 and float(x[1024]) == 0.0
    s, c = fresnel_reference(x)
    es, ec = float((s - torch.from_numpy(g['fresnel_s'])).abs().max()), float((c - torch.from_numpy(g['fresnel_c'])).abs().max())
    print(f'Fresnel on [-16, 16]: S within {es:.3e}, C within {ec:.3e} of scipy (bound {FRESNEL_TOL})')
    assert es <= FRESNEL_TOL and ec <= FRESNEL_TOL
    assert float(s[1024]) == 0.0 and float(c[1024]) == 0.0
    assert torch.equal(s.flip(0), -s) and torch.equal(c.flip(0), -c)                # odd (the grid is symmetric)
    s2, c2 = fresnel_reference(-x)
    assert torch.equal(s2, -s) and torch.equal(c2, -c)


# ---- the real kernel source, executed on the host (tests/hipcpu) ----
@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_sampler')
    lib = hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'))
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_sampler.py'), lib, str(tmp / 'out.npz')], env=env,
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(str(tmp / 'out.npz')))


@pytest.mark.parametrize('i', CASES)
def test_kernel_on_host_matches_the_reference_rows(host_kernel, i):
    g = H.load('sampler.npz')
    check_rows(host_kernel[f'c{i}_unsorted'], g[f'c{i}_rows'], f'kernel on the host, case {i}')


@pytest.mark.parametrize('i', CASES)
def test_kernel_on_host_against_torch_path(host_kernel, i):
    from stp3_amd.ops_plan import sample_trajectories_reference
    g = H.load('sampler.npz')
    v0, kappa, nf, m, draws = case(g, i)
    check_one_spacing(host_kernel[f'c{i}_unsorted'], sample_trajectories_reference(v0, kappa, nf, m, draws=draws, sort=False)[0].numpy(),
                      f'kernel on the host against the torch path, case {i}')
    rows, order = sample_trajectories_reference(v0, kappa, nf, m, draws=draws, return_order=True)
    assert np.array_equal(host_kernel[f'c{i}_order'], order[0].numpy())
    check_sorting(host_kernel[f'c{i}_sorted'], host_kernel[f'c{i}_order'], host_kernel[f'c{i}_unsorted'], g[f'c{i}_keys'],
                  f'kernel on the host, case {i}')


def test_kernel_on_host_batch_equals_single_launches(host_kernel):
    for n, i in enumerate(host_kernel['batch_cases']):
        assert np.array_equal(host_kernel['batch_sorted'][n].view(np.uint32), host_kernel[f'c{i}_sorted'].view(np.uint32))
        assert np.array_equal(host_kernel['batch_order'][n], host_kernel[f'c{i}_order'])
    assert len(host_kernel['batch_cases']) == 3


# ---- arguments ----
def test_c_entry_validates_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below is refused first

    def call(dims, v0=fake, kappa=fake, draws=fake, trajs=fake):
        return lib.stp3_traj_sample(ctypes.byref(dims) if dims is not None else None, v0, kappa, draws, trajs, None, None)
    good = (4, 1800, 720, 360, 720, 6, 0.5, 1)
    assert call(None) == -10001
    for field, value in (('B', 0), ('M', 0), ('n_future', 0), ('n_left', 719), ('n_straight', -360), ('dt', 0.0)):
        d = _lib.SamplerDims(*good)
        setattr(d, field, value)
        assert call(d) == -10001, field
    for null in ('v0', 'kappa', 'draws', 'trajs'):
        assert call(_lib.SamplerDims(*good), **{null: None}) == -10001, null
    assert call(_lib.SamplerDims(1, 8193, 3277, 1639, 3277, 6, 0.5, 1)) == -10002            # beyond one workgroup's LDS
    assert _lib.SamplerDims(*good).n_future == 6 and ctypes.sizeof(_lib.SamplerDims) == 40


def test_python_entry_validates():
    from stp3_amd.ops_plan import sample_trajectories, sampler_counts
    assert sampler_counts(1800) == (720, 360, 720) and sampler_counts(60) == (24, 12, 24)
    v0, kappa = torch.tensor([5.0, 6.0]), torch.tensor([0.0, 0.1])
    with pytest.raises(ValueError):
        sample_trajectories(v0, kappa, 6, 1801)                     # 720 + 360 + 720 != 1801
    with pytest.raises(ValueError):
        sample_trajectories(v0, kappa, 6, 60, possibility=(0.5, 0.2, 0.2))
    with pytest.raises(ValueError):
        sample_trajectories(v0, kappa, 0, 60)
    with pytest.raises(ValueError):
        sample_trajectories(v0, kappa[:1], 6, 60)
    with pytest.raises(ValueError):
        sample_trajectories(v0, kappa, 6, 60, draws=torch.rand(2, 275, dtype=torch.float64))   # 3 * 60 + 2 * 48 = 276
    rows = sample_trajectories(v0, kappa, 6, 60, generator=torch.Generator().manual_seed(1))
    again = sample_trajectories(v0, kappa, 6, 60, generator=torch.Generator().manual_seed(1))
    assert tuple(rows.shape) == (2, 60, 7, 3) and rows.dtype == torch.float32 and torch.equal(rows, again)
    assert torch.isfinite(rows).all() and (rows[:, :, -1, 0].diff(dim=1) >= 0).all()


def test_trajectory_sampling_curvature_and_flip():
    from stp3_amd import datas
    from stp3_amd.ops_plan import sample_trajectories
    steering = [0.11, -0.07, 0.0]
    kappa = datas.trajectory_curvature(torch.tensor(steering, dtype=torch.float64), torch.tensor([False, True, True]))
    assert kappa.dtype == torch.float64
    assert kappa.tolist() == [2 * 0.11 / 2.588, 2 * 0.07 / 2.588, 2 * -0.0 / 2.588]            # NuscenesData.py:418-425
    assert datas.trajectory_curvature(torch.tensor(steering, dtype=torch.float64), True).tolist() == [2 * -s / 2.588 for s in steering]
    speed = torch.tensor([4.0, 9.5, 0.0], dtype=torch.float64)
    draws = torch.rand(3, 3 * 600 + 2 * 480, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    angle = torch.tensor(steering, dtype=torch.float64)
    got = datas.trajectory_sampling(speed, angle, 4, 600, left_hand_traffic=True, draws=draws)
    want = sample_trajectories(speed, torch.tensor([2 * -s / 2.588 for s in steering], dtype=torch.float64), 4, 600, draws=draws)
    assert tuple(got.shape) == (3, 600, 5, 3) and got.dtype == torch.float32 and torch.equal(got, want)
    plain = datas.trajectory_sampling(speed, angle, 4, 600, draws=draws)
    assert torch.equal(plain, sample_trajectories(speed, torch.tensor([2 * s / 2.588 for s in steering], dtype=torch.float64), 4, 600,
                                                  draws=draws)) and not torch.equal(plain[0], got[0])
