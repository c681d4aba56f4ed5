"""CPU: the depthwise kernels (csrc/stp3_dwconv.hip) with the kernel sources executed on the host (tests/hipcpu) against the
float64 references of tests/dwconv_cases.py, the C ABI's argument checks, and the references themselves against float64
``F.conv2d`` with autograd.

* Kernel cases: the whole table of tests/dwconv_cases.py but the two tensors around 4 GiB -- the exact pass (integer data, every
  entry ``torch.equal`` to the reference, run twice, canary rows intact, each case's exactness precondition asserted on the
  reference alone), the real pass and the affine pass at their derived bounds -- in forward, reverse and random fiber order.
  What ``hipcc`` makes of the device code (contraction, v_exp_f32 / v_rcp_f32), the resident-round launch sizes of the MI355X and
  the 32 / 64-bit offset paths at 4 GiB are the job of the ``-m gpu`` file.
* Argument checks: every entry's return codes for arguments it must reject; each call returns before it launches.
* No kernel: ``ref_fwd`` / ``ref_bwd_data`` / ``ref_bwd_weight`` equal float64 ``F.conv2d`` and its autograd on every case --
  the tap sums written from the header's definition mean what torch's convolution means."""
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
sys.path.insert(0, HIPCPU)
import build as hipcpu_build  # noqa: E402

needs_clang = pytest.mark.skipif(not os.path.exists(hipcpu_build.CLANG) or shutil.which('gcc') is None,
                                 reason='needs the clang++ that ships with ROCm')
ORDERS = ('', 'reverse', 'random')


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


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    return hipcpu_build.build(str(tmp_path_factory.mktemp('hipcpu_dwconv') / 'libstp3hip_cpu.so'))


def _drive(lib, args, order):
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    env['HIPCPU_THREADS'] = '2'
    if order:
        env['HIPCPU_ORDER'] = order
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_dwconv.py'), lib, *args], env=env, capture_output=True,
                         text=True, timeout=1500)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    assert out.returncode == 0 and lines, out.stderr[-1500:]
    return json.loads(lines[-1][7:])


@pytest.fixture(scope='module')
def host_results(host_lib):
    """{order: figures of every host case} + {'abi': return codes}: four driver processes side by side."""
    with ThreadPoolExecutor(4) as pool:
        jobs = {order: pool.submit(_drive, host_lib, DC.host_names(), order) for order in ORDERS}
        jobs['abi'] = pool.submit(_drive, host_lib, ['abi'], '')
        return {k: j.result() for k, j in jobs.items()}


@needs_clang
@pytest.mark.parametrize('order', ORDERS)
def test_depthwise_kernels_equal_float64_reference_on_host(host_results, order):
    res = host_results[order]
    names = DC.host_names()
    assert len(names) == len(DC.case_list()) - 2 and all(n in res for n in names)
    for name in names:
        check(name, res[name])


@needs_clang
def test_depthwise_argument_checks_on_host(host_results):
    res = host_results['abi']['abi']
    assert len(res) >= 140
    for name, rc, want in res:
        assert rc == want, (name, rc, want)


# ---- the references against float64 F.conv2d and its autograd (no kernel) ------------------------------------------------
SMALL = [(n, kw) for n, kw in DC.case_list() if kw['kind'] == 'small']


@pytest.mark.parametrize('name,kw', SMALL, ids=[n for n, _ in SMALL])
def test_depthwise_references_equal_conv2d_autograd(name, kw):
    n, c, h, wd, k, s, pads = kw['shape']
    xk, wk, dyk, bk = DC.real_inputs(kw['shape'], kw['dtype'], kw['seed'])
    x, w, dy, bias = xk.double(), wk.double(), dyk.double(), bk.double()
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    wt = w.t().reshape(c, 1, k, k).contiguous().requires_grad_()
    y = F.conv2d(F.pad(xt, pads), wt, bias, stride=s, groups=c)
    gx, gw = torch.autograd.grad(y, (xt, wt), dy.permute(0, 3, 1, 2))
    ho, wo = DC.out_size(h, wd, k, s, pads)
    assert tuple(y.shape) == (n, c, ho, wo)
    for got, ref in ((DC.ref_fwd(x, w, bias, k, s, pads), y.detach().permute(0, 2, 3, 1)),
                     (DC.ref_bwd_data(dy, w, k, s, pads, h, wd), gx.permute(0, 2, 3, 1)),
                     (DC.ref_bwd_weight(x, dy, k, s, pads), gw.reshape(c, k * k).t())):
        scale = float(ref.abs().max())
        assert scale > 0 and float((got - ref).abs().max()) <= 1e-12 * scale, name
