"""CPU: the loss and label-warp kernels (csrc/stp3_loss.hip) with the kernel sources executed on the host (tests/hipcpu), the C
ABI's argument checks, and the float64 references of tests/loss_cases.py against the torch statements the project already trusts.

* Kernel cases: what the stand-in runs in seconds -- every cross-entropy case of at most 1025 pixels per row (``ties``,
  ``few-live`` and ``wide-range`` among them), every regression case but the 135 000-pixel one, every warp case -- in forward,
  reverse and random fiber order, with the bounds of tests/test_loss_gpu.py.  (Run twice and compared bit for bit in the forward
  order only: a second pass per order would double the file's time and the stand-in is deterministic under a fixed order.)  The
  register-cached / re-reading boundary (40 960 pixels), the grid-stride loop and what ``hipcc`` makes of the device code (FMA
  contraction, device expf / logf) are the job of the ``-m gpu`` file.
* Argument checks: null pointers and rows <= 0 -> STP3_EINVAL, an unknown dtype -> STP3_EUNSUP, a short workspace ->
  STP3_ENOSPACE, rows * P >= 2^31 -> STP3_EUNSUP; every call returns before it launches.
* No kernel: ``ref_ce_topk`` / ``ref_reg_loss`` / ``ref_warp_nearest`` equal the CPU route of ``stp3_amd.losses`` and
  ``geometry.warp_with_theta`` in float64 (pinned to the reference project by the goldens) to 1e-12 on every case without
  ties -- the new references mean what the project's own statements mean."""
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from tests import loss_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
sys.path.insert(0, HIPCPU)
import build as hipcpu_build  # noqa: E402

needs_clang = pytest.mark.skipif(not os.path.exists(hipcpu_build.CLANG) or shutil.which('gcc') is None,
                                 reason='needs the clang++ that ships with ROCm')
ORDERS = ('', 'reverse', 'random')
EINVAL, EUNSUP, ENOSPACE = -10001, -10002, -10003


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    return hipcpu_build.build(str(tmp_path_factory.mktemp('hipcpu_loss') / 'libstp3hip_cpu.so'))


def _drive(lib, args, order):
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    env['HIPCPU_THREADS'] = '2'                  # launches of a few workgroups: more workers only contend for their fiber stacks
    if order:
        env['HIPCPU_ORDER'] = order
    else:
        args = ['--repeat', *args]
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_loss.py'), lib, *args], env=env, capture_output=True,
                         text=True, timeout=1500)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    assert out.returncode == 0 and lines, out.stderr[-1500:]
    return json.loads(lines[-1][7:])


@pytest.fixture(scope='module')
def host_results(host_lib):
    """{order: figures of every host case} + {'abi': return codes}: four driver processes side by side."""
    with ThreadPoolExecutor(4) as pool:
        jobs = {order: pool.submit(_drive, host_lib, LC.host_names(), order) for order in ORDERS}
        jobs['abi'] = pool.submit(_drive, host_lib, ['abi'], '')
        return {k: j.result() for k, j in jobs.items()}


def _check(name, out, repeated):
    kind = out['kind']
    if kind == 'warp':
        assert out['distinct_sources'] and out['mismatches_sure'] == 0 and out['repeat_equal'], (name, out)
        if out['mode'] == 'exact':
            assert out['equal'], (name, out)
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
    assert out['repeat_equal'] is (True if repeated else None), (name, out)
    if kind == 'ce':
        assert out['ignored_are_bit_zero'] and out['grad_layout_kept'], (name, out)
    elif kind == 'hdmap':
        assert out['module_equal'], (name, out)
    else:
        assert out['masked_are_bit_zero'] and out['pad_zero'], (name, out)


@needs_clang
@pytest.mark.parametrize('order', ORDERS)
def test_kernels_equal_float64_reference_on_host(host_results, order):
    res = host_results[order]
    names = LC.host_names()
    assert len(names) == len(LC.case_list()) - len(LC.HOST_SKIP) and all(n in res for n in names)
    for name in names:
        _check(name, res[name], repeated=not order)


@needs_clang
def test_argument_checks_on_host(host_results):
    res = dict(host_results['abi'])
    res.pop('seconds')
    want = {'dtype': EUNSUP, '2g': EUNSUP, 'short_ws': ENOSPACE}
    assert len(res) >= 40
    for name, rc in res.items():
        assert rc == next((v for k, v in want.items() if name.endswith(k)), EINVAL), (name, rc)


# ---- the references against the torch statements (no kernel) -----------------------------------------------------------
def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _statement_ce(kw):
    from stp3_amd import losses as L
    *lead, c, h, w = kw['shape']
    k, p = kw['k'], h * w
    z, y = LC.ce_inputs(**{a: b for a, b in kw.items() if a not in ('kind', 'k')})
    x = z.double().requires_grad_()
    cw = torch.tensor(LC.WEIGHTS[c]) if kw.get('weights', True) else None
    rs = LC.row_scale_of(lead, kw.get('n_present'))
    ref = LC._ce_refs(z, y, cw, rs, k)
    if len(lead) == 3:                                   # the depth head: (b, s, n, D, h, w)
        assert cw is None and rs is None and k == 0
        value = L.DepthLoss()(x, y.long())
    else:
        b, s = (1, lead[0]) if len(lead) == 1 else lead
        top = 0 < k < p
        mod = L.SegmentationLoss(cw if cw is not None else torch.ones(c), use_top_k=top, top_k_ratio=(k + 0.5) / p,
                                 future_discount=LC.DISCOUNT if rs is not None else 1.0)
        n_present = kw.get('n_present') or s
        value = mod(x.view(b, s, c, h, w), y.long().view(b, s, 1, h, w), n_present)
    value.backward()
    return value.detach(), x.grad, ref['value'], ref['grad'].view(z.shape)


def _statement_hdmap(kw):
    from stp3_amd import losses as L
    pred, tgt = LC.hdmap_inputs(kw['seed'])
    b, _, h, w = pred.shape
    x = pred.double().requires_grad_()
    value = L.HDmapLoss(torch.tensor(LC.HD_WEIGHTS), LC.HD_TRAIN, LC.HD_TOPK, LC.HD_RATIO)(x, tgt)
    value.backward()
    ks = [int(LC.HD_RATIO[i] * h * w) if LC.HD_TOPK[i] else 0 for i in range(2)]
    refs = [LC.ref_ce_topk(pred[:, 2 * i:2 * i + 2].reshape(b, 2, h * w), tgt[:, i].reshape(b, h * w),
                           torch.tensor(LC.HD_WEIGHTS[i]), None, ks[i]) for i in range(2)]
    return (value.detach(), x.grad, sum(r['value'] * t for r, t in zip(refs, LC.HD_TRAIN)),
            torch.cat([r['grad'].view(b, 2, h, w) * t for r, t in zip(refs, LC.HD_TRAIN)], dim=1))


def _statement_reg(kw):
    from stp3_amd import losses as L
    b, s, c, h, w = kw['shape']
    pred, tgt = LC.reg_inputs(**{a: v for a, v in kw.items() if a != 'kind'})
    rs = LC.row_scale_of((b, s), kw.get('n_present'))
    ref = LC.ref_reg_loss(pred, tgt, rs, kw['norm'])
    x = pred.double().requires_grad_()
    mod = L.SpatialRegressionLoss(kw['norm'], ignore_index=LC.IGNORE, future_discount=LC.DISCOUNT if rs is not None else 1.0)
    value = mod(x, tgt.double(), kw.get('n_present') or s)
    value.backward()
    return value.detach(), x.grad, ref['value'], ref['grad']


STATEMENT_CASES = [(n, kw) for n, kw in LC.case_list() if kw['kind'] in ('ce', 'hdmap', 'reg') and not kw.get('ties')]


@pytest.mark.parametrize('name,kw', STATEMENT_CASES, ids=[n for n, _ in STATEMENT_CASES])
def test_loss_references_equal_torch_statements(name, kw):
    value, grad, ref_value, ref_grad = {'ce': _statement_ce, 'hdmap': _statement_hdmap, 'reg': _statement_reg}[kw['kind']](kw)
    if float(ref_value) == 0.0:
        assert float(value) == 0.0 and float(grad.abs().max()) == 0.0 and float(ref_grad.abs().max()) == 0.0
        return
    assert _rel(value, ref_value) <= 1e-12, (name, float(value), float(ref_value))
    assert _rel(grad, ref_grad) <= 1e-12, name


def test_warp_reference_equals_torch_statement_away_from_ties():
    from stp3_amd import geometry as geo
    for h, w in ((16, 16), (8, 32)):
        x, theta, identity, names, tie = LC.exact_warp_inputs(h, w)
        ref, unsure = LC.ref_warp_nearest(x, theta, identity)
        plain = [i for i, (t, fl) in enumerate(zip(tie, identity)) if not t and not fl]
        assert len(plain) >= 5 and not bool(unsure[plain].any())
        got = geo.warp_with_theta(x[plain].double(), theta[plain].double(), 'nearest')
        assert torch.equal(got, ref[plain].double()), (h, w)
    kw = dict(LC.case_list())['warp-general']
    x, theta = LC.general_warp_inputs(kw['seed'])
    ref, unsure = LC.ref_warp_nearest(x, theta, None)
    got = geo.warp_with_theta(x.double(), theta.double(), 'nearest')
    sure = ~unsure[:, None].expand_as(ref)
    assert float(unsure.double().mean()) <= 0.01
    assert torch.equal(got[sure], ref.double()[sure])
