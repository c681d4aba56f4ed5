"""CPU: the operand-side BatchNorm of the 1x1 convolutions (csrc/stp3_conv.hip, PRE) with the kernel sources executed on the
host (tests/hipcpu): stp3_conv2d_fwd_pre / stp3_conv2d_wgrad_pre / stp3_conv2d_wgrad_partials against stp3_bn_apply_fwd followed
by the plain entry points, bit for bit -- the two kernel cases of tests/test_conv_pre_gpu.py that the stand-in runs in seconds
(M = 70 pixels; Cout = 24 with ReLU and a bias, Cout = 136 without either), in forward and reverse fiber order.  What this
sees: the staging's index arithmetic, the constants' LDS table and its barrier, the zero-after-transform masks; the MI355X
itself is the job of the ``-m gpu`` file."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
sys.path.insert(0, HIPCPU)
import build as hipcpu_build  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(hipcpu_build.CLANG) or shutil.which('gcc') is None,
                                reason='needs the clang++ that ships with ROCm')
NAMES = ('m70-cout24-relu-bias', 'm70-cout136-none-nobias')


@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    return hipcpu_build.build(str(tmp_path_factory.mktemp('hipcpu_conv_pre') / 'libstp3hip_cpu.so'))


@pytest.mark.parametrize('order', ['', 'reverse'])
def test_fold_equals_apply_then_plain_on_host(host_lib, order):
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    if order:
        env['HIPCPU_ORDER'] = order
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_conv_pre.py'), host_lib, *NAMES], env=env,
                         capture_output=True, text=True, timeout=1500)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    assert out.returncode == 0 and lines, out.stderr[-1500:]
    res = json.loads(lines[-1][7:])
    for name in NAMES:
        r = res[name]
        assert r['shift_positive'] and r['x_is_slice'] and r['fwd_finite'] and r['fwd_nonzero'] and r['wgrad_nonzero'], (name, r)
        assert r['fwd_equal'] and r['wgrad_equal'] and r['wgrad_batched_equal'], (name, r)
