"""CPU: the inference engine's kernels and host code without a GPU (GPU side: tests/test_inference_gpu.py).

KERNEL EQUALITY on the host stand-in (tests/hipcpu: the repository's .hip sources compiled for the host).  The fused eval
operators must give the BITS of the two operators they replace -- stp3_conv2d_fwd_affine against stp3_conv2d_fwd followed by the
eval stp3_bn_apply_fwd (1x1 on each of the three convolution kernels, 3x3, dilated 3x3, 7x7 stride 2; with and without the skip,
in both skip modes; the three activations; a convolution bias; an output slot with ldy > Cout; 35 channels in 40 zero-padded
lanes; a per-sample bias on the tiled kernel), stp3_linear_fwd_affine against stp3_linear_fwd + eval apply on the (N, C, 1, 1)
descriptor, stp3_dwconv2d_fwd_affine against stp3_dwconv2d_fwd + eval apply (3x3 / 5x5, stride 1 / 2, on an odd 13 x 17 plane under
the frozen "same" padding of a canonical size, asymmetric at stride 2) -- and stp3_bn_eval_coefs the constants the plain path
derives: invstd = 1 / sqrt(var + eps), scale = gamma * invstd, shift = beta - mean * scale, each operation rounded to float32
(what numpy's float32 arithmetic gives: IEEE division and square root on both sides), zeros in the padded lanes.  No tolerance anywhere: equality of bit patterns.

ARGUMENTS: the three entry points validate without a GPU.  RESOURCES: their gfx950 kernels exist and use no scratch.

CALL TRACE (tests/host_trace.py, tests/inference_trace.py): inside the engine's scope the Decoder of Perception.yml issues NO
stand-alone stp3_bn_apply_fwd and no per-forward coefficient glue, and neither does the Encoder (its ASPP projections take their
per-sample bias in the convolution epilogue, the image-pooling descriptors their BatchNorm in stp3_linear_fwd_affine);
the whole Perception.yml forward issues exactly as many as that table lists as unfused; the plain eval forward's trace is
the parent's, call for call (tests/golden/eval_forward_trace.txt, recorded before the engine existed; buffer checksums
stripped)."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
PKG = os.path.join(ROOT, 'st-p3_amd', 'stp3_amd')
sys.path.insert(0, HIPCPU)
import run_inference as RI  # noqa: E402

CONV = sorted(RI.CONV_CASES)
DW = sorted(RI.DW_CASES)
LINEAR = sorted(RI.LINEAR_CASES)


# ---- the real kernel source, executed on the host (tests/hipcpu) ----
@pytest.fixture(scope='module')
def host_kernels(tmp_path_factory):
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_inference')
    lib = hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'))
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_inference.py'), lib, str(tmp / 'out.npz')], env=env,
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(str(tmp / 'out.npz')))


def _bf16(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize('name', CONV)
def test_conv2d_fwd_affine_bit_equal(host_kernels, name):
    plain, fused = host_kernels[f'{name}/plain'], host_kernels[f'{name}/fused']
    n, cin, h, w, ch, k, s, p, d, act, res_mode, has_bias, slot, c0 = RI.CONV_CASES[name]
    lanes = (ch + 7) // 8 * 8
    differ = int((plain != fused).sum())
    print(f'{name}: {plain.size} values, {differ} with another bit pattern; {int((fused != 0).sum())} non-zero')
    assert plain.shape == fused.shape and plain.dtype == np.uint16
    assert differ == 0
    body = fused[:, c0:c0 + lanes] if slot else fused
    assert np.isfinite(_bf16(body)).all() and (body[:, :ch] != 0).mean() > 0.2          # a real result, not zeros
    assert not body[:, ch:].any()                                                       # zero-padded lanes are written as zeros
    if slot:                                                                            # ... and nothing outside the slot
        outside = np.concatenate([fused[:, :c0], fused[:, c0 + lanes:]], axis=1)
        assert (outside == 0x4040).all()                                                # the 3.0 the buffer was filled with
    if act == RI.ACT_RELU and res_mode != RI.RES_AFTER_ACT:
        assert (_bf16(body) >= 0).all()
    # the fused operator did more than the convolution: its output differs from the convolution's
    assert (host_kernels[f'{name}/conv'] != (fused[:, c0:c0 + lanes] if slot else fused)).any()


@pytest.mark.parametrize('name', DW)
def test_dwconv2d_fwd_affine_bit_equal(host_kernels, name):
    plain, fused = host_kernels[f'{name}/plain'], host_kernels[f'{name}/fused']
    n, c, h, w, k, s = RI.DW_CASES[name]
    left, right, top, bottom = host_kernels[f'{name}/pad']
    assert (left, right) == (top, bottom) == RI.same_pad(RI.CANONICAL, k, s)
    if s == 2:
        assert left != right                                                            # the asymmetric frozen padding
    differ = int((plain != fused).sum())
    print(f'{name}: {plain.size} values, {differ} with another bit pattern; padding {left, right, top, bottom}')
    assert plain.shape == fused.shape == (n, c, (h + top + bottom - k) // s + 1, (w + left + right - k) // s + 1)
    assert differ == 0
    assert np.isfinite(_bf16(fused)).all() and (fused != 0).mean() > 0.9


@pytest.mark.parametrize('name', LINEAR)
def test_linear_fwd_affine_bit_equal(host_kernels, name):
    plain, fused, lin = host_kernels[f'{name}/plain'], host_kernels[f'{name}/fused'], host_kernels[f'{name}/linear']
    m, k, n, act = RI.LINEAR_CASES[name]
    differ = int((plain.view(np.uint32) != fused.view(np.uint32)).sum())
    print(f'{name}: {plain.size} values, {differ} with another bit pattern')
    assert plain.shape == fused.shape == (m, n) and plain.dtype == fused.dtype == np.float32
    assert differ == 0
    assert np.isfinite(fused).all() and (fused != lin).any()
    if act == RI.ACT_RELU:
        assert (fused >= 0).all() and (fused > 0).mean() > 0.2


def test_per_sample_bias_stays_off_the_streaming_kernels(host_kernels):
    """A layer the library routes to its streaming pointwise kernels takes no per-sample bias: the host keeps it on two operators
    (and the entry point answers STP3_EUNSUP: ``test_argument_validation_without_gpu``)."""
    assert not bool(host_kernels['sbias_pointwise_supported'])


@pytest.mark.parametrize('name', CONV + DW + LINEAR)
def test_bn_eval_coefs_are_the_plain_path_constants(host_kernels, name):
    get = lambda key: host_kernels[f'coefs/{name}/{key}']                               # noqa: E731
    arena, mean, var, gamma, beta = get('arena'), get('running_mean'), get('running_var'), get('weight'), get('bias')
    eps = np.float32(get('eps'))
    c = mean.shape[0]
    lanes = (c + 7) // 8 * 8
    assert arena.dtype == np.float32 and arena.shape == (2 * lanes,)
    invstd = np.float32(1.0) / np.sqrt(var + eps, dtype=np.float32)
    scale = (gamma * invstd).astype(np.float32)
    shift = (beta - (mean * scale).astype(np.float32)).astype(np.float32)
    assert np.array_equal(arena[:c].view(np.uint32), scale.view(np.uint32))
    assert np.array_equal(arena[lanes:lanes + c].view(np.uint32), shift.view(np.uint32))
    assert not arena[c:lanes].any() and not arena[lanes + c:].any()


# ---- argument validation: the gfx950 library, no GPU ----
def test_argument_validation_without_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUP = -10001, -10002
    bf16 = _lib.DTYPE_BF16
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 63) // 64 * 64                                                             # 16-byte aligned
    conv = lambda **kw: _lib.ConvDims(**{**dict(N=1, H=4, W=4, Cin=8, Ho=4, Wo=4, Cout=8, KH=1, KW=1, stride=1, pad_h=0, pad_w=0,  # noqa: E731
                                               dil_h=1, dil_w=1, ldx=8, ldy=8, out_dtype=bf16, has_bias=0), **kw})

    def affine(d, x=p, w=p, bias=None, coef=p, sbias=None, channels=8, act=0, res=None, ldres=0, res_mode=0, y=p):
        return lib.stp3_conv2d_fwd_affine(ctypes.byref(d) if d is not None else None, x, w, bias, coef, sbias, channels, act, res,
                                          ldres, res_mode, y, None)
    assert affine(None) == EINVAL
    assert affine(conv(), coef=None) == EINVAL
    assert affine(conv(), x=None) == EINVAL and affine(conv(), y=None) == EINVAL
    assert affine(conv(), act=3) == EINVAL and affine(conv(), res_mode=3) == EINVAL
    assert affine(conv(), res=p, res_mode=0) == EINVAL and affine(conv(), res=None, res_mode=2) == EINVAL
    assert affine(conv(), channels=0) == EINVAL and affine(conv(), channels=9) == EINVAL
    assert affine(conv(has_bias=1), bias=None) == EINVAL
    assert affine(conv(N=0)) == EINVAL
    assert affine(conv(Cout=16, ldy=16), channels=5) == EUNSUP                          # Cout is not the channels rounded up to 8
    assert affine(conv(out_dtype=_lib.DTYPE_F32)) == EUNSUP
    assert affine(conv(ldy=12)) == EUNSUP and affine(conv(ldy=4)) == EUNSUP
    assert affine(conv(), y=p + 2) == EUNSUP
    assert affine(conv(), res=p, ldres=12, res_mode=1) == EUNSUP and affine(conv(), res=p + 2, ldres=8, res_mode=2) == EUNSUP
    assert affine(conv(Cin=4, ldx=4)) == EUNSUP
    assert affine(conv(Cout=64, ldy=64), channels=64, sbias=p) == EUNSUP                # a streaming pointwise layer with an sbias

    def lin(m=2, k=8, n=4, x=p, w=p, ldw=8, coef=p, ldcoef=8, act=1, y=p):
        return lib.stp3_linear_fwd_affine(m, k, n, x, w, ldw, None, coef, ldcoef, act, y, None)
    assert lin(m=0) == EINVAL and lin(k=0) == EINVAL and lin(n=0) == EINVAL
    assert lin(x=None) == EINVAL and lin(w=None) == EINVAL and lin(y=None) == EINVAL and lin(coef=None) == EINVAL
    assert lin(ldw=4) == EINVAL and lin(ldcoef=2) == EINVAL and lin(act=3) == EINVAL

    dw = lambda **kw: _lib.DwConvDims(**{**dict(N=1, H=5, W=5, C=8, Ho=5, Wo=5, K=3, stride=1, pad_top=1, pad_left=1, dtype=bf16), **kw})  # noqa: E731

    def dwa(d, x=p, w=p, coef=p, act=2, y=p):
        return lib.stp3_dwconv2d_fwd_affine(ctypes.byref(d) if d is not None else None, x, w, coef, act, y, None)
    assert dwa(None) == EINVAL and dwa(dw(N=0)) == EINVAL
    assert dwa(dw(), coef=None) == EINVAL and dwa(dw(), x=None) == EINVAL and dwa(dw(), y=None) == EINVAL
    assert dwa(dw(), act=5) == EINVAL
    assert dwa(dw(dtype=_lib.DTYPE_F32)) == EUNSUP and dwa(dw(K=7)) == EUNSUP and dwa(dw(K=4)) == EUNSUP
    assert dwa(dw(C=12)) == EUNSUP and dwa(dw(stride=3)) == EUNSUP

    assert lib.stp3_bn_eval_coefs(None, 1, 1, None) == EINVAL
    assert lib.stp3_bn_eval_coefs(p, -1, 1, None) == EINVAL and lib.stp3_bn_eval_coefs(p, 1, -1, None) == EINVAL
    assert lib.stp3_bn_eval_coefs(p, 1, 1 << 31, None) == EUNSUP
    assert lib.stp3_bn_eval_coefs(None, 0, 0, None) == 0                                # nothing to do


def test_binding_matches_the_header_struct():
    """stp3_bn_coef_entry: five pointers, the block offset, channels / lanes / eps / reserved -- 64 bytes, as the header lays it out."""
    from stp3_amd import _lib
    assert ctypes.sizeof(_lib.BnCoefEntry) == 64
    assert [f[0] for f in _lib.BnCoefEntry._fields_] == ['running_mean', 'running_var', 'gamma', 'beta', 'out', 'first_block',
                                                         'channels', 'lanes', 'eps', 'reserved']
    header = open(os.path.join(ROOT, 'include', 'stp3_hip.h')).read()
    body = re.search(r'typedef struct stp3_bn_coef_entry \{(.*?)\} stp3_bn_coef_entry;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'\b(\w+)\s*(?:,|$)', decl.strip().split(' ', 1)[-1].replace('*', ' '))]
    assert names == [f[0] for f in _lib.BnCoefEntry._fields_], names
    for line in ('evaluate.py:88-91', 'stp3/models/stp3.py:132-184', 'encoder.py:57-97', 'decoder.py:91-140'):
        assert line in header, line                                                     # the reference lines the entry points serve


def test_streaming_pointwise_predicate_is_the_librarys():
    """``ops.conv2d_affine_supported`` keeps a layer with a per-sample bias off the fused operator where the library would hand it
    to its streaming pointwise kernels (which answer STP3_EUNSUP to an sbias).  It restates the conditions of ``pointwise_applies``
    that depend on the layer alone; this holds the two together."""
    from stp3_amd import ops
    src = open(os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_conv.hip')).read()
    assert int(re.search(r'constexpr int kPointwiseMaxCin = (\d+);', src).group(1)) == ops.POINTWISE_MAX_CIN
    body = re.search(r'bool pointwise_applies\(const stp3_conv_dims\* p, const void\* y\) \{(.*?)\n\}', src, re.S).group(1)
    terms = {t.strip() for t in re.sub(r'\s+', ' ', body).replace('return', '').rstrip('; ').split('&&')}
    restated = {'p->KH == 1', 'p->KW == 1', 'p->stride == 1', 'p->pad_h == 0', 'p->pad_w == 0', 'p->Cin <= kPointwiseMaxCin',
                'p->Cout >= 64', '!p->has_bias'}
    # the rest only NARROWS the streaming set (output geometry, type and alignment): the host is then merely conservative
    narrowing = {'p->H == p->Ho', 'p->W == p->Wo', 'p->out_dtype == STP3_DTYPE_BF16', 'p->Cout % 8 == 0', 'p->ldy % 8 == 0',
                 '!((uintptr_t)y & 15)'}
    assert terms == restated | narrowing, sorted(terms ^ (restated | narrowing))


def test_engine_gate_weights_are_rewritten_in_place():
    """The merged GRU gate weights a captured graph reads: inside the engine's scope ``ops_pred._merged_gate_weights`` hands out
    the ENGINE's buffers -- the values of the plain route's cache, at addresses ``refresh()`` keeps -- and outside the scope
    the cache, as before."""
    import torch
    import torch.nn as nn
    from stp3_amd import ops_pred
    from stp3_amd.layers import fused
    torch.manual_seed(0)
    cu, cr = nn.Conv2d(24, 16, 3, padding=1), nn.Conv2d(24, 16, 3, padding=1)
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)  # noqa: E731
    plain_w, plain_b = ops_pred._merged_gate_weights(cu, cr)
    gates = ops_pred.EngineGateWeights()
    with torch.no_grad(), fused.eval_fusion(None, gates):
        w, b = ops_pred._merged_gate_weights(cu, cr)
        assert ops_pred._merged_gate_weights(cu, cr)[0] is w                            # handed out, not rebuilt
    assert ops_pred.ENGINE_GATES is None and ops_pred._merged_gate_weights(cu, cr)[0] is plain_w
    assert w is not plain_w and w.shape == plain_w.shape and w.stride() == plain_w.stride() and w.dtype == plain_w.dtype
    assert torch.equal(bits(w), bits(plain_w)) and torch.equal(bits(b), bits(plain_b))
    where = (w.data_ptr(), b.data_ptr())
    with torch.no_grad():
        for p in (cu.weight, cu.bias, cr.weight, cr.bias):
            p.mul_(1.5).add_(0.01)
    assert torch.equal(bits(w), bits(plain_w))                                          # nothing moves before refresh()
    gates.refresh()
    new_w, new_b = ops_pred._merged_gate_weights(cu, cr)                                # the plain route on the new values
    assert new_w is not plain_w                                                         # (its cache REPLACES its tensors)
    assert (w.data_ptr(), b.data_ptr()) == where
    assert torch.equal(bits(w), bits(new_w)) and torch.equal(bits(b), bits(new_b)) and not torch.equal(bits(w), bits(plain_w))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('c++filt') is None, reason='needs hipcc')
def test_inference_kernels_use_no_scratch():
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py'), '--json'],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-1500:]
    rows = json.loads(out.stdout)
    wanted = {'igemm': [k for k in rows if re.match(r'void conv2d_igemm_kernel<\d+, 5, ', k['kernel'])],
              'rows': [k for k in rows if re.match(r'void pointwise_rows_kernel<\d+, \d+, 5>', k['kernel'])],
              'direct': [k for k in rows if re.match(r'void pointwise_direct_kernel<\d+, 5>', k['kernel'])],
              'dwconv': [k for k in rows if re.match(r'void dwconv_fwd_kernel<unsigned short, \d, \d, 4, false, unsigned (int|long), true>',
                                                     k['kernel'])],
              'coefs': [k for k in rows if k['kernel'].startswith('bn_eval_coefs_kernel')],
              'linear': [k for k in rows if k['kernel'].startswith('linear_fwd_kernel')]}
    assert len(wanted['igemm']) == 12 and len(wanted['rows']) == 5 and len(wanted['direct']) == 3, {k: len(v) for k, v in wanted.items()}
    assert len(wanted['dwconv']) == 8 and len(wanted['coefs']) == 1 and len(wanted['linear']) == 1, {k: len(v) for k, v in wanted.items()}
    for ks in wanted.values():
        for k in ks:
            assert k['scratch'] == 0 and k['vgpr_spills'] == 0 and k['sgpr_spills'] == 0, k
            assert k['vgpr'] + k['agpr'] <= 256, k                                      # two workgroups of 256 threads per CU at least


# ---- call trace ----
def _sections(path):
    out, name = {}, None
    for line in open(path).read().splitlines():
        if line.startswith('# '):
            name = line[2:].split()[0]
            out[name] = []
        elif name is not None:
            out[name].append(line)
    return out


def _strip(line):
    return re.sub(r':[0-9a-f]{8}\b', '', line)


@pytest.fixture(scope='module')
def traces(tmp_path_factory):
    from tests import host_trace
    tmp = tmp_path_factory.mktemp('inference_trace')
    recorder = host_trace.build_recorder(str(tmp / 'libstp3hip_recorder.so'))
    logs = {}
    for mode in ('plain', 'engine'):
        log = tmp / f'{mode}.log'
        env = dict(os.environ)
        env.update(STP3_HOST_DRYRUN='1', STP3_TRACE_LOG=str(log), STP3_REAL_LIB=os.path.join(PKG, 'libstp3hip.so'))
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'inference_trace.py'), recorder, mode], env=env, check=True,
                       timeout=900, stderr=subprocess.DEVNULL)
        lines = open(log).read().splitlines()
        assert lines[-1] == '# end', lines[-3:]
        logs[mode] = str(log)
    return logs


def _bn_dims(line):
    d = struct.unpack('<12i', bytes.fromhex(re.search(r'dims=([0-9a-f]+)', line).group(1)))
    return dict(zip('N rows C ldx ldy ldr dtype act res_mode has_sbias has_oscale cpad'.split(), d))


def _design_table():
    """Rows of DESIGN.md's table of Perception.yml's BatchNorm layers: (count, fused?)."""
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    table = text[text.index('<!-- inference-bn-table -->'):text.index('<!-- /inference-bn-table -->')]
    rows = []
    for line in table.splitlines():
        cells = [c.strip() for c in line.strip().strip('|').split('|')]
        if len(cells) >= 4 and cells[1].isdigit():
            rows.append((int(cells[1]), cells[2].lower().startswith('yes')))
    return rows


def test_plain_eval_forward_trace_is_the_parents(traces):
    want = open(os.path.join(ROOT, 'tests', 'golden', 'eval_forward_trace.txt')).read().splitlines()
    got = [_strip(line) for line in open(traces['plain']).read().splitlines()]
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    plain = _sections(traces['plain'])
    assert not [line for line in plain['full'] if 'affine' in line or 'stp3_bn_eval_coefs' in line]


def test_engine_scope_fuses_the_encoder_and_the_decoder(traces):
    plain, engine = _sections(traces['plain']), _sections(traces['engine'])
    name = lambda line: line.split()[0]                                                 # noqa: E731
    for part in ('encoder', 'decoder', 'full'):
        # the coefficient glue is one launch at construction, none per forward
        assert not [line for line in engine[part] if name(line) == 'stp3_bn_eval_coefs'], part
    assert sum(name(line) == 'stp3_bn_eval_coefs' for lines in _sections_with_preamble(traces['engine']) for line in lines) == 1
    # the Decoder: every BatchNorm in a convolution epilogue
    assert sum(name(line) == 'stp3_bn_apply_fwd' for line in plain['decoder']) == 21
    assert not [line for line in engine['decoder'] if name(line) == 'stp3_bn_apply_fwd']
    assert sum(name(line) == 'stp3_conv2d_fwd_affine' for line in engine['decoder']) == 21
    # the Encoder: 83 BatchNorm layers, none left stand-alone (81 in convolution epilogues, the two pooled descriptors in their
    # linear launch)
    assert sum(name(line) == 'stp3_bn_apply_fwd' for line in plain['encoder']) == 83
    left = [_bn_dims(line) for line in engine['encoder'] if name(line) == 'stp3_bn_apply_fwd']
    print(f'Encoder in engine mode: {len(left)} stand-alone stp3_bn_apply_fwd calls: {left}')
    assert not left, left
    assert sum(name(line) == 'stp3_linear_fwd_affine' for line in engine['encoder']) == 2
    assert sum(name(line) in ('stp3_conv2d_fwd_affine', 'stp3_dwconv2d_fwd_affine') for line in engine['encoder']) == 81
    assert sum(name(line) == 'stp3_dwconv2d_fwd_affine' for line in engine['encoder']) == 22
    assert not [line for line in engine['encoder'] if name(line) == 'stp3_dwconv2d_fwd']
    # an MBConv block with an expand layer: nine launches -> six
    mb_plain = sum(name(line) in ('stp3_conv2d_fwd', 'stp3_bn_apply_fwd', 'stp3_dwconv2d_fwd', 'stp3_se_pool', 'stp3_se_mlp_fwd',
                                  'stp3_se_scale') for line in plain['encoder'])
    mb_engine = sum(name(line) in ('stp3_conv2d_fwd', 'stp3_conv2d_fwd_affine', 'stp3_bn_apply_fwd', 'stp3_dwconv2d_fwd_affine',
                                   'stp3_se_pool', 'stp3_se_mlp_fwd', 'stp3_se_scale') for line in engine['encoder'])
    assert mb_plain - mb_engine == 83                                                   # one launch less per BatchNorm layer


def _sections_with_preamble(path):
    lines = open(path).read().splitlines()
    return [[line for line in lines if not line.startswith('#')]]


def test_whole_forward_leaves_what_the_design_table_lists(traces):
    plain, engine = _sections(traces['plain']), _sections(traces['engine'])
    name = lambda line: line.split()[0]                                                 # noqa: E731
    rows = _design_table()
    total = sum(n for n, _ in rows)
    unfused = sum(n for n, fused in rows if not fused)
    n_plain = sum(name(line) == 'stp3_bn_apply_fwd' for line in plain['full'])
    n_engine = sum(name(line) == 'stp3_bn_apply_fwd' for line in engine['full'])
    n_fused = sum(name(line) in ('stp3_conv2d_fwd_affine', 'stp3_dwconv2d_fwd_affine', 'stp3_linear_fwd_affine') for line in engine['full'])
    print(f'Perception.yml forward: {n_plain} BatchNorm layers, {n_fused} fused, {n_engine} stand-alone in the engine; '
          f'DESIGN.md lists {total} / {unfused} unfused')
    assert n_plain == total
    assert n_engine == unfused
    assert n_fused == total - unfused
    # same work otherwise: the launches that are neither convolution nor BatchNorm are the plain forward's
    other = lambda lines: sorted(name(line).replace('stp3_linear_fwd_affine', 'stp3_linear_fwd') for line in lines      # noqa: E731
                                 if name(line) not in ('stp3_conv2d_fwd', 'stp3_conv2d_fwd_affine', 'stp3_bn_apply_fwd', 'stp3_dwconv2d_fwd',
                                                       'stp3_dwconv2d_fwd_affine', 'stp3_conv2d_prep_weights'))
    assert other(plain['full']) == other(engine['full'])
