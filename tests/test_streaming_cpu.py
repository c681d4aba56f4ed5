"""CPU: the streaming inference engine's kernel and host code without a GPU (GPU side: tests/test_streaming_gpu.py).

KERNEL on the host stand-in (tests/hipcpu: csrc/stp3_window.hip compiled for the host, driver tests/hipcpu/run_window.py):
stp3_window_push against a numpy roll-and-append, exactly -- T in {1, 2, 3}, B in {1, 2}, frames of (N, fH, fW) = (2, 3, 5) with
12 and 8 channels in ONE launch (fewer vectors than a workgroup has threads, an odd pixel count), bf16 and float32 sources in
NCHW and channels-last memory, three successive pushes (shifted data is shifted again), a guard band behind each window.  The
stand-in's forward, REVERSE and RANDOM fiber schedules: the in-place shift rests on one thread owning a vector position in all T
frames -- a kernel in which a position changed hands between threads would read a frame another thread had already overwritten
under one of the orders.

ARGUMENTS: every limit of include/stp3_hip.h answers STP3_EINVAL / STP3_EUNSUP without a GPU.  RESOURCES: the gfx950 kernel
uses no scratch and spills nothing.  CALL TRACE (tests/host_trace.py, tests/streaming_trace.py): one tick issues exactly one
stp3_window_push and one stp3_lift_splat_fwd, and the encoder's calls of the full-window engine one for one, each on B * N
images where the full window carries B * T * N."""
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
import run_window as RW  # noqa: E402

ORDERS = [None, 'reverse', 'random']


# ---- the real kernel source, executed on the host (tests/hipcpu) ----
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_window')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_window.hip')])


@pytest.fixture(scope='module', params=ORDERS, ids=lambda o: o or 'forward')
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = {k: v for k, v in os.environ.items() if not k.startswith(('STP3_', 'HIPCPU_'))}
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "forward"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_window.py'), lib, path], env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return dict(np.load(path))


def roll_and_append(window, new):
    """window [B][T][NPIX][C], new [B*N][C][fH][fW] float32 -> the window one frame later."""
    b, t, npix, c = window.shape
    frame = new.reshape(b, -1, c, new.shape[2] * new.shape[3]).transpose(0, 1, 3, 2).reshape(b, npix, c)
    return np.concatenate([window[:, 1:], frame[:, None]], axis=1)


@pytest.mark.parametrize('name', sorted(RW.CASES))
def test_window_push_is_a_roll_and_append(host_kernel, name):
    b, t, dt, layout = RW.CASES[name]
    npix = RW.N * RW.FH * RW.FW
    pushes = RW.sources(name)
    for j, c in enumerate(RW.CHANNELS):
        size = b * t * npix * c
        want = RW.initial(name, c)[:size].reshape(b, t, npix, c)
        for k in range(RW.PUSHES):
            values = pushes[k][j][0]
            want = roll_and_append(want, values)
            got = host_kernel[f'{name}/{j}/{k}']
            assert got.dtype == np.float32 and got.shape == (size + RW.GUARD,)
            assert np.array_equal(got[:size].view(np.uint32), want.reshape(-1).view(np.uint32)), (name, j, k)
            assert (got[size:] == RW.GUARD_VALUE).all(), (name, j, k)                     # nothing behind the window is written
        if t == RW.PUSHES:                                                              # the first frame pushed is now frame 0
            first = roll_and_append(np.zeros((b, 1, npix, c), np.float32), pushes[0][j][0])
            assert np.array_equal(want[:, 0], first[:, 0])


# ---- argument validation: the gfx950 library, no GPU ----
def test_argument_validation_without_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUP = -10001, -10002
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 63) // 64 * 64

    def push(B=1, T=3, N=2, pixels=15, n_jobs=None, null_jobs=False, **fields):
        base = dict(src=p, window=p, stride_image=180, stride_channel=15, stride_pixel=1, channels=12, dtype=_lib.DTYPE_BF16)
        many = fields.pop('many', 1)
        jobs = (_lib.WindowJob * max(many, 1))()
        for job in jobs:
            for k, v in {**base, **fields}.items():
                setattr(job, k, v)
        return lib.stp3_window_push(B, T, N, pixels, many if n_jobs is None else n_jobs, None if null_jobs else jobs, None)

    assert push(T=0) == EINVAL and push(T=-1) == EINVAL                                  # T < 1
    assert push(B=0) == EINVAL and push(N=0) == EINVAL and push(pixels=0) == EINVAL
    assert push(src=None) == EINVAL and push(window=None) == EINVAL and push(null_jobs=True) == EINVAL   # null pointers
    assert push(channels=0) == EINVAL and push(stride_pixel=-1) == EINVAL and push(n_jobs=-1) == EINVAL
    assert push(channels=10) == EUNSUP and push(channels=6) == EUNSUP                    # channels % 4 != 0
    assert push(dtype=2) == EUNSUP
    assert push(window=p + 4) == EUNSUP                                                 # the window side is 16-byte vectors
    assert push(many=_lib.WINDOW_JOBS_MAX + 1) == EUNSUP
    # window bytes >= 2^32: B T N pixels channels 4 = 2^32 exactly, and far beyond
    assert push(B=4, T=4, N=64, pixels=1 << 16, channels=16) == EUNSUP
    assert push(B=1 << 20, T=1 << 20, N=1 << 20, pixels=1 << 20, channels=1 << 20) == EUNSUP
    assert push(n_jobs=0) == 0                                                          # nothing to do
    header = open(os.path.join(ROOT, 'include', 'stp3_hip.h')).read()
    assert int(re.search(r'#define STP3_WINDOW_JOBS_MAX (\d+)', header).group(1)) == _lib.WINDOW_JOBS_MAX == 4


def test_binding_matches_the_header_struct():
    from stp3_amd import _lib
    assert ctypes.sizeof(_lib.WindowJob) == 48
    header = open(os.path.join(ROOT, 'include', 'stp3_hip.h')).read()
    body = re.search(r'typedef struct stp3_window_job \{(.*?)\} stp3_window_job;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'\b(\w+)\s*(?:,|$)', decl.strip().split(' ', 1)[-1].replace('*', ' '))]
    assert names == [f[0] for f in _lib.WindowJob._fields_], names
    assert 'carla_agent.py:408-432' in header                                           # the reference lines the entry point serves


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('c++filt') is None, reason='needs hipcc')
def test_window_kernel_uses_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources
    rows = kernel_resources.kernels_of(os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_window.hip'))
    assert [k['kernel'] for k in rows] == ['window_push_kernel'], rows
    for k in rows:
        assert k['scratch'] == 0 and k['vgpr_spills'] == 0 and k['sgpr_spills'] == 0, k
        assert k['lds_static'] == 0 and k['vgpr'] + k['agpr'] <= 64, k                  # 8 workgroups of 256 threads per CU: the grid's round


# ---- call trace ----
def _sections(path):
    out, name = {}, None
    for line in open(path).read().splitlines():
        if line.startswith('# '):
            name = line[2:].split()[0]
            out[name] = [line[2:]]
        elif name is not None:
            out[name].append(line)
    return out


@pytest.fixture(scope='module')
def traces(tmp_path_factory):
    from tests import host_trace
    tmp = tmp_path_factory.mktemp('streaming_trace')
    recorder = host_trace.build_recorder(str(tmp / 'libstp3hip_recorder.so'))
    logs = {}
    for name, argv in (('tick', ['streaming_trace.py', recorder]), ('full', ['inference_trace.py', recorder, 'engine'])):
        log = tmp / f'{name}.log'
        env = dict(os.environ)
        env.update(STP3_HOST_DRYRUN='1', STP3_TRACE_LOG=str(log), STP3_REAL_LIB=os.path.join(PKG, 'libstp3hip.so'))
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', argv[0])] + argv[1:], env=env, check=True, timeout=900,
                       stderr=subprocess.DEVNULL)
        assert open(log).read().splitlines()[-1] == '# end'
        logs[name] = _sections(str(log))
    return logs


def _images(line):
    """(image count of an encoder call or None, the call with that count and every byte size blanked)."""
    line = re.sub(r':[0-9a-f]{8}\b', '', line)
    line = re.sub(r'\b(workspace_bytes|bytes)=\d+', r'\1=*', line)
    m = re.search(r' dims=([0-9a-f]{8})', line)
    if m:
        return struct.unpack('<i', bytes.fromhex(m.group(1)))[0], line[:m.start(1)] + '*' + line[m.end(1):]
    m = re.search(r' M=(\d+)', line)
    if m:
        return int(m.group(1)), line[:m.start(1)] + '*' + line[m.end(1):]
    return None, line


def test_one_tick_pushes_once_and_encodes_a_third(traces):
    tick, full = traces['tick'], traces['full']
    name = lambda line: line.split()[0]                                                 # noqa: E731
    b, t, n = (int(v) for v in tick['shapes'][0].split()[1:])
    assert t == 3 and b * n < b * t * n
    body = tick['tick'][1:]
    pushes = [line for line in body if name(line) == 'stp3_window_push']
    assert len(pushes) == 1, pushes
    assert f' B={b} T={t} N={n} ' in pushes[0] and ' n_jobs=2 ' in pushes[0], pushes[0]  # both caches in the one launch
    assert sum(name(line) == 'stp3_lift_splat_fwd' for line in body) == 1
    order = [name(line) for line in body if name(line) in ('stp3_window_push', 'stp3_lift_splat_fwd')]
    assert order == ['stp3_window_push', 'stp3_lift_splat_fwd']
    # the encoder: the full-window engine's calls one for one, each on B N images instead of B T N (the weight shadows are
    # prepared at a weight's first use, with no image count: left out on both sides)
    calls = lambda lines: [line for line in lines if name(line) != 'stp3_conv2d_prep_weights']      # noqa: E731
    want = calls(full['encoder'][1:])
    for part in (calls(tick['encoder'][1:]), calls(body[:body.index(pushes[0])])):
        assert len(part) == len(want) > 100, (len(part), len(want))
        for got_line, want_line in zip(part, want):
            (got_n, got_rest), (want_n, want_rest) = _images(got_line), _images(want_line)
            assert got_rest == want_rest, (got_line, want_line)
            assert want_n == b * t * n and got_n == b * n, (got_line, want_line)
        print(f'encoder: {len(part)} calls, each on {b * n} images where the full window has {b * t * n}')
    # behind the pool the tick is the full-window forward's tail, call for call
    tail = lambda lines: [re.sub(r':[0-9a-f]{8}\b', '', line) for line in lines[[name(x) for x in lines].index('stp3_lift_splat_fwd'):]]  # noqa: E731
    assert tail(calls(body)) == tail(calls(full['full'][1:]))
    assert tick['outputs'][0] == full['outputs'][0]
    assert tick['depth_prediction'][0].split()[1:4] == [str(b), str(t), str(n)]
