"""TEST INFRASTRUCTURE -- run csrc/stp3_window.hip on host memory through libstp3hip_cpu.so (tests/hipcpu/build.py) and store
what the kernel wrote.

    python tests/hipcpu/run_window.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_streaming_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Per case of ``CASES`` three successive stp3_window_push calls advance TWO windows (C and D channels) in one launch
each; ``<case>/<job>/<push>`` is the whole buffer after the push -- the window followed by a guard band of ``GUARD`` floats."""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

GUARD = 64
GUARD_VALUE = np.float32(-7.5)
PUSHES = 3
N, FH, FW, CHANNELS = 2, 3, 5, (12, 8)              # fewer vectors than one workgroup has threads; an odd pixel count
# name -> (B, T, source dtype, source layout)
CASES = {f'b{b}_t{t}_{dt}_{layout}': (b, t, dt, layout)
         for b, t, dt, layout in itertools.product((1, 2), (1, 2, 3), ('bf16', 'f32'), ('nchw', 'nhwc'))}


def sources(name):
    """The PUSHES new frames of both jobs: per push and job (values float32 [B*N][C][fH][fW] -- for bf16 exactly representable --,
    the memory image handed to the kernel, its element strides (image, channel, pixel))."""
    b, t, dt, layout = CASES[name]
    rng = np.random.default_rng(1000 * b + 100 * t + 10 * (dt == 'bf16') + (layout == 'nhwc'))
    out = []
    for _ in range(PUSHES):
        per_job = []
        for c in CHANNELS:
            v = rng.standard_normal((b * N, c, FH, FW)).astype(np.float32)
            if dt == 'bf16':
                v = (v.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
            mem = np.ascontiguousarray(v if layout == 'nchw' else v.transpose(0, 2, 3, 1))
            if dt == 'bf16':
                mem = (mem.view(np.uint32) >> 16).astype(np.uint16)
            strides = (c * FH * FW, FH * FW, 1) if layout == 'nchw' else (c * FH * FW, 1, c)
            per_job.append((v, mem, strides))
        out.append(per_job)
    return out


def initial(name, c):
    """The buffer before the first push: a window of recognisable values and the guard band."""
    b, t, _, _ = CASES[name]
    size = b * t * N * FH * FW * c
    return np.concatenate([np.arange(size, dtype=np.float32) * np.float32(0.25), np.full(GUARD, GUARD_VALUE, np.float32)])


def main(lib_path, out_path):
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    # the test builds csrc/stp3_window.hip alone (seconds instead of minutes): bind its entry only
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k == 'stp3_window_push'}
    lib = _lib.lib()
    out = {}
    for name, (b, t, dt, layout) in CASES.items():
        bufs = [initial(name, c) for c in CHANNELS]
        for k, per_job in enumerate(sources(name)):
            jobs = (_lib.WindowJob * len(CHANNELS))()
            for job, buf, c, (_, mem, strides) in zip(jobs, bufs, CHANNELS, per_job):
                job.src, job.window = mem.ctypes.data, buf.ctypes.data
                job.stride_image, job.stride_channel, job.stride_pixel = strides
                job.channels, job.dtype = c, _lib.DTYPE_BF16 if dt == 'bf16' else _lib.DTYPE_F32
            rc = lib.stp3_window_push(b, t, N, FH * FW, len(CHANNELS), jobs, None)
            assert rc == 0, (name, rc)
            for j, buf in enumerate(bufs):
                out[f'{name}/{j}/{k}'] = buf.copy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
