"""Writes tests/golden/sampler.npz: the reference's trajectory sampler (stp3/utils/sampler.py:8-146, unmodified, loaded from
the reference tree) on six (v0, kappa, M, n_future) cases, for tests/test_sampler_cpu.py / test_sampler_gpu.py.

    python scripts/make_golden_sampler.py [--time]

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, scipy and torch; the tests need none of the first two.

Per case ``c<i>_``:
  params   float64 [4] = v0, kappa, M, n_future
  draws    float64 [3 M + 2 Mc]: the uniform stream the reference consumed, in its order (accelerations [M], velocity
           candidates [M], velocity selection [M], clothoid scales [Mc], arc-or-clothoid pick [Mc]); ``np.random.seed(s)``
           followed by one long ``np.random.rand`` equals the reference's consecutive calls, and its
           ``np.random.choice([0, 1], p=(0.2, 0.8))`` consumes one uniform per element and equals ``u >= 0.2``
  rows     float32 [M][n_future + 1][3]: the rows in GENERATION order ([left | lines | right], sampler.py:142) at the coarse
           time stamps ([:, ::10], NuscenesData.py:436) -- a second call on the same seed with ``numpy.argsort`` patched to
           the identity for its duration, so that the unmodified code skips its (unstable) ordering
  keys     float64 [M]: the final-x keys of the normal call, in its sorted order
and ``fresnel_x / fresnel_s / fresnel_c``: scipy.special.fresnel on 2 049 points of [-16, 16] (float64).
``--time`` also prints the reference's host time per sample (after warm-up) with the CPU model it ran on.
"""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_stubs import REFERENCE_ROOT  # noqa: E402

CASES = [(5.0, 0.0, 1800, 6), (8.3, 0.05, 1800, 6), (0.0, -0.3, 1800, 6), (12.0, 0.004, 600, 4), (3.0, -0.004, 60, 4),
         (14.9, 0.9, 600, 6)]
SEED0 = 20240
OUT = os.path.join(ROOT, 'tests', 'golden', 'sampler.npz')


def load_reference():
    spec = importlib.util.spec_from_file_location('reference_sampler', os.path.join(REFERENCE_ROOT, 'stp3', 'utils', 'sampler.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def call(ref, v0, kappa, m, n_future, seed):
    """NuscenesData.get_trajectory_sampling :427-436 with the CAN values given."""
    t0 = np.array([0.0, 1.0])
    n0 = np.array([1.0, 0.0]) if kappa <= 0 else np.array([-1.0, 0.0])
    tt = np.arange(0, n_future * 0.5 + 0.05, 0.05)
    np.random.seed(seed)
    return ref.sample(v0, kappa, t0, n0, tt, m)


def main():
    ref = load_reference()
    out = {}
    for i, (v0, kappa, m, nf) in enumerate(CASES):
        seed = SEED0 + i
        fine = call(ref, v0, kappa, m, nf, seed)
        assert fine.shape == (m, 10 * nf + 1, 3) and np.isfinite(fine).all()
        keep = np.argsort
        np.argsort = lambda a, *args, **kw: np.arange(len(a))
        try:
            gen = call(ref, v0, kappa, m, nf, seed)
        finally:
            np.argsort = keep
        keys = fine[:, -1, 0]
        assert (np.diff(keys) >= 0).all() and np.array_equal(np.sort(gen[:, -1, 0]), keys)
        mc = int(m * 0.4) + int(m * 0.4)
        np.random.seed(seed)
        draws = np.random.rand(3 * m + 2 * mc)
        out[f'c{i}_params'] = np.array([v0, kappa, m, nf], dtype=np.float64)
        out[f'c{i}_draws'] = draws
        out[f'c{i}_rows'] = gen[:, ::10].astype(np.float32)
        out[f'c{i}_keys'] = keys.astype(np.float64)
    from scipy.special import fresnel
    x = np.linspace(-16.0, 16.0, 2049)
    s, c = fresnel(x)
    out['fresnel_x'], out['fresnel_s'], out['fresnel_c'] = x, s, c
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')
    if '--time' in sys.argv:
        cpu = [l.split(':', 1)[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name')][:1]
        for v0, kappa, m, nf in CASES[:3]:
            for _ in range(3):
                call(ref, v0, kappa, m, nf, 1)
            t = time.perf_counter()
            for _ in range(10):
                call(ref, v0, kappa, m, nf, 1)
            print(f'reference sample(v0={v0}, kappa={kappa}, M={m}, n_future={nf}): {(time.perf_counter() - t) * 100:.1f} ms per sample on {cpu}')


if __name__ == '__main__':
    main()
