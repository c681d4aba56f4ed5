"""TEST INFRASTRUCTURE -- the cases of the depth labels under the per-image augmentation (stp3_amd.datas.DepthLabeller with
``params``; csrc/stp3_depth_augment.hip), shared by scripts/make_golden_depth_augment.py (which records what the reference's
own statements make of them in tests/golden/depth_augment.npz), tests/test_depth_augment_cpu.py,
tests/hipcpu/run_depth_augment.py and tests/test_depth_augment_gpu.py.  The inputs are rebuilt from seeds
(tests/depth_cases.build_lidar, numpy.random.RandomState) and their sha256 is stored with the fixture.  numpy only.

Every small case is ONE call of six images (3 frames x 2 cameras) of 90 x 160 with the six parameter sets of
``augment_cases._small``: scales 0.3 / 0.55 / 1.4 (the up-scale makes one source pixel a tap of several outputs), crops that
leave the resized map on the left, the right, the bottom and with a negative top, flips on and off, the angles 0, 0.3, -5.4,
17.25, 90 and 180 degrees.  Windows: 24 x 40, and an odd 17 x 23 whose last label row and column (downsample 8) are partial.
  l24, l17   clouds dense enough that every image has at least MIN_NONZERO non-zero outputs in the reference's result
             (the generator asserts it)
  e24        a frame without points and a frame with one
  m64, m32   dense stored maps, float64 and float32
  real       6 x 900 x 1600 -> 224 x 480 -> 28 x 60, 35 000 points, the parameters of ``augment_cases._nuscenes``
``REPLAY``: a second parameter set per small case and ``replay_cloud`` another cloud (graph replay)."""
import hashlib

import numpy as np

from tests import augment_cases as AC
from tests import depth_cases as DC

LARGE, STRIDE = AC.LARGE, AC.STRIDE
MIN_NONZERO = 20
DOWNSAMPLE, D_BOUND = 8, (2.0, 50.0, 1.0)
SOURCE = (90, 160)
# the clouds cover the whole source image (scale / crop of depth_cases.build_lidar only place its targets)
_WHOLE = dict(F=3, N=2, repeats=300, source_hw=SOURCE, scale=0.3, crop=(0, 0, 48, 27))
CASES = {
    'l24': dict(kind='lidar', final=(24, 40), cloud=dict(base='small', seed=131, counts=(3000, 3000, 3000), **_WHOLE)),
    'l17': dict(kind='lidar', final=(17, 23), cloud=dict(base='small', seed=132, counts=(6000, 6000, 6000), **_WHOLE)),
    'e24': dict(kind='lidar', final=(24, 40), cloud=dict(base='small', seed=133, counts=(0, 1, 3000), **_WHOLE)),
    'm64': dict(kind='maps', final=(24, 40), seed=141, dtype='float64'),
    'm32': dict(kind='maps', final=(17, 23), seed=142, dtype='float32'),
    'real': dict(kind='lidar', final=(224, 480), source_hw=(900, 1600), cloud=dict(base='real', crop=(0, 0, 480, 270))),
}
SMALL = ('l24', 'l17', 'e24', 'm64', 'm32')
FRAMES_CAMERAS = {name: ((1, 6) if name == 'real' else (3, 2)) for name in CASES}


def source_hw(name):
    return CASES[name].get('source_hw', SOURCE)


def params(name):
    """The six parameter sets of a case, in (frame, camera) order."""
    if name == 'real':
        return AC._nuscenes()
    (h, w), (ho, wo) = SOURCE, CASES[name]['final']
    return AC._small(h, w, ho, wo)


def replay_params(name):
    """A second set for the same window: every image takes the next one's rotation and the other flip."""
    p = params(name)
    return [dict(a, flip=not a['flip'], rotate=b['rotate']) for a, b in zip(p, p[1:] + p[:1])]


def build(name, seed_offset=0):
    """{'points', 'offsets', 'steps', 'intrinsics'} of a lidar case or {'maps'} (3, 2, 90, 160) of a map case."""
    c = CASES[name]
    if c['kind'] == 'lidar':
        over = dict(c['cloud'])
        base = over.pop('base')
        if seed_offset:
            over['seed'] = over.get('seed', DC.LIDAR_CASES[base]['seed']) + seed_offset
        built = DC.build_lidar(base, **over)
        return {k: built[k] for k in DC.LIDAR_KEYS}
    rs = np.random.RandomState(c['seed'] + seed_offset)
    return {'maps': rs.uniform(0.0, 70.0, size=FRAMES_CAMERAS[name] + SOURCE).astype(c['dtype'])}


def input_keys(name):
    return DC.LIDAR_KEYS if CASES[name]['kind'] == 'lidar' else ('maps',)


def labeller(name):
    """The DepthLabeller of a case: its own fixed scale and crop play no part in a call with ``params``."""
    from stp3_amd.datas import DepthLabeller
    h, w = source_hw(name)
    return DepthLabeller(source_hw=(h, w), scale=0.3, crop=(0, 0, int(w * 0.3), int(h * 0.3)), downsample=DOWNSAMPLE, d_bound=D_BOUND)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def strided(a):
    return np.ascontiguousarray(a).reshape(-1)[::STRIDE].copy()
