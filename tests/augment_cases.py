"""The cases of the image augmentation (stp3_amd.datas.ImageAugmenter; csrc/stp3_image.hip: stp3_image_augment), shared by
scripts/make_golden_augment.py (which records what the reference and Pillow make of them in tests/golden/image_augment.npz),
tests/test_augment_cpu.py, tests/hipcpu/run_augment.py and tests/test_augment_gpu.py.  The input bytes are rebuilt from a seed
(tests.helpers.image_bytes) and their sha256 is stored with the fixture.

Every small case is ONE call of six images with six different parameter sets: scales 0.3 (nine taps), 0.55 and 1.4 (upscale,
three taps) mixed, so the tap count is padded; crops that leave the resized image on the left, the right and the bottom; flip on
and off; the angles 0, 0.3, -5.4, 17.25, 90 and 180 degrees.  `s37` has a source row of 159 bytes (not a multiple of 16: the
unstaged load path) and an odd output, `s90` a row of 480 bytes and an even one.  `t13` and `t19` are the same six parameter sets
at stronger down-scales: at most 13 taps (the second dword path of the horizontal pass; the Lift-Splat resize range needs 11 or
13) and 19 taps (the byte loop).  `nuscenes` is 6 x 900 x 1600 -> 224 x 480
with parameters inside the limits the timing script draws from (resize 0.193 .. 0.225, bottom 0 .. 0.22, +-5.4 degrees, flip)."""
import hashlib

import numpy as np

from tests import helpers as H

LARGE = 65536                                      # outputs above this many elements are stored as sha256 + strided sample
STRIDE = 97
SCALES = (0.3, 0.55, 1.4, 0.3, 0.55, 1.4)
ANGLES = (0.0, 0.3, -5.4, 17.25, 90.0, 180.0)
FLIPS = (False, True, False, True, True, False)


def _param(resize, dims, crop, flip, rotate):
    return {'resize': float(resize), 'resize_dims': (int(dims[0]), int(dims[1])), 'crop': tuple(int(c) for c in crop),
            'flip': bool(flip), 'rotate': float(rotate)}


def _small(h, w, ho, wo, scales=SCALES):
    out = []
    for i, (s, angle, flip) in enumerate(zip(scales, ANGLES, FLIPS)):
        wr, hr = int(w * s), int(h * s)
        left, top = [(-3, 1), (wr - wo + 5, 0), (2, hr - ho + 4), (2, 1), (0, 0), (1, -2)][i]    # left, right, bottom, ...
        out.append(_param(s, (wr, hr), (left, top, left + wo, top + ho), flip, angle))
    return out


def _nuscenes():
    h, w, ho, wo = 900, 1600, 224, 480
    draws = [(0.1937, 0.05, 0.3, True, -5.4), (0.2249, 0.0, 0.9, False, 5.4), (0.21, 0.22, 0.5, True, 0.0),
             (0.2003, 0.11, 0.0, False, 2.125), (0.2188, 0.17, 0.7, True, -0.001), (0.193, 0.02, 0.2, False, 3.3)]
    out = []
    for resize, bot, u, flip, angle in draws:
        wr, hr = int(w * resize), int(h * resize)
        top = int((1 - bot) * hr) - ho
        left = int(u * max(0, wr - wo))
        out.append(_param(resize, (wr, hr), (left, top, left + wo, top + ho), flip, angle))
    return out


CASES = {'s37': {'shape': (6, 37, 53, 3), 'seed': 451, 'final': (17, 23), 'params': _small(37, 53, 17, 23)},
         's90': {'shape': (6, 90, 160, 3), 'seed': 452, 'final': (24, 40), 'params': _small(90, 160, 24, 40)},
         't13': {'shape': (6, 53, 208, 3), 'seed': 454, 'final': (12, 30),
                 'params': _small(53, 208, 12, 30, (0.2, 0.17, 0.22, 0.25, 0.17, 0.2))},
         't19': {'shape': (6, 50, 208, 3), 'seed': 455, 'final': (12, 30),
                 'params': _small(50, 208, 12, 30, (0.12, 0.2, 0.3, 0.12, 0.17, 0.2))},
         'nuscenes': {'shape': (6, 900, 1600, 3), 'seed': 453, 'final': (224, 480), 'params': _nuscenes()}}
SMALL = ('s37', 's90', 't13', 't19')
KSIZE = {'s37': 9, 's90': 9, 't13': 13, 't19': 19}    # the call's padded tap count: the three paths of the horizontal pass
# a second parameter set for the small cases (graph replay: the static tables are rewritten): rotated by one image
REPLAY = {name: [dict(p, flip=not p['flip'], rotate=q['rotate']) for p, q in
                 zip(CASES[name]['params'], CASES[name]['params'][1:] + CASES[name]['params'][:1])] for name in SMALL}


def build(name, seed_offset=0):
    c = CASES[name]
    return H.image_bytes(c['shape'], c['seed'] + seed_offset)


def augmenter(name):
    from stp3_amd.datas import ImageAugmenter
    c = CASES[name]
    return ImageAugmenter(source_hw=c['shape'][1:3], final_dim=c['final'])


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def strided(a):
    return np.ascontiguousarray(a).reshape(-1)[::STRIDE].copy()
