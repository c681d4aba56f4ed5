"""Writes tests/golden/image_augment.npz: the reference's own ``resize_and_crop_image`` (stp3/utils/geometry.py:9-13) and
``img_transform`` (stp3/utils/tools.py:122-146), unmodified and loaded from the reference tree, on the cases of
tests/augment_cases.py, for tests/test_augment_cpu.py / test_augment_gpu.py.

    python scripts/make_golden_augment.py

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, torch, Pillow and matplotlib.  Data only; the inputs are
not stored: the tests rebuild them and check the sha256 stored here first.  ``oracle.ref_stubs`` is used unchanged; tqdm (if
absent) gets an empty stand-in here -- tools.py imports it at module level and these paths never use it.

Per image of a case:
  1. ``resize_and_crop_image(img, resize_dims, (0, 0) + resize_dims)``: the BILINEAR resize, no crop yet;
  2. ``img_transform(resized, eye(2), zeros(2), resize, resized.size, crop, flip, rotate)``: with ``resize_dims`` equal to the
     image's size its unnamed-filter resize is Pillow's same-size copy, so the crop, the flip and the rotation are the
     reference's own statements and the filter is the loader's.
``<case>/bytes``: the (n, Ho, Wo, 3) uint8 results (sha256 + every 97th byte where large), ``<case>/post_rot`` (n, 2, 2) and
``<case>/post_tran`` (n, 2) float32 from the same calls, ``<case>/sha`` the digest of the input bytes."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
from oracle import ref_stubs  # noqa: E402
from tests import augment_cases as AC  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'image_augment.npz')


def load_reference():
    ref_stubs.install()
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules['tqdm'] = types.ModuleType('tqdm')
        sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    import stp3.utils.geometry as G
    import stp3.utils.tools as T
    return G, T


def put(out, key, value):
    value = np.asarray(value)
    if value.size > AC.LARGE:
        out[f'{key}/sha'] = np.array(AC.digest(value))
        out[f'{key}/sample'] = AC.strided(value)
        out[f'{key}/shape'] = np.array(value.shape, dtype=np.int64)
    else:
        out[key] = value


def main():
    import PIL
    from PIL import Image
    G, T = load_reference()
    out = {'meta/pillow': np.array(PIL.__version__)}
    for name, case in AC.CASES.items():
        images = AC.build(name)
        out[f'{name}/sha'] = np.array(AC.digest(images))
        results, rots, trans = [], [], []
        for a, p in zip(images, case['params']):
            resized = G.resize_and_crop_image(Image.fromarray(a), p['resize_dims'], (0, 0) + p['resize_dims'])
            assert resized.size == p['resize_dims']
            img, post_rot, post_tran = T.img_transform(resized, torch.eye(2), torch.zeros(2), resize=p['resize'],
                                                       resize_dims=resized.size, crop=p['crop'], flip=p['flip'],
                                                       rotate=p['rotate'])
            results.append(np.asarray(img))
            rots.append(post_rot.numpy())
            trans.append(post_tran.numpy())
        results = np.stack(results)
        assert results.shape == (len(images),) + tuple(case['final']) + (3,) and results.dtype == np.uint8
        put(out, f'{name}/bytes', results)
        out[f'{name}/post_rot'] = np.stack(rots).astype(np.float32)
        out[f'{name}/post_tran'] = np.stack(trans).astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
