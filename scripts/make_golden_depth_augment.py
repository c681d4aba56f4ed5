"""Writes tests/golden/depth_augment.npz: the depth labels under the per-image augmentation, as the chain of the reference's
own statements (unmodified, loaded from the reference tree as scripts/make_golden_depth.py and make_golden_augment.py load
them) gives them on the cases of tests/depth_augment_cases.py, for tests/test_depth_augment_cpu.py / _gpu.py.

    python scripts/make_golden_depth_augment.py

Needs the reference tree (oracle/ref_stubs.REFERENCE_ROOT), numpy, torch, Pillow and matplotlib.  Data only; the inputs are
not stored: the tests rebuild them and check the sha256 stored here first.

The reference never combines ``img_transform`` with its depth branch; per image of a case with parameters p the chain is
  1. LiDAR: ``FuturePredictionDataset.get_depth_from_lidar`` (NuscenesData.py:289-300) unbound, with RESIZE_SCALE = p.resize
     and a crop that covers the whole resized map (scatter, F.interpolate with recompute_scale_factor=True, torch.round);
     maps: the depth branch of ``get_input_data`` (:257-267) with the same scale and crop (``make_golden_depth.map_reference``);
  2. ``img_transform`` (tools.py:122-146) on that rounded map as a Pillow mode-'F' image with ``resize_dims`` equal to its
     size (the resize is then Pillow's same-size copy): the crop, the flip and the rotation are the reference's own.
Stored per case: ``sha`` (digest of the inputs), ``depths`` int16 (F, N, Ho, Wo) (sha256 + every 97th value + shape where
large), ``labels`` int16 (trainer.py:269-276 restated on it, as make_golden_depth.labels_of), ``nonzero`` the non-zero outputs
per image, and
  margin    float64 routes: the smallest distance of a non-zero unrounded output from a half-integer (asserted > 1e-6; the
            distances are carried through the same img_transform, as a float32 image)
  excluded  the float32 map: int32 (k, 4) = (frame, camera, row, column) of the outputs whose unrounded value lies within 1e-3
            of a half-integer, carried through the same img_transform -- the tests compare those to +-1 and everything else
            exactly; at most 0.5 % of the case's outputs (asserted)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_augment as MA  # noqa: E402
import make_golden_depth as MD  # noqa: E402
from tests import depth_augment_cases as DA  # noqa: E402
from tests import depth_cases as DC  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'depth_augment.npz')


def resized_maps(ND, name, inputs, f, c, p):
    """(rounded, unrounded) resized map of image (f, c): the reference's depth branch at this image's scale, uncropped."""
    h, w = DA.source_hw(name)
    wr, hr = p['resize_dims']
    geo = dict(source_hw=(h, w), scale=p['resize'], crop=(0, 0, wr, hr), downsample=DA.DOWNSAMPLE, d_bound=DA.D_BOUND)
    if 'maps' in inputs:
        rounded, raw = MD.map_reference(ND, dict(maps=inputs['maps'][f:f + 1, c:c + 1], **geo))
    else:
        a, b = inputs['offsets'][f], inputs['offsets'][f + 1]
        one = dict(points=inputs['points'][a:b], offsets=np.array([0, b - a], np.int32), steps=inputs['steps'][f:f + 1, c:c + 1],
                   intrinsics=inputs['intrinsics'][f:f + 1, c:c + 1], **geo)
        if a == b:                                                     # (numpy cannot stack no points; the map is zero)
            rounded = raw = np.zeros((1, 1, hr, wr))
        else:
            rounded, raw, _ = MD.lidar_reference(ND, one)
    assert rounded.shape == (1, 1, hr, wr), (name, rounded.shape, (hr, wr))
    return rounded[0, 0], raw[0, 0]


def transformed(T, image, p):
    """``img_transform`` of a float map as a mode-'F' image."""
    from PIL import Image
    img = Image.fromarray(np.ascontiguousarray(image, dtype=np.float32), mode='F')
    out, _, _ = T.img_transform(img, torch.eye(2), torch.zeros(2), resize=p['resize'], resize_dims=img.size, crop=p['crop'],
                                flip=p['flip'], rotate=p['rotate'])
    return np.asarray(out)


def main():
    import PIL
    ND = MD.load_reference()
    _, T = MA.load_reference()
    out = {'meta/pillow': np.array(PIL.__version__),
           'meta/chain': np.array('get_depth_from_lidar / get_input_data at the image\'s scale with a crop covering the resized map, '
                                  'then img_transform on the rounded map as a mode-F image (resize_dims = its size)')}
    for name, case in DA.CASES.items():
        inputs, params = DA.build(name), DA.params(name)
        n_frames, n_cam = DA.FRAMES_CAMERAS[name]
        out[f'{name}/sha'] = np.array(DA.digest(*(inputs[k] for k in DA.input_keys(name))))
        results, excluded, margin = [], [], np.inf
        for i, p in enumerate(params):
            f, c = divmod(i, n_cam)
            rounded, raw = resized_maps(ND, name, inputs, f, c, p)
            assert np.array_equal(rounded, np.rint(rounded)) and rounded.min() >= 0 and rounded.max() < 2 ** 15
            dist = MD.half_distance(raw.astype(np.float64))
            if raw.dtype == np.float32:
                near = transformed(T, (dist < MD.HALF_MARGIN_F32).astype(np.float32), p)
                excluded += [(f, c, y, x) for y, x in np.argwhere(near > 0)]
            else:                                                      # (the distances of the values that reach an output)
                reach = transformed(T, (raw != 0).astype(np.float32), p) > 0
                if reach.any():
                    margin = min(margin, float(transformed(T, dist, p)[reach].min()))
            results.append(transformed(T, rounded, p))
            assert results[-1].shape == tuple(case['final']) and results[-1].dtype == np.float32
        depths = np.stack(results).reshape((n_frames, n_cam) + tuple(case['final']))
        nonzero = (depths != 0).reshape(len(params), -1).sum(axis=1)
        if name in ('l24', 'l17', 'real'):
            assert nonzero.min() >= DA.MIN_NONZERO, (name, nonzero)
        if case.get('dtype') == 'float32':
            assert len(excluded) <= MD.EXCLUDED_CAP * depths.size, (name, len(excluded), depths.size)
            out[f'{name}/excluded'] = np.array(excluded, dtype=np.int32).reshape(-1, 4)
        else:
            assert margin > MD.HALF_MARGIN_F64, (name, margin)
            out[f'{name}/margin'] = np.float64(margin)
        MA.put(out, f'{name}/depths', depths.astype(np.int16))
        out[f'{name}/labels'] = MD.labels_of(depths, dict(downsample=DA.DOWNSAMPLE, d_bound=DA.D_BOUND)).astype(np.int16)
        out[f'{name}/nonzero'] = nonzero.astype(np.int64)
        print(f'{name}: {depths.shape}, non-zero outputs per image {nonzero.tolist()}, margin {margin:.2e}, {len(excluded)} excluded')
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
