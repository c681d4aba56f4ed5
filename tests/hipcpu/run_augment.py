"""TEST INFRASTRUCTURE -- run stp3_image_augment (csrc/stp3_image.hip) on CPU tensors through libstp3hip_cpu.so
(tests/hipcpu/build.py) and store what the kernels wrote.

    python tests/hipcpu/run_augment.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_augment_cpu.py (which holds the checks); the fiber order of the stand-in (HIPCPU_ORDER) is read from the
environment.  Per small case of tests/augment_cases.py: ``<case>/out`` (float32), ``/bf16`` (bits), ``/replay`` (the plan's
tensors rewritten in place with the case's second parameter set and other bytes, float32), ``/plain`` (no flip, no rotation:
the single-launch path), ``/prep`` (ImagePreprocessor on the first image's parameters: the shared body through the old entry)
and ``/bad`` (the table entry of image 2 pointing outside the coefficient buffer: that image is left as it was)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import augment_cases as AC  # noqa: E402

SENTINEL = 77.0


def setup(lib_path):
    """As tests/hipcpu/run_carla.setup: the binding loads the host-built library, CPU tensors take the GPU route."""
    from stp3_amd import _lib
    _lib.LIB_PATH = lib_path
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if k.startswith('stp3_image_')}
    from stp3_amd import ops
    ops._need_gpu = lambda *a: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    torch.Tensor.is_cuda = property(lambda self: True)


def main(lib_path, out_path):
    setup(lib_path)
    from stp3_amd.datas import ImagePreprocessor
    out = {}
    for name in AC.SMALL:
        aug, params = AC.augmenter(name), AC.CASES[name]['params']
        images = torch.from_numpy(AC.build(name))
        out[f'{name}/out'] = aug(images, params).numpy()
        out[f'{name}/bf16'] = aug(images, params, out_dtype=torch.bfloat16).view(torch.int16).numpy()
        # the static tensors of one plan, rewritten: room reserved for what the second set needs
        second = aug.host_tables(AC.REPLAY[name], 4)
        plan = aug.plan(params, images.device, ksize=second[2], strip_rows=second[3], coef_len=second[1].size, rotate=True, cols=second[5])
        first = aug.run(images, plan).clone()
        assert torch.equal(first, torch.from_numpy(out[f'{name}/out']))
        assert aug.plan(AC.REPLAY[name], images.device, like=plan) is plan
        out[f'{name}/replay'] = aug.run(torch.from_numpy(AC.build(name, 100)), plan).numpy()
        plain = [dict(p, flip=False, rotate=0.0) for p in params]
        assert aug.plan(plain, images.device).rotate == 0
        out[f'{name}/plain'] = aug(images, plain).numpy()
        p0 = params[0]
        out[f'{name}/prep'] = ImagePreprocessor(resize_dims=p0['resize_dims'], crop=p0['crop'],
                                                source_hw=AC.CASES[name]['shape'][1:3])(images).numpy()
        bad = aug.plan(params, images.device)
        bad.table[2, 11] = bad.coef.numel()                                # kk_h of image 2
        held = torch.full((len(params), 3) + tuple(AC.CASES[name]['final']), SENTINEL)
        out[f'{name}/bad'] = aug.run(images, bad, out=held).numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
