"""GPU: stp3_image_augment (csrc/stp3_image.hip) on the MI355X against the torch statements of
``stp3_amd.datas.ImageAugmenter.reference`` -- which tests/test_augment_cpu.py pins against the reference's functions and
Pillow -- BIT FOR BIT, as tests/test_datas_gpu.py holds the plain kernel: the bytes are integer arithmetic, the float32
statements (x / 255 - mean) / std are the same correctly rounded operations on both sides, bf16 is one rounding of that float32.
The cases (tests/augment_cases.py) are single calls of six images with six different parameter sets."""
import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import helpers as H
from tests.test_augment_cpu import built, same, twin
from tests.test_datas_cpu import as_bytes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(AC.CASES))
def test_kernel_matches_twin(name):
    """`nuscenes`: 6 x 900 x 1600 -> 224 x 480 at the timing parameters; the small cases: padded tap counts, crops beyond three
    borders, both load paths, all six angles."""
    aug, params = AC.augmenter(name), AC.CASES[name]['params']
    images = built(name).cuda()
    y = aug(images, params)
    want = twin(name)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == tuple(want.shape)
    differ = (y.cpu() != want).flatten(1).sum(1).tolist()
    assert torch.equal(y.cpu(), want), f'{name}: differing outputs per image {differ}'
    same(as_bytes(y), f'{name}/bytes', 'kernel')                                        # and the reference's bytes themselves
    assert torch.equal(aug(images, params, out_dtype=torch.bfloat16), y.to(torch.bfloat16))


@pytest.mark.parametrize('name', AC.SMALL)
def test_without_flip_and_rotation_it_is_the_plain_kernel(name):
    """One launch (no image is rotated), per-image resize and crop: each image equals ImagePreprocessor with its parameters."""
    from stp3_amd.datas import ImagePreprocessor
    aug = AC.augmenter(name)
    params = [dict(p, flip=False, rotate=0.0) for p in AC.CASES[name]['params']]
    images = built(name).cuda()
    assert aug.plan(params, images.device).rotate == 0
    y = aug(images, params)
    for i, p in enumerate(params):
        prep = ImagePreprocessor(resize_dims=p['resize_dims'], crop=p['crop'], source_hw=AC.CASES[name]['shape'][1:3])
        assert torch.equal(y[i], prep(images[i:i + 1])[0]), i
    assert tuple(aug(images.view(2, 3, *images.shape[1:]), params).shape) == (2, 3) + tuple(y.shape[1:])


@pytest.mark.parametrize('name', AC.SMALL)
def test_captured_and_replayed_with_new_parameters(name):
    """Captured on one stream (it could not be if anything inside waited for the device); replayed after the parameter table,
    the coefficient tables and the bytes in the static buffers were rewritten."""
    aug, params, second = AC.augmenter(name), AC.CASES[name]['params'], AC.REPLAY[name]
    room = aug.host_tables(second, 4)
    static = built(name).cuda().clone()
    plan = aug.plan(params, static.device, ksize=room[2], strip_rows=room[3], coef_len=room[1].size, rotate=True, cols=room[5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.run(static, plan)                                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = aug.run(static, plan)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, aug(built(name).cuda(), params)) and torch.equal(out.cpu(), twin(name))
    static.copy_(built(name, 100))
    assert aug.plan(second, static.device, like=plan) is plan
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, aug(built(name, 100).cuda(), second)) and torch.equal(out.cpu(), twin(name, True))
    assert not torch.equal(twin(name), twin(name, True))


def test_flipped_and_rotated_camera_through_the_lift():
    """The path end to end: K' = P K of a flipped camera rotated by 10 degrees is a general 3 x 3 matrix; the voxel ids of the
    id kernel equal the oracle's restatement with the same K' (exactly, as for upper-triangular intrinsics)."""
    from stp3_amd import ops
    from stp3_amd.datas import ImageAugmenter
    cfg = H.SMALL
    intr, extr, ego, _, _ = H.lift_inputs(cfg, 1, 2, 2, seed=23)
    h, w = cfg['final_dim']
    aug = ImageAugmenter(source_hw=(h, w), final_dim=(h, w))
    params = [aug.make_params(1.0, (w, h), (0, 0, w, h), flip, angle) for flip, angle in
              ((True, 10.0), (False, 0.0), (True, -10.0), (False, 10.0))]
    k = aug.intrinsics(intr.float(), params)
    assert tuple(k.shape) == (1, 2, 2, 3, 3) and float(k[0, 0, 0, 1, 0].abs()) > 1.0 and float(k[0, 0, 0, 0, 0]) < 0.0
    assert torch.equal(k[0, 0, 1], intr.float()[0, 0, 1])                                # identity parameters leave K alone
    frustum, res, start, dim = H.grid_params(cfg)
    grid = ops.LiftGrid(frustum, res, start, dim, 'cuda')
    plan = ops.LiftPlan.build(grid, k, extr, ego, cfg['out_channels'])
    vox = H.oracle_vox(cfg, k, extr, ego)
    assert np.array_equal(plan.voxel_ids().cpu().numpy(), vox)
    assert (vox >= 0).sum() > 100 and not np.array_equal(vox, H.oracle_vox(cfg, intr, extr, ego))
