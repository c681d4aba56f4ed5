"""CPU: the per-image augmentation (stp3_amd.datas.ImageAugmenter; csrc/stp3_image.hip: stp3_image_augment) against the
reference's own ``resize_and_crop_image`` + ``img_transform`` recorded by scripts/make_golden_augment.py in
tests/golden/image_augment.npz on the cases of tests/augment_cases.py (the inputs are rebuilt here; their sha256 is checked
first), and against Pillow itself where it is installed.

Everything is compared EXACTLY: the chain is integer arithmetic up to the bytes (Pillow's 22-bit fixed-point resampler, its
16.16 fixed-point rotation), the homography is the reference's float32 torch statements run on the same machine.  The one
inequality is the geometric check that ties the bytes to the matrix: a bright blob must land within 2 px of P (u, v, 1) -- the
blob is 3 x 3 source pixels, halved by the resize, and NEAREST rotation moves a pixel by at most one; a wrong sign of the
rotation or a missing flip moves it by 10 px or more at these inputs (|x - centre| >= 30 px, |angle| >= 10 degrees)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_cases as AC
from tests import helpers as H
from tests.test_datas_cpu import as_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
LIMITS = dict(resize_lim=(0.193, 0.225), bot_pct_lim=(0.0, 0.22), rot_lim=(-5.4, 5.4), rand_flip=True)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(H.load('image_augment.npz'))


@functools.lru_cache(maxsize=None)
def built(name, seed_offset=0):
    images = AC.build(name, seed_offset)
    if not seed_offset:
        assert AC.digest(images) == str(fixture()[f'{name}/sha']), f'{name}: the case builder drifted'
    return torch.from_numpy(images)


@functools.lru_cache(maxsize=None)
def twin(name, replay=False):
    """The torch statements on a case (computed once, shared by the tests of this file and of tests/test_augment_gpu.py)."""
    params = AC.REPLAY[name] if replay else AC.CASES[name]['params']
    return AC.augmenter(name).reference(built(name, 100 if replay else 0), params)


def same(got, key, what):
    g = fixture()
    got = np.asarray(got)
    if f'{key}/sha' in g:
        assert got.shape == tuple(g[f'{key}/shape']) and got.dtype == g[f'{key}/sample'].dtype, (what, key, got.shape, got.dtype)
        assert np.array_equal(AC.strided(got), g[f'{key}/sample']), f'{what}: {key} (sample)'
        assert AC.digest(got) == str(g[f'{key}/sha']), f'{what}: {key} (digest)'
    else:
        assert got.shape == g[key].shape and got.dtype == g[key].dtype, (what, key, got.shape, got.dtype)
        assert np.array_equal(got, g[key]), f'{what}: {key}, {int((got != g[key]).sum())} elements differ'


def pillow_chain(image, p):
    from PIL import Image
    img = Image.fromarray(image).resize(p['resize_dims'], resample=Image.BILINEAR).crop(p['crop'])
    if p['flip']:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(img.rotate(p['rotate']))


def test_fixture_holds_data_only():
    g = fixture()
    assert os.path.getsize(os.path.join(H.GOLDEN, 'image_augment.npz')) <= 200 * 1024
    assert all(v.dtype.kind in 'iufU' for v in g.values())
    assert sorted({k.split('/')[0] for k in g} - {'meta'}) == sorted(AC.CASES)


def test_cases_cover_what_they_claim():
    for name in AC.SMALL:
        c = AC.CASES[name]
        ho, wo = c['final']
        aug = AC.augmenter(name)
        _, _, ksize, _, rotate, cols = aug.host_tables(c['params'], 4)
        assert 1 <= cols <= wo
        taps = {aug._axis(c['shape'][2], p['resize_dims'][0])[0].shape[1] for p in c['params']}
        assert ksize == AC.KSIZE[name] == max(taps) and len(taps) == 3 and rotate        # padded tap counts in one call
        if ksize == 9:
            assert taps == {9, 5, 3}
        assert any(p['crop'][0] < 0 for p in c['params']) and any(p['crop'][2] > p['resize_dims'][0] for p in c['params'])
        assert any(p['crop'][3] > p['resize_dims'][1] for p in c['params']) and {p['flip'] for p in c['params']} == {False, True}
        assert [p['rotate'] for p in c['params']] == [0.0, 0.3, -5.4, 17.25, 90.0, 180.0]
    assert (AC.CASES['s37']['shape'][2] * 3) % 16 != 0 and (AC.CASES['s90']['shape'][2] * 3) % 16 == 0
    for p in AC.CASES['nuscenes']['params']:
        assert 0.193 <= p['resize'] <= 0.225 and abs(p['rotate']) <= 5.4 and p['resize_dims'] == (int(1600 * p['resize']), int(900 * p['resize']))


@pytest.mark.parametrize('name', sorted(AC.CASES))
def test_torch_statements_match_the_reference(name):
    y = twin(name)
    ho, wo = AC.CASES[name]['final']
    assert y.dtype == torch.float32 and tuple(y.shape) == (6, 3, ho, wo)
    same(as_bytes(y), f'{name}/bytes', 'reference twin')
    same(AC.augmenter(name).reference_bytes(built(name), AC.CASES[name]['params']).numpy(), f'{name}/bytes', 'reference_bytes')
    if name in AC.SMALL:                                                                # CPU tensors take that route
        assert torch.equal(AC.augmenter(name)(built(name), AC.CASES[name]['params']), y)
        assert torch.equal(AC.augmenter(name)(built(name), AC.CASES[name]['params'], out_dtype=torch.bfloat16), y.to(torch.bfloat16))


@pytest.mark.parametrize('name', AC.SMALL)
def test_torch_statements_match_pillow_directly(name):
    pytest.importorskip('PIL')
    images = built(name).numpy()
    for params, offset in ((AC.CASES[name]['params'], 0), (AC.REPLAY[name], 100)):
        images = built(name, offset).numpy()
        want = np.stack([pillow_chain(a, p) for a, p in zip(images, params)])
        got = AC.augmenter(name).reference_bytes(torch.from_numpy(images), params).numpy()
        assert np.array_equal(got, want), [int((g != w).sum()) for g, w in zip(got, want)]


def test_rotation_integers_are_pillows():
    """Image.rotate with its defaults on five sizes and thirteen angles, the short-cut ones (0, 180, 90 / 270) included."""
    pytest.importorskip('PIL')
    from PIL import Image
    from stp3_amd.datas import ROTATE_IDENTITY, pil_rotate_fixed, rotate_nearest_pil
    assert pil_rotate_fixed(0.0, (480, 224)) == pil_rotate_fixed(360.0, (7, 13)) == ROTATE_IDENTITY
    for k, (ho, wo) in enumerate(((7, 13), (17, 23), (24, 40), (64, 64), (224, 480))):
        a = H.image_bytes((ho, wo, 3), 470 + k)
        for angle in (0.0, 5.4, -5.4, 1e-3, -1e-3, 17.25, 45.0, 90.0, -90.0, 180.0, 270.0, 359.9, 123.456):
            want = np.asarray(Image.fromarray(a).rotate(angle))
            got = rotate_nearest_pil(torch.from_numpy(a), pil_rotate_fixed(angle, (wo, ho))).numpy()
            assert np.array_equal(got, want), (ho, wo, angle, int((got != want).sum()))


@pytest.mark.parametrize('name', sorted(AC.CASES))
def test_post_homography_is_the_references(name):
    g = fixture()
    rot, tran = AC.augmenter(name).post_homography(AC.CASES[name]['params'])
    assert rot.dtype == tran.dtype == torch.float32
    assert torch.equal(rot, torch.from_numpy(g[f'{name}/post_rot'])) and torch.equal(tran, torch.from_numpy(g[f'{name}/post_tran']))


def test_intrinsics_without_flip_and_rotation_are_update_intrinsics():
    from stp3_amd.config import perception_cfg
    from stp3_amd.datas import ImageAugmenter, ImagePreprocessor, update_intrinsics
    k = torch.tensor([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]])
    cfg = perception_cfg()
    aug = ImageAugmenter(cfg)
    params = aug.sample(6, train=False)
    assert torch.equal(aug.intrinsics(k.expand(6, 3, 3), params), ImagePreprocessor(cfg).intrinsics(k).expand(6, 3, 3))
    assert torch.equal(aug.intrinsics(k, params[:1])[0], ImagePreprocessor(cfg).intrinsics(k))
    # drawn resizes and crops, leading dimensions, a principal point off the axis
    aug = ImageAugmenter(cfg, resize_lim=LIMITS['resize_lim'], bot_pct_lim=LIMITS['bot_pct_lim'])
    params = aug.sample(6, torch.Generator().manual_seed(3))
    ks = k.repeat(2, 3, 1, 1) + torch.arange(6.0).view(2, 3, 1, 1) * torch.tensor([[1.5, 0, 2.25], [0, -0.5, 1.0], [0, 0, 0]])
    got = aug.intrinsics(ks, params)
    assert tuple(got.shape) == (2, 3, 3, 3)
    for i, p in enumerate(params):
        assert not p['flip'] and p['rotate'] == 0.0
        want = update_intrinsics(ks.view(6, 3, 3)[i], p['crop'][1], p['crop'][0], p['resize'], p['resize'])
        assert torch.equal(got.view(6, 3, 3)[i], want), i


def test_eval_parameters_reproduce_the_preprocessor():
    from stp3_amd.config import perception_cfg
    from stp3_amd.datas import ImageAugmenter, ImagePreprocessor
    cfg = perception_cfg()
    images = torch.from_numpy(H.image_bytes((2, 900, 1600, 3), 402))
    aug = ImageAugmenter(cfg, **LIMITS)
    params = aug.sample(2, train=False)
    assert params[0] == params[1] and params[0]['resize_dims'] == (480, 270) and params[0]['crop'] == (0, 46, 480, 270)
    assert torch.equal(aug(images, params), ImagePreprocessor(cfg)(images))
    assert tuple(aug(images.view(1, 2, 900, 1600, 3), params).shape) == (1, 2, 3, 224, 480)


def test_sample_is_deterministic_and_inside_its_limits():
    from stp3_amd.config import perception_cfg
    from stp3_amd.datas import ImageAugmenter
    aug = ImageAugmenter(perception_cfg(), **LIMITS)
    a = aug.sample(200, torch.Generator().manual_seed(5))
    assert a == aug.sample(200, torch.Generator().manual_seed(5)) and a != aug.sample(200, torch.Generator().manual_seed(6))
    for p in a:
        wr, hr = p['resize_dims']
        left, top, right, bottom = p['crop']
        assert 0.193 <= p['resize'] <= 0.225 and -5.4 <= p['rotate'] <= 5.4 and (wr, hr) == (int(1600 * p['resize']), int(900 * p['resize']))
        assert (right - left, bottom - top) == (480, 224) and 0 <= left <= max(0, wr - 480)
        assert int(0.78 * hr) - 224 - 1 <= top <= hr - 224
    assert 60 < sum(p['flip'] for p in a) < 140 and len({p['resize_dims'] for p in a}) > 20
    assert not any(p['flip'] for p in ImageAugmenter(perception_cfg(), resize_lim=(0.2, 0.3)).sample(50, torch.Generator().manual_seed(1)))
    with pytest.raises(ValueError):
        ImageAugmenter(source_hw=(90, 160), final_dim=(24, 40), resize_lim=(0.3, 0.5)).sample(1, train=False)


@pytest.mark.parametrize('angle,flip', [(12.0, True), (-15.0, True), (25.0, True), (-12.0, False)])
def test_bytes_and_matrix_agree_on_where_a_blob_lands(angle, flip):
    from stp3_amd.datas import ImageAugmenter
    aug = ImageAugmenter(source_hw=(180, 270), final_dim=(64, 96))
    p = aug.make_params(0.5, (135, 90), (20, 15, 116, 79), flip, angle)
    u, v = 200, 90                                                   # centre pixel of the blob in the source
    image = torch.zeros(1, 180, 270, 3, dtype=torch.uint8)
    image[0, v - 1:v + 2, u - 1:u + 2] = 255
    out = aug.reference_bytes(image, [p])[0].long().sum(-1)
    assert int(out.max()) > 100
    y, x = divmod(int(out.argmax()), 96)
    mapped = aug.intrinsics(torch.eye(3), [p])[0] @ torch.tensor([u + 0.5, v + 0.5, 1.0])      # pixel centres
    unrotated = aug.intrinsics(torch.eye(3), [dict(p, rotate=0.0)])[0] @ torch.tensor([u + 0.5, v + 0.5, 1.0])
    assert abs(float(unrotated[0]) - 48.0) >= 30.0 and abs(angle) >= 10.0               # the premise of the 2 px bound
    assert abs(x + 0.5 - float(mapped[0])) <= 2.0 and abs(y + 0.5 - float(mapped[1])) <= 2.0, (x, y, mapped)


def test_wrapper_raises():
    aug, params = AC.augmenter('s90'), AC.CASES['s90']['params']
    ok = built('s90')
    with pytest.raises(ValueError):
        aug(ok, params[:5] + [dict(params[5], crop=(0, 0, 41, 24))])                     # mixed crop sizes
    with pytest.raises(ValueError):
        aug(ok, [dict(p, crop=(0, 0, 8193, 24)) for p in params])                        # Pillow's rotation would overflow
    with pytest.raises(ValueError):
        aug(ok, [dict(p, crop=(0, 0, 40, 8193)) for p in params])
    with pytest.raises(ValueError):
        aug(ok.float(), params)                                                          # not uint8
    with pytest.raises(ValueError):
        aug(ok, params, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        aug(ok[:5], params)                                                              # five images, six parameter sets
    with pytest.raises(ValueError):
        aug(ok[:, :80], params)                                                          # another source size
    with pytest.raises(ValueError):
        aug(ok[..., :2], params)


def test_c_entry_validates_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                       # never dereferenced: every call below is refused first
    base = dict(N=6, H=900, W=1600, Wo=480, Ho=224, cols=360, ksize=11, strip_rows=40, rotate=1, coef_len=1000, out_dtype=0)

    def call(images=fake, table=fake, coef=fake, workspace=fake, nbytes=6 * 224 * 480 * 3, out=fake, **k):
        d = _lib.AugmentDims(**{**base, **k})
        return lib.stp3_image_augment(ctypes.byref(d), images, table, coef, workspace, nbytes, out, None)

    for bad in (dict(N=0), dict(H=0), dict(W=-1), dict(Wo=0), dict(Ho=0), dict(ksize=0), dict(strip_rows=0), dict(coef_len=0),
                dict(rotate=2), dict(cols=0), dict(cols=481), dict(Wo=8193), dict(Ho=8193), dict(images=None), dict(table=None), dict(coef=None),
                dict(out=None), dict(workspace=None), dict(nbytes=6 * 224 * 480 * 3 - 1)):
        assert call(**bad) == -10001, bad
    for unsupported in (dict(out_dtype=2), dict(N=70000, nbytes=1 << 40), dict(strip_rows=400)):       # (LDS: 400 strip rows)
        assert call(**unsupported) == -10002, unsupported
    assert lib.stp3_image_augment(None, fake, fake, fake, fake, 0, fake, None) == -10001
    need = ctypes.c_size_t(1)
    d = _lib.AugmentDims(**base)
    assert lib.stp3_image_augment_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == 0 and need.value == 6 * 224 * 480 * 3
    d.rotate = 0
    assert lib.stp3_image_augment_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == 0 and need.value == 0
    d.Wo = 8193
    assert lib.stp3_image_augment_workspace_bytes(ctypes.byref(d), ctypes.byref(need)) == -10001
    assert lib.stp3_image_augment_workspace_bytes(None, ctypes.byref(need)) == -10001


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_augment')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_image.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_augment.py'), lib, path], env=env, capture_output=True,
                         text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return request.param or 'plain', dict(np.load(path))


def test_kernels_on_host_match_the_twin(host_kernel):
    from stp3_amd.datas import ImagePreprocessor
    order, out = host_kernel
    for name in AC.SMALL:
        params, y = AC.CASES[name]['params'], twin(name)
        same(as_bytes(torch.from_numpy(out[f'{name}/out'])), f'{name}/bytes', f'kernels on the host ({order} order)')
        assert np.array_equal(out[f'{name}/out'], y.numpy()), (order, name)
        assert np.array_equal(out[f'{name}/bf16'], y.to(torch.bfloat16).view(torch.int16).numpy()), (order, name)
        assert np.array_equal(out[f'{name}/replay'], twin(name, True).numpy()), (order, name)
        plain = AC.augmenter(name).reference(built(name), [dict(p, flip=False, rotate=0.0) for p in params])
        assert np.array_equal(out[f'{name}/plain'], plain.numpy()), (order, name)
        # the shared band body behind the old entry: its result, and the same floats as the new entry without flip / rotation
        prep = ImagePreprocessor(resize_dims=params[0]['resize_dims'], crop=params[0]['crop'], source_hw=AC.CASES[name]['shape'][1:3])
        assert np.array_equal(out[f'{name}/prep'], prep.reference(built(name)).numpy()), (order, name)
        assert np.array_equal(out[f'{name}/prep'][0], out[f'{name}/plain'][0]), (order, name)
        # a table entry that points outside the coefficient buffer: that image is skipped, the others are untouched by it
        bad = out[f'{name}/bad']
        assert (bad[2] == 77.0).all() and np.array_equal(np.delete(bad, 2, 0), np.delete(y.numpy(), 2, 0)), (order, name)
