"""Input side of the path: what the reference's loader does to every camera image between
the decoder and the network (``stp3/datas/NuscenesData.py:150-172, 236-253``; ``stp3/utils/geometry.py:9-37``) --

    PIL resize (BILINEAR) to ``resize_dims`` -> crop -> ToTensor (/ 255) -> Normalize(ImageNet mean / std)
    and the matching update of the camera intrinsics

-- for all images of a batch in ONE launch of ``stp3_image_prep`` (csrc/stp3_image.hip), byte-exact with Pillow's
resampler.  The nuScenes devkit queries around it (sample records, CAN bus, map API, annotation boxes) are third-party
data access and stay what they are.

CPU tensors take ``resize_bilinear_pil`` / ``ImagePreprocessor.reference`` below -- the same integer arithmetic written
with torch operators -- which is what the host-side tests pin against Pillow itself.

``ImageAugmenter`` is the same path with a different resize, crop, horizontal flip and in-plane rotation per image -- the
Lift-Splat augmentation the reference carries as ``img_transform`` (``stp3/utils/tools.py:115-146``) -- behind
``stp3_image_augment``, with the matching post-homography for the intrinsics.

``JpegDecoder`` (at the end of the file) moves the boundary into the JPEG decoder: the Huffman bit stream of a baseline file is
decoded on host threads, the rest of the decode is one kernel (``stp3_jpeg_reconstruct``) whose output, byte for byte Pillow's,
is what the two classes above read.

``PngDecoder`` (after it) is the same split for the PNG files of the CARLA loader: chunks and DEFLATE on host threads with the
standard library's ``zlib``, the scanline filters in one kernel (``stp3_png_unfilter``), byte for byte Pillow's decode;
``carla.load_carla_sample`` runs a sample from its files' bytes with it.
"""
import collections
import concurrent.futures
import ctypes
import io
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib, ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)              # NuscenesData.py:68-72
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 32 - 8 - 2                         # Pillow, src/libImaging/Resample.c


def get_resizing_and_cropping_parameters(cfg):
    """``NuscenesData.get_resizing_and_cropping_parameters`` (:150-172): resize by IMAGE.RESIZE_SCALE, crop TOP_CROP rows
    and centre the FINAL_DIM window horizontally."""
    oh, ow = cfg.IMAGE.ORIGINAL_HEIGHT, cfg.IMAGE.ORIGINAL_WIDTH
    fh, fw = cfg.IMAGE.FINAL_DIM
    scale = cfg.IMAGE.RESIZE_SCALE
    resize_dims = (int(ow * scale), int(oh * scale))
    crop_h = cfg.IMAGE.TOP_CROP
    crop_w = int(max(0, (resize_dims[0] - fw) / 2))
    return {'scale_width': scale, 'scale_height': scale, 'resize_dims': resize_dims,
            'crop': (crop_w, crop_h, crop_w + fw, crop_h + fh)}


def update_intrinsics(intrinsics, top_crop=0.0, left_crop=0.0, scale_width=1.0, scale_height=1.0):
    """Focal lengths and principal point after resize + crop (stp3/utils/geometry.py:16-37); (..., 3, 3)."""
    k = intrinsics.clone()
    k[..., 0, 0] *= scale_width
    k[..., 0, 2] *= scale_width
    k[..., 1, 1] *= scale_height
    k[..., 1, 2] *= scale_height
    k[..., 0, 2] -= left_crop
    k[..., 1, 2] -= top_crop
    return k


def pil_bilinear_coefficients(in_size, out_size):
    """Pillow's resampling coefficients for one axis (Resample.c ``precompute_coeffs`` with the bilinear (triangle)
    filter over the whole axis, then ``normalize_coeffs_8bpc``): (kk (out_size, ksize) int32 in 22-bit fixed point,
    bounds (out_size, 2) int32 = first source index and count).  Python floats are C doubles: the same numbers."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(v * one - 0.5) if v < 0 else int(v * one + 0.5)
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _resample_axis(img, kk, bounds, axis):
    """One Pillow pass along ``axis`` of an integer tensor of bytes: sum of taps in fixed point, + 2^21, >> 22, clip."""
    src = img.movedim(axis, 0).to(torch.int64)
    kk_t, b_t = torch.from_numpy(kk).to(img.device).long(), torch.from_numpy(bounds).to(img.device).long()
    taps = torch.arange(kk.shape[1], device=img.device)
    idx = (b_t[:, :1] + taps).clamp(max=src.shape[0] - 1)                  # (out, ksize); weights beyond the count are 0
    w = torch.where(taps[None] < b_t[:, 1:], kk_t, torch.zeros_like(kk_t))
    g = src[idx]                                                            # (out, ksize, ...)
    acc = (g * w.view(*w.shape, *([1] * (src.dim() - 1)))).sum(dim=1) + (1 << (PRECISION_BITS - 1))
    return (acc >> PRECISION_BITS).clamp(0, 255).to(torch.uint8).movedim(0, axis)


def resize_bilinear_pil(images, resize_dims):
    """``PIL.Image.resize(resize_dims, BILINEAR)`` of (..., H, W, 3) uint8 images, bit for bit (horizontal pass, bytes,
    vertical pass -- Pillow's order), with torch operators."""
    wr, hr = resize_dims
    h, w = images.shape[-3], images.shape[-2]
    kh, bh = pil_bilinear_coefficients(w, wr)
    kv, bv = pil_bilinear_coefficients(h, hr)
    return _resample_axis(_resample_axis(images, kh, bh, images.dim() - 2), kv, bv, images.dim() - 3)


class ImagePreprocessor:
    """``resize_and_crop_image`` + ``normalise_image`` of the reference's loader for whole batches.

        prep = ImagePreprocessor(cfg)
        x = prep(images_uint8)            # (..., H, W, 3) uint8 on the GPU -> (..., 3, FINAL_H, FINAL_W) float32 | bf16
        k = prep.intrinsics(k_raw)        # (..., 3, 3)
    """

    def __init__(self, cfg=None, resize_dims=None, crop=None, source_hw=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if cfg is not None:
            p = get_resizing_and_cropping_parameters(cfg)
            resize_dims, crop = p['resize_dims'], p['crop']
            source_hw = (cfg.IMAGE.ORIGINAL_HEIGHT, cfg.IMAGE.ORIGINAL_WIDTH)
            self.scale = (p['scale_width'], p['scale_height'])
        else:
            self.scale = (resize_dims[0] / source_hw[1], resize_dims[1] / source_hw[0])
        self.resize_dims, self.crop, self.source_hw = tuple(resize_dims), tuple(crop), tuple(source_hw)
        self.mean, self.std = tuple(mean), tuple(std)
        self.kk_h, self.bounds_h = pil_bilinear_coefficients(source_hw[1], resize_dims[0])
        self.kk_v, self.bounds_v = pil_bilinear_coefficients(source_hw[0], resize_dims[1])
        self._tables = {}

    def intrinsics(self, intrinsics):
        return update_intrinsics(intrinsics, self.crop[1], self.crop[0], self.scale[0], self.scale[1])

    def reference(self, images):
        """The torch statements of the same chain (CPU tensors; what the tests compare with Pillow)."""
        left, top, right, bottom = self.crop
        wr, hr = self.resize_dims
        small = resize_bilinear_pil(images, self.resize_dims)
        window = torch.zeros(*images.shape[:-3], bottom - top, right - left, 3, dtype=torch.uint8, device=images.device)
        y0, y1, x0, x1 = max(top, 0), min(bottom, hr), max(left, 0), min(right, wr)      # PIL pads a crop with zeros
        window[..., y0 - top:y1 - top, x0 - left:x1 - left, :] = small[..., y0:y1, x0:x1, :]
        x = window.movedim(-1, -3).to(torch.float32).div(255)                               # ToTensor
        mean = torch.tensor(self.mean, dtype=torch.float32, device=x.device).view(3, 1, 1)
        std = torch.tensor(self.std, dtype=torch.float32, device=x.device).view(3, 1, 1)
        return (x - mean) / std                                                              # Normalize

    def _strip_rows(self, rows_per_wg):
        left, top, right, bottom = self.crop
        hr = self.resize_dims[1]
        worst = 1
        for r0 in range(0, bottom - top, rows_per_wg):
            rows = [y for y in range(top + r0, min(top + r0 + rows_per_wg, bottom)) if 0 <= y < hr]
            if rows:
                lo = min(int(self.bounds_v[y, 0]) for y in rows)
                hi = max(int(self.bounds_v[y, 0] + self.bounds_v[y, 1]) for y in rows)
                worst = max(worst, hi - lo)
        return worst

    def __call__(self, images, out_dtype=torch.float32):
        if not images.is_cuda:
            return self.reference(images).to(out_dtype)
        assert images.dtype == torch.uint8 and images.shape[-1] == 3 and tuple(images.shape[-3:-1]) == self.source_hw
        lead = images.shape[:-3]
        flat = images.reshape(-1, *images.shape[-3:]).contiguous()
        dev = flat.device
        lib = _lib.lib()
        key = str(dev)
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(a).to(dev).contiguous()
                                      for a in (self.kk_h, self.bounds_h, self.kk_v, self.bounds_v)) + (
                                          self._strip_rows(lib.stp3_image_prep_rows_per_workgroup()),)
        kk_h, b_h, kk_v, b_v, strip = self._tables[key]
        left, top, right, bottom = self.crop
        d = _lib.ImageDims()
        d.N, d.H, d.W = flat.shape[0], self.source_hw[0], self.source_hw[1]
        d.Wr, d.Hr = self.resize_dims
        d.left, d.top, d.Wo, d.Ho = left, top, right - left, bottom - top
        d.ksize_h, d.ksize_v = self.kk_h.shape[1], self.kk_v.shape[1]
        d.out_dtype = _lib.DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.DTYPE_F32
        for c in range(3):
            d.mean[c], d.std[c] = self.mean[c], self.std[c]
        out = torch.empty(flat.shape[0], 3, d.Ho, d.Wo, dtype=out_dtype, device=dev)
        _lib.check(lib.stp3_image_prep(ctypes.byref(d), ops._ptr(flat), ops._ptr(kk_h), ops._ptr(b_h), ops._ptr(kk_v),
                                       ops._ptr(b_v), strip, ops._ptr(out), ops._stream()), 'stp3_image_prep')
        return out.view(*lead, 3, d.Ho, d.Wo)


# ----------------------------------------------------------------------------------------------------------------------
# Per-image augmentation: the Lift-Splat step the reference carries as img_transform (stp3/utils/tools.py:115-146).
# ----------------------------------------------------------------------------------------------------------------------
MAX_ROTATE_SIDE = 8192                              # Pillow accumulates the rotation's addresses in 32-bit integers


def pil_rotate_fixed(angle, size):
    """The six 16.16 fixed-point integers ``PIL.Image.rotate(angle)`` (NEAREST, no expand, centre = size / 2) hands to its
    inner loop, computed in float64 as Pillow does (Image.rotate: the matrix rounded to 15 decimals and recentred;
    Geometry.c ``affine_fixed``: FIX(v) = floor(v * 65536 + 0.5), the half-pixel offset folded into a2 and a5).  ``size`` =
    (width, height).  Source address of output pixel (x, y): ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16)."""
    wo, ho = size
    r = -math.radians(angle % 360.0)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = wo / 2.0, ho / 2.0
    m[2] = (m[0] * -cx + m[1] * -cy + m[2]) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + m[5]) + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))                                     # noqa: E731
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


ROTATE_IDENTITY = (65536, 0, 32768, 0, 65536, 32768)    # = pil_rotate_fixed(0, any size)


def rotate_nearest_pil(window, fixed):
    """``PIL.Image.rotate`` of a (Ho, Wo, C) byte window from its six integers: nearest gather, zero fill."""
    ho, wo = window.shape[0], window.shape[1]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in fixed)
    y = torch.arange(ho, dtype=torch.int64, device=window.device).view(ho, 1)
    x = torch.arange(wo, dtype=torch.int64, device=window.device).view(1, wo)
    xin, yin = (a2 + x * a0 + y * a1) >> 16, (a5 + x * a3 + y * a4) >> 16
    inside = (xin >= 0) & (xin < wo) & (yin >= 0) & (yin < ho)
    picked = window[yin.clamp(0, ho - 1), xin.clamp(0, wo - 1)]
    return torch.where(inside.unsqueeze(-1), picked, torch.zeros_like(picked))


def get_rot(h):
    """tools.py:115-119: numpy float64 cos / sin into a float32 tensor."""
    return torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])


class AugmentPlan:
    """The device-side description of one ``ImageAugmenter`` call: parameter table, coefficient tables, scratch.  The
    tensors are static: ``ImageAugmenter.plan(params, like=plan)`` rewrites them in place (a captured graph then replays
    with the new parameters)."""

    def __init__(self, n, size, cols, ksize, strip_rows, rotate, table, coef, workspace):
        self.n, self.size, self.cols, self.ksize, self.strip_rows, self.rotate = n, size, cols, ksize, strip_rows, rotate
        self.table, self.coef, self.workspace = table, coef, workspace


class ImageAugmenter:
    """``img_transform`` of the reference (stp3/utils/tools.py:122-146; the Lift-Splat augmentation) for whole batches,
    with a different resize, crop, horizontal flip and in-plane rotation PER IMAGE, plus ``normalise_image``:

        Image.resize(resize_dims_i, BILINEAR) -> .crop(crop_i) -> [.transpose(FLIP_LEFT_RIGHT)] -> .rotate(rotate_i)
        -> ToTensor (/ 255) -> Normalize(mean, std)

    byte for byte.  The resize filter is the loader's (``resize_and_crop_image``, geometry.py:9-13: BILINEAR);
    ``img_transform`` itself names none and would take Pillow's default.

        aug = ImageAugmenter(cfg, resize_lim=(0.193, 0.225), bot_pct_lim=(0.0, 0.22), rot_lim=(-5.4, 5.4), rand_flip=True)
        params = aug.sample(n, generator)       # host: one dict per image (resize, resize_dims, crop, flip, rotate)
        x = aug(images_uint8, params)           # (..., H, W, 3) uint8 -> (..., 3, Ho, Wo) float32 | bf16
        k = aug.intrinsics(k_raw, params)       # K' = P K with P = [[post_rot, post_tran], [0, 0, 1]]

    GPU tensors run stp3_image_augment (csrc/stp3_image.hip), CPU tensors ``reference`` -- the same integer arithmetic
    with torch operators.  ``sample(train=False)`` gives the loader's fixed parameters: the call then equals
    ``ImagePreprocessor(cfg)``.

    The depth labels of LIFT.GT_DEPTH follow the same draw: ``DepthLabeller.from_lidar(..., params=params)`` and
    ``from_maps(maps, params=params)`` resample, crop, flip and rotate the depth map of every image with its parameter
    set, so one list drives images, intrinsics and depth labels of a sample."""

    def __init__(self, cfg=None, source_hw=None, final_dim=None, resize_lim=None, bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0),
                 rand_flip=False, eval_params=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if cfg is not None:
            p = get_resizing_and_cropping_parameters(cfg)
            source_hw = (cfg.IMAGE.ORIGINAL_HEIGHT, cfg.IMAGE.ORIGINAL_WIDTH)
            final_dim = tuple(cfg.IMAGE.FINAL_DIM)
            eval_params = {'resize': p['scale_width'], 'resize_dims': p['resize_dims'], 'crop': p['crop']}
            if resize_lim is None:
                resize_lim = (p['scale_width'], p['scale_width'])
        if source_hw is None or final_dim is None:
            raise ValueError('ImageAugmenter: a configuration, or source_hw and final_dim')
        self.source_hw, self.final_dim = (int(source_hw[0]), int(source_hw[1])), (int(final_dim[0]), int(final_dim[1]))
        self.resize_lim = None if resize_lim is None else tuple(float(v) for v in resize_lim)
        self.bot_pct_lim, self.rot_lim = tuple(float(v) for v in bot_pct_lim), tuple(float(v) for v in rot_lim)
        self.rand_flip, self.eval_params = bool(rand_flip), eval_params
        self.mean, self.std = tuple(mean), tuple(std)
        self._axes, self._spans = {}, {}

    # ---- parameters ----------------------------------------------------------------------------------------------------
    @staticmethod
    def make_params(resize, resize_dims, crop, flip=False, rotate=0.0):
        return {'resize': float(resize), 'resize_dims': (int(resize_dims[0]), int(resize_dims[1])),
                'crop': tuple(int(c) for c in crop), 'flip': bool(flip), 'rotate': float(rotate)}

    def sample(self, n, generator=None, train=True):
        """The parameters of ``n`` images, drawn on the host by the Lift-Splat rule (the reference has no such function):
        resize ~ U(resize_lim), resize_dims = (int(W resize), int(H resize)); crop_h = int((1 - U(bot_pct_lim)) newH) - Ho,
        crop_w = int(U(0, 1) max(0, newW - Wo)); flip a fair coin if ``rand_flip``; rotate ~ U(rot_lim) degrees.  Five float64
        draws per image from ``generator``.  ``train=False``: the loader's fixed resize and crop, no flip, no rotation."""
        if not train:
            if self.eval_params is None:
                raise ValueError('ImageAugmenter.sample(train=False): built without a configuration or eval_params')
            e = self.eval_params
            return [self.make_params(e['resize'], e['resize_dims'], e['crop']) for _ in range(n)]
        if self.resize_lim is None:
            raise ValueError('ImageAugmenter.sample: resize_lim is not set')
        (h, w), (ho, wo) = self.source_hw, self.final_dim
        u = torch.rand(n, 5, dtype=torch.float64, generator=generator).tolist()
        between = lambda lim, t: lim[0] + (lim[1] - lim[0]) * t                             # noqa: E731
        out = []
        for u_resize, u_bot, u_left, u_flip, u_rot in u:
            resize = between(self.resize_lim, u_resize)
            new_w, new_h = int(w * resize), int(h * resize)
            crop_h = int((1.0 - between(self.bot_pct_lim, u_bot)) * new_h) - ho
            crop_w = int(u_left * max(0, new_w - wo))
            out.append(self.make_params(resize, (new_w, new_h), (crop_w, crop_h, crop_w + wo, crop_h + ho),
                                        self.rand_flip and u_flip >= 0.5, between(self.rot_lim, u_rot)))
        return out

    def _check_params(self, params, n=None):
        if not len(params) or (n is not None and len(params) != n):
            raise ValueError(f'ImageAugmenter: {len(params)} parameter sets for {n} images')
        sizes = {(p['crop'][2] - p['crop'][0], p['crop'][3] - p['crop'][1]) for p in params}
        if len(sizes) != 1:
            raise ValueError(f'ImageAugmenter: the crops of one call have one size, got {sorted(sizes)}')
        wo, ho = next(iter(sizes))
        if wo < 1 or ho < 1 or any(min(p['resize_dims']) < 1 for p in params):
            raise ValueError('ImageAugmenter: an empty crop or resized image')
        if wo > MAX_ROTATE_SIDE or ho > MAX_ROTATE_SIDE:
            raise ValueError(f'ImageAugmenter: a crop of {wo} x {ho} (at most {MAX_ROTATE_SIDE}: Pillow\'s rotation overflows)')
        return wo, ho

    def _check_images(self, images):
        if images.dtype != torch.uint8 or images.dim() < 3 or images.shape[-1] != 3 or \
                tuple(images.shape[-3:-1]) != self.source_hw:
            raise ValueError(f'ImageAugmenter: images (..., {self.source_hw[0]}, {self.source_hw[1]}, 3) uint8')

    # ---- the matching homography ---------------------------------------------------------------------------------------
    def post_homography(self, params):
        """``post_rot`` (n, 2, 2) and ``post_tran`` (n, 2) of ``img_transform`` (tools.py:133-144) started from identity and
        zero, with its float32 torch statements: a pixel (u, v) of the source lands at post_rot (u, v) + post_tran."""
        rots, trans = [], []
        for p in params:
            crop = p['crop']
            post_rot, post_tran = torch.eye(2), torch.zeros(2)
            post_rot *= p['resize']
            post_tran -= torch.Tensor(crop[:2])
            if p['flip']:
                a = torch.Tensor([[-1, 0], [0, 1]])
                b = torch.Tensor([crop[2] - crop[0], 0])
                post_rot = a.matmul(post_rot)
                post_tran = a.matmul(post_tran) + b
            a = get_rot(p['rotate'] / 180 * np.pi)
            b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
            b = a.matmul(-b) + b
            rots.append(a.matmul(post_rot))
            trans.append(a.matmul(post_tran) + b)
        return torch.stack(rots), torch.stack(trans)

    def intrinsics(self, intrinsics, params):
        """K' = [[post_rot, post_tran], [0, 0, 1]] K for (n, 3, 3) intrinsics (any leading shape with n matrices, or one
        (3, 3) matrix for all).  Products and sums are separate float32 roundings in the order k = 0, 1, 2: without flip and
        rotation the result equals ``update_intrinsics`` for the same scale and crop."""
        rot, tran = self.post_homography(params)
        n = len(params)
        p = torch.zeros(n, 3, 3)
        p[:, :2, :2], p[:, :2, 2], p[:, 2, 2] = rot, tran, 1.0
        k = intrinsics.to(torch.float32)
        p = p.to(k.device)
        if k.dim() > 2:
            p = p.view(*k.shape[:-2], 3, 3)
        return p[..., :, 0:1] * k[..., 0:1, :] + p[..., :, 1:2] * k[..., 1:2, :] + p[..., :, 2:3] * k[..., 2:3, :]

    # ---- the torch statements ------------------------------------------------------------------------------------------
    def reference_bytes(self, images, params):
        """The augmented byte windows (n, Ho, Wo, 3) of (n, H, W, 3) images: what Pillow's chain produces."""
        wo, ho = self._check_params(params, images.shape[0])
        out = torch.zeros(images.shape[0], ho, wo, 3, dtype=torch.uint8, device=images.device)
        for i, p in enumerate(params):
            wr, hr = p['resize_dims']
            left, top, right, bottom = p['crop']
            small = resize_bilinear_pil(images[i], (wr, hr))
            y0, y1, x0, x1 = max(top, 0), min(bottom, hr), max(left, 0), min(right, wr)      # PIL pads a crop with zeros
            if y0 < y1 and x0 < x1:
                out[i, y0 - top:y1 - top, x0 - left:x1 - left] = small[y0:y1, x0:x1]
            window = out[i].flip(1) if p['flip'] else out[i]
            out[i] = rotate_nearest_pil(window, pil_rotate_fixed(p['rotate'], (wo, ho)))
        return out

    def reference(self, images, params):
        """The torch statements of the whole chain (CPU tensors; what the tests compare with Pillow)."""
        self._check_images(images)
        lead = images.shape[:-3]
        window = self.reference_bytes(images.reshape(-1, *images.shape[-3:]), params)
        x = window.movedim(-1, -3).to(torch.float32).div(255)                               # ToTensor
        mean = torch.tensor(self.mean, dtype=torch.float32, device=x.device).view(3, 1, 1)
        std = torch.tensor(self.std, dtype=torch.float32, device=x.device).view(3, 1, 1)
        return ((x - mean) / std).view(*lead, 3, *window.shape[1:3])                        # Normalize

    # ---- the kernel ------------------------------------------------------------------------------------------------------
    def _axis(self, n_in, n_out):
        if (n_in, n_out) not in self._axes:
            self._axes[(n_in, n_out)] = pil_bilinear_coefficients(n_in, n_out)
        return self._axes[(n_in, n_out)]

    def _span(self, hr, top, ho, rows_per_wg):
        """The most source rows the vertical taps of one workgroup's window rows span (``ImagePreprocessor._strip_rows``)."""
        key = (hr, top, ho, rows_per_wg)
        if key not in self._spans:
            bounds = self._axis(self.source_hw[0], hr)[1].astype(np.int64)
            y = top + np.arange(-(-ho // rows_per_wg) * rows_per_wg)
            ok = (y >= 0) & (y < hr) & (y < top + ho)
            yc = np.clip(y, 0, hr - 1)
            lo = np.where(ok, bounds[yc, 0], np.iinfo(np.int64).max).reshape(-1, rows_per_wg).min(axis=1)
            hi = np.where(ok, bounds[yc, 0] + bounds[yc, 1], 0).reshape(-1, rows_per_wg).max(axis=1)
            self._spans[key] = int(max(1, (hi - lo).max()))
        return self._spans[key]

    def host_tables(self, params, rows_per_wg, ksize=0):
        """(table (n, 16) int32 = stp3_augment_image records, coef int32, ksize, strip_rows, any rotation, cols): the
        coefficient tables deduplicated by (source size, resized size), their rows padded with zeros to the largest tap count;
        ``cols``: the most window columns of one image that lie inside its resized image (what the LDS strip holds)."""
        wo, ho = self._check_params(params)
        h, w = self.source_hw
        axes = sorted({(w, p['resize_dims'][0]) for p in params} | {(h, p['resize_dims'][1]) for p in params})
        ksize = max([ksize] + [self._axis(*a)[0].shape[1] for a in axes])
        parts, where, at = [], {}, 0
        for a in axes:
            kk, bounds = self._axis(*a)
            padded = np.zeros((kk.shape[0], ksize), dtype=np.int32)
            padded[:, :kk.shape[1]] = kk
            where[a] = (at, at + padded.size)
            parts += [padded.reshape(-1), bounds.reshape(-1)]
            at += padded.size + bounds.size
        table = np.zeros((len(params), 16), dtype=np.int32)
        strip_rows, rotate, cols = 1, False, 1
        for i, p in enumerate(params):
            wr, hr = p['resize_dims']
            left = p['crop'][0]
            first, end = (left + wo - wr, left + wo) if p['flip'] else (-left, wr - left)
            cols = max(cols, min(wo, end) - max(0, first))
            fixed = pil_rotate_fixed(p['rotate'], (wo, ho))
            rotate = rotate or fixed != ROTATE_IDENTITY
            table[i] = (wr, hr, p['crop'][0], p['crop'][1], int(p['flip'])) + fixed + where[(w, wr)] + where[(h, hr)] + (0,)
            strip_rows = max(strip_rows, self._span(hr, p['crop'][1], ho, rows_per_wg))
        return table, np.concatenate(parts).astype(np.int32), ksize, strip_rows, rotate, cols

    def plan(self, params, device, like=None, ksize=0, strip_rows=0, coef_len=0, rotate=None, cols=0):
        """The ``AugmentPlan`` of ``params`` on ``device``.  ``ksize`` / ``strip_rows`` / ``coef_len`` / ``rotate`` / ``cols`` reserve
        room for later parameters; ``like``: rewrite that plan's tensors in place instead (it must have the room)."""
        lib = _lib.lib()
        rows_per_wg = lib.stp3_image_prep_rows_per_workgroup()
        if like is not None:
            ksize = like.ksize
        table, coef, ksize, span, rot, inside = self.host_tables(params, rows_per_wg, ksize)
        wo, ho = self._check_params(params)
        if like is not None:
            if (len(params), (wo, ho)) != (like.n, like.size) or ksize > like.ksize or span > like.strip_rows or \
                    coef.size > like.coef.numel() or (rot and not like.rotate) or inside > like.cols:
                raise ValueError('ImageAugmenter.plan: the parameters do not fit the plan they are to replace')
            like.table.copy_(torch.from_numpy(table))
            like.coef[:coef.size].copy_(torch.from_numpy(coef))
            return like
        rot = rot if rotate is None else (rot or bool(rotate))
        buf = np.zeros(max(coef.size, coef_len), dtype=np.int32)
        buf[:coef.size] = coef
        workspace = torch.empty(len(params) * ho * wo * 3 if rot else 0, dtype=torch.uint8, device=device)
        return AugmentPlan(len(params), (wo, ho), min(wo, max(inside, cols)), ksize, max(span, strip_rows), int(rot),
                           torch.from_numpy(table).to(device),
                           torch.from_numpy(buf).to(device), workspace)

    def run(self, images, plan, out_dtype=torch.float32, out=None):
        """One call of stp3_image_augment with a prepared plan: enqueues only (capturable)."""
        self._check_images(images)
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('ImageAugmenter: out_dtype torch.float32 or torch.bfloat16')
        lead = images.shape[:-3]
        flat = images.reshape(-1, *images.shape[-3:]).contiguous()
        wo, ho = plan.size
        if flat.shape[0] != plan.n:
            raise ValueError(f'ImageAugmenter: {flat.shape[0]} images for a plan of {plan.n}')
        d = _lib.AugmentDims()
        d.N, d.H, d.W, d.Wo, d.Ho, d.cols = plan.n, self.source_hw[0], self.source_hw[1], wo, ho, plan.cols
        d.ksize, d.strip_rows, d.rotate, d.coef_len = plan.ksize, plan.strip_rows, plan.rotate, plan.coef.numel()
        d.out_dtype = _lib.DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.DTYPE_F32
        for c in range(3):
            d.mean[c], d.std[c] = self.mean[c], self.std[c]
        if out is None:
            out = torch.empty(plan.n, 3, ho, wo, dtype=out_dtype, device=flat.device)
        elif out.dtype != out_dtype or out.numel() != plan.n * 3 * ho * wo or not out.is_contiguous():
            raise ValueError('ImageAugmenter: out does not match the plan')
        _lib.check(_lib.lib().stp3_image_augment(ctypes.byref(d), ops._ptr(flat), ops._ptr(plan.table), ops._ptr(plan.coef),
                                                 ops._ptr(plan.workspace) if plan.rotate else None, plan.workspace.numel(),
                                                 ops._ptr(out), ops._stream()), 'stp3_image_augment')
        return out.view(*lead, 3, ho, wo)

    def __call__(self, images, params, out_dtype=torch.float32):
        self._check_images(images)
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('ImageAugmenter: out_dtype torch.float32 or torch.bfloat16')
        n = images.numel() // (self.source_hw[0] * self.source_hw[1] * 3)
        self._check_params(params, n)
        if not images.is_cuda:
            return self.reference(images, params).to(out_dtype)
        return self.run(images, self.plan(params, images.device), out_dtype)


# ----------------------------------------------------------------------------------------------------------------------
# BEV labels: what NuscenesData.get_birds_eye_view_label / get_label / __getitem__ do AFTER
# the nuScenes devkit has answered (annotation boxes, ego poses): box polygons -> label maps, instance ids -> centerness /
# offset / displacement labels, frames -> one sample dictionary.
# ----------------------------------------------------------------------------------------------------------------------
MAX_POLY_VERTICES = 8


def box_polygons(bottom_corners_xy, bev_start_position, bev_resolution):
    """``_get_poly_region_in_image`` (NuscenesData.py:340-353) after the devkit's ``Box``: the (n, 4, 2) ego-frame bottom
    corners of the annotation boxes -> integer polygon vertices as cv2.fillPoly takes them, (n, 4, 2) int32 with
    [..., 0] the BEV column and [..., 1] the BEV row (the reference rounds to cells, then swaps the two coordinates)."""
    pts = np.asarray(bottom_corners_xy, dtype=np.float64)
    start = np.asarray(bev_start_position, dtype=np.float64)[:2]
    res = np.asarray(bev_resolution, dtype=np.float64)[:2]
    cells = np.round((pts - start + res / 2.0) / res).astype(np.int32)
    return cells[..., [1, 0]]


def fill_polygons_reference(polys, values, map_index, n_maps, hw):
    """cv2.fillPoly, restated (edge walking; the statement CPU tensors take and the tests compare the kernel with):
    see csrc/stp3_labels.hip for the algorithm and its provenance.  polys: sequence of (nv, 2) integer (column, row)
    vertex arrays in paint order -> (n_maps, H, W) float32."""
    h, w = hw
    maps = np.zeros((n_maps, h, w), dtype=np.float32)
    for poly, value, mi in zip(polys, values, map_index):
        poly = np.asarray(poly, dtype=np.int64)
        img = maps[mi]
        nv = len(poly)
        edges = []
        for v in range(nv):
            (ax, ay), (bx, by) = poly[v - 1], poly[v]
            _bresenham(img, int(ax), int(ay), int(bx), int(by), value)
            if ay == by:
                continue
            y0, y1, x0 = (ay, by, ax) if ay < by else (by, ay, bx)
            num = int(bx - ax) << 16
            den = int(by - ay)
            slope = abs(num) // abs(den) * (1 if (num < 0) == (den < 0) else -1)        # C integer division: toward zero
            edges.append((int(y0), int(y1), int(x0) << 16, slope))
        if not edges:
            continue
        for y in range(max(min(e[0] for e in edges), 0), min(max(e[1] for e in edges), h)):
            xs = sorted(x0 + slope * (y - y0) for y0, y1, x0, slope in edges if y0 <= y < y1)
            for left, right in zip(xs[0::2], xs[1::2]):
                x1, x2 = (left + 65535) >> 16, right >> 16
                if x1 < w and x2 >= 0:
                    img[y, max(x1, 0):min(x2, w - 1) + 1] = value
    return torch.from_numpy(maps)


def _bresenham(img, x0, y0, x1, y1, value):
    """OpenCV's LineIterator, 8-connected, walked left to right (drawing.cpp ``Line``), clipped to the image."""
    h, w = img.shape
    if x0 > x1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    sy = -1 if dy < 0 else 1
    ady = abs(dy)
    steep = ady > dx
    big, small = (ady, dx) if steep else (dx, ady)
    err = big - 2 * small
    x, y = x0, y0
    for _ in range(big + 1):
        if 0 <= x < w and 0 <= y < h:
            img[y, x] = value
        diag = err < 0
        err += -2 * small + (2 * big if diag else 0)
        if steep:
            y += sy
            x += 1 if diag else 0
        else:
            x += 1
            y += sy if diag else 0


def fill_polygons(polys, values, map_index, n_maps, hw, device=None):
    """cv2.fillPoly of integer polygons into ``n_maps`` zero-initialised (H, W) float32 maps, in order (a later polygon
    overwrites an earlier one); ``polys``: sequence of (nv <= 8, 2) integer (column, row) arrays, ``values`` / ``map_index``
    per polygon.  On a GPU ``device``: one launch of stp3_fill_polygons; otherwise the restatement above."""
    device = torch.device(device) if device is not None else torch.device('cpu')
    if not torch.empty(0, device=device).is_cuda:
        return fill_polygons_reference(polys, values, map_index, n_maps, hw)
    h, w = hw
    arr = (_lib.Poly * max(len(polys), 1))()
    for rec, poly, value, mi in zip(arr, polys, values, map_index):
        poly = np.asarray(poly, dtype=np.int64)
        if not 1 <= len(poly) <= MAX_POLY_VERTICES:
            raise _lib.Stp3HipError(f'fill_polygons: {len(poly)} vertices (1 .. {MAX_POLY_VERTICES} supported)')
        rec.map, rec.nv, rec.value = int(mi), len(poly), float(value)
        for k, (px, py) in enumerate(poly):
            rec.xy[2 * k], rec.xy[2 * k + 1] = int(px), int(py)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    maps = torch.zeros(n_maps, h, w, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().stp3_fill_polygons(ops._ptr(table), len(polys), n_maps, h, w, ops._ptr(maps), ops._stream()),
               'stp3_fill_polygons')
    return maps


def bev_labels_from_boxes(bottom_corners_xy, categories, instance_ids, bev_start_position, bev_resolution, bev_dimension,
                          device=None):
    """``get_birds_eye_view_label`` (NuscenesData.py:303-338) for one frame, after the devkit: boxes (n, 4, 2) ego-frame
    bottom corners in annotation order, ``categories`` 'vehicle' / 'human' / anything else (skipped), ``instance_ids`` the
    ids the reference's ``instance_map`` assigns -> (segmentation, instance, pedestrian) int64 maps (H, W).  Vehicles paint
    their id into the instance map (later boxes overwrite earlier ones) and 1 into the segmentation, pedestrians 1 into
    the pedestrian map."""
    h, w = int(bev_dimension[0]), int(bev_dimension[1])
    polys = box_polygons(bottom_corners_xy, bev_start_position, bev_resolution) if len(categories) else []
    plist, values, index = [], [], []
    for poly, cat, iid in zip(polys, categories, instance_ids):
        if 'vehicle' in cat:
            plist += [poly, poly]
            values += [float(iid), 1.0]
            index += [1, 0]
        elif 'human' in cat:
            plist.append(poly)
            values.append(1.0)
            index.append(2)
    maps = fill_polygons(plist, values, index, 3, (h, w), device).long()
    return maps[0], maps[1], maps[2]


def instance_labels_reference(instance, future_egomotion, num_instances, ignore_index=255, subtract_egomotion=True,
                              sigma=3, spatial_extent=None):
    """``convert_instance_mask_to_center_and_offset_label`` (stp3/utils/instance.py:12-77) with whole-tensor torch
    operators (CPU tensors; the same arithmetic as the kernel: integer moments, float32 mean, round half to even)."""
    from .geometry import mat2pose_vec, pose_vec2mat, warp_features
    t_, h, w = instance.shape
    dev = instance.device
    center = torch.zeros(t_, 1, h, w, device=dev)
    offset = ignore_index * torch.ones(t_, 2, h, w, device=dev)
    flow = ignore_index * torch.ones(t_, 2, h, w, device=dev)
    if num_instances == 0:
        return center, offset, flow
    warped = _warp_instances(instance, future_egomotion, subtract_egomotion, spatial_extent)
    ids = torch.arange(1, num_instances + 1, device=dev).view(1, -1, 1, 1)
    rows = torch.arange(h, dtype=torch.float32, device=dev).view(1, 1, h, 1)
    cols = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w)

    def moments(maps):                                  # (T, K): count, rounded mean row, rounded mean column
        m = (maps.unsqueeze(1) == ids).float()
        cnt = m.sum(dim=(2, 3))
        safe = cnt.clamp_min(1.0)
        return cnt, torch.round((m * rows).sum(dim=(2, 3)) / safe), torch.round((m * cols).sum(dim=(2, 3)) / safe)
    cnt, xc, yc = moments(instance)
    wcnt, wxc, wyc = moments(warped)
    present = cnt > 0
    ox = xc.view(t_, -1, 1, 1) - rows                   # (T, K, H, W)
    oy = yc.view(t_, -1, 1, 1) - cols
    g = torch.exp(-(ox ** 2 + oy ** 2) / sigma ** 2)
    center[:, 0] = torch.where(present.view(t_, -1, 1, 1), g, torch.zeros(())).amax(dim=1)
    own = (instance.unsqueeze(1) == ids)                # (T, K, H, W): at most one id per pixel
    sel = own.float()
    has = own.any(dim=1)
    offset[:, 0] = torch.where(has, (sel * ox).sum(1), offset[:, 0])
    offset[:, 1] = torch.where(has, (sel * oy).sum(1), offset[:, 1])
    if t_ > 1:
        ok = present[:-1] & present[1:] & (wcnt[1:] > 0)                     # (T-1, K)
        dxy = torch.stack([wxc[1:] - xc[:-1], wyc[1:] - yc[:-1]], dim=1)     # (T-1, 2, K)
        moving = own[:-1] & ok.view(t_ - 1, -1, 1, 1)
        hit = moving.any(dim=1)
        for a in range(2):
            val = (moving.float() * dxy[:, a].view(t_ - 1, -1, 1, 1)).sum(1)
            flow[:-1, a] = torch.where(hit, val, flow[:-1, a])
    return center, offset, flow


def _warp_instances(instance, future_egomotion, subtract_egomotion, spatial_extent):
    """Frame t's instance map warped into frame t - 1 (instance.py:21-31); frame 0 is a copy that nothing reads.  The
    reference applies the warp only when ``subtract_egomotion`` (its inverse-motion tensor does not exist otherwise)."""
    from .geometry import mat2pose_vec, pose_vec2mat, warp_features
    if not subtract_egomotion:
        raise NotImplementedError('subtract_egomotion=False: the reference itself fails (future_egomotion_inv is undefined)')
    inv = mat2pose_vec(torch.inverse(pose_vec2mat(future_egomotion.float())))
    out = instance.float().clone()
    if instance.shape[0] > 1:
        out[1:] = warp_features(instance[1:].unsqueeze(1).float(), inv[:-1].to(instance.device), mode='nearest',
                                spatial_extent=spatial_extent)[:, 0]
    return out


def instance_labels(instance, future_egomotion, num_instances, ignore_index=255, subtract_egomotion=True, sigma=3,
                    spatial_extent=None):
    """``convert_instance_mask_to_center_and_offset_label`` (stp3/utils/instance.py:12-77): instance (T, H, W) int64 ids,
    future_egomotion (T, 6) -> centerness (T, 1, H, W), offset (T, 2, H, W), future displacement (T, 2, H, W), float32.
    GPU tensors: the warp through stp3_warp_nearest, the labels through stp3_instance_labels (integer moments, no
    per-instance Python loop)."""
    if not instance.is_cuda:
        return instance_labels_reference(instance, future_egomotion, num_instances, ignore_index, subtract_egomotion, sigma,
                                         spatial_extent)
    from . import ops_loss
    from .geometry import mat2pose_vec, pose_vec2mat, warp_theta
    t_, h, w = instance.shape
    dev = instance.device
    inst = instance.long().contiguous()
    warped = None
    if t_ > 1:
        if not subtract_egomotion:
            raise NotImplementedError('subtract_egomotion=False: the reference itself fails (future_egomotion_inv is undefined)')
        inv = mat2pose_vec(torch.inverse(pose_vec2mat(future_egomotion.detach().float().cpu())))
        theta = torch.cat([torch.zeros(1, 2, 3), warp_theta(inv[:-1], spatial_extent)], dim=0)
        warped = ops_loss.warp_nearest(inst.float().unsqueeze(1), theta, [1] + [0] * (t_ - 1))[:, 0].contiguous()
    lib = _lib.lib()
    need = ctypes.c_size_t()
    _lib.check(lib.stp3_instance_labels_workspace_bytes(t_, int(num_instances), ctypes.byref(need)),
               'stp3_instance_labels_workspace_bytes')
    ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=dev)
    center = torch.empty(t_, 1, h, w, dtype=torch.float32, device=dev)
    offset = torch.empty(t_, 2, h, w, dtype=torch.float32, device=dev)
    flow = torch.empty(t_, 2, h, w, dtype=torch.float32, device=dev)
    _lib.check(lib.stp3_instance_labels(t_, h, w, int(num_instances), float(ignore_index), float(sigma), ops._ptr(inst),
                                        ops._ptr(warped) if warped is not None else None, ops._ptr(ws), need.value,
                                        ops._ptr(center), ops._ptr(offset), ops._ptr(flow), ops._stream()),
               'stp3_instance_labels')
    return center, offset, flow


WHEEL_BASE = 2.588                                  # metres between the axles (NuscenesData.py:425)


def trajectory_curvature(steering, left_hand_traffic=False):
    """Curvature (1/m, positive: left) from the CAN bus' steering-angle feedback (rad), float64 (B,):
    ``Kappa = 2 * steering / 2.588``, the steering negated where the map drives on the left (singapore-*),
    NuscenesData.py:418-425.  ``left_hand_traffic``: one flag, or one per sample."""
    steering = torch.as_tensor(steering).double().reshape(-1)
    flip = torch.as_tensor(left_hand_traffic, device=steering.device).bool().reshape(-1).expand_as(steering)
    return 2.0 * torch.where(flip, steering * -1.0, steering) / WHEEL_BASE


def trajectory_sampling(speed, steering, n_future, sample_num, left_hand_traffic=False, draws=None, generator=None,
                        possibility=(0.4, 0.2, 0.4)):
    """``NuscenesData.get_trajectory_sampling`` (NuscenesData.py:389-437) after its CAN-bus lookup, for a batch: ``speed``
    (m/s, the pose message's longitudinal velocity) and ``steering`` (rad) tensors (B,) -> the batch's ``sample_trajectory``
    entry, (B, sample_num, n_future + 1, 3) float32 on the inputs' device, ordered by the lateral position of the last
    pose as ``Planning.command_samples`` expects it.  One launch of ``stp3_traj_sample`` for GPU tensors
    (``ops_plan.sample_trajectories``, which documents ``draws`` / ``generator``)."""
    from . import ops_plan
    speed = torch.as_tensor(speed)
    kappa = trajectory_curvature(torch.as_tensor(steering, device=speed.device), left_hand_traffic)
    return ops_plan.sample_trajectories(speed, kappa, n_future, sample_num, draws=draws, generator=generator,
                                        possibility=possibility)


SAMPLE_CAT_KEYS = ('image', 'intrinsics', 'extrinsics', 'depths', 'segmentation', 'instance', 'future_egomotion', 'hdmap',
                   'pedestrian')


def assemble_sample(frames, receptive_field, num_instances, planning=None, gt_depth=False, ignore_index=255,
                    spatial_extent=None):
    """``NuscenesData.__getitem__`` (NuscenesData.py:569-646) after the per-frame queries: ``frames`` = one dictionary per
    time step with the tensors the reference's helpers return for it -- image (1, N, 3, H, W), intrinsics (1, N, 3, 3),
    extrinsics (1, N, 4, 4) [, depths (1, N, H, W)] for the first ``receptive_field`` frames; segmentation / pedestrian
    (1, 1, X, Y), instance (1, X, Y), future_egomotion (1, 6), hdmap (1, C, X, Y) and ``index`` for all -- concatenated
    over time under the reference's keys, plus the instance-derived labels.  ``planning``: the present frame's
    gt_trajectory / command / sample_trajectory (dict), placeholders of the reference's shapes otherwise."""
    data = {k: [] for k in SAMPLE_CAT_KEYS}
    data['indices'] = []
    for i, fr in enumerate(frames):
        if i < receptive_field:
            for k in ('image', 'intrinsics', 'extrinsics'):
                data[k].append(fr[k])
            if gt_depth:
                data['depths'].append(fr['depths'])
        for k in ('segmentation', 'instance', 'pedestrian', 'future_egomotion', 'hdmap'):
            data[k].append(fr[k])
        data['indices'].append(fr.get('index', i))
    for k in SAMPLE_CAT_KEYS:
        if k == 'depths' and not gt_depth:
            continue
        data[k] = torch.cat(data[k], dim=0)
    planning = planning or {}
    data['gt_trajectory'] = planning.get('gt_trajectory', torch.zeros(1, 3))
    data['command'] = planning.get('command', 'FORWARD')
    data['sample_trajectory'] = planning.get('sample_trajectory', torch.zeros(1, 1, 3))
    data['target_point'] = torch.tensor([0., 0.])
    data['centerness'], data['offset'], data['flow'] = instance_labels(
        data['instance'], data['future_egomotion'], num_instances, ignore_index=ignore_index, subtract_egomotion=True,
        spatial_extent=spatial_extent)
    return data


# ----------------------------------------------------------------------------------------------------------------------
# Depth labels (LIFT.GT_DEPTH): batch['depths'] from the LiDAR sweep or from stored maps.
#   (a) projection    NuScenesExplorer.map_pointcloud_to_image of the nuScenes devkit: third-party, restated from its
#                     published source, PARITY UNPINNED (csrc/stp3_depth.hip states the arithmetic this project defines)
#   (b) scatter       NuscenesData.get_depth_from_lidar (NuscenesData.py:291-293): last point of a pixel wins
#   (c) resample      :294-299 and get_input_data :261-266: bilinear, align_corners=False, crop, round half to even
#   (d) class ids     trainer.py:269-276
# ----------------------------------------------------------------------------------------------------------------------
DEVKIT_BEFORE = (False, False, True, True)          # map_pointcloud_to_image: steps 3 and 4 translate, then rotate


def depth_resample_axis(n_src, scale, out_index, dtype=np.float64, step=None):
    """Taps and weights of ``F.interpolate(scale_factor=scale, mode='bilinear', align_corners=False)`` along one axis for
    the output indices ``out_index``, as ATen builds them in the map's dtype (UpSampleKernel.cpp: source =
    max(0, step (o + 0.5) - 0.5), i0 = min(trunc, n - 1), i1 = min(i0 + 1, n - 1), lambda = source - i0 in [0, 1]),
    and the numbering of the source indices that are taps ("slots", ascending).  The source step is 1 / scale (the scale
    factor handed on) unless ``step`` names it: with ``recompute_scale_factor=True`` ATen takes n_src / n_out in ``dtype``.
    Returns a dict of numpy arrays: tap (n_out, 2) int32 slots, weight (n_out, 2) float64 holding the ``dtype`` values,
    slot_src (n_slot,), src_slot (n_src,)."""
    t = np.dtype(dtype).type
    o = np.asarray(out_index, dtype=np.int64).astype(t)
    step = t(1.0 / scale) if step is None else t(step)
    src = np.maximum(step * (o + t(0.5)) - t(0.5), t(0.0))
    i0 = np.minimum(src.astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    lam = np.clip(src - i0.astype(t), t(0.0), t(1.0))
    slot_src = np.unique(np.concatenate([i0, i1]))
    src_slot = np.full(n_src, -1, dtype=np.int32)
    src_slot[slot_src] = np.arange(len(slot_src), dtype=np.int32)
    return {'tap': np.stack([src_slot[i0], src_slot[i1]], axis=1).astype(np.int32),
            'weight': np.stack([t(1.0) - lam, lam], axis=1).astype(np.float64),
            'slot_src': slot_src.astype(np.int32), 'src_slot': src_slot}


class DepthLabeller:
    """``NuscenesData.get_depth_from_lidar`` / the depth branch of ``get_input_data`` and the trainer's class ids, for
    all frames and cameras of a batch.

        lab = DepthLabeller(cfg)      # or source_hw=, scale=, crop=(left, top, right, bottom), downsample=, d_bound=
        pixels, depth, keep = lab.project(points, offsets, steps, before, intrinsics)       # (a)
        depths = lab.from_pixels(pixels, depth, keep, offsets)                              # (b) + (c): (F, N, Ho, Wo)
        depths = lab.from_lidar(points, offsets, steps, before, intrinsics)                 # (a) - (c) fused
        labels = lab.from_lidar(points, offsets, steps, before, intrinsics, labels=True)    # (a) - (d): (F, N, fH, fW) int64
        depths = lab.from_maps(maps)                                                        # (c) of stored (F, N, H, W) maps
        labels = lab.class_ids(depths)                                                      # (d)
        depths = lab.from_lidar(..., params=params)     # under ImageAugmenter's per-image parameters: (F, N, Ho, Wo) of the crop
        depths = lab.from_maps(maps, params=params)     # (csrc/stp3_depth_augment.hip); plan=augment_plan(...)

    points (n, 3) float32: the sweeps of the F frames one after the other, offsets (F + 1,) int32 their boundaries;
    steps (F, N, 4, 12) float64: rotation (row-major) and translation of the four rigid steps; before: per step whether it
    translates before it rotates (``DEVKIT_BEFORE``); intrinsics (F, N, 3, 3) float64.  ``depths`` is float32 by default
    (``out_dtype=torch.float64`` on request; the values are integers): a frame's slice ``depths[f:f + 1]`` is the
    ``depths`` entry ``assemble_sample(gt_depth=True)`` takes.  GPU tensors run csrc/stp3_depth.hip, CPU tensors the
    ``reference_*`` methods -- the same statements with torch operators, which also run on GPU tensors."""

    def __init__(self, cfg=None, source_hw=None, scale=None, crop=None, downsample=None, d_bound=None):
        if cfg is not None:
            p = get_resizing_and_cropping_parameters(cfg)
            source_hw = (cfg.IMAGE.ORIGINAL_HEIGHT, cfg.IMAGE.ORIGINAL_WIDTH)
            scale, crop = cfg.IMAGE.RESIZE_SCALE, p['crop']
            downsample, d_bound = cfg.MODEL.ENCODER.DOWNSAMPLE, tuple(cfg.LIFT.D_BOUND)
        self.source_hw, self.scale, self.crop = (int(source_hw[0]), int(source_hw[1])), float(scale), tuple(int(c) for c in crop)
        self.downsample, self.d_bound = int(downsample), tuple(float(b) for b in d_bound)
        h, w = self.source_hw
        left, top, right, bottom = self.crop
        hr, wr = int(math.floor(h * self.scale)), int(math.floor(w * self.scale))            # F.interpolate's output size
        if min(left, top) < 0 or self.downsample < 1 or h < 3 or w < 3:
            raise ValueError('DepthLabeller: negative crop origin, downsample < 1 or a source below 3 x 3')
        self.rows, self.cols = np.arange(top, min(bottom, hr)), np.arange(left, min(right, wr))   # a slice clips
        if len(self.rows) < 1 or len(self.cols) < 1:
            raise ValueError('DepthLabeller: the crop window lies outside the resized map')
        self.out_hw = (len(self.rows), len(self.cols))
        self.label_hw = (len(self.rows[::self.downsample]), len(self.cols[::self.downsample]))
        self._axes, self._device_axes = {}, {}
        self.label_bands = 0                         # labels-only kernel: at least this many bands of label rows per image

    # ---- configuration-only tables -----------------------------------------------------------------------------------
    def axes(self, labels, dtype=np.float64):
        """(rows' table, columns' table) of ``depth_resample_axis`` for the full map or for the label rows / columns."""
        key = (bool(labels), np.dtype(dtype).name)
        if key not in self._axes:
            step = self.downsample if labels else 1
            self._axes[key] = (depth_resample_axis(self.source_hw[0], self.scale, self.rows[::step], dtype),
                               depth_resample_axis(self.source_hw[1], self.scale, self.cols[::step], dtype))
        return self._axes[key]

    def _tables(self, labels, dtype, device):
        key = (bool(labels), np.dtype(dtype).name, str(device))
        if key not in self._device_axes:
            self._device_axes[key] = tuple({k: torch.from_numpy(v).to(device).contiguous() for k, v in ax.items()}
                                           for ax in self.axes(labels, dtype))
        return self._device_axes[key]

    def class_ids(self, depths):
        """trainer.py:269-276: every ``downsample``-th row and column, clamp(D_BOUND[0], D_BOUND[1] - 1) - D_BOUND[0], int64."""
        ds = self.downsample
        return self._clamp(depths[..., ::ds, ::ds])

    def _clamp(self, depths):
        return (torch.clamp(depths, self.d_bound[0], self.d_bound[1] - 1) - self.d_bound[0]).long().contiguous()

    # ---- validation ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _before_mask(before):
        before = [bool(b) for b in before]
        if len(before) != 4:
            raise ValueError('before: one flag per rigid step (4)')
        return sum(1 << s for s, b in enumerate(before) if b)

    @staticmethod
    def _check_offsets(offsets, n_total, check):
        if offsets.dim() != 1 or offsets.numel() < 2 or offsets.dtype != torch.int32:
            raise ValueError('offsets: (F + 1,) int32')
        if check:
            o = offsets.detach().cpu().long()
            if int(o[0]) < 0 or int(o[-1]) > n_total or bool((o[1:] < o[:-1]).any()):
                raise ValueError('offsets: not ascending inside [0, number of points]')
        return offsets.numel() - 1

    def _check_cloud(self, points, offsets, steps, intrinsics, check):
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError('points: (n, 3) float32')
        f = self._check_offsets(offsets, points.shape[0], check)
        if steps.dim() != 4 or steps.shape[0] != f or tuple(steps.shape[2:]) != (4, 12) or steps.dtype != torch.float64:
            raise ValueError('steps: (F, N, 4, 12) float64')
        n = steps.shape[1]
        if tuple(intrinsics.shape) != (f, n, 3, 3) or intrinsics.dtype != torch.float64:
            raise ValueError('intrinsics: (F, N, 3, 3) float64')
        if len({t.device for t in (points, offsets, steps, intrinsics)}) != 1:
            raise ValueError('points, offsets, steps and intrinsics live on different devices')
        return f, n

    def _check_pixels(self, pixels, depth, keep, offsets, check):
        n_total = pixels.shape[0]
        if pixels.dim() != 3 or pixels.shape[2] != 2 or pixels.dtype != torch.int32:
            raise ValueError('pixels: (n, N, 2) int32')
        n = pixels.shape[1]
        if tuple(depth.shape) != (n_total, n) or depth.dtype != torch.float64:
            raise ValueError('depth: (n, N) float64')
        if tuple(keep.shape) != (n_total, n) or keep.dtype != torch.bool:
            raise ValueError('keep: (n, N) bool')
        if len({t.device for t in (pixels, depth, keep, offsets)}) != 1:
            raise ValueError('pixels, depth, keep and offsets live on different devices')
        return self._check_offsets(offsets, n_total, check), n

    @staticmethod
    def _out_dtype(labels, out_dtype):
        if labels:
            return torch.int64, _lib.DEPTH_OUT_LABELS
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError('out_dtype: torch.float32 or torch.float64')
        return out_dtype, (_lib.DEPTH_OUT_F32 if out_dtype == torch.float32 else _lib.DEPTH_OUT_F64)

    # ---- the torch statements ------------------------------------------------------------------------------------------
    @staticmethod
    def _frames(offsets, n_total):
        """(frame of every point clamped to a valid index, its index inside the frame, whether a frame owns it)."""
        o = offsets.long()
        p = torch.arange(n_total, device=offsets.device)
        frame = torch.bucketize(p, o[1:].contiguous(), right=True)
        owned = (frame < o.numel() - 1) & (p >= o[0])
        frame = frame.clamp(max=o.numel() - 2)
        return frame, p - o[frame], owned

    def reference_project(self, points, offsets, steps, before, intrinsics):
        """(a) in elementwise torch statements (no matmul: its summation order is the BLAS's)."""
        self._check_cloud(points, offsets, steps, intrinsics, not points.is_cuda)
        mask = self._before_mask(before)
        h, w = self.source_hw
        frame, _, owned = self._frames(offsets, points.shape[0])
        st, k = steps[frame], intrinsics[frame]                                              # (n, N, 4, 12), (n, N, 3, 3)
        x, y, z = (points[:, i:i + 1].expand(-1, steps.shape[1]) for i in range(3))
        for s in range(4):
            r = st[:, :, s]
            if (mask >> s) & 1:
                x, y, z = ((x.double() + r[..., 9]).float(), (y.double() + r[..., 10]).float(), (z.double() + r[..., 11]).float())
            dx, dy, dz = x.double(), y.double(), z.double()
            x = (r[..., 0] * dx + r[..., 1] * dy + r[..., 2] * dz).float()
            y = (r[..., 3] * dx + r[..., 4] * dy + r[..., 5] * dz).float()
            z = (r[..., 6] * dx + r[..., 7] * dy + r[..., 8] * dz).float()
            if not (mask >> s) & 1:
                x, y, z = ((x.double() + r[..., 9]).float(), (y.double() + r[..., 10]).float(), (z.double() + r[..., 11]).float())
        dx, dy, dz = x.double(), y.double(), z.double()
        p0 = k[..., 0, 0] * dx + k[..., 0, 1] * dy + k[..., 0, 2] * dz
        p1 = k[..., 1, 0] * dx + k[..., 1, 1] * dy + k[..., 1, 2] * dz
        p2 = k[..., 2, 0] * dx + k[..., 2, 1] * dy + k[..., 2, 2] * dz
        u, v = p0 / p2, p1 / p2
        keep = (z > 1.0) & (u > 1.0) & (u < float(w - 1)) & (v > 1.0) & (v < float(h - 1)) & owned[:, None]
        zero = torch.zeros((), dtype=torch.float64, device=points.device)
        pixels = torch.stack([torch.where(keep, u, zero), torch.where(keep, v, zero)], dim=-1).to(torch.int32)   # toward zero
        return pixels, torch.where(owned[:, None], dz, zero), keep

    @staticmethod
    def _blend(tab, ay, ax, dtype):
        """hy0 (wx0 A + wx1 B) + hy1 (wx0 C + wx1 D) of a (..., n_slot_y, n_slot_x) table, rounded half to even."""
        ty, tx = ay['tap'].long(), ax['tap'].long()
        hy, wx = ay['weight'].to(dtype), ax['weight'].to(dtype)
        top, bot = tab[..., ty[:, 0], :], tab[..., ty[:, 1], :]
        a, b, c, d = top[..., tx[:, 0]], top[..., tx[:, 1]], bot[..., tx[:, 0]], bot[..., tx[:, 1]]
        hy0, hy1, wx0, wx1 = hy[:, 0:1], hy[:, 1:2], wx[:, 0], wx[:, 1]
        return torch.round(hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d))

    def reference_from_pixels(self, pixels, depth, keep, offsets, labels=False, out_dtype=torch.float32):
        """(b) + (c) [+ (d)]: the winner of a source pixel is the highest point index (an integer amax: deterministic on
        every device), taken only where the pixel is a tap of a kept output (with ``labels``: of a label's row and column);
        then the four-tap blend in float64."""
        f, n = self._check_pixels(pixels, depth, keep, offsets, not pixels.is_cuda)
        dev = pixels.device
        ay, ax = self._tables(labels, np.float64, dev)
        nsy, nsx = ay['slot_src'].numel(), ax['slot_src'].numel()
        h, w = self.source_hw
        frame, local, owned = self._frames(offsets, pixels.shape[0])
        px, py = pixels[..., 0].long(), pixels[..., 1].long()
        inside = keep & owned[:, None] & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        sx, sy = ax['src_slot'].long()[px.clamp(0, w - 1)], ay['src_slot'].long()[py.clamp(0, h - 1)]
        ok = inside & (sx >= 0) & (sy >= 0)
        cam = torch.arange(n, device=dev)
        lin = ((frame[:, None] * n + cam[None]) * nsy + sy) * nsx + sx
        win = torch.zeros(f * n * nsy * nsx, dtype=torch.int64, device=dev)
        win.scatter_reduce_(0, torch.where(ok, lin, torch.zeros_like(lin)).reshape(-1),
                            torch.where(ok, (local + 1)[:, None].expand_as(lin), torch.zeros_like(lin)).reshape(-1), 'amax')
        win = win.view(f, n, nsy, nsx)
        point = offsets.long()[:-1].view(f, 1, 1, 1) + win - 1
        flat = depth.reshape(-1)
        if flat.numel() == 0:
            tab = torch.zeros(f, n, nsy, nsx, dtype=torch.float64, device=dev)
        else:
            tab = torch.where(win > 0, flat[(point.clamp(0, pixels.shape[0] - 1) * n + cam.view(1, n, 1, 1))],
                              torch.zeros((), dtype=torch.float64, device=dev))
        out = self._blend(tab, ay, ax, torch.float64)
        return self._clamp(out.float()) if labels else out.to(out_dtype)

    def reference_from_lidar(self, points, offsets, steps, before, intrinsics, labels=False, out_dtype=torch.float32,
                             params=None):
        pixels, depth, keep = self.reference_project(points, offsets, steps, before, intrinsics)
        if params is not None:
            return self._reference_augmented(params, pixels.shape[1], labels, out_dtype, (pixels, depth, keep, offsets), None)
        return self.reference_from_pixels(pixels, depth, keep, offsets, labels, out_dtype)

    def reference_from_maps(self, maps, labels=False, out_dtype=torch.float32, params=None):
        """(c) [+ (d)] of stored maps (F, N, H, W), float64 or float32, in the maps' dtype."""
        self._check_maps(maps)
        if params is not None:
            return self._reference_augmented(params, maps.shape[1], labels, out_dtype, None, maps)
        ay, ax = self._tables(labels, np.float64 if maps.dtype == torch.float64 else np.float32, maps.device)
        tab = maps[..., ay['slot_src'].long(), :][..., ax['slot_src'].long()]
        out = self._blend(tab, ay, ax, maps.dtype)
        return self._clamp(out.float()) if labels else out.to(out_dtype)

    def _check_maps(self, maps):
        if maps.dim() != 4 or tuple(maps.shape[2:]) != self.source_hw or maps.dtype not in (torch.float32, torch.float64):
            raise ValueError(f'maps: (F, N, {self.source_hw[0]}, {self.source_hw[1]}) float64 or float32')

    # ---- the kernels ---------------------------------------------------------------------------------------------------
    def _dims(self, f, n, n_total, labels, out_kind, dtype, device):
        ay, ax = self._tables(labels, dtype, device)
        d = _lib.DepthDims()
        d.F, d.N, d.n_total, d.out_kind = f, n, n_total, out_kind
        d.d_lo, d.d_hi = self.d_bound[0], self.d_bound[1] - 1                  # (ctypes rounds to float32, as torch.clamp)
        for axis, t, n_src in ((d.y, ay, self.source_hw[0]), (d.x, ax, self.source_hw[1])):
            axis.tap, axis.weight = t['tap'].data_ptr(), t['weight'].data_ptr()
            axis.slot_src, axis.src_slot = t['slot_src'].data_ptr(), t['src_slot'].data_ptr()
            axis.n_out, axis.n_slot, axis.n_src = t['tap'].shape[0], t['slot_src'].numel(), n_src
        return d

    def _workspace(self, d, device):
        need = ctypes.c_size_t()
        _lib.check(_lib.lib().stp3_depth_workspace_bytes(ctypes.byref(d), ctypes.byref(need)), 'stp3_depth_workspace_bytes')
        return torch.empty(max(need.value, 16), dtype=torch.uint8, device=device), need.value

    def project(self, points, offsets, steps, before, intrinsics, check=False):
        """(a): pixels (n, N, 2) int32 = (u, v) truncated toward zero (0 where not kept), depth (n, N) float64 (the
        float32 z), keep (n, N) bool."""
        if not points.is_cuda:
            return self.reference_project(points, offsets, steps, before, intrinsics)
        f, n = self._check_cloud(points, offsets, steps, intrinsics, check)
        dev, n_total = points.device, points.shape[0]
        points, offsets, steps, intrinsics = (t.contiguous() for t in (points, offsets, steps, intrinsics))
        pixels = torch.empty(n_total, n, 2, dtype=torch.int32, device=dev)
        depth = torch.empty(n_total, n, dtype=torch.float64, device=dev)
        keep = torch.empty(n_total, n, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().stp3_depth_project(f, n, n_total, self.source_hw[0], self.source_hw[1], ops._ptr(points),
                                                 ops._ptr(offsets), ops._ptr(steps), self._before_mask(before),
                                                 ops._ptr(intrinsics), ops._ptr(pixels), ops._ptr(depth), ops._ptr(keep),
                                                 ops._stream()), 'stp3_depth_project')
        return pixels, depth, keep.view(torch.bool)

    def from_pixels(self, pixels, depth, keep, offsets, labels=False, out_dtype=torch.float32, check=False):
        """(b) + (c) [+ (d)] of projected points: depths (F, N, Ho, Wo), or int64 class ids (F, N, fH, fW)."""
        if not pixels.is_cuda:
            return self.reference_from_pixels(pixels, depth, keep, offsets, labels, out_dtype)
        f, n = self._check_pixels(pixels, depth, keep, offsets, check)
        dev = pixels.device
        dtype, kind = self._out_dtype(labels, out_dtype)
        d = self._dims(f, n, pixels.shape[0], labels, kind, np.float64, dev)
        pixels, depth, keep, offsets = (t.contiguous() for t in (pixels, depth, keep, offsets))
        ws, nbytes = self._workspace(d, dev)
        out = torch.empty(f, n, d.y.n_out, d.x.n_out, dtype=dtype, device=dev)
        _lib.check(_lib.lib().stp3_depth_from_pixels(ctypes.byref(d), ops._ptr(pixels), ops._ptr(depth),
                                                     ops._ptr(keep.view(torch.uint8)), ops._ptr(offsets), ops._ptr(ws), nbytes,
                                                     ops._ptr(out), ops._stream()), 'stp3_depth_from_pixels')
        return out

    def from_lidar(self, points, offsets, steps, before, intrinsics, labels=False, out_dtype=torch.float32, check=False,
                   fused=False, params=None, plan=None):
        """(a) - (c) [- (d)] from the sweeps.  ``labels=True``: int64 class ids (F, N, fH, fW), equal to
        ``class_ids(from_lidar(...))``, through the winner table of the label rows and columns in global memory like the
        full map (the default: measured faster at the trained shape); with ``fused`` in one launch
        that keeps the winners of an image in LDS and needs no scratch.  ``params`` (F N dictionaries of
        ``ImageAugmenter.sample`` in (frame, camera) order) or a prepared ``plan`` (``augment_plan``): the labels under the
        per-image augmentation, (F, N, Ho, Wo) of the parameters' crop size (class ids: every ``downsample``-th row and
        column of it)."""
        if params is not None or plan is not None:
            if fused:
                raise ValueError('DepthLabeller.from_lidar: the one-launch labels kernel takes no augmentation parameters')
            if not points.is_cuda:
                return self.reference_from_lidar(points, offsets, steps, before, intrinsics, labels, out_dtype, params)
            f, n = self._check_cloud(points, offsets, steps, intrinsics, check)
            plan = self._plan_for(params, plan, f * n, points.device, labels, None, points.shape[0] * n)
            return self._run_augmented(plan, f, n, out_dtype, cloud=(points, offsets, steps, before, intrinsics))
        if not points.is_cuda:
            return self.reference_from_lidar(points, offsets, steps, before, intrinsics, labels, out_dtype)
        f, n = self._check_cloud(points, offsets, steps, intrinsics, check)
        dev = points.device
        dtype, kind = self._out_dtype(labels, out_dtype)
        d = self._dims(f, n, points.shape[0], labels, kind, np.float64, dev)
        points, offsets, steps, intrinsics = (t.contiguous() for t in (points, offsets, steps, intrinsics))
        mask = self._before_mask(before)
        out = torch.empty(f, n, d.y.n_out, d.x.n_out, dtype=dtype, device=dev)
        lib = _lib.lib()
        if labels and fused:
            _lib.check(lib.stp3_depth_labels_from_lidar(ctypes.byref(d), ops._ptr(points), ops._ptr(offsets), ops._ptr(steps),
                                                        mask, ops._ptr(intrinsics), self.label_bands, ops._ptr(out),
                                                        ops._stream()), 'stp3_depth_labels_from_lidar')
            return out
        ws, nbytes = self._workspace(d, dev)
        _lib.check(lib.stp3_depth_from_lidar(ctypes.byref(d), ops._ptr(points), ops._ptr(offsets), ops._ptr(steps), mask,
                                             ops._ptr(intrinsics), ops._ptr(ws), nbytes, ops._ptr(out), ops._stream()),
                   'stp3_depth_from_lidar')
        return out

    def from_maps(self, maps, labels=False, out_dtype=torch.float32, params=None, plan=None):
        """(c) [- (d)] of stored dense maps (F, N, H, W), float64 or float32, arithmetic in the maps' dtype; with ``params``
        or a ``plan`` under the per-image augmentation, as ``from_lidar``."""
        if not maps.is_cuda:
            return self.reference_from_maps(maps, labels, out_dtype, params)
        self._check_maps(maps)
        if params is not None or plan is not None:
            f, n = maps.shape[:2]
            plan = self._plan_for(params, plan, f * n, maps.device, labels, maps.dtype, 0)
            return self._run_augmented(plan, f, n, out_dtype, maps=maps)
        dtype, kind = self._out_dtype(labels, out_dtype)
        f, n = maps.shape[:2]
        is64 = maps.dtype == torch.float64
        d = self._dims(f, n, 0, labels, kind, np.float64 if is64 else np.float32, maps.device)
        maps = maps.contiguous()
        out = torch.empty(f, n, d.y.n_out, d.x.n_out, dtype=dtype, device=maps.device)
        _lib.check(_lib.lib().stp3_depth_from_maps(ctypes.byref(d), ops._ptr(maps), _lib.DEPTH_OUT_F64 if is64 else
                                                   _lib.DEPTH_OUT_F32, ops._ptr(out), ops._stream()), 'stp3_depth_from_maps')
        return out

    # ---- under the per-image augmentation of the camera images ------------------------------------
    def _check_params(self, params, n=None):
        if params is None or not len(params) or (n is not None and len(params) != n):
            raise ValueError(f'DepthLabeller: {0 if params is None else len(params)} parameter sets for {n} images')
        sizes = {(p['crop'][2] - p['crop'][0], p['crop'][3] - p['crop'][1]) for p in params}
        if len(sizes) != 1:
            raise ValueError(f'DepthLabeller: the crops of one call have one size, got {sorted(sizes)}')
        wo, ho = next(iter(sizes))
        if wo < 1 or ho < 1 or any(min(p['resize_dims']) < 1 for p in params):
            raise ValueError('DepthLabeller: an empty crop or resized map')
        if wo > MAX_ROTATE_SIDE or ho > MAX_ROTATE_SIDE:
            raise ValueError(f'DepthLabeller: a crop of {wo} x {ho} (at most {MAX_ROTATE_SIDE}: Pillow\'s rotation overflows)')
        h, w = self.source_hw
        for p in params:
            want = (int(math.floor(w * p['resize'])), int(math.floor(h * p['resize'])))      # F.interpolate's output size
            if tuple(p['resize_dims']) != want:
                raise ValueError(f'DepthLabeller: resize_dims {tuple(p["resize_dims"])} where F.interpolate gives {want}')
        return wo, ho

    @staticmethod
    def _source_step(n_src, n_res, maps):
        """The source step of a route: NuscenesData.py:295 recomputes the scale factor (n_src / n_res), :262 hands 1 / resize on."""
        return np.float64(n_src) / np.float64(n_res) if maps is None else None

    def _reference_augmented(self, params, n_cam, labels, out_dtype, cloud, maps):
        """The composition of DESIGN.md section 4.9c in torch operators, image by image: the winners (or the stored map) at
        the taps of the resized rows and columns inside the crop window, ``_blend`` (which rounds), the zero-padded window,
        the flip, Pillow's nearest rotation from its fixed-point integers; class ids as ``class_ids`` of that."""
        h, w = self.source_hw
        if cloud is not None:
            pixels, depth, keep, offsets = cloud
            dev, n_frames, dtype = pixels.device, offsets.numel() - 1, torch.float64
            bounds = offsets.tolist()
        else:
            dev, n_frames, dtype = maps.device, maps.shape[0], maps.dtype
        wo, ho = self._check_params(params, n_frames * n_cam)
        np_dtype = np.float64 if dtype == torch.float64 else np.float32
        out = torch.zeros(n_frames * n_cam, ho, wo, dtype=dtype, device=dev)
        for i, p in enumerate(params):
            f, c = divmod(i, n_cam)
            wr, hr = p['resize_dims']
            left, top, right, bottom = p['crop']
            y0, y1, x0, x1 = max(top, 0), min(bottom, hr), max(left, 0), min(right, wr)          # PIL pads a crop with zeros
            if y0 < y1 and x0 < x1:
                ay = depth_resample_axis(h, p['resize'], np.arange(y0, y1), np_dtype, self._source_step(h, hr, maps))
                ax = depth_resample_axis(w, p['resize'], np.arange(x0, x1), np_dtype, self._source_step(w, wr, maps))
                ay, ax = ({k: torch.from_numpy(v).to(dev) for k, v in t.items()} for t in (ay, ax))
                if cloud is None:
                    tab = maps[f, c][ay['slot_src'].long(), :][:, ax['slot_src'].long()]
                else:
                    nsy, nsx = ay['slot_src'].numel(), ax['slot_src'].numel()
                    a, b = max(0, bounds[f]), min(pixels.shape[0], bounds[f + 1])
                    tab = torch.zeros(nsy, nsx, dtype=dtype, device=dev)
                    if a < b:
                        px, py, z = pixels[a:b, c, 0].long(), pixels[a:b, c, 1].long(), depth[a:b, c]
                        ok = keep[a:b, c] & (px >= 0) & (px < w) & (py >= 0) & (py < h)
                        sx, sy = ax['src_slot'].long()[px.clamp(0, w - 1)], ay['src_slot'].long()[py.clamp(0, h - 1)]
                        ok = ok & (sx >= 0) & (sy >= 0)
                        zero = torch.zeros_like(sx)
                        local = torch.arange(1, b - a + 1, device=dev)                           # last point in point order wins
                        win = torch.zeros(nsy * nsx, dtype=torch.int64, device=dev)
                        win.scatter_reduce_(0, torch.where(ok, sy * nsx + sx, zero), torch.where(ok, local, zero), 'amax')
                        tab = torch.where(win > 0, z[(win - 1).clamp(min=0)], torch.zeros((), dtype=dtype, device=dev)).view(nsy, nsx)
                out[i, y0 - top:y1 - top, x0 - left:x1 - left] = self._blend(tab, ay, ax, dtype)
            window = out[i].flip(1) if p['flip'] else out[i]
            out[i] = rotate_nearest_pil(window.unsqueeze(-1), pil_rotate_fixed(p['rotate'], (wo, ho))).squeeze(-1)
        out = out.view(n_frames, n_cam, ho, wo)
        return self.class_ids(out.float()) if labels else out.to(out_dtype)

    def _augment_layout(self, n, n_y, n_x):
        """Where the tables lie in a plan's one buffer of int32 words (the weights: float64, at an even word)."""
        sizes = (('records', 16 * n), ('tap_y', 2 * n * n_y), ('tap_x', 2 * n * n_x), ('slot_y', 2 * n * n_y), ('slot_x', 2 * n * n_x),
                 ('weight_y', 4 * n * n_y), ('weight_x', 4 * n * n_x))
        at, out = 0, {}
        for k, size in sizes:
            out[k] = (at, at + size)
            at += size
        return out, at

    def _augment_host(self, params, separable, maps):
        """The records and tables of stp3_augment_depth_* (include/stp3_hip.h) for ``params`` as one int32 array: per axis
        the arithmetic of ``depth_resample_axis`` for all images at once (a batch of 72 images is 144 tables)."""
        wo, ho = self._check_params(params)
        h, w = self.source_hw
        st = self.downsample if separable else 1
        n, n_y, n_x = len(params), -(-ho // st), -(-wo // st)
        layout, words = self._augment_layout(n, n_y, n_x)
        blob = np.zeros(words, dtype=np.int32)
        part = {k: blob[a:b] for k, (a, b) in layout.items()}
        records = part['records'].reshape(n, 16)
        t = np.float32 if maps == torch.float32 else np.float64
        resize = np.array([p['resize'] for p in params], dtype=np.float64)
        image = np.arange(n)[:, None]
        for name, n_src, side, count, at, flips in (('y', h, ho, n_y, 1, None), ('x', w, wo, n_x, 0, [p['flip'] for p in params])):
            n_res = np.array([p['resize_dims'][at] for p in params], dtype=np.int64)[:, None]
            origin = np.array([p['crop'][at] for p in params], dtype=np.int64)[:, None]
            k = (np.arange(count, dtype=np.int64) * st)[None]
            if flips is not None:
                k = np.where(np.array(flips, dtype=bool)[:, None], side - 1 - k, k)
            r = origin + k                                                                   # the resized row / column of an entry
            valid = (r >= 0) & (r < n_res)
            step = (1.0 / resize).astype(t) if maps is not None else (np.float64(n_src) / n_res[:, 0].astype(np.float64))
            src = np.maximum(step[:, None] * (r.astype(t) + t(0.5)) - t(0.5), t(0.0))
            i0 = np.minimum(src.astype(np.int64), n_src - 1)
            i1 = np.minimum(i0 + 1, n_src - 1)
            lam = np.clip(src - i0.astype(t), t(0.0), t(1.0))
            present = np.zeros((n, n_src), dtype=bool)                                       # the source indices that are taps
            rows = np.broadcast_to(image, r.shape)[valid]
            present[rows, i0[valid]] = True
            present[rows, i1[valid]] = True
            src_slot = np.cumsum(present, axis=1) - 1
            n_slot = present.sum(axis=1)
            first = np.cumsum(n_slot) - n_slot
            slots = np.nonzero(present)[1]                                                   # image after image, ascending
            part['slot_' + name][:len(slots)] = slots
            tap = part['tap_' + name].reshape(n, count, 2)
            tap[..., 0] = np.where(valid, src_slot[image, i0], -1)
            tap[..., 1] = np.where(valid, src_slot[image, i1], -1)
            weight = part['weight_' + name].view(np.float64).reshape(n, count, 2)
            weight[..., 0] = np.where(valid, t(1.0) - lam, t(0.0))
            weight[..., 1] = np.where(valid, lam, t(0.0))
            records[:, 6 + (1 - at)] = np.arange(n) * count
            records[:, 8 + (1 - at)] = first
            records[:, 10 + (1 - at)] = n_slot
        records[:, :6] = [pil_rotate_fixed(p['rotate'], (wo, ho)) for p in params]
        return blob

    @staticmethod
    def _rotates(params, size):
        return any(pil_rotate_fixed(p['rotate'], size) != ROTATE_IDENTITY for p in params)

    def augment_plan(self, params, device, labels=False, like=None, maps=None, points=0, rotate=None):
        """The ``DepthAugmentPlan`` of ``params`` (F N dictionaries, (frame, camera) order) on ``device``: records, axis tables
        and the winner-table workspace as static tensors.  ``maps``: None for ``from_lidar``, the maps' dtype for
        ``from_maps`` (the two reference branches take their taps differently, and a float32 map its weights in float32).
        ``points``: room for the depths of that many (point, camera) pairs (``from_lidar`` grows it outside a capture).
        With ``labels`` and no rotating image the tables hold the label rows and columns only; ``rotate=True`` reserves the
        window's tables for later parameters that rotate.  ``like``: rewrite that plan's tensors in place instead, so that
        a captured call replays with the new parameters; ValueError if they do not fit the room it reserved."""
        wo, ho = self._check_params(params)
        rotates = self._rotates(params, (wo, ho))
        if like is not None:
            if (len(params), (wo, ho)) != (like.n, like.size) or (rotates and like.separable):
                raise ValueError('DepthLabeller.augment_plan: the parameters do not fit the plan they are to replace')
            like.blob.copy_(torch.from_numpy(self._augment_host(params, like.separable, like.maps)))
            return like
        if maps not in (None, torch.float32, torch.float64):
            raise ValueError('DepthLabeller.augment_plan: maps is None (LiDAR), torch.float64 or torch.float32')
        separable = bool(labels) and not rotates and not rotate
        blob = torch.from_numpy(self._augment_host(params, separable, maps)).to(device)
        st = self.downsample if separable else 1
        plan = DepthAugmentPlan(len(params), (wo, ho), bool(labels), separable, maps, blob,
                                self._augment_layout(len(params), -(-ho // st), -(-wo // st))[0])
        if maps is None:
            plan.table_bytes = len(params) * 4 * -(-ho // st) * -(-wo // st) * 4
            plan.workspace = torch.empty(plan.table_bytes + 4 * int(points), dtype=torch.uint8, device=device)
        return plan

    def _plan_for(self, params, plan, n, device, labels, maps, pairs):
        if plan is None:
            self._check_params(params, n)
            return self.augment_plan(params, device, labels, maps=maps, points=pairs)
        if plan.n != n or plan.maps != maps or plan.labels != bool(labels) or plan.blob.device != device:
            raise ValueError('DepthLabeller: the plan was made for other images, another route or another output')
        if maps is None and plan.workspace.numel() < plan.table_bytes + 4 * pairs:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError('DepthLabeller: the plan has no room for this cloud (augment_plan(points=...))')
            plan.workspace = torch.empty(plan.table_bytes + 4 * pairs, dtype=torch.uint8, device=device)
        return plan

    def _augment_dims(self, plan, f, n, n_total, kind):
        wo, ho = plan.size
        d = _lib.AugmentDepthDims()
        d.F, d.N, d.n_total, d.out_kind = f, n, n_total, kind
        d.d_lo, d.d_hi = self.d_bound[0], self.d_bound[1] - 1
        d.H, d.W, d.Ho, d.Wo = self.source_hw[0], self.source_hw[1], ho, wo
        d.stride, d.separable = self.downsample if plan.labels else 1, int(plan.separable)
        d.records = plan.part('records').data_ptr()
        for axis, name in ((d.y, 'y'), (d.x, 'x')):
            axis.tap, axis.weight, axis.slot_src = (plan.part(k + name).data_ptr() for k in ('tap_', 'weight_', 'slot_'))
            axis.entries, axis.slots = plan.part('tap_' + name).numel() // 2, plan.part('slot_' + name).numel()
        return d

    def _run_augmented(self, plan, f, n, out_dtype, cloud=None, maps=None):
        """One call of stp3_augment_depth_from_lidar / _from_maps with a prepared plan: enqueues only (capturable)."""
        dtype, kind = self._out_dtype(plan.labels, out_dtype)
        wo, ho = plan.size
        d = self._augment_dims(plan, f, n, 0 if cloud is None else cloud[0].shape[0], kind)
        out = torch.empty(f, n, -(-ho // d.stride), -(-wo // d.stride), dtype=dtype, device=plan.blob.device)
        lib = _lib.lib()
        if cloud is None:
            maps = maps.contiguous()
            _lib.check(lib.stp3_augment_depth_from_maps(ctypes.byref(d), ops._ptr(maps), _lib.DEPTH_OUT_F64 if maps.dtype ==
                                                        torch.float64 else _lib.DEPTH_OUT_F32, ops._ptr(out), ops._stream()),
                       'stp3_augment_depth_from_maps')
            return out
        points, offsets, steps, before, intrinsics = cloud
        points, offsets, steps, intrinsics = (t.contiguous() for t in (points, offsets, steps, intrinsics))
        _lib.check(lib.stp3_augment_depth_from_lidar(ctypes.byref(d), ops._ptr(points), ops._ptr(offsets), ops._ptr(steps),
                                                     self._before_mask(before), ops._ptr(intrinsics), ops._ptr(plan.workspace),
                                                     plan.workspace.numel(), ops._ptr(out), ops._stream()),
                   'stp3_augment_depth_from_lidar')
        return out


class DepthAugmentPlan:
    """The device-side description of one augmented ``DepthLabeller`` call: the per-image records and the axis tables in one
    static buffer, the winner-table workspace.  ``DepthLabeller.augment_plan(params, like=plan)`` rewrites them in place (a
    captured graph then replays with the new parameters)."""

    def __init__(self, n, size, labels, separable, maps, blob, layout):
        self.n, self.size, self.labels, self.separable, self.maps, self.blob, self.layout = n, size, labels, separable, maps, blob, layout
        self.workspace, self.table_bytes = None, 0

    def part(self, name):
        a, b = self.layout[name]
        return self.blob[a:b]


# ----------------------------------------------------------------------------------------------------------------------
# JPEG camera frames: the Huffman half on host threads (csrc/stp3_jpeg_entropy.h), the dense half in one kernel
# (csrc/stp3_jpeg.hip: stp3_jpeg_reconstruct), byte-exact with Pillow's decode.  Its output is the input of
# ImagePreprocessor / ImageAugmenter above.
# ----------------------------------------------------------------------------------------------------------------------
class JpegUnsupported(ValueError):
    """A stream the entropy decoder does not take (progressive, CMYK, another sampling, ...) met with ``fallback=False``."""


JpegGeometry = collections.namedtuple('JpegGeometry', 'width height components hs vs')
JpegInfo = collections.namedtuple('JpegInfo', 'width height components hs vs mcus_x mcus_y blocks restart_interval coef_count')
_SOF_NAMES = {0xC2: 'progressive', 0xC3: 'lossless', 0xC5: 'hierarchical', 0xC6: 'hierarchical progressive', 0xC7: 'hierarchical lossless',
              0xC9: 'arithmetic coding', 0xCA: 'progressive, arithmetic coding', 0xCB: 'lossless, arithmetic coding',
              0xCD: 'hierarchical, arithmetic coding', 0xCE: 'hierarchical, arithmetic coding', 0xCF: 'hierarchical, arithmetic coding'}


def _geometry(info):
    return JpegGeometry(info.width, info.height, info.components, info.hs, info.vs)


def _coef_count(g):
    mx, my = -(-g.width // (8 * g.hs)), -(-g.height // (8 * g.vs))
    return mx * my * (g.hs * g.vs + (2 if g.components == 3 else 0)) * 64


def jpeg_unsupported_reason(data):
    """Why stp3_jpeg_info answered STP3_EUNSUP, in words (the C entry returns the code only): a walk over the markers."""
    data = bytes(data)
    pos, frame, jfif, adobe = 2, None, False, None
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + n]
        if m in _SOF_NAMES:
            return _SOF_NAMES[m]
        if m in (0xC0, 0xC1) and len(seg) >= 6:
            frame = seg
        jfif = jfif or (m == 0xE0 and seg[:5] == b'JFIF\0')
        if m == 0xEE and seg[:5] == b'Adobe' and len(seg) >= 12:
            adobe = seg[11]
        if m == 0xDA and frame is not None:
            nc = frame[5]
            comps = [(frame[6 + 3 * c], frame[7 + 3 * c] >> 4, frame[7 + 3 * c] & 15) for c in range(nc)]
            if frame[0] != 8:
                return f'{frame[0]}-bit samples'
            if nc not in (1, 3):
                return f'{nc} components' + (' (CMYK / YCCK)' if nc == 4 else '')
            if max((frame[1] << 8) | frame[2], (frame[3] << 8) | frame[4]) > 16384:
                return 'a side above 16 384 pixels'
            if nc == 3 and (comps[0][1:] not in ((1, 1), (2, 1), (2, 2)) or comps[1][1:] != (1, 1) or comps[2][1:] != (1, 1)):
                return 'sampling factors ' + ', '.join(f'{h}x{v}' for _, h, v in comps)
            if nc == 3 and not jfif and (adobe == 0 or (adobe is None and bytes(c[0] for c in comps) == b'RGB')):
                return 'an RGB stream (no YCbCr transform)'
            if seg and seg[0] != nc:
                return 'more than one scan'
            break
        pos += 2 + n
    return 'not a stream of the supported kind'


class JpegGroup:
    """The images of a ``JpegBatch`` that share one geometry: where they sit in the call, their coefficients (n, coef_count)
    int16 and quantisation tables (n, 3, 64) uint16 bits in int16 storage, both in pinned host memory where there is a GPU."""

    def __init__(self, geometry, indices, pin):
        self.geometry, self.indices = geometry, list(indices)
        self.coef = torch.empty(len(self.indices), _coef_count(geometry), dtype=torch.int16, pin_memory=pin)
        self.quant = torch.empty(len(self.indices), 3, 64, dtype=torch.int16, pin_memory=pin)


class JpegBatch:
    """What ``JpegDecoder.entropy`` returns: per geometry a ``JpegGroup``; ``fallback`` maps the index of every stream the
    entropy decoder does not take to (reason, its bytes) -- Pillow decodes those on the host."""

    def __init__(self, n, groups, fallback, sizes):
        self.n, self.groups, self.fallback, self.sizes = n, groups, fallback, sizes          # sizes: (height, width) per image

    def layout(self):
        return [(g.geometry, tuple(g.indices)) for g in self.groups]


class JpegScanGroup:
    """The images of a ``JpegScanBatch`` that share one geometry, prepared for the device entropy decode: per image the scan
    buffer stp3_jpeg_scan_prepare wrote (``scans`` (n, stride) uint8), its descriptor (``descs`` (n, sizeof desc) uint8) and
    its quantisation tables (``quant`` (n, 3, 64)), pinned where there is a GPU.  ``host``: positions in the group whose stream
    goes to the host decoder (STP3_JPEG_IRREGULAR)."""

    def __init__(self, geometry, indices, stride, pin):
        self.geometry, self.indices, self.stride = geometry, list(indices), stride
        n = len(self.indices)
        self.scans = torch.empty(n, stride, dtype=torch.uint8, pin_memory=pin)
        self.descs = torch.zeros(n, ctypes.sizeof(_lib.JpegScanDesc), dtype=torch.uint8, pin_memory=pin)
        self.quant = torch.empty(n, 3, 64, dtype=torch.int16, pin_memory=pin)
        self.host, self.max_subs, self.max_segs = [], 1, 1


class JpegScanBatch:
    """What ``JpegDecoder.prepare`` returns: per geometry a ``JpegScanGroup``; ``fallback`` as in ``JpegBatch``; ``streams``:
    the bytes of the call (the host decoder reads them for whatever the device does not take)."""

    def __init__(self, n, groups, fallback, sizes, streams):
        self.n, self.groups, self.fallback, self.sizes, self.streams = n, groups, fallback, sizes, streams

    def layout(self):
        return [(g.geometry, tuple(g.indices)) for g in self.groups]


JpegDeviceGroup = collections.namedtuple('JpegDeviceGroup', 'geometry indices coef quant')
JPEG_SYNC_ROUNDS = 2                                                        # (twice the largest number of rounds measured)


class JpegDecoder:
    """JPEG bytes -> (N, H, W, 3) uint8 RGB on the GPU, equal to ``PIL.Image.open(...).convert('RGB')`` byte for byte.

        dec = JpegDecoder()
        images = dec(list_of_bytes, 'cuda')                  # entropy decode on host threads + one kernel per geometry
        x = ImagePreprocessor(cfg)(images)                   # or ImageAugmenter(cfg, ...)(images, params)

    ``workers``: host threads of the entropy decode (ctypes releases the GIL), at most ``min(16, os.cpu_count())`` by default.
    ``fallback``: a stream the entropy decoder answers with STP3_EUNSUP (progressive, CMYK, 4:1:1, ...) is decoded by Pillow on
    the host and uploaded into the same slot of the result; ``fallback=False`` raises ``JpegUnsupported`` instead.  A corrupt
    stream (STP3_EINVAL) always raises.

    ``entropy='device'`` decodes the Huffman scan on the GPU as well (csrc/stp3_jpeg_huff.hip): the host only strips the byte
    stuffing and cuts the scan at its restart markers (``prepare``), the compressed scan is uploaded instead of the
    coefficients.  The result is the same by construction: an image the device reports (a stream it calls corrupt, one whose
    subsequences had not synchronised after ``sync_rounds`` further launches) or ``prepare`` calls irregular goes through the
    host decoder above, which raises what it raises in host mode.  On a CPU ``device`` the mode is the host decoder.
    ``last_stats``: per call, how many images the device decoded, the host decoder, Pillow."""

    def __init__(self, workers=None, fallback=True, entropy='host', sync_rounds=JPEG_SYNC_ROUNDS):
        if entropy not in ('host', 'device'):
            raise ValueError("entropy must be 'host' or 'device'")
        if not 0 <= int(sync_rounds) <= 64:
            raise ValueError('sync_rounds must be in [0, 64]')
        self.workers = max(1, int(workers)) if workers is not None else min(16, os.cpu_count() or 1)
        self.fallback = fallback
        self.entropy_mode, self.sync_rounds = entropy, int(sync_rounds)
        self.last_stats = {'device': 0, 'host': 0, 'pillow': 0}
        self.last_flags = []                                                    # per group: the (n, sync_rounds + 3) words of the call
        self._workspace = {}
        self._pool = None

    # ---- host ---------------------------------------------------------------------------------------------------------
    def info(self, data):
        data = bytes(data)
        h = _lib.JpegHeader()
        rc = _lib.lib().stp3_jpeg_info(data, len(data), ctypes.byref(h))
        if rc == _lib.STP3_EUNSUP:
            raise JpegUnsupported(jpeg_unsupported_reason(data))
        _lib.check(rc, 'stp3_jpeg_info')
        blocks = tuple((h.blocks_y[c], h.blocks_x[c]) for c in range(h.components))
        return JpegInfo(h.width, h.height, h.components, h.hs, h.vs, h.mcus_x, h.mcus_y, blocks, h.restart_interval, h.coef_count)

    def _map(self, fn, items):
        if self.workers == 1 or len(items) < 2:
            return [fn(i) for i in items]
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers)
        return list(self._pool.map(fn, items))

    def entropy(self, streams, out=None):
        """Huffman-decode ``streams`` (bytes-like objects) into a ``JpegBatch``; ``out``: a batch of the same layout to refill."""
        streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]
        lib = _lib.lib()
        def header(s):
            try:
                return self.info(s)
            except (JpegUnsupported, _lib.Stp3HipError) as e:
                return e

        infos, fallback = self._map(header, streams), {}
        for i, f in enumerate(infos):
            if isinstance(f, JpegUnsupported):
                if not self.fallback:
                    raise JpegUnsupported(f'image {i}: {f}') from None
                fallback[i] = (str(f), streams[i])
                infos[i] = None
            elif isinstance(f, Exception):
                raise _lib.Stp3HipError(f'image {i}: {f}') from None
        order = {}
        for i, f in enumerate(infos):
            if f is not None:
                order.setdefault(_geometry(f), []).append(i)
        layout = [(g, tuple(idx)) for g, idx in order.items()]
        if out is not None and out.layout() == layout and out.n == len(streams):
            groups = out.groups
        else:
            if out is not None:
                raise ValueError('the batch to refill has another layout (geometry or order of the images)')
            groups = [JpegGroup(g, idx, torch.cuda.is_available()) for g, idx in layout]
        jobs = [(grp, k, i) for grp in groups for k, i in enumerate(grp.indices)]

        def decode(job):
            grp, k, i = job
            h = _lib.JpegHeader()
            return lib.stp3_jpeg_entropy(streams[i], len(streams[i]), grp.coef[k].data_ptr(), grp.coef.shape[1],
                                         grp.quant[k].data_ptr(), ctypes.byref(h))

        for (grp, k, i), rc in zip(jobs, self._map(decode, jobs)):
            if rc != 0:
                raise _lib.Stp3HipError(f'image {i}: stp3_jpeg_entropy failed: {_lib._ERRORS.get(rc, rc)}')
        sizes = [(f.height, f.width) if f is not None else None for f in infos]
        for i, (_, s) in fallback.items():
            sizes[i] = self._pillow_size(s)                                     # (the header only: Pillow decodes lazily)
        return JpegBatch(len(streams), groups, fallback, sizes)

    @staticmethod
    def _pillow_open(data):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError('Pillow is not installed: JpegDecoder.reference and the fallback for unsupported streams need it') from e
        return Image.open(io.BytesIO(bytes(data)))

    @classmethod
    def _pillow(cls, data):
        return np.asarray(cls._pillow_open(data).convert('RGB'))

    @classmethod
    def _pillow_size(cls, data):
        width, height = cls._pillow_open(data).size
        return (height, width)

    def reference(self, streams):
        """Pillow's decode of every stream, stacked: (N, H, W, 3) uint8 on the CPU."""
        return torch.from_numpy(np.stack([self._pillow(s) for s in streams]))

    # ---- the arithmetic of the kernel, stated with numpy --------------------------------------------------------------
    @staticmethod
    def _idct_pass(x, shift):
        """One 8-point pass of jpeg_idct_islow (jidctint.c) along axis 1 of an int64 array."""
        i0, i1, i2, i3, i4, i5, i6, i7 = (x[:, k] for k in range(8))
        z1 = (i2 + i6) * 4433
        tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
        tmp0, tmp1 = (i0 + i4) * 8192, (i0 - i4) * 8192
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = i7, i5, i3, i1
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        rows = (tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3)
        # (the kernel forms the sums in 32 bits, two's complement: the same bits wherever int32 does not overflow)
        wrap = lambda v: ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        return np.stack([wrap(r + (1 << (shift - 1))) >> shift for r in rows], axis=1)

    @classmethod
    def _plane(cls, coef, quant, by, bx):
        """(by * bx * 64,) coefficients + a (64,) table -> the (by * 8, bx * 8) samples of the padded block grid."""
        x = coef.reshape(-1, 8, 8).astype(np.int64) * quant.reshape(1, 8, 8).astype(np.int64)
        ws = cls._idct_pass(x, 13 - 2)                                           # columns: along the row index
        px = cls._idct_pass(ws.transpose(0, 2, 1), 13 + 2 + 3).transpose(0, 2, 1)   # rows
        i = px & 1023                                                             # the range-limit table of jdmaster.c
        s = np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
        return s.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)

    @staticmethod
    def _upsample_h(s, rounding_even, rounding_odd, shift, edge):
        """The horizontal triangle filter of h2v1 (on samples) / h2v2 (on column sums) over the true width."""
        wc = s.shape[1]
        last, nxt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + last + rounding_even) >> shift, (3 * s + nxt + rounding_odd) >> shift
        even[:, 0], odd[:, -1] = edge(s[:, 0], rounding_even), edge(s[:, -1], rounding_odd)
        return np.stack([even, odd], axis=2).reshape(s.shape[0], 2 * wc)

    @classmethod
    def _image(cls, g, coef, quant):
        mx, my = -(-g.width // (8 * g.hs)), -(-g.height // (8 * g.vs))
        n_y = mx * g.hs * my * g.vs * 64
        luma = cls._plane(coef[:n_y], quant[0], my * g.vs, mx * g.hs)[:g.height, :g.width]
        if g.components == 1:
            return np.repeat(luma[:, :, None], 3, axis=2).astype(np.uint8)
        wc, hc = -(-g.width // g.hs), -(-g.height // g.vs)
        chroma = []
        for c in (1, 2):
            s = cls._plane(coef[n_y + (c - 1) * mx * my * 64:n_y + c * mx * my * 64], quant[c], my, mx)[:hc, :wc]
            if g.hs == 2 and wc <= 2:                                            # jdsample.c: no fancy up-sampling this narrow
                s = np.repeat(np.repeat(s, g.vs, axis=0), 2, axis=1)
            elif g.hs == 2 and g.vs == 1:
                s = cls._upsample_h(s, 1, 2, 2, lambda v, r: v)
            elif g.hs == 2:
                up, down = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
                sums = np.stack([3 * s + up, 3 * s + down], axis=1).reshape(2 * hc, wc)
                s = cls._upsample_h(sums, 8, 7, 4, lambda v, r: (4 * v + r) >> 4)
            chroma.append(s[:g.height, :g.width] - 128)
        u, v = chroma
        rgb = np.stack([luma + ((91881 * v + 32768) >> 16), luma + ((-22554 * u + 32768 - 46802 * v) >> 16),
                        luma + ((116130 * u + 32768) >> 16)], axis=2)
        return rgb.clip(0, 255).astype(np.uint8)

    def reconstruct_reference(self, batch):
        """The kernel's integer arithmetic on the CPU (what CPU tensors take): (N, H, W, 3) uint8, or a list of (H, W, 3)
        tensors when the images of the batch differ in size."""
        images = [None] * batch.n
        for grp in batch.groups:
            coef, quant = grp.coef.numpy(), grp.quant.numpy().view(np.uint16)
            for k, i in enumerate(grp.indices):
                images[i] = torch.from_numpy(self._image(grp.geometry, coef[k], quant[k]))
        for i, (_, s) in batch.fallback.items():
            images[i] = torch.from_numpy(self._pillow(s).copy())
        return torch.stack(images) if len(set(batch.sizes)) == 1 else images

    # ---- device -------------------------------------------------------------------------------------------------------
    def reconstruct_device(self, geometry, coef, quant, out=None):
        """The kernel alone on tensors that already are on the GPU -- coef (N, coef_count) int16, quant (N, 3, 64) 16-bit --
        into ``out`` (N, H, W, 3) uint8: no copy, no allocation when ``out`` is given (what a captured graph holds)."""
        g = geometry
        n = coef.shape[0]
        if coef.dtype != torch.int16 or quant.element_size() != 2 or tuple(coef.shape) != (n, _coef_count(g)) or \
                tuple(quant.shape) != (n, 3, 64) or not coef.is_contiguous() or not quant.is_contiguous():
            raise ValueError('coef must be (N, coef_count) int16 and quant (N, 3, 64) 16-bit, both contiguous')
        ops._need_gpu(coef, quant)
        if out is None:
            out = torch.empty(n, g.height, g.width, 3, dtype=torch.uint8, device=coef.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, g.height, g.width, 3) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous uint8 tensor of shape {(n, g.height, g.width, 3)}')
        ops._need_gpu(out)
        d = _lib.JpegDims(n, g.width, g.height, g.components, g.hs, g.vs)
        _lib.check(_lib.lib().stp3_jpeg_reconstruct(ctypes.byref(d), ops._ptr(coef), ops._ptr(quant), ops._ptr(out), ops._stream()),
                   'stp3_jpeg_reconstruct')
        return out

    def reconstruct(self, batch, device, out=None):
        """One non-blocking host-to-device copy of the coefficients and one launch per geometry; streams behind the fallback
        are uploaded as Pillow decoded them.  (N, H, W, 3) uint8 on ``device`` (into ``out`` when given), or a list of
        (H, W, 3) tensors in the order of the call when the images differ in size."""
        dev = torch.device(device)
        stacked = len(set(batch.sizes)) == 1
        if out is not None and (not stacked or tuple(out.shape) != (batch.n,) + tuple(batch.sizes[0]) + (3,) or out.dtype != torch.uint8
                                or out.device.type != dev.type or not out.is_contiguous()):
            raise ValueError('out must be a contiguous uint8 tensor (N, H, W, 3) on the device of the call')
        staged = [(grp, grp.coef.to(dev, non_blocking=True), grp.quant.to(dev, non_blocking=True)) for grp in batch.groups]
        if staged and not staged[0][1].is_cuda or not staged and dev.type != 'cuda':
            ref = self.reconstruct_reference(batch)
            if out is not None:
                out.copy_(ref)
            return out if out is not None else ref
        return self._reconstruct_staged(batch, staged, dev, stacked, out)

    def _reconstruct_staged(self, batch, staged, dev, stacked, out):
        """The launches of ``reconstruct`` on coefficients that are on the device: staged = [(group, coef, quant)]."""
        if stacked and out is None:
            out = torch.empty((batch.n,) + tuple(batch.sizes[0]) + (3,), dtype=torch.uint8, device=dev)
        images = [None] * batch.n
        for grp, coef, quant in staged:
            first = grp.indices[0]
            if stacked and grp.indices == list(range(first, first + len(grp.indices))):
                self.reconstruct_device(grp.geometry, coef, quant, out[first:first + len(grp.indices)])
                continue
            part = self.reconstruct_device(grp.geometry, coef, quant)
            if stacked:
                out.index_copy_(0, torch.tensor(grp.indices, device=dev), part)
            for k, i in enumerate(grp.indices):
                images[i] = part[k]
        for i, (_, s) in batch.fallback.items():
            host = torch.from_numpy(self._pillow(s).copy())
            if stacked:
                out[i].copy_(host, non_blocking=True)
            else:
                images[i] = host.to(dev)
        return out if stacked else images

    # ---- entropy decode on the device -----------------------------------------------------------------------------------
    def prepare(self, streams, out=None):
        """Headers and stp3_jpeg_scan_prepare on the thread pool, grouped by geometry as ``entropy`` groups: a
        ``JpegScanBatch``; ``out``: a batch of the same layout whose buffers are large enough, to refill."""
        streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]
        lib = _lib.lib()

        def header(s):
            h = _lib.JpegHeader()
            rc = lib.stp3_jpeg_info(s, len(s), ctypes.byref(h))
            if rc == _lib.STP3_EUNSUP:
                return JpegUnsupported(jpeg_unsupported_reason(s))
            if rc != 0:
                return _lib.Stp3HipError(f'stp3_jpeg_info failed: {_lib._ERRORS.get(rc, rc)}')
            return h

        heads, fallback = self._map(header, streams), {}
        for i, h in enumerate(heads):
            if isinstance(h, JpegUnsupported):
                if not self.fallback:
                    raise JpegUnsupported(f'image {i}: {h}') from None
                fallback[i] = (str(h), streams[i])
                heads[i] = None
            elif isinstance(h, Exception):
                raise _lib.Stp3HipError(f'image {i}: {h}') from None
        order = {}
        for i, h in enumerate(heads):
            if h is not None:
                order.setdefault(_geometry(h), []).append(i)
        layout = [(g, tuple(idx)) for g, idx in order.items()]
        need = [-(-max(lib.stp3_jpeg_scan_bytes(ctypes.byref(heads[i]), len(streams[i])) for i in idx) // 128) * 128 for _, idx in layout]
        if out is not None:
            if out.layout() != layout or out.n != len(streams) or any(g.stride < b for g, b in zip(out.groups, need)):
                raise ValueError('the batch to refill has another layout (geometry or order of the images) or smaller scan buffers')
            groups = out.groups
        else:
            groups = [JpegScanGroup(g, idx, b, torch.cuda.is_available()) for (g, idx), b in zip(layout, need)]
        jobs = [(grp, k, i) for grp in groups for k, i in enumerate(grp.indices)]

        def job(j):
            grp, k, i = j
            return lib.stp3_jpeg_scan_prepare(streams[i], len(streams[i]), grp.scans[k].data_ptr(), grp.stride, grp.descs[k].data_ptr(),
                                              grp.quant[k].data_ptr())

        for grp in groups:
            grp.host = []
        for (grp, k, i), rc in zip(jobs, self._map(job, jobs)):
            if rc != 0:                                                         # irregular (or anything else): the host decoder's
                grp.host.append(k)
                grp.descs[k].zero_()
        for grp in groups:
            words = grp.descs.numpy().view(np.int32)
            grp.max_subs, grp.max_segs = max(1, int(words[:, 0].max())), max(1, int(words[:, 1].max()))
        sizes = [(h.height, h.width) if h is not None else None for h in heads]
        for i, (_, s) in fallback.items():
            sizes[i] = self._pillow_size(s)
        return JpegScanBatch(len(streams), groups, fallback, sizes, streams)

    def _work(self, dev, nbytes):
        ws = self._workspace.get(dev)
        if ws is None or ws.numel() < nbytes:
            ws = self._workspace[dev] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        return ws

    def entropy_device_launch(self, grp, scans, descs, coef, status, workspace=None):
        """stp3_jpeg_entropy_device alone on tensors that are on the GPU: the scans and descriptors of a ``JpegScanGroup``
        into ``coef`` (n, coef_count) int16 and ``status`` (n,) int32.  Enqueues only."""
        g, n = grp.geometry, len(grp.indices)
        if coef.dtype != torch.int16 or tuple(coef.shape) != (n, _coef_count(g)) or status.dtype != torch.int32 or status.numel() != n or \
                tuple(scans.shape) != (n, grp.stride) or not all(t.is_contiguous() for t in (scans, descs, coef, status)):
            raise ValueError('coef must be (N, coef_count) int16, status (N,) int32, scans (N, stride) uint8, all contiguous')
        ops._need_gpu(scans, descs, coef, status)
        d = _lib.JpegHuffDims(n, g.width, g.height, g.components, g.hs, g.vs, grp.stride, grp.max_subs, grp.max_segs)
        nbytes = _lib.c_size_t()
        lib = _lib.lib()
        _lib.check(lib.stp3_jpeg_entropy_workspace_bytes(ctypes.byref(d), self.sync_rounds, ctypes.byref(nbytes)),
                   'stp3_jpeg_entropy_workspace_bytes')
        if workspace is None:
            workspace = self._work(coef.device, nbytes.value)
        _lib.check(lib.stp3_jpeg_entropy_device(ctypes.byref(d), ops._ptr(scans), ops._ptr(descs), ops._ptr(coef), ops._ptr(status),
                                                ops._ptr(workspace), workspace.numel(), self.sync_rounds, ops._stream()),
                   'stp3_jpeg_entropy_device')
        return workspace

    def _entropy_device(self, batch, dev, staged_quant=None):
        """The device decode of a prepared batch: [(group, coef, quant)] on ``dev``, every image the device did not take decoded
        by the host decoder and uploaded into its slot; one copy of the status words, one synchronise."""
        lib = _lib.lib()
        total = sum(len(g.indices) for g in batch.groups)
        status = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        staged, at, self.last_flags = [], 0, []
        keep_flags = getattr(self, 'keep_flags', False)
        for gi, grp in enumerate(batch.groups):
            n = len(grp.indices)
            quant = staged_quant[gi] if staged_quant is not None else grp.quant.to(dev, non_blocking=True)
            scans, descs = grp.scans.to(dev, non_blocking=True), grp.descs.to(dev, non_blocking=True)
            coef = torch.empty(n, _coef_count(grp.geometry), dtype=torch.int16, device=dev)
            # one workspace per group while the launches of the call are in flight
            ws = self.entropy_device_launch(grp, scans, descs, coef, status[at:at + n],
                                            workspace=None if len(batch.groups) == 1 else self._group_workspace(grp, dev))
            if keep_flags:
                self.last_flags.append(ws[:n * (self.sync_rounds + 3) * 4].clone())
            staged.append((grp, coef, quant))
            at += n
        codes = status.cpu().tolist()                                          # the one synchronise of the call
        if keep_flags:
            self.last_flags = [f.cpu().numpy().view(np.int32).reshape(-1, self.sync_rounds + 3) for f in self.last_flags]
        at, on_host = 0, 0
        for grp, coef, quant in staged:
            n = len(grp.indices)
            redo = sorted(set(grp.host) | {k for k in range(n) if codes[at + k] != 0})
            at += n
            if not redo:
                continue
            host_coef = torch.empty(len(redo), coef.shape[1], dtype=torch.int16, pin_memory=torch.cuda.is_available())
            host_quant = torch.empty(len(redo), 3, 64, dtype=torch.int16, pin_memory=torch.cuda.is_available())

            def decode(j):
                s, h = batch.streams[grp.indices[redo[j]]], _lib.JpegHeader()
                return lib.stp3_jpeg_entropy(s, len(s), host_coef[j].data_ptr(), host_coef.shape[1], host_quant[j].data_ptr(), ctypes.byref(h))

            for j, rc in enumerate(self._map(decode, list(range(len(redo))))):
                if rc != 0:
                    raise _lib.Stp3HipError(f'image {grp.indices[redo[j]]}: stp3_jpeg_entropy failed: {_lib._ERRORS.get(rc, rc)}')
            where = torch.tensor(redo, device=dev)
            coef.index_copy_(0, where, host_coef.to(dev, non_blocking=True))
            quant.index_copy_(0, where, host_quant.to(dev, non_blocking=True))
            on_host += len(redo)
        self.last_stats = {'device': total - on_host, 'host': on_host, 'pillow': len(batch.fallback)}
        return staged

    def _group_workspace(self, grp, dev):
        g, n = grp.geometry, len(grp.indices)
        d = _lib.JpegHuffDims(n, g.width, g.height, g.components, g.hs, g.vs, grp.stride, grp.max_subs, grp.max_segs)
        nbytes = _lib.c_size_t()
        _lib.check(_lib.lib().stp3_jpeg_entropy_workspace_bytes(ctypes.byref(d), self.sync_rounds, ctypes.byref(nbytes)),
                   'stp3_jpeg_entropy_workspace_bytes')
        return torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)

    def entropy_device(self, streams, device):
        """The entropy decode alone, on the device: ([JpegDeviceGroup(geometry, indices, coef, quant)], the prepared batch) -- what
        ``entropy`` returns per group, in device memory.  Streams behind the Pillow fallback are in ``batch.fallback`` only."""
        dev = torch.device(device)
        batch = self.prepare(streams)
        quants = [grp.quant.to(dev, non_blocking=True) for grp in batch.groups]
        if quants and not quants[0].is_cuda or not quants and dev.type != 'cuda':
            raise _lib.Stp3HipError('entropy_device needs a GPU device: there is no fallback path')
        staged = self._entropy_device(batch, dev, quants)
        return [JpegDeviceGroup(grp.geometry, tuple(grp.indices), coef, quant) for grp, coef, quant in staged], batch

    def __call__(self, streams, device, out=None):
        if self.entropy_mode == 'device':
            dev = torch.device(device)
            batch = self.prepare(streams)
            quants = [grp.quant.to(dev, non_blocking=True) for grp in batch.groups]
            if quants and quants[0].is_cuda or not quants and dev.type == 'cuda':
                stacked = len(set(batch.sizes)) == 1
                if out is not None and (not stacked or tuple(out.shape) != (batch.n,) + tuple(batch.sizes[0]) + (3,) or out.dtype != torch.uint8
                                        or out.device.type != dev.type or not out.is_contiguous()):
                    raise ValueError('out must be a contiguous uint8 tensor (N, H, W, 3) on the device of the call')
                return self._reconstruct_staged(batch, self._entropy_device(batch, dev, quants), dev, stacked, out)
        batch = self.entropy(streams)                                           # (a CPU device: the host decoder is the mode)
        self.last_stats = {'device': 0, 'host': batch.n - len(batch.fallback), 'pillow': len(batch.fallback)}
        return self.reconstruct(batch, device, out=out)


# ----------------------------------------------------------------------------------------------------------------------
# PNG images of the CARLA loader: chunks and DEFLATE on host threads (struct + zlib of the standard library), the scanline
# filters in one kernel (csrc/stp3_png.hip: stp3_png_unfilter), byte-exact with Pillow's decode.  Its output is what
# carla.CarlaDecoder reads (carla.load_carla_sample).
# ----------------------------------------------------------------------------------------------------------------------
class PngUnsupported(ValueError):
    """A stream the decoder does not take (bit depth 1 / 2 / 4 / 16, Adam7, APNG, a side above 16 384) met with ``fallback=False``."""


PngGeometry = collections.namedtuple('PngGeometry', 'height width bpp')
PngInfo = collections.namedtuple('PngInfo', 'width height bit_depth colour_type interlace bpp shape idat')
_PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}                              # colour type -> samples per pixel
_PNG_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
_PNG_CHECKED = (b'IHDR', b'PLTE', b'IDAT', b'IEND')                         # the chunks whose CRC is verified
_PNG_MAX_SIDE = 16384
_PNG_PILLOW_BYTE_MODES = ('1', 'L', 'LA', 'P', 'PA', 'RGB', 'RGBA')         # what the fallback can put into a uint8 result


def _png_shape(g):
    return (g.height, g.width) if g.bpp == 1 else (g.height, g.width, g.bpp)


class PngGroup:
    """The images of a ``PngBatch`` that share one geometry: where they sit in the call and their scanlines as inflate wrote
    them, (n, H, 1 + W * bpp) uint8 -- one filter byte, then the filtered bytes, no padding --, pinned where there is a GPU."""

    def __init__(self, geometry, indices, pin):
        self.geometry, self.indices = geometry, list(indices)
        self.rows = torch.empty(len(self.indices), geometry.height, 1 + geometry.width * geometry.bpp, dtype=torch.uint8,
                                pin_memory=pin)


class PngBatch:
    """What ``PngDecoder.inflate`` returns: per geometry a ``PngGroup``; ``fallback`` maps the index of every stream the
    decoder does not take to (reason, its bytes) -- Pillow decodes those on the host; ``shapes``: the decoded shape per image."""

    def __init__(self, n, groups, fallback, shapes):
        self.n, self.groups, self.fallback, self.shapes = n, groups, fallback, shapes

    def layout(self):
        return [(g.geometry, tuple(g.indices)) for g in self.groups]


class PngDecoder:
    """PNG bytes -> uint8 tensors on the GPU, equal to ``np.asarray(PIL.Image.open(...))`` byte for byte: (H, W) for grey and
    palette images (the palette INDICES, Pillow's mode ``P``), (H, W, C) for grey + alpha, RGB and RGBA.

        png = PngDecoder()
        frames = png(list_of_bytes, 'cuda')                 # chunks + inflate on host threads, one kernel per geometry
        x = carla.CarlaDecoder(cfg).images(frames)          # (carla.load_carla_sample does a whole sample)

    Taken: 8-bit samples, not interlaced, colour types 0, 2, 3, 4, 6, sides up to 16 384.  ``workers``: host threads of the
    inflate (zlib releases the interpreter lock), at most ``min(16, os.cpu_count())`` by default.  ``fallback``: a stream of
    another bit depth, an Adam7 stream, an APNG or a larger one is decoded by Pillow on the host and uploaded into the same slot
    of the result; ``fallback=False`` raises ``PngUnsupported`` instead.  That is decided from the headers, before anything is
    inflated.  The result is uint8 throughout: a 1-bit image, which Pillow hands out as booleans, arrives as 0 / 1, and a
    stream Pillow decodes to more than 8 bits per sample (16-bit grey: ``I;16``) raises ``PngUnsupported`` whatever ``fallback``
    is -- it is never cut to 8 bits (Pillow itself reduces 16-bit RGB, RGBA and grey + alpha to 8 bits; those take the fallback).  A corrupt stream always raises ``Stp3HipError`` and is NOT handed to Pillow: a bad signature, a chunk that runs
    past the file, a wrong CRC of IHDR / PLTE / IDAT / IEND (ancillary chunks are skipped unread), a zlib error or a zlib
    stream without its end, an inflated length other than H * (1 + W * bpp), a filter byte above 4.  This is stricter than
    Pillow on purpose: Pillow 12.2 accepts a stream whose data ends one scanline early and pads the missing row; this decoder
    refuses it."""

    def __init__(self, workers=None, fallback=True):
        self.workers = max(1, int(workers)) if workers is not None else min(16, os.cpu_count() or 1)
        self.fallback = fallback
        self._pool = None

    _map = JpegDecoder._map

    # ---- host ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def info(data):
        """The header and the concatenated IDAT payloads of one stream.  Raises ``PngUnsupported`` as soon as the headers say
        so, ``Stp3HipError`` for a malformed stream."""
        data = bytes(data)
        bad = lambda what: _lib.Stp3HipError(f'PNG: {what}')
        if data[:8] != _PNG_SIGNATURE:
            raise bad('bad signature')
        pos, header, idat, ended = 8, None, [], False
        while not ended:
            if pos + 12 > len(data):
                raise bad('truncated: a chunk header runs past the data (no IEND)')
            length, kind = struct.unpack_from('>I4s', data, pos)
            if pos + 12 + length > len(data):
                raise bad(f'truncated: chunk {kind!r} runs past the data')
            body = data[pos + 8:pos + 8 + length]
            if (header is None) != (kind == b'IHDR'):
                raise bad('IHDR must be the first chunk and the only one of its kind')
            if kind in _PNG_CHECKED and zlib.crc32(body, zlib.crc32(kind)) != struct.unpack_from('>I', data, pos + 8 + length)[0]:
                raise bad(f'CRC of chunk {kind.decode()} is wrong')
            if kind == b'IHDR':
                if length != 13:
                    raise bad('IHDR of another length than 13')
                header = struct.unpack('>IIBBBBB', body)
                width, height, depth, colour, compression, filtering, interlace = header
                if (width < 1 or height < 1 or width >= 1 << 31 or height >= 1 << 31 or colour not in _PNG_CHANNELS or
                        depth not in _PNG_DEPTHS[colour] or compression != 0 or filtering != 0 or interlace > 1):
                    raise bad(f'illegal IHDR {header}')
                if depth != 8:
                    raise PngUnsupported(f'{depth}-bit samples')
                if interlace:
                    raise PngUnsupported('Adam7 interlace')
                if max(width, height) > _PNG_MAX_SIDE:
                    raise PngUnsupported('a side above 16 384 pixels')
            elif kind == b'acTL':
                raise PngUnsupported('an animated PNG (acTL)')
            elif kind == b'IDAT':
                idat.append(body)
            elif kind == b'IEND':
                ended = True
            pos += 12 + length
        if not idat:
            raise bad('no IDAT chunk')
        bpp = _PNG_CHANNELS[colour]
        return PngInfo(width, height, depth, colour, interlace, bpp, _png_shape(PngGeometry(height, width, bpp)), b''.join(idat))

    def inflate(self, streams, out=None):
        """Parse and inflate ``streams`` (bytes-like objects) into a ``PngBatch``; ``out``: a batch of the same layout to refill."""
        streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]

        def header(s):
            try:
                return self.info(s)
            except (PngUnsupported, _lib.Stp3HipError) as e:
                return e

        infos, fallback = self._map(header, streams), {}
        for i, f in enumerate(infos):
            if isinstance(f, PngUnsupported):
                if not self.fallback:
                    raise PngUnsupported(f'image {i}: {f}') from None
                fallback[i] = (str(f), streams[i])
                infos[i] = None
            elif isinstance(f, Exception):
                raise _lib.Stp3HipError(f'image {i}: {f}') from None
        order = {}
        for i, f in enumerate(infos):
            if f is not None:
                order.setdefault(PngGeometry(f.height, f.width, f.bpp), []).append(i)
        layout = [(g, tuple(idx)) for g, idx in order.items()]
        if out is not None and out.layout() == layout and out.n == len(streams):
            groups = out.groups
        else:
            if out is not None:
                raise ValueError('the batch to refill has another layout (geometry or order of the images)')
            groups = [PngGroup(g, idx, torch.cuda.is_available()) for g, idx in layout]
        jobs = [(grp, k, i) for grp in groups for k, i in enumerate(grp.indices)]

        def decode(job):
            grp, k, i = job
            g = grp.geometry
            want = g.height * (1 + g.width * g.bpp)
            z = zlib.decompressobj()
            try:
                raw = z.decompress(infos[i].idat, want + 1)                     # (bounded: a stream cannot inflate without end)
            except zlib.error as e:
                return f'zlib: {e}'
            if len(raw) != want:
                return f'{"more than " if len(raw) > want else ""}{len(raw)} bytes inflated, {g.height} scanlines of {1 + g.width * g.bpp} expected'
            if not z.eof:
                return 'the zlib stream has no end (truncated, or its checksum is missing)'
            rows = grp.rows[k].numpy()
            rows.reshape(-1)[:] = np.frombuffer(raw, dtype=np.uint8)
            worst = int(rows[:, 0].max())                                       # H filter bytes through a strided view
            return f'filter type {worst}' if worst > 4 else None

        for (grp, k, i), err in zip(jobs, self._map(decode, jobs)):
            if err is not None:
                raise _lib.Stp3HipError(f'image {i}: PNG: {err}')
        shapes = [f.shape if f is not None else None for f in infos]
        for i, (reason, s) in fallback.items():
            try:
                shapes[i] = self._pillow_shape(s)
            except PngUnsupported as e:
                raise PngUnsupported(f'image {i}: {reason}, and {e}') from None
        return PngBatch(len(streams), groups, fallback, shapes)

    @staticmethod
    def _pillow_open(data):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError('Pillow is not installed: PngDecoder.reference and the fallback for unsupported streams need it') from e
        return Image.open(io.BytesIO(bytes(data)))

    @classmethod
    def _pillow(cls, data):
        return np.asarray(cls._pillow_open(data))

    @classmethod
    def _pillow_bytes(cls, data):
        """Pillow's decode of a stream behind the fallback as uint8 (a 1-bit image, which Pillow hands out as booleans: 0 / 1)."""
        array = cls._pillow(data)
        if array.dtype == np.bool_:
            array = array.astype(np.uint8)
        if array.dtype != np.uint8:
            raise PngUnsupported(f'Pillow decodes it to {array.dtype}, which the uint8 result cannot hold')
        return torch.from_numpy(np.ascontiguousarray(array).copy())

    @classmethod
    def _pillow_shape(cls, data):
        im = cls._pillow_open(data)                                              # (the header only: Pillow decodes lazily)
        if im.mode not in _PNG_PILLOW_BYTE_MODES:
            raise PngUnsupported(f'Pillow decodes it to mode {im.mode!r}, more than 8 bits per sample, which the uint8 result cannot hold')
        bands = len(im.getbands())
        return (im.size[1], im.size[0]) if bands == 1 else (im.size[1], im.size[0], bands)

    def reference(self, streams):
        """Pillow's decode of every stream, ``np.asarray(Image.open(...))``: a list of arrays."""
        return [self._pillow(s) for s in streams]

    # ---- the arithmetic of the kernel, stated with numpy ------------------------------------------------------------
    @staticmethod
    def unfilter_reference(rows, bpp):
        """(n, H, 1 + W * bpp) uint8 scanlines -> (n, H, W * bpp) uint8, the filters of the PNG specification undone row by
        row (what CPU tensors take; a tensor gives a tensor, an array an array).  Sub is a prefix sum per channel and Up an
        addition of the finished row above, both modulo 256; Average and Paeth are recurrences and loop over the bytes."""
        src = rows.numpy() if torch.is_tensor(rows) else np.asarray(rows)
        if src.dtype != np.uint8 or src.ndim != 3 or bpp not in (1, 2, 3, 4) or (src.shape[2] - 1) % bpp or src.shape[2] < 1 + bpp:
            raise ValueError('unfilter_reference: rows must be (n, H, 1 + W * bpp) uint8 with bpp in 1 .. 4')
        n, h, line = src.shape[0], src.shape[1], src.shape[2] - 1
        out = np.zeros((n, h, line), dtype=np.uint8)
        for i in range(n):
            above = np.zeros(line, dtype=np.uint8)
            for r in range(h):
                ft, raw = int(src[i, r, 0]), src[i, r, 1:]
                if ft == 1:
                    cur = np.cumsum(raw.reshape(-1, bpp), axis=0, dtype=np.uint8).reshape(-1)      # (uint8 sums wrap modulo 256)
                elif ft == 2:
                    cur = raw + above
                elif ft in (3, 4):
                    x, b, cur = raw.tolist(), above.tolist(), [0] * line
                    for k in range(line):
                        a = cur[k - bpp] if k >= bpp else 0
                        if ft == 3:
                            pred = (a + b[k]) >> 1
                        else:
                            c = b[k - bpp] if k >= bpp else 0
                            p = a + b[k] - c
                            pa, pb, pc = abs(p - a), abs(p - b[k]), abs(p - c)
                            pred = a if pa <= pb and pa <= pc else b[k] if pb <= pc else c
                        cur[k] = (x[k] + pred) & 255
                    cur = np.array(cur, dtype=np.uint8)
                else:                                                            # None; the kernel treats a type above 4 alike
                    cur = raw
                out[i, r] = cur
                above = out[i, r]
        return torch.from_numpy(out) if torch.is_tensor(rows) else out

    # ---- device -----------------------------------------------------------------------------------------------------
    def unfilter_device(self, geometry, rows, out=None):
        """The kernel alone on tensors that already are on the GPU -- rows (n, H, 1 + W * bpp) uint8 -- into ``out`` (n, H, W)
        (bpp 1) or (n, H, W, bpp) uint8: no copy, no allocation when ``out`` is given (what a captured graph holds)."""
        g = geometry
        n = rows.shape[0] if rows.dim() == 3 else 0
        if rows.dtype != torch.uint8 or tuple(rows.shape) != (n, g.height, 1 + g.width * g.bpp) or n < 1 or not rows.is_contiguous():
            raise ValueError(f'rows must be a contiguous uint8 tensor (n, {g.height}, {1 + g.width * g.bpp})')
        ops._need_gpu(rows)
        shape = (n,) + _png_shape(g)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=rows.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous uint8 tensor of shape {shape}')
        ops._need_gpu(out)
        _lib.check(_lib.lib().stp3_png_unfilter(ops._ptr(rows), n, g.height, g.width, g.bpp, ops._ptr(out), ops._stream()),
                   'stp3_png_unfilter')
        return out

    def unfilter(self, batch, device, out=None):
        """One non-blocking host-to-device copy of the scanlines and one launch per geometry; streams behind the fallback are
        uploaded as Pillow decoded them.  One uint8 tensor (N, H, W[, C]) on ``device`` (``out`` when given) when all images
        have one shape, else a list of tensors in the order of the call."""
        dev = torch.device(device)
        stacked = len(set(batch.shapes)) == 1
        shape = (batch.n,) + tuple(batch.shapes[0]) if stacked else None
        if out is not None and (not stacked or tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device.type != dev.type
                                or not out.is_contiguous()):
            raise ValueError('out must be a contiguous uint8 tensor (N, H, W[, C]) on the device of the call')
        if stacked and out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        images = [None] * batch.n
        for grp in batch.groups:
            first, count = grp.indices[0], len(grp.indices)
            whole = stacked and grp.indices == list(range(first, first + count))
            if dev.type != 'cuda':
                part = self.unfilter_reference(grp.rows, grp.geometry.bpp).view((count,) + _png_shape(grp.geometry))
                if whole:
                    out[first:first + count].copy_(part)
            else:
                rows = grp.rows.to(dev, non_blocking=True)
                part = self.unfilter_device(grp.geometry, rows, out[first:first + count] if whole else None)
            if stacked and not whole:
                out.index_copy_(0, torch.tensor(grp.indices, device=dev), part)
            for k, i in enumerate(grp.indices):
                images[i] = part[k]
        for i, (_, s) in batch.fallback.items():
            host = self._pillow_bytes(s)
            if stacked:
                out[i].copy_(host, non_blocking=True)
            else:
                images[i] = host.to(dev)
        return out if stacked else images

    def __call__(self, streams, device, out=None):
        return self.unfilter(self.inflate(streams), device, out=out)
