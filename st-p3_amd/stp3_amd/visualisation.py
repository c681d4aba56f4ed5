"""The training video -- drop-in for the reference's ``stp3/utils/visualisation.py``: ``visualise_output`` and, under their
names there, the pieces it is made of.

``visualise_output(labels, output, cfg)`` returns ``(1, T, 3, 7 H, 2 W)`` uint8: per frame seven rows of panels (instance,
future flow, segmentation, centerness, offset, pedestrian, planning), labels left and predictions right, every panel showing
cell ``(H - 1 - r, W - 1 - c)`` at pixel ``(r, c)`` inside a one-pixel black border; a panel whose head is disabled is zero.
GPU tensors are painted by ONE call of ``stp3_vis_render`` (csrc/stp3_vis.hip: at most two launches, nothing pulled to the
host, no synchronisation; capturable after one eager call, which uploads the colour tables); CPU tensors take
``visualise_output_reference``, the numpy statement of the same arithmetic in the reference's own dtypes.  Inputs are never
written to (the reference zeroes ``labels['offset']`` / ``['flow']`` in place when they live on the CPU).

Byte for byte the reference's (visualisation.py:208-322) except:
  * the flow-type panels where numpy's float32 ``arctan2`` and the kernel's (float64, rounded to float32) differ by an ulp
    and that moves a byte, by 1 (tests/visualisation_cases.py bounds the share of such bytes);
  * the planning row.  The reference renders it with matplotlib's anti-aliased canvas (``figure.canvas.tostring_rgb``, gone
    from matplotlib 3.10); here it is an integer drawing, ``plot_planning`` below: white, ``hd_map[0] != 0`` (255, 230, 220),
    ``hd_map[1] != 0`` (230, 216, 227) painted later -- the reference's two tints at alpha 0.2 over white --, the ego box
    (118, 185, 0) on the cells ``cost.footprint_cells`` gives, the trajectory (31, 119, 180) as a one-pixel 8-connected line
    between the cells the cost function reads for consecutive points.

The two colour tables are data: ``INSTANCE_COLOURS`` (the 70 colours instance ids cycle through) and ``JET_BYTES``
(``uint8(lut * 255)`` of matplotlib's 256-entry jet map, truncated as the reference truncates it).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check as _check

INSTANCE_COLOURS = np.array([
    0, 0, 0, 255, 179, 0, 128, 62, 117, 255, 104, 0, 166, 189, 215, 193, 0, 32, 206, 162, 98, 129, 112, 102, 0, 125, 52,
    246, 118, 142, 0, 83, 138, 255, 122, 92, 83, 55, 122, 255, 142, 0, 179, 40, 81, 244, 200, 0, 127, 24, 13, 147, 170, 0,
    89, 51, 21, 241, 58, 19, 35, 44, 22, 112, 224, 255, 70, 184, 160, 153, 0, 255, 71, 255, 0, 255, 0, 163, 255, 204, 0,
    0, 255, 235, 255, 0, 235, 255, 0, 122, 255, 245, 0, 10, 190, 212, 214, 255, 0, 0, 204, 255, 20, 0, 255, 255, 255, 0,
    0, 153, 255, 0, 255, 204, 41, 255, 0, 173, 0, 255, 0, 245, 255, 71, 0, 255, 0, 255, 184, 0, 92, 255, 184, 255, 0,
    255, 214, 0, 25, 194, 194, 92, 0, 255, 220, 220, 220, 255, 9, 92, 112, 9, 255, 8, 255, 214, 255, 184, 6, 10, 255, 71,
    255, 41, 10, 7, 255, 255, 224, 255, 8, 102, 8, 255, 255, 61, 6, 255, 194, 7, 0, 255, 20, 255, 8, 41, 255, 5, 153,
    6, 51, 255, 235, 12, 255, 160, 150, 20, 0, 163, 255, 140, 140, 140, 250, 10, 15, 20, 255, 0], dtype=np.uint8).reshape(70, 3)

JET_BYTES = np.frombuffer(bytes.fromhex(
    '00007f00008400008800008d00009100009600009a00009f0000a30000a80000ac0000b10000b60000ba0000bf0000c30000c80000cc0000d10000d5'
    '0000da0000de0000e30000e80000ec0000f10000f50000fa0000fe0000ff0000ff0000ff0000ff0004ff0008ff000cff0010ff0014ff0018ff001cff'
    '0020ff0024ff0028ff002cff0030ff0034ff0038ff003cff0040ff0044ff0048ff004cff0050ff0054ff0058ff005cff0060ff0064ff0068ff006cff'
    '0070ff0074ff0078ff007cff0080ff0084ff0088ff008cff0090ff0094ff0098ff009cff00a0ff00a4ff00a8ff00acff00b0ff00b4ff00b8ff00bcff'
    '00c0ff00c4ff00c8ff00ccff00d0ff00d4ff00d8ff00dcfe00e0fa00e4f702e8f405ecf108f0ed0cf4ea0ff8e712fce415ffe118ffdd1cffda1fffd7'
    '22ffd425ffd029ffcd2cffca2fffc732ffc336ffc039ffbd3cffba3fffb742ffb346ffb049ffad4cffaa4fffa653ffa356ffa059ff9d5cff9a5fff96'
    '63ff9366ff9069ff8d6cff8970ff8673ff8376ff8079ff7d7cff7980ff7683ff7386ff7089ff6c8dff6990ff6693ff6396ff5f9aff5c9dff59a0ff56'
    'a3ff53a6ff4faaff4cadff49b0ff46b3ff42b7ff3fbaff3cbdff39c0ff36c3ff32c7ff2fcaff2ccdff29d0ff25d4ff22d7ff1fdaff1cddff18e0ff15'
    'e4ff12e7ff0feaff0cedff08f1fc05f4f802f7f400faf000feed00ffe900ffe500ffe200ffde00ffda00ffd700ffd300ffcf00ffcb00ffc800ffc400'
    'ffc000ffbd00ffb900ffb500ffb100ffae00ffaa00ffa600ffa300ff9f00ff9b00ff9800ff9400ff9000ff8c00ff8900ff8500ff8100ff7e00ff7a00'
    'ff7600ff7300ff6f00ff6b00ff6700ff6400ff6000ff5c00ff5900ff5500ff5100ff4d00ff4a00ff4600ff4200ff3f00ff3b00ff3700ff3400ff3000'
    'ff2c00ff2800ff2500ff2100ff1d00ff1a00ff1600fe1200fa0f00f50b00f10700ec0300e80000e30000de0000da0000d50000d10000cc0000c80000'
    'c30000bf0000ba0000b60000b10000ac0000a80000a300009f00009a00009600009100008d00008800008400007f0000'), dtype=np.uint8).reshape(256, 3)

SEMANTIC_COLOURS = np.array([[255, 255, 255], [0, 0, 0]], dtype=np.uint8)
HDMAP_COLOURS = ((255, 230, 220), (230, 216, 227))
EGO_COLOUR, TRAJECTORY_COLOUR = (118, 185, 0), (31, 119, 180)
PANEL_ROWS = ('instance', 'flow', 'segmentation', 'centerness', 'offset', 'pedestrian', 'planning')


def make_color_wheel():
    """The 55-entry flow colour wheel, float64 (55, 3) of whole numbers: six ramps between the primary and secondary colours
    (red -> yellow 15 steps, -> green 6, -> cyan 4, -> blue 11, -> magenta 13, -> red 6), ``floor(255 i / n)`` along each."""
    wheel, at = np.zeros((55, 3)), 0
    for n, fixed, moving, rising in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True),
                                     (6, 0, 2, False)):
        ramp = np.floor(255 * np.arange(n) / n)
        wheel[at:at + n, fixed] = 255
        wheel[at:at + n, moving] = ramp if rising else 255 - ramp
        at += n
    return wheel


COLOUR_WHEEL = make_color_wheel()


def _numpy(x):
    """numpy view of a CPU tensor (bf16 widened exactly) or the array itself; never a copy the caller could see written."""
    if isinstance(x, torch.Tensor):
        x = x.detach()
        if x.is_cuda:
            raise TypeError('this routine is the CPU route (numpy / CPU tensors); GPU tensors go through visualise_output')
        return (x.float() if x.dtype == torch.bfloat16 else x).numpy()
    return np.asarray(x)


def compute_color(u, v):
    """Flow colours float64 (H, W, 3) in [0, 1] of float32 components ``u``, ``v`` (H, W), in the reference's mixed precision:
    radius and angle float32, the position between two wheel entries and the blend float64.  NaN vectors come out black.
    Unlike the reference's, this does not write to ``u`` / ``v``."""
    assert u.shape == v.shape
    nan_mask = np.isnan(u) | np.isnan(v)
    u, v = np.where(nan_mask, np.float32(0), u), np.where(nan_mask, np.float32(0), v)
    ncols = len(COLOUR_WHEEL)
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    f_k = (a + 1) / 2 * (ncols - 1) + 1
    k_0 = np.floor(f_k).astype(int)
    k_1 = k_0 + 1
    k_1[k_1 == ncols + 1] = 1
    f = f_k - k_0
    img = np.zeros(u.shape + (3,))
    small = rad <= 1
    for i in range(3):
        col = (1 - f) * (COLOUR_WHEEL[k_0 - 1, i] / 255) + f * (COLOUR_WHEEL[k_1 - 1, i] / 255)
        col = np.where(small, 1 - rad * (1 - col), col * 0.75)
        img[:, :, i] = col * (1 - nan_mask)
    return img


def flow_to_image(flow, autoscale=False):
    """(2, H, W) float32 flow -> (H, W, 3) uint8 (visualisation.py:13-31)."""
    flow = _numpy(flow)
    u, v = flow[0], flow[1]
    if autoscale:
        maxrad = np.max(np.sqrt(u ** 2 + v ** 2))
        u, v = u / (maxrad + np.finfo(float).eps), v / (maxrad + np.finfo(float).eps)
    return np.uint8(compute_color(u, v) * 255)


def _normalise(image):
    lower = np.min(image)
    delta = np.max(image) - lower
    if delta == 0:
        delta = 1
    return (image.astype(np.float32) - lower) / delta


def jet_bytes(image):
    """matplotlib's Colormap.__call__ on a float32 image followed by ``uint8(rgb * 255)``, through ``JET_BYTES``: index
    ``trunc(x * 256)`` in float32 with 256 -> 255, values below 0 the first entry, above the last, NaN black."""
    xa = np.array(image, dtype=np.float32) * np.float32(256)
    xa[xa == 256] = 255
    bad = np.isnan(xa)
    with np.errstate(invalid='ignore'):
        index = np.clip(np.where(bad, 0, xa), 0, 255).astype(int)
    out = JET_BYTES[index]
    out[bad] = 0
    return out


def heatmap_image(image, cmap=None, autoscale=True):
    """A float (H, W) or (1, H, W) image through the jet map, a (2, H, W) one through ``flow_to_image`` -> (H, W, 3) uint8
    (visualisation.py:68-78).  ``cmap``: a matplotlib colour map to use instead of the built-in jet bytes."""
    image = _numpy(image)
    if not issubclass(image.dtype.type, np.floating):
        raise ValueError(f'Expected a ndarray of float type, but got dtype {image.dtype}')
    if not (image.ndim == 2 or (image.ndim == 3 and image.shape[0] in [1, 2])):
        raise ValueError(f'Expected a ndarray of shape [H, W] or [1, H, W] or [2, H, W], but got shape {image.shape}')
    if image.ndim == 3 and image.shape[0] == 2:
        return flow_to_image(image, autoscale=autoscale)
    image = image[0] if image.ndim == 3 else image
    if autoscale:
        image = _normalise(image)
    if cmap is not None:
        return np.uint8(cmap(image)[:, :, :3] * 255)
    return jet_bytes(image)


def make_contour(img, colour=(0, 0, 0), double_line=False):
    """A copy of ``img`` (H, W, 3) with a one-pixel (``double_line``: two-pixel) frame (visualisation.py:167-185)."""
    out = img.copy()
    for k in range(2 if double_line else 1):
        out[[k, -1 - k], :] = colour
        out[:, [k, -1 - k]] = colour
    return out


def generate_instance_colours(instance_map):
    """{instance id: colour} for {instance id: global id}: the palette cycles with the global id."""
    return {i: INSTANCE_COLOURS[g % len(INSTANCE_COLOURS)] for i, g in instance_map.items()}


def plot_instance_map(instance_image, instance_map, instance_colours=None, bg_image=None):
    """(H, W) ids -> (H, W, 3) uint8: white (or ``bg_image``, written in place as in the reference) with every id of
    ``instance_map`` in its colour (visualisation.py:188-205)."""
    instance_image = _numpy(instance_image)
    if instance_colours is None:
        instance_colours = generate_instance_colours(instance_map)
    if instance_image.ndim > 2:
        instance_image = instance_image.reshape(instance_image.shape[-2:])
    plot_image = 255 * np.ones(instance_image.shape + (3,), dtype=np.uint8) if bg_image is None else bg_image
    for key, value in instance_colours.items():
        plot_image[instance_image == key] = value
    return plot_image


_GRIDS = {}


def _grid(cfg):
    """(dx (2,), bx (2,) float32 numpy: rows then columns; ego cells (K, 2) int64) of a configuration, cached by value."""
    key = (tuple(cfg.LIFT.X_BOUND), tuple(cfg.LIFT.Y_BOUND), tuple(cfg.LIFT.Z_BOUND), cfg.EGO.WIDTH, cfg.EGO.HEIGHT)
    if key not in _GRIDS:
        from .cost import BaseCost
        base = BaseCost(cfg)
        _GRIDS[key] = (base.dx.detach().numpy().copy(), base.bx.detach().numpy().copy(), base.footprint(0))
    return _GRIDS[key]


def trajectory_cells(traj, cfg, shape):
    """(n, 2) int64 (row, column): the cell ``cost.BaseCost.discretize`` reads for every point of ``traj`` (n, >= 2) metres
    after ``Cost_Function.forward`` has mirrored x -- float32 arithmetic, truncation, clipped to ``shape``."""
    dx, bx, _ = _grid(cfg)
    traj = _numpy(traj).astype(np.float32)
    with np.errstate(invalid='ignore'):
        rows = np.nan_to_num(np.clip((traj[:, 1] - bx[0]) / dx[0], 0, shape[0] - 1), nan=0.0)
        cols = np.nan_to_num(np.clip((-traj[:, 0] - bx[1]) / dx[1], 0, shape[1] - 1), nan=0.0)
    return np.stack([rows.astype(np.int64), cols.astype(np.int64)], axis=1)


def line_cells(r0, c0, r1, c1):
    """The one-pixel 8-connected line between two cells: (r0 + round(i dr / n), c0 + round(i dc / n)), i = 0..n,
    n = max(|dr|, |dc|), halves rounded up."""
    dr, dc = r1 - r0, c1 - c0
    n = max(abs(dr), abs(dc))
    if n == 0:
        return [(r0, c0)]
    return [(r0 + (2 * i * dr + n) // (2 * n), c0 + (2 * i * dc + n) // (2 * n)) for i in range(n + 1)]


def plot_planning(hd_map, traj, cfg):
    """The planning panel (H, W, 3) uint8 as it is shown (cell (H - 1 - r, W - 1 - c) at pixel (r, c)), without its border:
    this project's integer drawing, see the module text.  ``hd_map`` (2, H, W): non-zero marks the lane dividers and the
    drivable area; ``traj`` (n, >= 2) metres."""
    hd_map = _numpy(hd_map)
    h, w = hd_map.shape[-2:]
    image = np.full((h, w, 3), 255, dtype=np.uint8)
    for channel, colour in zip(hd_map, HDMAP_COLOURS):
        image[channel != 0] = colour
    ego = _grid(cfg)[2]
    ego = ego[(ego[:, 0] < h) & (ego[:, 1] < w)]
    image[ego[:, 0], ego[:, 1]] = EGO_COLOUR
    cells = [tuple(int(v) for v in rc) for rc in trajectory_cells(traj, cfg, (h, w))]
    for (r0, c0), (r1, c1) in zip(cells[:1] + cells[:-1], cells):
        for r, c in line_cells(r0, c0, r1, c1):
            image[r, c] = TRAJECTORY_COLOUR
    return image[::-1, ::-1]


def _predicted_hdmap(logits):
    """(4, H, W) logits -> (2, H, W): the argmax of each channel pair."""
    return np.stack([logits[1] > logits[0], logits[3] > logits[2]]).astype(np.int64)


def _flags(cfg):
    return (cfg.INSTANCE_SEG.ENABLED, cfg.INSTANCE_FLOW.ENABLED, cfg.SEMANTIC_SEG.PEDESTRIAN.ENABLED,
            cfg.SEMANTIC_SEG.HDMAP.ENABLED)


def _sources(labels, output, cfg, sample, consistent_instance_seg):
    """The tensors of ``sample`` that the enabled panels read, each (T, C, H, W) -- trajectories (n, 2), hd maps (C, H, W) --
    as {name: (labels' tensor, predictions' tensor)}, after their shapes and dtypes have been checked."""
    instance, flow, pedestrian, hdmap = _flags(cfg)
    seg = labels['segmentation']
    if seg.ndim != 5 or seg.shape[2] != 1:
        raise ValueError(f"labels['segmentation']: expected (B, T, 1, H, W), got {tuple(seg.shape)}")
    B, T, _, H, W = seg.shape
    if not 0 <= sample < B:
        raise ValueError(f'sample {sample} of a batch of {B}')
    if H < 3 or W < 3:
        raise ValueError(f'maps of {H} x {W} cells: a panel needs at least 3 x 3')
    pairs = {'segmentation': (seg, output['segmentation'])}
    shapes = {'segmentation': ((T, 1, H, W), (T, 2, H, W))}
    if pedestrian:
        pairs['pedestrian'] = (labels['pedestrian'], output['pedestrian'])
        shapes['pedestrian'] = shapes['segmentation']
    if instance:
        if consistent_instance_seg is None:
            from .instance import predict_instance_segmentation_and_trajectories
            consistent_instance_seg = predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False)
        pairs['instance'] = (labels['instance'].unsqueeze(2), consistent_instance_seg.unsqueeze(2))
        pairs['centerness'] = (labels['centerness'], output['instance_center'])
        pairs['offset'] = (labels['offset'], output['instance_offset'])
        shapes.update(instance=((T, 1, H, W),) * 2, centerness=((T, 1, H, W),) * 2, offset=((T, 2, H, W),) * 2)
    if flow:
        pairs['flow'] = (labels['flow'], output['instance_flow'])
        shapes['flow'] = ((T, 2, H, W),) * 2
    out = {}
    for name, pair in pairs.items():
        picked = []
        for side, (x, shape) in enumerate(zip(pair, shapes[name])):
            x = x.detach()[sample]
            ids = name == 'instance' or (side == 0 and name in ('segmentation', 'pedestrian'))
            if tuple(x.shape) != shape or x.device != seg.device:
                raise ValueError(f"{name} of the {'predictions' if side else 'labels'}: expected {shape} on {seg.device}, got "
                                 f'{tuple(x.shape)} on {x.device}')
            if x.dtype not in ((torch.int64,) if ids else (torch.float32, torch.bfloat16)):
                raise ValueError(f"{name} of the {'predictions' if side else 'labels'}: unsupported dtype {x.dtype}")
            picked.append(x)
        out[name] = tuple(picked)
    hd = [labels['hdmap'].detach()[sample]]
    traj = [labels['gt_trajectory'].detach()[sample][:, :2].float()]
    if hdmap:
        hd.append(output['hdmap'].detach()[sample])
        traj.append(output['selected_traj'].detach()[sample][:, :2].float())
        if hd[1].dtype not in (torch.float32, torch.bfloat16) or tuple(hd[1].shape) != (4, H, W):
            raise ValueError(f"output['hdmap']: expected float32 | bfloat16 (B, 4, {H}, {W}), got {hd[1].dtype} {tuple(hd[1].shape)}")
    if tuple(hd[0].shape) != (2, H, W):
        raise ValueError(f"labels['hdmap']: expected (B, 2, {H}, {W}), got {tuple(labels['hdmap'].shape)}")
    hd[0] = hd[0].long()
    out['hdmap'], out['trajectory'] = tuple(hd), tuple(traj)
    return out, (T, H, W)


def visualise_output_reference(labels, output, cfg, sample=0, consistent_instance_seg=None):
    """``visualise_output`` in numpy, on CPU tensors: the reference's statements in the reference's dtypes."""
    src, (T, H, W) = _sources(labels, output, cfg, sample, consistent_instance_seg)
    instance, flow, pedestrian, hdmap = _flags(cfg)
    src = {k: tuple(_numpy(x) for x in v) for k, v in src.items()}
    blank = np.zeros((H, W, 3), dtype=np.uint8)
    classes = (src['segmentation'][0][:, 0], (src['segmentation'][1][:, 1] > src['segmentation'][1][:, 0]).astype(np.int64))
    video = []
    for t in range(T):
        columns = []
        for side in range(2):
            seg = classes[side][t]
            panels = dict.fromkeys(PANEL_ROWS, blank)
            panels['segmentation'] = make_contour(SEMANTIC_COLOURS[seg[::-1, ::-1]])
            if pedestrian:
                ped = src['pedestrian'][side][t]
                ped = ped[0] if side == 0 else (ped[1] > ped[0]).astype(np.int64)
                panels['pedestrian'] = make_contour(SEMANTIC_COLOURS[ped[::-1, ::-1]])
            if instance:
                ids = src['instance'][side][t, 0]
                shown = np.unique(ids)[1:]
                panels['instance'] = make_contour(plot_instance_map(ids, dict(zip(shown, shown)))[::-1, ::-1])
                panels['centerness'] = make_contour(heatmap_image(src['centerness'][side][t, 0])[::-1, ::-1])
                masked = np.where(seg != 1, np.float32(0), src['offset'][side][t].astype(np.float32))
                panels['offset'] = make_contour(flow_to_image(masked)[::-1, ::-1])
            if flow:
                masked = np.where(seg != 1, np.float32(0), src['flow'][side][t].astype(np.float32))
                panels['flow'] = make_contour(flow_to_image(masked)[::-1, ::-1])
            if side == 0 or hdmap:
                hd = src['hdmap'][side] if side == 0 else _predicted_hdmap(src['hdmap'][side])
                panels['planning'] = make_contour(plot_planning(hd, src['trajectory'][side], cfg))
            columns.append(np.concatenate([panels[k] for k in PANEL_ROWS], axis=0))
        video.append(np.concatenate(columns, axis=1).transpose(2, 0, 1))
    return torch.from_numpy(np.stack(video)[None].copy())


_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.int64: _lib.VIS_DTYPE_I64}
_TABLES = {}


def _tables(device, cfg):
    """The colour tables and the ego cells of ``cfg`` in device memory (uploaded once per device and grid)."""
    key = (str(device), id(_grid(cfg)[2]))
    if key not in _TABLES:
        wheel = COLOUR_WHEEL.astype(np.uint8)
        ego = _grid(cfg)[2].astype(np.int32)
        _TABLES[key] = tuple(torch.tensor(a, device=device) for a in (INSTANCE_COLOURS, JET_BYTES, wheel, ego))
    return _TABLES[key]


def _fill_map(m, x):
    m.ptr = x.data_ptr()
    m.stride_t, m.stride_c, m.stride_h, m.stride_w = x.stride()
    m.dtype = _DTYPES[x.dtype]


def _render(src, dims, cfg, out):
    """One call of ``stp3_vis_render`` on the checked sources of ``_sources``."""
    from . import ops
    T, H, W = dims
    instance, flow, pedestrian, hdmap = _flags(cfg)
    device = src['segmentation'][0].device
    palette, jet, wheel, ego = _tables(device, cfg)
    dx, bx, _ = _grid(cfg)
    d = _lib.VisDesc()
    d.T, d.H, d.W = T, H, W
    d.panels = (_lib.VIS_INSTANCE * bool(instance) | _lib.VIS_FLOW * bool(flow) | _lib.VIS_PEDESTRIAN * bool(pedestrian) |
                _lib.VIS_PLAN_LABELS | _lib.VIS_PLAN_PRED * bool(hdmap))
    for field, name in (('seg', 'segmentation'), ('ped', 'pedestrian'), ('inst', 'instance'), ('center', 'centerness'),
                        ('offset', 'offset'), ('flow', 'flow')):
        if name in src:
            for side in range(2):
                _fill_map(getattr(d, field)[side], src[name][side])
    for side, (hd, traj) in enumerate(zip(src['hdmap'], src['trajectory'])):
        p = d.plan[side]
        p.hdmap, p.hd_dtype = hd.data_ptr(), _DTYPES[hd.dtype]
        p.hd_stride_c, p.hd_stride_h, p.hd_stride_w = hd.stride()
        p.traj, p.n_points = traj.data_ptr(), traj.shape[0]
        p.traj_stride_p, p.traj_stride_c = traj.stride()
    d.ego_cells, d.n_ego = ego.data_ptr(), ego.shape[0]
    d.palette, d.jet, d.wheel = palette.data_ptr(), jet.data_ptr(), wheel.data_ptr()
    d.dx0, d.dx1, d.bx0, d.bx1 = float(dx[0]), float(dx[1]), float(bx[0]), float(bx[1])
    lib = _lib.lib()
    nbytes = ctypes.c_size_t()
    _check(lib.stp3_vis_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)), 'stp3_vis_workspace_bytes')
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    _check(lib.stp3_vis_render(ctypes.byref(d), ops._ptr(out), ops._ptr(workspace), ops._stream()), 'stp3_vis_render')
    return out


def visualise_output(labels, output, cfg, sample=0, consistent_instance_seg=None, out=None):
    """The video ``(1, T, 3, 7 H, 2 W)`` uint8 of sample ``sample`` on the inputs' device (visualisation.py:208-322; the
    reference shows sample 0).  ``consistent_instance_seg`` (B, T, H, W) int64: the instance ids of the predictions, by default
    ``instance.predict_instance_segmentation_and_trajectories(output, compute_matched_centers=False)``; ``out``: a contiguous
    tensor to paint into (GPU route)."""
    if not labels['segmentation'].is_cuda:
        video = visualise_output_reference(labels, output, cfg, sample, consistent_instance_seg)
        return video if out is None else out.copy_(video)
    src, (T, H, W) = _sources(labels, output, cfg, sample, consistent_instance_seg)
    shape, device = (1, T, 3, 7 * H, 2 * W), labels['segmentation'].device
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError(f'out: expected a contiguous uint8 {shape} tensor on {device}, got {tuple(out.shape)} {out.dtype}')
    return _render(src, (T, H, W), cfg, out)
