"""Cases, fixture access and the comparison rule of the training video (stp3_amd/visualisation.py, csrc/stp3_vis.hip), shared by
scripts/make_golden_visualisation.py, tests/test_visualisation_cpu.py and tests/test_visualisation_gpu.py.

Cases (tests/golden/visualisation.npz holds their inputs and the reference's videos, planning row zeroed):
  full   every head on, 24 x 22 cells (not square, 2 W = 44 is a multiple of 4 but W is not), T = 3, B = 2, samples 0 and 1.
         Instance ids 1, 3, 5 and 74 (74 mod 70 = 4); frame (0, 2) of the labels has no background cell, so its smallest id (1) is
         the one left white; the label centre map of frame (0, 1) is constant; offset and flow vectors lie on both sides of
         |v| = 1; two cells of the predicted segmentation have equal logits (class 0)
  off    instance, flow, pedestrian and hd-map heads off (their tensors are not even in the dictionaries), T = 2, B = 1
  t1     T = 1, B = 1, 10 x 9 cells: W is odd, the video's rows are not word aligned
Every float input is representable in bfloat16, so the same golden video holds for float32 and bfloat16 head outputs.

Comparison rule (``compare``).  Every byte equals the reference's, except
  * in the two flow-type rows (future flow, offset): a byte is FRAGILE when moving the float32 angle atan2(-v, -u) by up to
    +-2 ulp changes it in the numpy restatement ``flow_bytes`` below (numpy's float32 arctan2 and the kernel's float64 atan2
    rounded to float32 may differ in the last place; everything else in that chain is exactly rounded).  Fragile bytes may
    differ by 1, all others must be equal, and fragile bytes are fewer than 2 % of each flow panel;
  * the planning row, which the reference draws with matplotlib (not reproducible, not runnable on a current matplotlib): it
    is compared with ``planning_expected``, an integer statement of this project's drawing, not with the file.
"""
import functools
import os
from fractions import Fraction

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'visualisation.npz')
ROWS = ('instance', 'flow', 'segmentation', 'centerness', 'offset', 'pedestrian', 'planning')
FRAGILE_ULPS, FRAGILE_SHARE = 2, 0.02

# blocks: (id, rows, columns, first frame); ``fill``: ((sample, frame), id) gives the background of one label frame an id
CASES = {
    'full': dict(B=2, T=3, H=24, W=22, samples=(0, 1), instance=True, flow=True, pedestrian=True, hdmap=True, seed=7,
                 blocks=((3, (3, 8), (4, 9), 0), (74, (12, 18), (10, 15), 0), (1, (15, 20), (2, 6), 1)), fill=((0, 2), 5),
                 constant_centre=(0, 1), ties=((0, 0, 4, 5), (1, 2, 13, 11))),
    'off': dict(B=1, T=2, H=24, W=22, samples=(0,), instance=False, flow=False, pedestrian=False, hdmap=False, seed=8,
                blocks=((3, (3, 8), (4, 9), 0), (2, (12, 18), (10, 15), 0)), fill=None, constant_centre=None, ties=()),
    't1': dict(B=1, T=1, H=10, W=9, samples=(0,), instance=True, flow=True, pedestrian=True, hdmap=True, seed=9,
               blocks=((2, (1, 4), (1, 4), 0), (74, (5, 9), (4, 8), 0)), fill=None, constant_centre=None, ties=()),
}
TRAJECTORIES = {                                   # (x, y) metres; the last label point leaves the map and is clipped
    'gt': ((0.0, 0.0), (0.4, 1.3), (1.1, 2.9), (2.7, 4.1), (9.0, 8.0)),
    'selected': ((0.0, 0.0), (-0.3, 0.9), (-2.2, 1.4), (-2.4, 4.6), (0.6, 3.3)),
}


def cfg_of(name):
    """The configuration of a case: the heads' switches and a BEV grid of H x W cells of 0.5 m."""
    from stp3_amd.config import get_cfg
    c = CASES[name]
    return get_cfg(cfg_dict={'LIFT': {'X_BOUND': [-c['H'] / 4, c['H'] / 4, 0.5], 'Y_BOUND': [-c['W'] / 4, c['W'] / 4, 0.5]},
                             'INSTANCE_SEG': {'ENABLED': c['instance']}, 'INSTANCE_FLOW': {'ENABLED': c['flow']},
                             'SEMANTIC_SEG': {'PEDESTRIAN': {'ENABLED': c['pedestrian']}, 'HDMAP': {'ENABLED': c['hdmap']}}})


def _q(x):
    return x.bfloat16().float()


def build(name):
    """(labels, output): CPU tensors of a case, float32 heads with bfloat16-representable values."""
    c = CASES[name]
    B, T, H, W = c['B'], c['T'], c['H'], c['W']
    g = torch.Generator().manual_seed(c['seed'])
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    inst = torch.zeros(B, T, H, W, dtype=torch.int64)
    centre = _q(rand(B, T, 1, H, W) * 0.05)
    offset = _q(randn(B, T, 2, H, W))
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    for ident, (r0, r1), (c0, c1), first in c['blocks']:
        inst[:, first:, r0:r1, c0:c1] = ident
        cr, cc = (r0 + r1) // 2, (c0 + c1) // 2
        centre[:, first:, 0, cr, cc] = _q(torch.tensor(0.9))
        offset[:, first:, 0, r0:r1, c0:c1] = (cr - rows[r0:r1, c0:c1]).float() + 0.125       # (an eighth off the centre: the
        offset[:, first:, 1, r0:r1, c0:c1] = (cc - cols[r0:r1, c0:c1]).float() - 0.125       # centre cell's own vector is short)
    foreground = inst > 0
    margin = _q(0.5 + rand(B, T, H, W))
    seg_logits = torch.stack([torch.where(foreground, -margin, margin), torch.where(foreground, margin, -margin)], dim=2)
    for b, t, r, col in c['ties']:
        seg_logits[b, t, :, r, col] = 0.25
    label_inst = inst.clone()
    if c['fill'] is not None:
        (b, t), ident = c['fill']
        label_inst[b, t][label_inst[b, t] == 0] = ident
    labels = {'segmentation': (label_inst > 0).long().unsqueeze(2),
              'hdmap': (rand(B, 2, H, W) > 0.7).long(),
              'gt_trajectory': torch.cat([torch.tensor(TRAJECTORIES['gt']), torch.zeros(len(TRAJECTORIES['gt']), 1)], dim=1).repeat(B, 1, 1)}
    output = {'segmentation': seg_logits}
    if c['pedestrian']:
        labels['pedestrian'] = (rand(B, T, 1, H, W) > 0.9).long()
        output['pedestrian'] = _q(randn(B, T, 2, H, W))
    if c['instance']:
        labels['instance'] = label_inst
        labels['centerness'] = _q(rand(B, T, 1, H, W))
        if c['constant_centre'] is not None:
            labels['centerness'][c['constant_centre']] = 0.5
        labels['offset'] = _q(randn(B, T, 2, H, W) * 1.5)
        output['instance_center'] = centre
        output['instance_offset'] = offset
    if c['flow']:
        labels['flow'] = _q(randn(B, T, 2, H, W) * 0.7)
        output['instance_flow'] = _q(randn(B, T, 2, H, W) * 0.6)
    if c['hdmap']:
        output['hdmap'] = _q(randn(B, 4, H, W))
        output['selected_traj'] = torch.cat([torch.tensor(TRAJECTORIES['selected']), torch.zeros(len(TRAJECTORIES['selected']), 1)],
                                            dim=1).repeat(B, 1, 1)
    return labels, output


# ---- the fixture -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def stored(name, device='cpu', head_dtype=torch.float32):
    """(labels, output, consistent ids or None) of a case from the fixture; float head OUTPUTS in ``head_dtype``."""
    g = fixture()
    groups = {'labels': {}, 'output': {}}
    for key, value in g.items():
        parts = key.split('/')
        if parts[0] == name and parts[1] in groups:
            x = torch.from_numpy(value)
            x = x.long() if x.dtype in (torch.int16, torch.uint8) else x
            if parts[1] == 'output' and x.is_floating_point() and parts[2] != 'selected_traj':
                x = x.to(head_dtype)
            groups[parts[1]][parts[2]] = x.to(device)
    consistent = g.get(f'{name}/consistent')
    consistent = None if consistent is None else torch.from_numpy(consistent).long().to(device)
    return groups['labels'], groups['output'], consistent


def golden_video(name, sample):
    return fixture()[f'{name}/video'][CASES[name]['samples'].index(sample)]


# ---- the comparison rule ---------------------------------------------------------------------------------------------------
def panel(video, t, row, side, H, W):
    """(3, H, W) view of one panel of a (1, T, 3, 7 H, 2 W) video."""
    r = ROWS.index(row) if isinstance(row, str) else row
    return video[0, t, :, r * H:(r + 1) * H, side * W:(side + 1) * W]


def wheel():
    from stp3_amd.visualisation import COLOUR_WHEEL
    return COLOUR_WHEEL


def flow_bytes(u, v, shift=0):
    """(H, W, 3) uint8 colours of float32 flow components, the angle moved by ``shift`` ulps: the reference's compute_color
    (visualisation.py:81-113) restated -- float32 radius and angle, float64 blend."""
    u, v = u.astype(np.float32), v.astype(np.float32)
    rad = np.sqrt(u * u + v * v)
    angle = np.arctan2(-v, -u)
    for _ in range(abs(shift)):
        angle = np.nextafter(angle, np.float32(np.inf if shift > 0 else -np.inf))
    fk = (angle / np.float32(np.pi) + np.float32(1)) / np.float32(2) * np.float32(54) + np.float32(1)
    assert rad.dtype == fk.dtype == np.float32
    k0 = np.clip(np.floor(fk).astype(np.int64), 1, 55)
    k1 = np.where(k0 == 55, 1, k0 + 1)
    f = fk.astype(np.float64) - k0
    table = wheel()
    col = (1 - f)[..., None] * (table[k0 - 1] / 255) + f[..., None] * (table[k1 - 1] / 255)
    col = np.where((rad <= 1)[..., None], 1 - rad.astype(np.float64)[..., None] * (1 - col), col * 0.75)
    return np.uint8(col * 255)


def fragile_bytes(u, v):
    """(3, H, W) bool, in panel orientation: the bytes of a flow panel that an angle +-FRAGILE_ULPS away would change."""
    base = flow_bytes(u, v)
    moved = np.zeros(base.shape, dtype=bool)
    for shift in range(-FRAGILE_ULPS, FRAGILE_ULPS + 1):
        moved |= flow_bytes(u, v, shift) != base
    return moved[::-1, ::-1].transpose(2, 0, 1)


def classes(labels, output, sample):
    """(labels' classes, predicted classes) (T, H, W) bool of the vehicle segmentation."""
    logits = output['segmentation'][sample].float().cpu().numpy()
    return labels['segmentation'][sample, :, 0].cpu().numpy() == 1, logits[:, 1] > logits[:, 0]


def flow_sources(labels, output, sample, instance=True, flow=True):
    """{(row, side): (T, 2, H, W) float32 masked vectors} of the enabled flow-type panels."""
    keys = ([('offset', 'offset', 'instance_offset')] if instance else []) + ([('flow', 'flow', 'instance_flow')] if flow else [])
    seg = classes(labels, output, sample)
    out = {}
    for row, lk, ok in keys:
        for side, x in enumerate((labels[lk], output[ok])):
            x = x[sample].float().cpu().numpy()
            out[(row, side)] = np.where(seg[side][:, None], x, np.float32(0))
    return out


def planning_expected(hd, traj, cfg, H, W):
    """(3, H, W) uint8: the planning panel as an integer statement.  ``hd`` (2, H, W) integers, ``traj`` (n, >= 2) metres."""
    from stp3_amd.cost import BaseCost
    base = BaseCost(cfg)
    dx, bx = base.dx.detach().numpy(), base.bx.detach().numpy()
    image = np.full((H, W, 3), 255, dtype=np.uint8)
    image[hd[0] != 0] = (255, 230, 220)
    image[hd[1] != 0] = (230, 216, 227)
    for r, c in base.footprint(0):
        if r < H and c < W:
            image[r, c] = (118, 185, 0)
    cells = []
    for x, y in np.asarray(traj, dtype=np.float32)[:, :2]:
        r = int((y - bx[0]) / dx[0])                                 # float32 arithmetic, truncation: cost.BaseCost.discretize
        c = int((-x - bx[1]) / dx[1])                                # (Cost_Function.forward mirrors x first)
        cells.append((min(max(r, 0), H - 1), min(max(c, 0), W - 1)))
    for (r0, c0), (r1, c1) in zip(cells[:1] + cells[:-1], cells):
        n = max(abs(r1 - r0), abs(c1 - c0))
        for i in range(n + 1):
            step = Fraction(i, n) if n else Fraction(0)
            image[r0 + int(np.floor(step * (r1 - r0) + Fraction(1, 2))), c0 + int(np.floor(step * (c1 - c0) + Fraction(1, 2)))] = (31, 119, 180)
    image = image[::-1, ::-1].copy()
    image[[0, -1], :] = 0
    image[:, [0, -1]] = 0
    return image.transpose(2, 0, 1)


def planning_panels(labels, output, sample, cfg):
    """The two expected planning panels (labels, predictions); the predictions' is blank without the hd-map head."""
    H, W = labels['hdmap'].shape[-2:]
    out = [planning_expected(labels['hdmap'][sample].cpu().numpy(), labels['gt_trajectory'][sample].float().cpu().numpy(), cfg, H, W)]
    if cfg.SEMANTIC_SEG.HDMAP.ENABLED:
        logits = output['hdmap'][sample].float().cpu().numpy()
        hd = np.stack([logits[1] > logits[0], logits[3] > logits[2]]).astype(np.int64)
        out.append(planning_expected(hd, output['selected_traj'][sample].float().cpu().numpy(), cfg, H, W))
    else:
        out.append(np.zeros((3, H, W), dtype=np.uint8))
    return out


def compare_videos(video, want, sources, plans, what):
    """Assert the rule of the module text on ``video`` against ``want`` (1, T, 3, 7 H, 2 W) uint8 (numpy).  ``sources``: the
    masked vectors of the flow-type panels (``flow_sources``); ``plans``: the expected planning panels, or None to compare that
    row with ``want`` like every other.  Returns the largest share of fragile bytes over the flow panels."""
    video = np.asarray(video)
    assert video.dtype == np.uint8 and video.shape == want.shape and video.ndim == 5, (what, video.shape, video.dtype)
    T, H, W = video.shape[1], video.shape[3] // 7, video.shape[4] // 2
    worst = 0.0
    for t in range(T):
        for row in ROWS:
            for side in range(2):
                got, ref = panel(video, t, row, side, H, W), panel(want, t, row, side, H, W)
                where = f'{what}: frame {t} {row} panel, {"predictions" if side else "labels"}'
                if row == 'planning' and plans is not None:
                    assert np.array_equal(got, plans[side]), f'{where}: {int((got != plans[side]).sum())} bytes differ from the drawing'
                elif (row, side) in sources:
                    u, v = sources[(row, side)][t]
                    fragile = fragile_bytes(u, v)
                    share = fragile.mean()
                    worst = max(worst, share)
                    assert share < FRAGILE_SHARE, f'{where}: {share:.2%} of the bytes are fragile'
                    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
                    assert diff[~fragile].max(initial=0) == 0, f'{where}: {int((diff[~fragile] > 0).sum())} stable bytes differ'
                    assert diff[fragile].max(initial=0) <= 1, f'{where}: a fragile byte differs by {int(diff[fragile].max())}'
                else:
                    assert np.array_equal(got, ref), f'{where}: {int((got != ref).sum())} bytes differ'
    return worst


def compare(name, video, sample, labels, output, what):
    """``compare_videos`` of a fixture case against the reference's video; the planning row against ``planning_expected``."""
    c = CASES[name]
    return compare_videos(video, golden_video(name, sample), flow_sources(labels, output, sample, c['instance'], c['flow']),
                          planning_panels(labels, output, sample, cfg_of(name)), f'{what}: {name} sample {sample}')


def random_case(B, T, H, W, seed, device='cpu'):
    """(labels, output, consistent ids, cfg) of random maps at the default 0.5 m grid, every head on: what the kernel route is
    compared with the CPU route on at sizes the fixture does not hold."""
    from stp3_amd.config import get_cfg
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    ids = lambda: (torch.randint(0, 150, (B, T, H // 8 + 1, W // 8 + 1), generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)[..., :H, :W]
                   * (rand(B, T, H, W) > 0.5)).contiguous()
    inst = ids()
    traj = lambda: torch.cat([(rand(B, 7, 2) - 0.5) * torch.tensor([30.0, 90.0]), torch.zeros(B, 7, 1)], dim=2)
    labels = {'segmentation': (inst > 0).long().unsqueeze(2), 'pedestrian': (rand(B, T, 1, H, W) > 0.9).long(), 'instance': inst,
              'centerness': rand(B, T, 1, H, W), 'offset': randn(B, T, 2, H, W) * 2, 'flow': randn(B, T, 2, H, W),
              'hdmap': (rand(B, 2, H, W) > 0.6).long(), 'gt_trajectory': traj()}
    output = {'segmentation': randn(B, T, 2, H, W), 'pedestrian': randn(B, T, 2, H, W), 'instance_center': rand(B, T, 1, H, W),
              'instance_offset': randn(B, T, 2, H, W) * 2, 'instance_flow': randn(B, T, 2, H, W), 'hdmap': randn(B, 4, H, W),
              'selected_traj': traj()}
    cfg = get_cfg(cfg_dict={'LIFT': {'X_BOUND': [-H / 4, H / 4, 0.5], 'Y_BOUND': [-W / 4, W / 4, 0.5]}})
    move = lambda d: {k: v.to(device) for k, v in d.items()}
    return move(labels), move(output), ids().to(device), cfg
