"""TEST INFRASTRUCTURE -- the deterministic inputs of the instance post-processing fixture (tests/golden/instance.npz):
scripts/make_golden_instance.py (which runs the reference on them) and tests/test_instance_*.py build the SAME arrays from
``numpy.random.RandomState(seed)``, whose stream is frozen across numpy versions; the fixture stores a sha256 of every array
so that a drifting builder fails loudly.  numpy only.

A scene: rectangular vehicles that move with a constant velocity over S frames (integer centre positions), some appearing
late (three at the same step, so that the order of fresh ids matters), some leaving, one "ghost" per sample (in the heads,
not in the ground truth: false positives), one "missed" (ground truth only: false negatives), one "jumping" vehicle whose
flow says 0 while it moves 6 pixels a frame (never re-identified: an inconsistent id at every step).  Heads: Gaussian
centerness around every centre, offsets pointing at the centre and flow pointing at the next centre inside the boxes, with
mild noise, two-class segmentation logits with rare background speckle."""
import hashlib

import numpy as np

BIG = dict(H=200, W=200)
SMALL = dict(H=40, W=56, n=4, small=True, B=1, S=4)
CASES = {
    'clean': dict(seed=11, B=4, S=7, n=16, **BIG),
    'integer': dict(seed=12, B=2, S=5, n=14, integer=True, **BIG),
    'crowded': dict(seed=13, B=1, S=4, n=26, crowded=True, **BIG),
    'nonsquare': dict(seed=14, B=2, S=4, H=48, W=72, n=5, small=True),
    'deg_mid_empty': dict(seed=15, empty=((0, 2),), **SMALL),
    'deg_first_empty': dict(seed=16, empty=((0, 0),), **SMALL),
    'deg_all_foreground': dict(seed=17, all_foreground=((0, 1),), **SMALL),
    'deg_no_flow': dict(seed=18, no_flow=True, **SMALL),
    'deg_not_consistent': dict(seed=19, make_consistent=False, **SMALL),
    'deg_matched_centers': dict(seed=20, matched=True, **SMALL),
}
NON_INTEGER = [k for k, v in CASES.items() if not v.get('integer')]
HOST_KERNEL_CASES = ['nonsquare'] + [k for k in CASES if k.startswith('deg_')]        # + sample 0 of 'clean' (200 x 200)


def _place(rs, p, S, H, W):
    """Vehicles (dicts) whose boxes, grown by a margin, never overlap in any frame and stay inside the image."""
    small = p.get('small', False)
    placed = []
    for k in range(p['n']):
        for _ in range(2000):
            hh, hw = (int(rs.randint(1, 3)), int(rs.randint(2, 4))) if small else (int(rs.randint(2, 4)), int(rs.randint(4, 7)))
            jumping = k == 7 % p['n'] and not small
            v = np.array([0.0, 6.0]) if jumping else rs.uniform(-2.5, 2.5, size=2) * (0.5 if small else 1.0)
            pos0 = np.array([rs.uniform(hh + 2, H - hh - 3), rs.uniform(hw + 2, W - hw - 3)])
            cen = np.rint(pos0[None] + v[None] * np.arange(S + 1)[:, None]).astype(np.int64)      # (+ 1: the last frame's flow)
            if (cen[:, 0] < hh + 2).any() or (cen[:, 0] > H - hh - 3).any() or (cen[:, 1] < hw + 2).any() or \
                    (cen[:, 1] > W - hw - 3).any():
                continue
            margin = 2 if small else 4
            if all((np.abs(cen[:, 0] - o['cen'][:, 0]) > hh + o['hh'] + margin).all() or
                   (np.abs(cen[:, 1] - o['cen'][:, 1]) > hw + o['hw'] + margin).all() for o in placed):
                break
        else:
            raise RuntimeError('no room for another vehicle')
        t0, t1 = 0, S
        if not small:
            t0 = 2 if k < 3 else (4 if k < 5 and S > 5 else 0)
            t1 = S - 2 if k in (5, 6) else S
        elif k == 0:
            t0 = 1
        placed.append(dict(hh=hh, hw=hw, cen=cen, t0=t0, t1=t1, ghost=(k == 8 % p['n'] and not small),
                           missed=(k == 9 % p['n'] and not small), jumping=jumping))
    return placed


def build(name, **overrides):
    """The inputs of case ``name`` (``overrides`` replace its parameters: the timing scripts' larger batches): a dict with 'segmentation' (B, S, 2, H, W), 'instance_center' (B, S, 1, H, W),
    'instance_offset' (B, S, 2, H, W), 'instance_flow' (B, S, 2, H, W) or None -- float32 --, 'gt_instance' (B, S, H, W) int64
    and the call's options 'make_consistent', 'matched' (compute_matched_centers)."""
    p = {**CASES[name], **overrides}
    rs = np.random.RandomState(p['seed'])
    B, S, H, W = p['B'], p['S'], p['H'], p['W']
    integer, crowded, small = p.get('integer', False), p.get('crowded', False), p.get('small', False)
    sigma = 1.5 if small else 2.0
    rows, cols = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    seg = np.empty((B, S, 2, H, W), np.float32)
    center = np.zeros((B, S, 1, H, W), np.float32)
    offset = np.zeros((B, S, 2, H, W), np.float32)
    flow = np.zeros((B, S, 2, H, W), np.float32)
    gt = np.zeros((B, S, H, W), np.int64)
    for b in range(B):
        vehicles = _place(rs, p, S, H, W)
        for t in range(S):
            fg = np.zeros((H, W), bool)
            g = np.zeros((H, W))
            off = np.zeros((2, H, W)) if integer else rs.standard_normal((2, H, W))
            fl = np.zeros((2, H, W)) if integer else 0.5 * rs.standard_normal((2, H, W))
            for k, v in enumerate(vehicles):
                if not v['t0'] <= t < v['t1']:
                    continue
                cr, cc = v['cen'][t]
                box = (slice(cr - v['hh'], cr + v['hh'] + 1), slice(cc - v['hw'], cc + v['hw'] + 1))
                if not v['ghost']:
                    gt[b, t][box] = k + 1
                if v['missed']:
                    continue
                fg[box] = True
                g = np.maximum(g, np.exp(-((rows - cr) ** 2 + (cols - cc) ** 2) / (2 * sigma ** 2)))
                shape = fg[box].shape
                off[0][box] = np.broadcast_to(cr - rows, (H, W))[box] + (0.0 if integer else 0.3 * rs.standard_normal(shape))
                off[1][box] = np.broadcast_to(cc - cols, (H, W))[box] + (0.0 if integer else 0.3 * rs.standard_normal(shape))
                step = (0, 0) if v['jumping'] else v['cen'][t + 1] - v['cen'][t]
                fl[0][box] = step[0] + (0.0 if integer else 0.2 * rs.standard_normal(shape))
                fl[1][box] = step[1] + (0.0 if integer else 0.2 * rs.standard_normal(shape))
            if integer:
                # exact ties: the left column of every box points at the integer midpoint between its own centre and another
                # vehicle's, where there is one -- both are then equally far and the lower index has to win
                live = [v for v in vehicles if v['t0'] <= t < v['t1'] and not v['missed']]
                for i, v in enumerate(live):
                    o = live[(i + 1) % len(live)]
                    d = o['cen'][t] - v['cen'][t]
                    if o is v or d[0] % 2 or d[1] % 2:
                        continue
                    cr, cc = v['cen'][t]
                    mid = v['cen'][t] + d // 2
                    rr = np.arange(cr - v['hh'], cr + v['hh'] + 1)
                    off[0][rr, cc - v['hw']] = mid[0] - rr
                    off[1][rr, cc - v['hw']] = mid[1] - (cc - v['hw'])
            if crowded:
                g = np.minimum(g, 0.85)                                  # a plateau of five pixels on every vehicle
            elif not integer:
                g = g + 0.002 * rs.standard_normal((H, W))
            speckle = rs.uniform(size=(H, W)) < (0.0 if integer else 2e-4)
            fg = fg | speckle
            if (b, t) in p.get('all_foreground', ()):
                fg[:] = True
            if (b, t) in p.get('empty', ()):
                g = g * 0.05
            logit = np.where(fg, 2.0, -2.0) + (0.0 if integer else 0.3 * rs.standard_normal((H, W)))
            seg[b, t, 0], seg[b, t, 1] = -logit, logit
            center[b, t, 0], offset[b, t], flow[b, t] = g, off, fl
    return {'segmentation': seg, 'instance_center': center, 'instance_offset': offset,
            'instance_flow': None if p.get('no_flow') else flow, 'gt_instance': gt,
            'make_consistent': p.get('make_consistent', True), 'matched': p.get('matched', False)}


INPUT_KEYS = ('segmentation', 'instance_center', 'instance_offset', 'instance_flow', 'gt_instance')


def digest(case):
    """{key: sha256 hex} of the arrays of a built case (None: the digest of nothing)."""
    return {k: hashlib.sha256(b'' if case[k] is None else np.ascontiguousarray(case[k]).tobytes()).hexdigest() for k in INPUT_KEYS}


def renaming(raw, tracked):
    """The tracked maps of ONE sample ((S, H, W), any consistent order of fresh ids) with the ids created at each step
    renamed so that they ascend with the id the vehicle has in the raw frame -- computed from the two maps alone.  Returns
    (renamed maps, number of fresh ids per step)."""
    raw, tracked = np.asarray(raw).astype(np.int64), np.asarray(tracked).astype(np.int64)
    out, fresh_counts = tracked.copy(), [0]
    largest = int(tracked[0].max())
    mapping = {}
    for t in range(1, len(raw)):
        pairs = sorted({(int(r), int(c)) for r, c in zip(raw[t].reshape(-1), tracked[t].reshape(-1)) if c > largest})
        ids = sorted(c for _, c in pairs)
        assert len({c for _, c in pairs}) == len(pairs) == len({r for r, _ in pairs}), 'a fresh id on two raw ids'
        assert ids == list(range(largest + 1, largest + 1 + len(ids))), 'fresh ids are not the next free ones'
        for new, (_, c) in zip(ids, pairs):
            mapping[c] = new
        largest += len(ids)
        fresh_counts.append(len(ids))
    for c, new in mapping.items():
        out[tracked == c] = new
    return out, fresh_counts
