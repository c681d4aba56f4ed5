"""TEST INFRASTRUCTURE -- the deterministic inputs of the depth-label fixture (tests/golden/depth_labels.npz):
scripts/make_golden_depth.py (which runs the reference on them) and tests/test_depth_*.py build the SAME arrays from
``numpy.random.RandomState(seed)``; the fixture stores a sha256 of every array so that a drifting builder fails loudly.
numpy only.

A lidar case: N pinhole cameras looking outwards at yaw 360 / N apart, four rigid steps per camera (sensor -> ego at the
sweep time, ego -> global, global -> ego at the image time, ego -> camera; the last two translate before they rotate, as the
devkit's map_pointcloud_to_image) with small random rotations and translations, and a cloud built backwards: for every
point a camera, a target pixel position and a depth, carried through the inverse chain and rounded to float32.  ``project``
below is the devkit's projection restated with the arithmetic this project defines (csrc/stp3_depth.hip): points for which
any camera sees a coordinate within ``MARGIN`` of an integer or of a bound of the keep mask (or a depth that close to 1)
are dropped, so that the pixel and the mask of every point do not hang on the last bits of the arithmetic.  Targets cover
the first and last source rows and columns that a kept output pixel reads, and ``repeats`` points re-use the ray of an
earlier point with another depth (same pixel: the last one has to win)."""
import hashlib

import numpy as np

MARGIN = 1e-3
BEFORE = (False, False, True, True)
SMALL = dict(source_hw=(90, 160), scale=0.3, crop=(0, 3, 48, 27), downsample=8, d_bound=(2.0, 50.0, 1.0))
LIDAR_CASES = {
    'small': dict(seed=31, F=2, N=2, counts=(1000, 37), repeats=100, focal=60.0, **SMALL),
    'sparse': dict(seed=32, F=3, N=2, counts=(0, 1, 5), repeats=0, focal=60.0, **SMALL),
    'half': dict(seed=33, F=1, N=3, counts=(400,), repeats=40, focal=70.0, source_hw=(90, 160), scale=0.5,
                 crop=(8, 5, 72, 37), downsample=8, d_bound=(2.0, 50.0, 1.0)),
    'real': dict(seed=34, F=1, N=6, counts=(35000,), repeats=2000, focal=1266.0, source_hw=(900, 1600), scale=0.3,
                 crop=(0, 46, 480, 270), downsample=8, d_bound=(2.0, 50.0, 1.0)),
}
MAP_CASES = {
    'map64': dict(seed=41, F=1, N=2, dtype='float64', **SMALL),
    'map32': dict(seed=42, F=2, N=2, dtype='float32', **SMALL),
}
GEOMETRY_KEYS = ('source_hw', 'scale', 'crop', 'downsample', 'd_bound')
LIDAR_KEYS = ('points', 'offsets', 'steps', 'intrinsics')


def geometry(p):
    return {k: p[k] for k in GEOMETRY_KEYS}


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    return np.array(m[axis], dtype=np.float64)


def _small_rotation(rs, size):
    a = rs.uniform(-size, size, size=3)
    return _rot(2, a[2]) @ _rot(1, a[1]) @ _rot(0, a[0])


def project(points, steps, intrinsics, hw, before=BEFORE):
    """One frame: points (n, 3) float32, steps (N, 4, 12), intrinsics (N, 3, 3) -> u, v (n, N) float64, depth (n, N)
    float32, keep (n, N).  LidarPointCloud.rotate / .translate per step on float32 storage, every component evaluated left
    to right in float64; view_points with normalize=True; the devkit's mask."""
    h, w = hw
    n_cam = steps.shape[0]
    x, y, z = (np.repeat(points[:, i:i + 1], n_cam, axis=1).astype(np.float32) for i in range(3))
    for s in range(4):
        r = steps[None, :, s]
        if before[s]:
            x, y, z = ((x.astype(np.float64) + r[..., 9]).astype(np.float32), (y.astype(np.float64) + r[..., 10]).astype(np.float32),
                       (z.astype(np.float64) + r[..., 11]).astype(np.float32))
        dx, dy, dz = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        x = (r[..., 0] * dx + r[..., 1] * dy + r[..., 2] * dz).astype(np.float32)
        y = (r[..., 3] * dx + r[..., 4] * dy + r[..., 5] * dz).astype(np.float32)
        z = (r[..., 6] * dx + r[..., 7] * dy + r[..., 8] * dz).astype(np.float32)
        if not before[s]:
            x, y, z = ((x.astype(np.float64) + r[..., 9]).astype(np.float32), (y.astype(np.float64) + r[..., 10]).astype(np.float32),
                       (z.astype(np.float64) + r[..., 11]).astype(np.float32))
    dx, dy, dz = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
    k = intrinsics[None]
    p0 = k[..., 0, 0] * dx + k[..., 0, 1] * dy + k[..., 0, 2] * dz
    p1 = k[..., 1, 0] * dx + k[..., 1, 1] * dy + k[..., 1, 2] * dz
    p2 = k[..., 2, 0] * dx + k[..., 2, 1] * dy + k[..., 2, 2] * dz
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = p0 / p2, p1 / p2
        keep = (z > 1.0) & (u > 1.0) & (u < w - 1) & (v > 1.0) & (v < h - 1)
    return u, v, z, keep


def _fragile(u, v, z, hw):
    """Points whose pixel or mask in some camera hangs on less than MARGIN."""
    h, w = hw
    with np.errstate(invalid='ignore'):
        front = z > 0.5                                                           # (behind the camera: masked whatever u, v)
        near_int = (np.abs(u - np.rint(u)) < MARGIN) | (np.abs(v - np.rint(v)) < MARGIN)
        bad = (front & near_int) | (np.abs(z - 1.0) < MARGIN) | ~np.isfinite(u) | ~np.isfinite(v)
    return bad.any(axis=1)


def _tap_range(n_src, scale, first, last):
    """First and last source index that the kept outputs first .. last read (ATen's taps, float64)."""
    lo = int(max(0.0, (1.0 / scale) * (first + 0.5) - 0.5))
    hi = min(int(max(0.0, (1.0 / scale) * (last + 0.5) - 0.5)) + 1, n_src - 1)
    return lo, hi


def build_lidar(name, **overrides):
    """{'points' (n, 3) float32, 'offsets' (F + 1,) int32, 'steps' (F, N, 4, 12), 'intrinsics' (F, N, 3, 3)} + the geometry
    (``overrides`` replace the case's parameters: the timing script's 12 frames)."""
    p = {**LIDAR_CASES[name], **overrides}
    rs = np.random.RandomState(p['seed'])
    (h, w), n_cam, scale = p['source_hw'], p['N'], p['scale']
    left, top, right, bottom = p['crop']
    hr, wr = int(np.floor(h * scale)), int(np.floor(w * scale))
    y_lo, y_hi = _tap_range(h, scale, top, min(bottom, hr) - 1)
    x_lo, x_hi = _tap_range(w, scale, left, min(right, wr) - 1)
    cam_to_ego = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)       # camera z forward, x right, y down
    all_points, all_steps, all_k, offsets = [], [], [], [0]
    for f in range(p['F']):
        steps = np.zeros((n_cam, 4, 12))
        ks = np.zeros((n_cam, 3, 3))
        r_l, t_l = _small_rotation(rs, 0.03), rs.uniform(-1, 1, size=3) + np.array([0.9, 0.0, 1.8])
        r_e, t_e = _rot(2, rs.uniform(-3, 3)) @ _small_rotation(rs, 0.02), rs.uniform(-400, 400, size=3)
        inverse = []
        for c in range(n_cam):
            r_e2, t_e2 = r_e @ _small_rotation(rs, 0.01), t_e + rs.uniform(-0.5, 0.5, size=3)
            r_c = _rot(2, 2 * np.pi * c / n_cam + rs.uniform(-0.05, 0.05)) @ _small_rotation(rs, 0.02) @ cam_to_ego
            t_c = rs.uniform(-1, 1, size=3) + np.array([0.0, 0.0, 1.5])
            for s, (rot, tr) in enumerate(((r_l, t_l), (r_e, t_e), (r_e2.T, -t_e2), (r_c.T, -t_c))):
                steps[c, s, :9], steps[c, s, 9:] = rot.reshape(-1), tr
            ks[c] = [[p['focal'] * rs.uniform(0.98, 1.02), 0, w / 2 + rs.uniform(-8, 8)],
                     [0, p['focal'] * rs.uniform(0.98, 1.02), h / 2 + rs.uniform(-8, 8)], [0, 0, 1]]
            # camera -> lidar: undo the four steps
            inverse.append(lambda q, a=(r_l, t_l, r_e, t_e, r_e2, t_e2, r_c, t_c):
                           (((q @ a[6].T + a[7]) @ a[4].T + a[5] - a[3]) @ a[2] - a[1]) @ a[0])
        want = p['counts'][f]
        kept = np.zeros((0, 3), np.float32)
        if want:
            m = int(want * 1.3) + 16
            cam = rs.randint(0, n_cam, size=m)
            u = rs.uniform(1.2, w - 1.2, size=m)
            v = rs.uniform(max(1.2, y_lo - 4.0), min(h - 1.2, y_hi + 5.0), size=m)
            d = rs.uniform(1.5, 70.0, size=m)
            edge = np.arange(m)
            if x_lo >= 1:
                u[edge % 9 == 1] = x_lo + 0.5
            if x_hi <= w - 2:
                u[edge % 9 == 2] = x_hi + 0.5
            if y_lo >= 1:
                v[edge % 9 == 3] = y_lo + 0.5
            if y_hi <= h - 2:
                v[edge % 9 == 4] = y_hi + 0.5
            rep = p['repeats'] * want // sum(p['counts'])
            if rep:
                src = rs.randint(0, m - rep, size=rep)
                cam[m - rep:], u[m - rep:], v[m - rep:] = cam[src], np.floor(u[src]) + 0.5, np.floor(v[src]) + 0.5
                u[src], v[src] = np.floor(u[src]) + 0.5, np.floor(v[src]) + 0.5
            order = rs.permutation(m)
            cam, u, v, d = cam[order], u[order], v[order], d[order]
            pts = np.empty((m, 3))
            for c in range(n_cam):
                sel = cam == c
                k = ks[c]
                q = np.stack([(u[sel] - k[0, 2]) / k[0, 0] * d[sel], (v[sel] - k[1, 2]) / k[1, 1] * d[sel], d[sel]], axis=1)
                pts[sel] = inverse[c](q)
            pts = pts.astype(np.float32)
            pu, pv, pz, _ = project(pts, steps, ks, (h, w))
            kept = pts[~_fragile(pu, pv, pz, (h, w))][:want]
            assert len(kept) == want, f'{name}: frame {f}: {len(kept)} robust points of {want}'
        all_points.append(kept)
        all_steps.append(steps)
        all_k.append(ks)
        offsets.append(offsets[-1] + len(kept))
    return {'points': np.concatenate(all_points).astype(np.float32), 'offsets': np.array(offsets, np.int32),
            'steps': np.stack(all_steps), 'intrinsics': np.stack(all_k), **geometry(p)}


def projected(case):
    """``project`` for every frame of a built lidar case: pixels (n, N, 2) int32 (0 where not kept), depth (n, N) float64,
    keep (n, N) bool -- what DepthLabeller.project has to return."""
    n_cam = case['steps'].shape[1]
    n = len(case['points'])
    pixels, depth, keep = np.zeros((n, n_cam, 2), np.int32), np.zeros((n, n_cam)), np.zeros((n, n_cam), bool)
    off = case['offsets']
    for f in range(len(off) - 1):
        sl = slice(off[f], off[f + 1])
        u, v, z, k = project(case['points'][sl], case['steps'][f], case['intrinsics'][f], case['source_hw'])
        pixels[sl, :, 0], pixels[sl, :, 1] = np.where(k, u, 0.0).astype(np.int32), np.where(k, v, 0.0).astype(np.int32)
        depth[sl], keep[sl] = z.astype(np.float64), k
    return pixels, depth, keep


def build_map(name):
    """{'maps' (F, N, H, W) float64 | float32: dense, uniform depths} + the geometry."""
    p = MAP_CASES[name]
    rs = np.random.RandomState(p['seed'])
    maps = rs.uniform(0.0, 70.0, size=(p['F'], p['N']) + tuple(p['source_hw'])).astype(p['dtype'])
    return {'maps': maps, **geometry(p)}


def digest(case, keys):
    return [hashlib.sha256(np.ascontiguousarray(case[k]).tobytes()).hexdigest() for k in keys]
