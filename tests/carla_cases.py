"""TEST INFRASTRUCTURE -- the cases of the CARLA decoder and host arithmetic (stp3_amd.carla; csrc/stp3_carla.hip), shared by
scripts/make_golden_carla.py (which records the reference's outputs in tests/golden/carla.npz), tests/test_carla_cpu.py,
tests/test_carla_gpu.py and tests/hipcpu/run_carla.py.  Inputs are never stored: every user rebuilds them with the seeded
builders below (numpy's frozen RandomState) and compares ``digest`` with the fixture first.

The smallest shapes at which each kernel can go wrong, plus the real shapes once:
  frames   11 x 13 sources with crop 6 (the window starts at byte 9 of a 3-channel image: unaligned) and crop 7 (odd row length),
           3 and 4 channels, both channel orders, 1 and 5 images; a source equal to the crop (no margin); 300 x 400 x 4 BGRA with
           crop 256, 4 images
  depth    20 x 24 with crop 20 and downsample 8 (label rows 0, 8, 16: the crop is no multiple of the step), bytes PLANTED: for
           every k in 2..49 the two 24-bit codes either side of k * 16777.215 -- the only places where a class id can flip --
           plus codes 0 and 2^24 - 1, all on kept pixels; 11 x 13 with crop 7 and downsample 2 (unaligned window); 300 x 400 once
  hdmap    9 x 11 with crop 4 and 210 x 214 with crop 200 (odd margins); lane and drivable colours and the near-misses
           (255,0,254), (254,0,255), (54,52,47), (54,53,46) drawn from a palette
  topdown  23 x 29, 500 x 500 and 512 x 512 at scale 1.1 (resized 20 x 26, 454 x 454, 465 x 465); crops 200 (whole ego box), 100
           (box rows clipped at 100), 50 (box outside the window) and 20 / 7 for the small source; classes from {0, 3, 4, 5, 9, 10,
           11, 255} with vehicles planted inside and beside the ego box
  sample   one recorded sequence at the real shapes (T = 3 past and 4 future frames): ``CarlaDataset.__getitem__`` itself
  host     poses (one theta is nan), command points, and 60 steps of way points and speeds for the PID controllers."""
import hashlib

import numpy as np

D_BOUND, DOWNSAMPLE = (2.0, 50.0, 1.0), 8
DEPTH_CODES = 16777215
TOPDOWN_SCALE = 1.1
TOPDOWN_CLASSES = (0, 3, 4, 5, 9, 10, 11, 255)
PALETTE = ((255, 0, 255), (54, 52, 46), (255, 0, 254), (254, 0, 255), (54, 52, 47), (54, 53, 46), (0, 0, 0), (255, 255, 255),
           (46, 52, 54), (255, 0, 0))

FRAME_CASES = {f'f{crop}_{order}{cs}_n{n}': dict(hw=(11, 13), cs=cs, crop=crop, order=order, n=n, seed=100 + 8 * crop + 4 * cs + n)
               for crop in (6, 7) for cs in (3, 4) for order in ('rgb', 'bgr') for n in (1, 5)}
FRAME_CASES['same'] = dict(hw=(7, 7), cs=3, crop=7, order='rgb', n=2, seed=31)
FRAME_CASES['real'] = dict(hw=(300, 400), cs=4, crop=256, order='bgr', n=4, seed=32)

DEPTH_CASES = {'planted': dict(hw=(20, 24), crop=20, ds=8, n=11, seed=41),
               'small': dict(hw=(11, 13), crop=7, ds=2, n=2, seed=42),
               'real': dict(hw=(300, 400), crop=256, ds=8, n=4, seed=43)}

HDMAP_CASES = {'small': dict(hw=(9, 11), crop=4, n=3, seed=51), 'odd': dict(hw=(210, 214), crop=200, n=1, seed=52)}

TOPDOWN_CASES = {'t23_c20': dict(hw=(23, 29), crop=20, n=2, seed=61), 't23_c7': dict(hw=(23, 29), crop=7, n=2, seed=62),
                 't500_c200': dict(hw=(500, 500), crop=200, n=1, seed=63), 't512_c200': dict(hw=(512, 512), crop=200, n=1, seed=64),
                 't500_c100': dict(hw=(500, 500), crop=100, n=1, seed=65), 't512_c50': dict(hw=(512, 512), crop=50, n=2, seed=66)}

# the cases at the real image size: the host stand-in of the kernels runs them once, in one fiber order
REAL_SIZE = {'frames': ('real',), 'depth': ('real',), 'hdmap': (), 'topdown': ('t500_c200',)}

LARGE = 1 << 16          # outputs with more elements are stored as a digest and a strided sample
SAMPLE_STRIDE = 97


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def build_frames(name):
    c = FRAME_CASES[name]
    return np.random.RandomState(c['seed']).randint(0, 256, size=(c['n'],) + c['hw'] + (c['cs'],)).astype(np.uint8)


def planted_codes():
    """0, 2^24 - 1 and, for k = 2..49, floor and floor + 1 of k * 16777.215 (v = code / 16777215 * 1000 crosses k between them)."""
    codes = [0, DEPTH_CODES]
    for k in range(2, 50):
        lo = (k * DEPTH_CODES) // 1000
        codes += [lo, lo + 1]
    return codes


def build_depth(name):
    c = DEPTH_CASES[name]
    h, w = c['hw']
    frames = np.random.RandomState(c['seed']).randint(0, 256, size=(c['n'], h, w, 3)).astype(np.uint8)
    if name == 'planted':
        y0, x0 = h // 2 - c['crop'] // 2, w // 2 - c['crop'] // 2
        kept = [(i, y0 + r, x0 + x) for i in range(c['n']) for r in range(0, c['crop'], c['ds']) for x in range(0, c['crop'], c['ds'])]
        codes = planted_codes()
        assert len(codes) <= len(kept)
        for (i, y, x), code in zip(kept, codes):
            frames[i, y, x] = (code >> 16, (code >> 8) & 255, code & 255)
    elif name == 'real':
        frames[..., 0] = frames[..., 0] % 16          # most of the image within 62 m: the class ids are not all the last one
    return frames


def build_hdmap(name):
    c = HDMAP_CASES[name]
    rs = np.random.RandomState(c['seed'])
    pick = rs.randint(0, len(PALETTE), size=(c['n'],) + c['hw'])
    return np.array(PALETTE, dtype=np.uint8)[pick]


def build_topdown(name):
    c = TOPDOWN_CASES[name]
    h, w = c['hw']
    rs = np.random.RandomState(c['seed'])
    frames = np.array(TOPDOWN_CLASSES, dtype=np.uint8)[rs.randint(0, len(TOPDOWN_CLASSES), size=(c['n'], h, w))]
    hr, wr = int(h // TOPDOWN_SCALE), int(w // TOPDOWN_SCALE)
    y0, x0 = hr // 2 - c['crop'] // 2, wr // 2 - c['crop'] // 2
    if c['crop'] > 89:
        # vehicles inside and beside the ego box (window rows 89..111, columns 96..104): the source region that covers window
        # rows 80..120 and columns 90..110, most of its pixels vehicles
        r0, r1 = int((y0 + 80) * TOPDOWN_SCALE), min(int((y0 + 121) * TOPDOWN_SCALE), h)
        c0, c1 = int((x0 + 90) * TOPDOWN_SCALE), min(int((x0 + 111) * TOPDOWN_SCALE), w)
        block = frames[:, r0:r1, c0:c1]
        block[rs.rand(*block.shape) < 0.7] = 10
    return frames


# ---- the recorded sequence and the host arithmetic --------------------------------------------------------------------------
SAMPLE = dict(receptive_field=3, n_future=4, image_hw=(300, 400), hdmap_hw=(220, 230), topdown_hw=(500, 500), seed=71)


def build_sample():
    """The decoded bytes and measurements of one sequence: images / depths (3, 4, 300, 400, 3), hdmaps (3, 220, 230, 3), topdowns
    (7, 500, 500) and the measurements of ``host_poses()[0]``."""
    s = SAMPLE
    rs = np.random.RandomState(s['seed'])
    t, n = s['receptive_field'], s['receptive_field'] + s['n_future']
    h, w = s['image_hw']
    images = rs.randint(0, 256, size=(t, 4, h, w, 3)).astype(np.uint8)
    depths = rs.randint(0, 256, size=(t, 4, h, w, 3)).astype(np.uint8)
    depths[..., 0] = depths[..., 0] % 16
    hdmaps = np.array(PALETTE, dtype=np.uint8)[rs.randint(0, len(PALETTE), size=(t,) + s['hdmap_hw'])]
    topdowns = np.array(TOPDOWN_CLASSES, dtype=np.uint8)[rs.randint(0, len(TOPDOWN_CLASSES), size=(n,) + s['topdown_hw'])]
    topdowns[:, 225:275, 236:264][rs.rand(n, 50, 28) < 0.7] = 10
    return {'images': images, 'depths': depths, 'hdmaps': hdmaps, 'topdowns': topdowns}


def host_poses():
    """Three sequences of 7 poses with their measurements; the first has a nan theta among the past frames."""
    rs = np.random.RandomState(81)
    out = []
    for k in range(3):
        theta0 = rs.uniform(-np.pi, np.pi)
        theta = (theta0 + np.cumsum(rs.uniform(-0.15, 0.15, size=7))).tolist()
        step = rs.uniform(0.2, 4.0, size=7)
        x = (rs.uniform(-300, 300) + np.cumsum(step * np.cos(theta))).tolist()
        y = (rs.uniform(-300, 300) + np.cumsum(step * np.sin(theta))).tolist()
        if k == 0:
            theta[1] = float('nan')
        out.append({'x': x, 'y': y, 'theta': theta, 'x_command': x[2] + float(rs.uniform(-30, 30)),
                    'y_command': y[2] + float(rs.uniform(-30, 30)), 'command': [1, 2, 4][k], 'steer': float(rs.uniform(-0.6, 0.6)),
                    'throttle': float(rs.uniform(0, 0.75)), 'brake': 0.0, 'velocity': float(rs.uniform(0, 8))})
    return out


def control_sequence():
    """60 steps for ``control_pid``: way points (60, 1, 4, 3) float32 (x lateral, y forward: a vehicle that speeds up, turns and
    nearly stops) and speeds (60,) float32, some of them above 1.2 x the desired speed (the brake branch)."""
    rs = np.random.RandomState(91)
    k = np.arange(60)
    pace = 0.2 + 2.5 * np.abs(np.sin(k / 9.0))                                  # metres per way point
    bend = 0.5 * np.sin(k / 7.0)
    steps = np.arange(1, 5)
    wp = np.zeros((60, 1, 4, 3), dtype=np.float32)
    wp[:, 0, :, 1] = (pace[:, None] * steps).astype(np.float32)
    wp[:, 0, :, 0] = (bend[:, None] * steps ** 2 * 0.3 + rs.uniform(-0.05, 0.05, size=(60, 4))).astype(np.float32)
    speed = (2.0 * pace * rs.uniform(0.5, 1.5, size=60)).astype(np.float32)
    return wp, speed


def pack(mask):
    """A 0 / 1 map as bits (np.packbits over the flattened map)."""
    return np.packbits(np.asarray(mask).astype(bool).reshape(-1))


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape)


def strided(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1)[::SAMPLE_STRIDE])
