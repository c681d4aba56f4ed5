"""The CARLA half of the reference: recorded samples (``stp3/datas/CarlaData.py``) and the closed-loop tick (``carla_agent.py``)
from decoded bytes to tensors and from tensors to steer / throttle / brake.

``CarlaDecoder`` starts at decoded bytes (the directory scan of ``get_train_val`` and the simulator classes stay outside);
``load_carla_sample`` starts at the PNG files' bytes, with ``datas.PngDecoder`` -- chunks and zlib on host threads, the scanline
filters in a kernel -- in front.  Everything from bytes to tensors is ONE launch per kind for all frames and cameras of a call
(csrc/stp3_carla.hip):

    dec = CarlaDecoder(cfg)                                  # or crop=256, bev_crop=200, topdown_scale=1.1, downsample=, d_bound=
    x = dec.images(frames, order='rgb')                      # (..., Hs, Ws, 3 | 4) uint8 -> (..., 3, crop, crop) float32 | bf16
    d = dec.depths(frames)                                   # (..., Hs, Ws, 3) uint8 -> (..., crop, crop) metres, float32 | float64
    ids = dec.depths(frames, labels=True)                    # -> the trainer's class ids (..., ceil(crop / ds), ceil(crop / ds)) int64
    hd = dec.hdmap(frames)                                   # (..., Hm, Wm, 3) uint8 -> (..., 2, bev_crop, bev_crop): lane, drivable
    veh, ped = dec.topdown(frames)                           # (..., Ht, Wt) uint8 -> two (..., 1, bev_crop, bev_crop)

GPU tensors run the kernels, CPU tensors the ``reference_*`` twins -- the same statements with torch operators, which also run on
GPU tensors (``datas.DepthLabeller``'s arrangement).  The host arithmetic around them (camera matrices, ego motion, the expert
trajectory, the command point, the PID controllers) restates the reference's statements in its own operation order;
``assemble_carla_sample`` puts one sequence together as ``CarlaDataset.__getitem__`` does and ``ClosedLoopDriver`` is the agent's
``run_step`` on ``inference.StreamingEngine``, without the simulator classes.  ``scale != 1`` is not offered: the reference never
uses it (Pillow's default filter there would be bicubic)."""
import ctypes
from collections import deque

import numpy as np
import torch

from . import _lib, ops
from .datas import IMAGENET_MEAN, IMAGENET_STD, trajectory_sampling, update_intrinsics
from .geometry import mat2pose_vec

VEHICLE_CLASS, PEDESTRIAN_CLASS = 10, 4             # CarlaData.py:271,275: class ids of the top-down semantic camera
LANE_COLOUR, DRIVABLE_COLOUR = (255, 0, 255), (54, 52, 46)          # CarlaData.py:249,252
EGO_BOX = (89, 112, 96, 105)                        # CarlaData.py:274: rows, columns of the window the ego vehicle covers
DEPTH_CODES = 256 * 256 * 256 - 1                   # CarlaData.py:352
CAMERAS = ((1.3, 0.0, 2.3, 0.0, 0.0, 0.0), (1.3, 0.0, 2.3, 0.0, 0.0, -60.0), (1.3, 0.0, 2.3, 0.0, 0.0, 60.0),
           (-1.3, 0.0, 2.3, 0.0, 0.0, 180.0))      # front, left, right, rear: x, y, z, roll, pitch, yaw (CarlaData.py:310-313)
SENSOR = {'width': 400, 'height': 300, 'fov': 100}  # CarlaData.py:320-324
_MAP_KINDS = {torch.float32: _lib.CARLA_OUT_F32, torch.float64: _lib.CARLA_OUT_F64, torch.int64: _lib.CARLA_OUT_I64}


def window_start(size, crop):
    """First row / column of the centre window (``scale_and_crop_image``, CarlaData.py:461-462)."""
    return size // 2 - crop // 2


def quaternion_rotation_matrix(w, x, y, z):
    """The rotation matrix of a unit quaternion as pyquaternion builds it (``Quaternion.rotation_matrix``: the lower right 3 x 3
    block of Q . conj(Qbar)^T), float64.  Parity with pyquaternion unpinned: the package is restated from its published source."""
    q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]], dtype=np.float64)
    q_bar = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]], dtype=np.float64)
    return np.dot(q, q_bar.conj().transpose())[1:][:, 1:]


def cam_para(crop=256):
    """``get_cam_para`` (CarlaData.py:298-343; carla_agent.py:187-231 with the yaw in degrees as the loader has it):
    (extrinsics (4, 4, 4), intrinsics (4, 3, 3)) float32 of the front, left, right and rear camera -- yaw 0 / -60 / 60 / 180
    degrees about z, the pinhole of fov 100 at 400 x 300 through ``update_intrinsics`` for the centre window."""
    cams = []
    for dof in CAMERAS:
        yaw = dof[5] * (np.pi / 180)
        rotation = quaternion_rotation_matrix(np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2))
        translation = np.array(dof[:3])[:, None]
        cam_to_ego = np.vstack([np.hstack((rotation, translation)), np.array([0, 0, 0, 1])])
        cams.append(torch.from_numpy(cam_to_ego).float().unsqueeze(0))
    extrinsic = torch.cat(cams, dim=0)
    w, h, fov = SENSOR['width'], SENSOR['height'], SENSOR['fov']
    f = w / (2 * np.tan(fov * np.pi / 360))
    intrinsic = torch.Tensor([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
    intrinsic = update_intrinsics(intrinsic, (h - crop) / 2, (w - crop) / 2, scale_width=1, scale_height=1)
    return extrinsic, intrinsic.unsqueeze(0).expand(4, 3, 3)


def _pose_matrix(x, y, theta):
    matrix = np.zeros((4, 4), dtype=np.float32)
    matrix[:2, :2] = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    matrix[2, 2] = 1
    matrix[0, 3] = x
    matrix[1, 3] = y
    matrix[3, 3] = 1
    return matrix


def _invert_pose_numpy(egopose):
    """``invert_matrix_egopose_numpy`` (stp3/utils/geometry.py:86-94)."""
    inverse = np.zeros((4, 4), dtype=np.float32)
    rotation, translation = egopose[:3, :3], egopose[:3, 3]
    inverse[:3, :3] = rotation.T
    inverse[:3, 3] = -np.dot(rotation.T, translation)
    inverse[3, 3] = 1.0
    return inverse


def future_egomotion(seq_x, seq_y, seq_theta):
    """``get_future_egomotion`` (CarlaData.py:211-238; carla_agent.py:233-260): (len - 1, 6) float32, row i the pose vector of
    inverse(pose[i + 1]) . pose[i]; the matrices are float32."""
    rows = []
    for i in range(len(seq_x) - 1):
        t0 = _pose_matrix(seq_x[i], seq_y[i], seq_theta[i])
        t1 = _pose_matrix(seq_x[i + 1], seq_y[i + 1], seq_theta[i + 1])
        motion = _invert_pose_numpy(t1).dot(t0)
        motion[3, :3] = 0.0
        motion[3, 3] = 1.0
        rows.append(mat2pose_vec(torch.Tensor(motion).float()).unsqueeze(0))
    return torch.cat(rows, dim=0)


def transform_2d_points(xyz, r1, t1_x, t1_y, r2, t2_x, t2_y):
    """``transform_2d_points`` (CarlaData.py:467-490): points of frame 1 (rotation r1, translation t1) expressed in frame 2."""
    xy1 = xyz.copy()
    xy1[:, 2] = 1
    c, s = np.cos(r1), np.sin(r1)
    r1_to_world = np.array([[c, s, t1_x], [-s, c, t1_y], [0, 0, 1]])
    world = r1_to_world @ xy1.T
    c, s = np.cos(r2), np.sin(r2)
    r2_to_world = np.array([[c, s, t2_x], [-s, c, t2_y], [0, 0, 1]])
    world_to_r2 = np.linalg.inv(r2_to_world)
    out = np.ascontiguousarray((world_to_r2 @ world).T)
    out[:, 2] = xyz[:, 2]
    return out


def gt_trajectory(seq_x, seq_y, seq_theta, receptive_field):
    """The expert's way points (CarlaData.py:404-417): the positions of frames receptive_field - 1 .. in the present frame, y
    negated; (len - receptive_field + 1, 3) float64.  A theta that is nan counts as 0 (the reference's fix)."""
    theta = [0.0 if np.isnan(t) else t for t in seq_theta]
    present = receptive_field - 1
    ego_x, ego_y, ego_theta = seq_x[present], seq_y[present], theta[present]
    rows = []
    for i in range(present, len(seq_x)):
        local = transform_2d_points(np.zeros((1, 3)), np.pi / 2 - theta[i], -seq_x[i], -seq_y[i], np.pi / 2 - ego_theta, -ego_x,
                                    -ego_y)
        rows.append(torch.from_numpy(local * [1.0, -1.0, 1.0]))
    return torch.cat(rows, dim=0)


def local_command_point(pos, theta, target):
    """The route's next command point in the ego frame (CarlaData.py:422-428 with the present theta; carla_agent.py:349-357
    with the compass): rotation by pi / 2 + theta, y negated; (2,) float64."""
    angle = np.pi / 2 + theta
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    point = np.array([target[0] - pos[0], target[1] - pos[1]])
    point = rot.T.dot(point)
    return torch.from_numpy(point * [1.0, -1.0])


def command_name(code):
    """CarlaData.py:431-438; carla_agent.py:398-405."""
    return {1: 'LEFT', 2: 'RIGHT', 3: 'FORWARD'}.get(code, 'LANE')


class CarlaDecoder:
    """See the module text.  ``cfg``: FINAL_DIM (square) gives ``crop``, MODEL.ENCODER.DOWNSAMPLE and LIFT.D_BOUND the class ids."""

    def __init__(self, cfg=None, crop=256, bev_crop=200, topdown_scale=1.1, downsample=None, d_bound=None, scale=1.0,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if scale != 1:
            raise ValueError('CarlaDecoder: scale != 1 is not offered (the reference never uses it)')
        if cfg is not None:
            fh, fw = cfg.IMAGE.FINAL_DIM
            if fh != fw:
                raise ValueError(f'CarlaDecoder: IMAGE.FINAL_DIM {(fh, fw)} is not the square centre window of the CARLA loader')
            crop = fh
            downsample = cfg.MODEL.ENCODER.DOWNSAMPLE if downsample is None else downsample
            d_bound = tuple(cfg.LIFT.D_BOUND) if d_bound is None else d_bound
        self.crop, self.bev_crop, self.topdown_scale = int(crop), int(bev_crop), float(topdown_scale)
        if self.crop < 1 or self.bev_crop < 1 or self.topdown_scale <= 0:
            raise ValueError('CarlaDecoder: crop, bev_crop and topdown_scale must be positive')
        self.downsample = None if downsample is None else int(downsample)
        self.d_bound = None if d_bound is None else tuple(float(b) for b in d_bound)
        if self.downsample is not None and self.downsample < 1:
            raise ValueError('CarlaDecoder: downsample < 1')
        self.mean, self.std = tuple(mean), tuple(std)
        self._mean_c, self._std_c = (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std)
        self._axes = {}

    # ---- configuration ---------------------------------------------------------------------------------------------------
    @staticmethod
    def nearest_axis(n_src, n_out):
        """Source index of every output index of Pillow's NEAREST resize along one axis (``ImagingScaleAffine``): a = n_src /
        n_out in double, the first coordinate a * 0.5, then repeated addition of a, each truncated; (n_out,) int32."""
        a = n_src / n_out
        v = a * 0.5
        tab = np.empty(n_out, dtype=np.int32)
        for i in range(n_out):
            tab[i] = min(int(v), n_src - 1)
            v += a
        return tab

    def topdown_dims(self, ht, wt):
        """(Hr, Wr) of the resized top-down image: int(size // scale), CarlaData.py:264."""
        return int(ht // self.topdown_scale), int(wt // self.topdown_scale)

    def _tables(self, ht, wt, device):
        key = (ht, wt, str(device))
        if key not in self._axes:
            hr, wr = self.topdown_dims(ht, wt)
            self._axes[key] = tuple(torch.from_numpy(self.nearest_axis(s, r)).to(device) for s, r in ((ht, hr), (wt, wr)))
        return self._axes[key]

    def class_ids(self, depths):
        """stp3/trainer.py:269-276 on a metre map, as ``datas.DepthLabeller.class_ids``."""
        self._need_labels()
        ds = self.downsample
        return (torch.clamp(depths[..., ::ds, ::ds], self.d_bound[0], self.d_bound[1] - 1) - self.d_bound[0]).long().contiguous()

    def _need_labels(self):
        if self.downsample is None or self.d_bound is None:
            raise ValueError('CarlaDecoder: class ids need downsample and d_bound (or a cfg)')

    # ---- validation ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(frames, channels, crop, what, trailing=1):
        dims = 2 + trailing
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
            raise ValueError(f'{what}: uint8 tensor expected, got {getattr(frames, "dtype", type(frames))}')
        if frames.dim() < dims or (trailing and frames.shape[-1] not in channels):
            raise ValueError(f'{what}: (..., H, W{", C" if trailing else ""}) with C in {channels} expected, got {tuple(frames.shape)}')
        h, w = frames.shape[-dims], frames.shape[-dims + 1]
        if h < crop or w < crop:
            raise ValueError(f'{what}: the source {h} x {w} is smaller than the window {crop}')
        return h, w

    @staticmethod
    def _map_dtype(out_dtype):
        if out_dtype not in _MAP_KINDS:
            raise ValueError(f'out_dtype must be float32, float64 or int64: {out_dtype}')
        return _MAP_KINDS[out_dtype]

    def _window(self, frames, h, w, crop, trailing=1):
        y0, x0 = window_start(h, crop), window_start(w, crop)
        return frames[..., y0:y0 + crop, x0:x0 + crop, :] if trailing else frames[..., y0:y0 + crop, x0:x0 + crop]

    # ---- camera images ---------------------------------------------------------------------------------------------------
    def reference_images(self, frames, order='rgb', out_dtype=torch.float32):
        """``images`` with torch operators: window, channel order, ToTensor (float32 / 255), Normalize -- two true divisions."""
        h, w = self._check(frames, (3, 4), self.crop, 'images')
        bgr = self._order(order)
        win = self._window(frames, h, w, self.crop)[..., :3]
        if bgr:
            win = win.flip(-1)
        x = win.movedim(-1, -3).to(torch.float32)
        x = x / torch.tensor(255.0, dtype=torch.float32, device=x.device)
        mean = torch.tensor(self.mean, dtype=torch.float32, device=x.device).view(3, 1, 1)
        std = torch.tensor(self.std, dtype=torch.float32, device=x.device).view(3, 1, 1)
        return ((x - mean) / std).to(out_dtype).contiguous()

    @staticmethod
    def _order(order):
        if order not in ('rgb', 'bgr'):
            raise ValueError(f"order must be 'rgb' or 'bgr': {order!r}")
        return order == 'bgr'

    def images(self, frames, order='rgb', out_dtype=torch.float32, out=None):
        """(..., Hs, Ws, 3 | 4) uint8 -> (..., 3, crop, crop): ``scale_and_crop_image`` + ``normalise_image``; ``order='bgr'`` for
        the simulator's BGRA frames.  ``out``: a contiguous tensor of that shape and dtype to write (an engine's static input)."""
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'images: out_dtype must be float32 or bfloat16: {out_dtype}')
        if not torch.is_tensor(frames) or not frames.is_cuda:
            res = self.reference_images(frames, order, out_dtype)
            return res if out is None else out.copy_(res.view(out.shape))
        h, w = self._check(frames, (3, 4), self.crop, 'images')
        bgr = self._order(order)
        lead, cs, c = frames.shape[:-3], frames.shape[-1], self.crop
        flat = frames.reshape(-1, h, w, cs).contiguous()
        given = out is not None
        if not given:
            out = torch.empty(flat.shape[0], 3, c, c, dtype=out_dtype, device=flat.device)
        elif (out.numel() != flat.shape[0] * 3 * c * c or out.dtype != out_dtype or not out.is_contiguous() or
              out.device != flat.device or tuple(out.shape[-3:]) != (3, c, c)):
            raise ValueError(f'images: out must be a contiguous {out_dtype} tensor of {flat.shape[0]} x (3, {c}, {c}) on {flat.device}')
        _lib.check(_lib.lib().stp3_carla_frames(flat.shape[0], h, w, cs, c, int(bgr), self._mean_c, self._std_c,
                                                _lib.DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.DTYPE_F32, ops._ptr(flat),
                                                ops._ptr(out), ops._stream()), 'stp3_carla_frames')
        return out if given else out.view(*lead, 3, c, c)

    # ---- depth -----------------------------------------------------------------------------------------------------------
    def reference_depths(self, frames, labels=False, out_dtype=torch.float32):
        """``depths`` with torch operators: float64(R 65536 + G 256 + B) / 16777215 * 1000 on the window (``get_depth``)."""
        h, w = self._check(frames, (3,), self.crop, 'depths')
        win = self._window(frames, h, w, self.crop).to(torch.int64)
        code = win[..., 0] * 65536 + win[..., 1] * 256 + win[..., 2]
        # (a tensor divisor: with a Python scalar torch multiplies GPU tensors by the reciprocal, which is not the division)
        metres = code.to(torch.float64) / torch.tensor(float(DEPTH_CODES), dtype=torch.float64, device=code.device) * 1000.0
        return self.class_ids(metres) if labels else metres.to(out_dtype).contiguous()

    def depths(self, frames, labels=False, out_dtype=torch.float32):
        """(..., Hs, Ws, 3) uint8 -> the metre map (..., crop, crop) float32 | float64, or with ``labels`` the trainer's class ids
        (..., ceil(crop / downsample), ceil(crop / downsample)) int64, equal to ``class_ids`` of the float64 map."""
        if labels:
            self._need_labels()
        elif out_dtype not in (torch.float32, torch.float64):
            raise ValueError(f'depths: out_dtype must be float32 or float64: {out_dtype}')
        if not torch.is_tensor(frames) or not frames.is_cuda:
            return self.reference_depths(frames, labels, out_dtype)
        h, w = self._check(frames, (3,), self.crop, 'depths')
        lead, c = frames.shape[:-3], self.crop
        flat = frames.reshape(-1, h, w, 3).contiguous()
        if labels:
            side, kind, dtype = -(-c // self.downsample), _lib.DEPTH_OUT_LABELS, torch.int64
            ds, lo, hi = self.downsample, self.d_bound[0], self.d_bound[1] - 1
        else:
            side, kind, dtype = c, _lib.DEPTH_OUT_F64 if out_dtype == torch.float64 else _lib.DEPTH_OUT_F32, out_dtype
            ds, lo, hi = 1, 0.0, 0.0
        out = torch.empty(flat.shape[0], side, side, dtype=dtype, device=flat.device)
        _lib.check(_lib.lib().stp3_carla_depth(flat.shape[0], h, w, c, kind, ds, lo, hi, ops._ptr(flat), ops._ptr(out),
                                               ops._stream()), 'stp3_carla_depth')
        return out.view(*lead, side, side)

    # ---- hd map ----------------------------------------------------------------------------------------------------------
    def reference_hdmap(self, frames, out_dtype=torch.float32):
        """``hdmap`` with torch operators (``get_hdmap``)."""
        self._map_dtype(out_dtype)
        h, w = self._check(frames, (3,), self.bev_crop, 'hdmap')
        win = self._window(frames, h, w, self.bev_crop)
        lane = (win == win.new_tensor(LANE_COLOUR)).all(dim=-1)
        drivable = torch.logical_or((win == win.new_tensor(DRIVABLE_COLOUR)).all(dim=-1), lane)
        return torch.stack([lane.flip(-2, -1), drivable.flip(-2, -1)], dim=-3).to(out_dtype).contiguous()

    def hdmap(self, frames, out_dtype=torch.float32):
        """(..., Hm, Wm, 3) uint8 -> (..., 2, bev_crop, bev_crop): channel 0 the lane, channel 1 the drivable area, 0 / 1."""
        if not torch.is_tensor(frames) or not frames.is_cuda:
            return self.reference_hdmap(frames, out_dtype)
        kind = self._map_dtype(out_dtype)
        h, w = self._check(frames, (3,), self.bev_crop, 'hdmap')
        lead, c = frames.shape[:-3], self.bev_crop
        flat = frames.reshape(-1, h, w, 3).contiguous()
        out = torch.empty(flat.shape[0], 2, c, c, dtype=out_dtype, device=flat.device)
        _lib.check(_lib.lib().stp3_carla_hdmap(flat.shape[0], h, w, c, kind, ops._ptr(flat), ops._ptr(out), ops._stream()),
                   'stp3_carla_hdmap')
        return out.view(*lead, 2, c, c)

    # ---- top-down labels -------------------------------------------------------------------------------------------------
    def _topdown_check(self, frames):
        ht, wt = self._check(frames, (), self.bev_crop, 'topdown', trailing=0)
        hr, wr = self.topdown_dims(ht, wt)
        if hr < self.bev_crop or wr < self.bev_crop:
            raise ValueError(f'topdown: the resized image {hr} x {wr} is smaller than the window {self.bev_crop}')
        return ht, wt, hr, wr

    def reference_topdown(self, frames, out_dtype=torch.float32):
        """``topdown`` with torch operators (``get_labels``)."""
        self._map_dtype(out_dtype)
        ht, wt, hr, wr = self._topdown_check(frames)
        rows, cols = self._tables(ht, wt, frames.device)
        small = frames[..., rows.long(), :][..., cols.long()]
        win = self._window(small, hr, wr, self.bev_crop, trailing=0)
        vehicle = (win == VEHICLE_CLASS).to(out_dtype)
        vehicle[..., EGO_BOX[0]:EGO_BOX[1], EGO_BOX[2]:EGO_BOX[3]] = 0
        pedestrian = (win == PEDESTRIAN_CLASS).to(out_dtype)
        return tuple(m.flip(-2, -1).unsqueeze(-3).contiguous() for m in (vehicle, pedestrian))

    def topdown(self, frames, out_dtype=torch.float32):
        """(..., Ht, Wt) uint8 class ids -> (vehicle, pedestrian), each (..., 1, bev_crop, bev_crop), 0 / 1."""
        if not torch.is_tensor(frames) or not frames.is_cuda:
            return self.reference_topdown(frames, out_dtype)
        kind = self._map_dtype(out_dtype)
        ht, wt, hr, wr = self._topdown_check(frames)
        rows, cols = self._tables(ht, wt, frames.device)
        lead, c = frames.shape[:-2], self.bev_crop
        flat = frames.reshape(-1, ht, wt).contiguous()
        vehicle = torch.empty(flat.shape[0], 1, c, c, dtype=out_dtype, device=flat.device)
        pedestrian = torch.empty_like(vehicle)
        _lib.check(_lib.lib().stp3_carla_topdown(flat.shape[0], ht, wt, hr, wr, c, ops._ptr(rows), ops._ptr(cols), kind, ops._ptr(flat),
                                                 ops._ptr(vehicle), ops._ptr(pedestrian), ops._stream()), 'stp3_carla_topdown')
        return vehicle.view(*lead, 1, c, c), pedestrian.view(*lead, 1, c, c)


def assemble_carla_sample(decoder, images, depths, hdmaps, topdowns, seq_x, seq_y, seq_theta, x_command, y_command, command, steer,
                          throttle, brake, velocity, receptive_field, sample_num, draws=None, generator=None):
    """``CarlaDataset.__getitem__`` (CarlaData.py:355-450) after the PNG decoder: the decoded bytes of one sequence of S =
    receptive_field + n_future frames plus its measurements -> the sample dictionary with the reference's keys, shapes and types.

    images, depths (T, 4, Hs, Ws, 3) uint8: the four cameras (front, left, right, rear) of the T = receptive_field past frames;
    hdmaps (T, Hm, Wm, 3); topdowns (S, Ht, Wt); seq_x / seq_y / seq_theta: S floats; x_command, y_command, command, steer, throttle,
    brake, velocity: the present frame's measurements.  The tensors live where the bytes live; ``sample_trajectory`` comes from
    ``datas.trajectory_sampling`` (``draws`` / ``generator`` as there)."""
    t, s = int(receptive_field), len(seq_x)
    if images.shape[0] != t or depths.shape[0] != t or hdmaps.shape[0] != t or topdowns.shape[0] != s or s < t or \
            len(seq_y) != s or len(seq_theta) != s:
        raise ValueError(f'assemble_carla_sample: {t} past frames of images / depths / hdmaps and {s} of topdowns and poses expected')
    dev = images.device
    theta = [0.0 if np.isnan(v) else v for v in seq_theta]
    extrinsics, intrinsics = cam_para(decoder.crop)
    segmentation, pedestrian = decoder.topdown(topdowns, out_dtype=torch.float64)
    present = t - 1
    data = {
        'image': decoder.images(images),
        'depths': decoder.depths(depths, out_dtype=torch.float64),
        'segmentation': segmentation,
        'pedestrian': pedestrian,
        'extrinsics': extrinsics.unsqueeze(0).repeat(t, 1, 1, 1).to(dev),
        'intrinsics': intrinsics.unsqueeze(0).repeat(t, 1, 1, 1).to(dev),
        'hdmap': decoder.hdmap(hdmaps, out_dtype=torch.float64),
        'gt_trajectory': gt_trajectory(seq_x, seq_y, theta, t).to(dev),
        'target_point': local_command_point((seq_x[present], seq_y[present]), theta[present], (x_command, y_command)).to(dev),
        'command': command_name(command),
        'steer': steer, 'throttle': throttle, 'brake': brake, 'velocity': velocity,
        'future_egomotion': future_egomotion(seq_x, seq_y, theta).to(dev),
    }
    speed = torch.tensor([velocity], dtype=torch.float64, device=dev)
    steering = torch.tensor([steer], dtype=torch.float64, device=dev)
    data['sample_trajectory'] = trajectory_sampling(speed, steering, s - t, sample_num, draws=draws, generator=generator)[0]
    return data


def _decode_kind(png, files, what, three_channels, device):
    """All PNG files of one kind in one call of ``png``: a stacked uint8 tensor (len(files), H, W[, 3]) on ``device``."""
    if not files:
        raise ValueError(f'load_carla_sample: no {what} files')
    batch = png.inflate(files)
    for i, shape in enumerate(batch.shapes):
        if three_channels and (len(shape) != 3 or shape[2] != 3):
            raise ValueError(f'load_carla_sample: {what} file {i} decodes to {shape}, an RGB image (H, W, 3) is expected')
        if not three_channels and len(shape) != 2:
            raise ValueError(f'load_carla_sample: {what} file {i} decodes to {shape}, a 2-D image of class ids is expected')
        if shape != batch.shapes[0]:
            raise ValueError(f'load_carla_sample: {what} file {i} is {shape}, file 0 is {batch.shapes[0]}')
    return png.unfilter(batch, device)


def load_carla_sample(decoder, png, image_files, depth_files, hdmap_files, topdown_files, seq_x, seq_y, seq_theta, x_command,
                      y_command, command, steer, throttle, brake, velocity, receptive_field, sample_num, draws=None, generator=None,
                      device='cuda'):
    """``CarlaDataset.__getitem__`` (CarlaData.py:355-450) from the files' BYTES: ``assemble_carla_sample`` with a
    ``datas.PngDecoder`` in front of it instead of ``Image.open`` per file (CarlaData.py:240-266,377-397).

    image_files, depth_files: T rows of 4 PNG byte strings (front, left, right, rear) of the T = receptive_field past frames;
    hdmap_files: T byte strings; topdown_files: S byte strings; the rest as ``assemble_carla_sample``.  Four calls of ``png``,
    one per kind, each one host-to-device copy and one launch.  A camera, depth or hd-map file that is not RGB, or a top-down
    file that is not a single-channel image, raises ``ValueError`` with the file's index (in row-major order of the argument)
    -- the reference's own comparisons fail on such files."""
    t = int(receptive_field)
    cameras = [bytes(f) for row in image_files for f in row]
    ranges = [bytes(f) for row in depth_files for f in row]
    if len(cameras) != 4 * t or len(ranges) != 4 * t or any(len(row) != 4 for row in list(image_files) + list(depth_files)):
        raise ValueError(f'load_carla_sample: {t} rows of 4 camera files and of 4 depth files expected')
    images = _decode_kind(png, cameras, 'camera', True, device)
    depths = _decode_kind(png, ranges, 'depth', True, device)
    hdmaps = _decode_kind(png, list(hdmap_files), 'hd-map', True, device)
    topdowns = _decode_kind(png, list(topdown_files), 'top-down', False, device)
    return assemble_carla_sample(decoder, images.view(t, 4, *images.shape[1:]), depths.view(t, 4, *depths.shape[1:]), hdmaps, topdowns,
                                 seq_x, seq_y, seq_theta, x_command, y_command, command, steer, throttle, brake, velocity,
                                 receptive_field, sample_num, draws=draws, generator=generator)


# ----------------------------------------------------------------------------------------------------------------------------
# Control (carla_agent.py:54-76,278-321): host numpy -- the result returns to the simulator, a device version would save nothing.
# ----------------------------------------------------------------------------------------------------------------------------
class PIDController:
    """carla_agent.py:54-76: proportional + mean of a window of n errors + last difference."""

    def __init__(self, K_P=1.0, K_I=0.0, K_D=0.0, n=20):
        self._K_P, self._K_I, self._K_D = K_P, K_I, K_D
        self._window = deque([0 for _ in range(n)], maxlen=n)
        self._max = 0.0
        self._min = 0.0

    def step(self, error):
        self._window.append(error)
        self._max = max(self._max, abs(error))
        self._min = -abs(self._max)
        if len(self._window) >= 2:
            integral = np.mean(self._window)
            derivative = (self._window[-1] - self._window[-2])
        else:
            integral = 0.0
            derivative = 0.0
        return self._K_P * error + self._K_I * integral + self._K_D * derivative


def turn_controller():
    return PIDController(K_P=1.25, K_I=0.75, K_D=0.3, n=40)          # carla_agent.py:116


def speed_controller():
    return PIDController(K_P=5.0, K_I=0.5, K_D=1.0, n=40)            # carla_agent.py:117


def control_pid(waypoints, speed, turn, speed_ctrl, command=None):
    """``MVPAgent.control_pid`` (carla_agent.py:278-321): the planned way points (1, T >= 2, >= 2) (tensor or array; float32 as the
    planner returns them) and the speedometer value -> (steer, throttle, brake, metadata).  ``turn`` / ``speed_ctrl``: the two
    ``PIDController``s, advanced by the call."""
    if torch.is_tensor(waypoints):
        waypoints = waypoints.detach().cpu().numpy()
    assert waypoints.shape[0] == 1
    waypoints = waypoints[0]
    speed = np.asarray(speed.detach().cpu().numpy() if torch.is_tensor(speed) else speed, dtype=np.float32).reshape(())

    aim = (waypoints[1] + waypoints[0]) / 2.0
    angle = np.degrees(np.pi / 2 - np.arctan2(aim[1], aim[0])) / 90
    steer = turn.step(angle)
    steer = np.clip(steer, -1.0, 1.0)

    desired_speed = np.linalg.norm(waypoints[0] - waypoints[1]) * 2.0
    brake = (speed / desired_speed) > 1.2

    delta = np.clip(desired_speed - speed, 0.0, 0.25)
    throttle = speed_ctrl.step(delta)
    throttle = np.clip(throttle, 0.0, 0.75)
    throttle = throttle if not brake else 0.0

    metadata = {'speed': float(speed.astype(np.float64)), 'steer': float(steer), 'throttle': float(throttle), 'brake': float(brake)}
    for k in range(min(4, len(waypoints)), 0, -1):
        metadata[f'wp_{k}'] = tuple(waypoints[k - 1].astype(np.float64))
    metadata.update({'command': command, 'desired_speed': float(desired_speed.astype(np.float64)),
                     'angle': float(angle.astype(np.float64)), 'aim': tuple(aim.astype(np.float64)),
                     'delta': float(delta.astype(np.float64))})
    return steer, throttle, brake, metadata


# ----------------------------------------------------------------------------------------------------------------------------
# The closed-loop tick (carla_agent.py:363-480) without the simulator classes.
# ----------------------------------------------------------------------------------------------------------------------------
class DriveResult:
    """What one tick returns: ``steer`` / ``throttle`` / ``brake`` (floats, after the agent's post-rules), the PID ``metadata``
    dictionary (None during the warm-up) and the planned ``trajectory`` (1, n_future, 3) float32 on the host (None during it)."""
    __slots__ = ('steer', 'throttle', 'brake', 'metadata', 'trajectory')

    def __init__(self, steer=0.0, throttle=0.0, brake=0.0, metadata=None, trajectory=None):
        self.steer, self.throttle, self.brake, self.metadata, self.trajectory = steer, throttle, brake, metadata, trajectory


class ClosedLoopDriver:
    """``MVPAgent.run_step`` (carla_agent.py:363-480) on ``inference.StreamingEngine``:

        driver = ClosedLoopDriver(model)                       # STP3 with the planner, eval mode, on the GPU
        res = driver.run_step(frames, pos, compass, speed, next_command, next_wp)

    ``frames`` (4, Hs, Ws, 4) uint8 BGRA (front, left, right, rear) on the device or in pinned host memory; ``pos`` the position
    in the route planner's frame, ``compass`` / ``speed`` the IMU's and the speedometer's values, ``next_command`` /
    ``next_wp`` the route planner's answer for ``pos``.  Per tick: ONE ``stp3_carla_frames`` launch straight into the engine's
    static image, the pose windows, ``StreamingEngine.step``, the trajectory sampler with the last steer, the planner, one copy
    of the chosen trajectory to the host, ``control_pid`` and the agent's post-rules.  The first ``warm_ticks`` ticks return zero
    control and only buffer (the engine's tail runs on them and its result is discarded).  ``planner``: 'forward' (the default) --
    the agent's own statements, argmax / logical_or / ``model.planning(...)``, whose GRU refinement runs in the autocast dtype: the
    tick is then bit-equal to the agent's written out with the plain model -- or 'drive' -- ``ops_plan.plan_scene`` +
    ``Planning.drive``, two launches with the refinement in float32 (the same candidate is selected; the refined way points differ
    from the autocast ones by the bf16 rounding of that path, 2.4e-3 m in tests/test_carla_gpu.py).  ``generator``: the device
    generator the sampler draws from."""

    def __init__(self, model, warm_ticks=4, source_hw=(SENSOR['height'], SENSOR['width']), autocast_dtype=torch.bfloat16,
                 image_dtype=torch.float32, planner='forward', generator=None, decoder=None):
        from .inference import StreamingEngine
        if planner not in ('drive', 'forward'):
            raise ValueError(f"planner must be 'drive' or 'forward': {planner!r}")
        cfg = model.cfg
        self.model, self.planner, self.generator, self.autocast_dtype = model, planner, generator, autocast_dtype
        self.frames_t, self.n_future = int(model.receptive_field), int(cfg.N_FUTURE_FRAMES)
        self.sample_num = int(cfg.PLANNING.SAMPLE_NUM)
        self.warm_ticks = int(warm_ticks)
        if self.warm_ticks < self.frames_t - 1:
            raise ValueError(f'warm_ticks = {warm_ticks}: the window of {self.frames_t} frames is not full after them')
        self.decoder = decoder if decoder is not None else CarlaDecoder(cfg)
        self.source_hw = tuple(source_hw)
        self.device = next(model.parameters()).device
        c, t = self.decoder.crop, self.frames_t
        extrinsics, intrinsics = cam_para(c)
        self.extrinsics = extrinsics.unsqueeze(0).expand(t, 4, 4, 4).unsqueeze(0).contiguous()
        self.intrinsics = intrinsics.unsqueeze(0).expand(t, 4, 3, 3).unsqueeze(0).contiguous()
        example = (torch.zeros(1, t, 4, 3, c, c, dtype=image_dtype, device=self.device), self.intrinsics, self.extrinsics,
                   torch.zeros(1, t, 6))
        self.engine = StreamingEngine(model, example, autocast_dtype=autocast_dtype)
        self.reset()

    def reset(self):
        """A new route: clears the pose windows, the PID state, ``last_steer`` and the engine's caches."""
        self.step = -1
        self.gps, self.thetas = deque(maxlen=self.frames_t), deque(maxlen=self.frames_t)
        self.turn, self.speed = turn_controller(), speed_controller()
        self.last_steer = 0
        self.engine.reset()

    def _egomotion(self):
        """(1, T, 6): ``future_egomotion`` of the pose windows (T - 1 rows) and one zero row (the model reads the first T - 1); a
        window that is not full yet (warm-up) is padded with its oldest pose."""
        pad = self.frames_t - len(self.gps)
        gps, thetas = [self.gps[0]] * pad + list(self.gps), [self.thetas[0]] * pad + list(self.thetas)
        ego = future_egomotion([p[0] for p in gps], [p[1] for p in gps], thetas)
        return torch.cat([ego, torch.zeros(1, 6)], dim=0).unsqueeze(0)

    @torch.no_grad()
    def run_step(self, frames, pos, compass, speed, next_command, next_wp):
        self.step += 1
        engine, dev = self.engine, self.device
        if tuple(frames.shape) != (4,) + self.source_hw + (4,) or frames.dtype != torch.uint8:
            raise ValueError(f'frames: (4, {self.source_hw[0]}, {self.source_hw[1]}, 4) uint8 BGRA expected, got '
                             f'{tuple(frames.shape)} {frames.dtype}')
        if not frames.is_cuda:
            frames = frames.to(dev, non_blocking=True)
        self.decoder.images(frames, order='bgr', out_dtype=engine.image.dtype, out=engine.image)
        self.gps.append((pos[0], pos[1]))
        self.thetas.append(compass)
        out = engine.step(engine.image, self.intrinsics, self.extrinsics, self._egomotion())
        if self.step < self.warm_ticks:
            return DriveResult()
        rf, model = self.frames_t, self.model
        command = command_name(next_command)
        target = local_command_point(pos, compass, next_wp).to(dev, dtype=torch.float32).unsqueeze(0)
        trajs = trajectory_sampling(torch.tensor([speed], dtype=torch.float64, device=dev),
                                    torch.tensor([self.last_steer], dtype=torch.float64, device=dev), self.n_future,
                                    self.sample_num, generator=self.generator)
        with torch.autocast('cuda', dtype=self.autocast_dtype, enabled=self.autocast_dtype is not None):
            if self.planner == 'drive':
                from . import ops_plan
                occupancy, lane, drivable = ops_plan.plan_scene(out['segmentation'], out['pedestrian'], out['hdmap'], rf)
                final = model.planning.drive(out['cam_front'], trajs[:, :, 1:], out['costvolume'][:, rf:], occupancy, lane, drivable,
                                             ops_plan.command_codes([command], device=dev), target)[0]
            else:
                seg = torch.argmax(out['segmentation'], dim=2, keepdim=True)
                ped = torch.argmax(out['pedestrian'], dim=2, keepdim=True)
                occupancy = torch.logical_or(seg, ped)
                _, final = model.planning(cam_front=out['cam_front'], trajs=trajs[:, :, 1:], gt_trajs=None,
                                          cost_volume=out['costvolume'][:, rf:], semantic_pred=occupancy[:, rf:].squeeze(2),
                                          hd_map=out['hdmap'], commands=[command], target_points=target)
        trajectory = final.float().cpu().numpy()                                # the tick's one device-to-host copy
        steer, throttle, brake, metadata = control_pid(trajectory, np.float32(speed), self.turn, self.speed, command=next_command)
        self.last_steer = steer
        if brake < 0.05:
            brake = 0.0
        if throttle > brake:
            brake = 0.0
        return DriveResult(float(steer), float(throttle), float(brake), metadata, trajectory)
