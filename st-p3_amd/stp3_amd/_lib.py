"""ctypes binding of libstp3hip.so (the C ABI declared in include/stp3_hip.h).

The library is the product: there is no CPU or PyTorch fallback for the operators it
exports.  ``lib()`` raises if the shared object is missing or lacks a symbol, and every
operator in ``stp3_amd.ops`` raises if it is handed non-GPU tensors.
"""
import ctypes
import os

from . import profiling

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libstp3hip.so')
_PRODUCT_LIB_PATH = LIB_PATH

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_int32 = ctypes.c_int32
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t


class LiftDims(ctypes.Structure):
    """struct stp3_lift_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('B', 'T', 'N', 'D', 'fH', 'fW', 'C', 'X', 'Y', 'Z')]

    @property
    def BT(self):
        return self.B * self.T

    @property
    def NPIX(self):
        return self.N * self.fH * self.fW

    @property
    def P(self):
        return self.NPIX * self.D

    @property
    def V(self):
        return self.X * self.Y * self.Z


class DwConvDims(ctypes.Structure):
    """struct stp3_dwconv_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'H', 'W', 'C', 'Ho', 'Wo', 'K', 'stride', 'pad_top', 'pad_left',
                                              'dtype')]


class WgradJob(ctypes.Structure):
    """struct stp3_wgrad_job (include/stp3_hip.h)."""
    _fields_ = [('partials', ctypes.c_void_p), ('dw', ctypes.c_void_p), ('numel', ctypes.c_int64), ('splits', ctypes.c_int32),
                ('reserved', ctypes.c_int32)]


class LayerNormDims(ctypes.Structure):
    """struct stp3_layernorm_dims (include/stp3_hip.h)."""
    _fields_ = [('rows', ctypes.c_int64), ('C', ctypes.c_int32), ('ldx', ctypes.c_int32), ('ldy', ctypes.c_int32),
                ('dtype', ctypes.c_int32), ('act', ctypes.c_int32), ('eps', ctypes.c_float)]


class GruDims(ctypes.Structure):
    """struct stp3_gru_dims (include/stp3_hip.h)."""
    _fields_ = [('rows', ctypes.c_int64), ('Cx', ctypes.c_int32), ('C', ctypes.c_int32), ('dtype', ctypes.c_int32),
                ('bias_init', ctypes.c_float)]


class BnDims(ctypes.Structure):
    """struct stp3_bn_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'rows', 'C', 'ldx', 'ldy', 'ldr', 'dtype', 'act', 'res_mode',
                                              'has_sbias', 'has_oscale', 'cpad')]


class ConvDims(ctypes.Structure):
    """struct stp3_conv_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad_h',
                                              'pad_w', 'dil_h', 'dil_w', 'ldx', 'ldy', 'out_dtype', 'has_bias')]


class SeDims(ctypes.Structure):
    """struct stp3_se_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'rows', 'C', 'ld', 'dtype')]


class WprepEntry(ctypes.Structure):
    """struct stp3_wprep_entry (include/stp3_hip.h)."""
    _fields_ = [('src', ctypes.c_void_p), ('fwd', ctypes.c_void_p), ('flip', ctypes.c_void_p),
                ('stride_co', ctypes.c_int64), ('stride_ci', ctypes.c_int64), ('stride_kh', ctypes.c_int64),
                ('stride_kw', ctypes.c_int64), ('first_block', ctypes.c_int64),
                ('cout', ctypes.c_int32), ('cin', ctypes.c_int32), ('kh', ctypes.c_int32), ('kw', ctypes.c_int32),
                ('dst_cout', ctypes.c_int32), ('dst_cin', ctypes.c_int32), ('co_off', ctypes.c_int32),
                ('ci_off', ctypes.c_int32), ('fwd_f32', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class BnCoefEntry(ctypes.Structure):
    """struct stp3_bn_coef_entry (include/stp3_hip.h)."""
    _fields_ = [('running_mean', ctypes.c_void_p), ('running_var', ctypes.c_void_p), ('gamma', ctypes.c_void_p),
                ('beta', ctypes.c_void_p), ('out', ctypes.c_void_p), ('first_block', ctypes.c_int64),
                ('channels', ctypes.c_int32), ('lanes', ctypes.c_int32), ('eps', ctypes.c_float), ('reserved', ctypes.c_int32)]


class SeMlpDims(ctypes.Structure):
    """struct stp3_se_mlp_dims (include/stp3_hip.h)."""
    _fields_ = [('N', ctypes.c_int32), ('C', ctypes.c_int32), ('S', ctypes.c_int32), ('inv_rows', ctypes.c_float)]


class PairDims(ctypes.Structure):
    """struct stp3_pair_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('frames', 'T', 'rows', 'C', 'ldx', 'dtype')]


class UpsampleDims(ctypes.Structure):
    """struct stp3_upsample_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'H', 'W', 'C', 'scale', 'ldx', 'ldy', 'dtype')]


class CeDims(ctypes.Structure):
    """struct stp3_ce_dims (include/stp3_hip.h)."""
    _fields_ = [('rows', ctypes.c_int32), ('P', ctypes.c_int32), ('C', ctypes.c_int32), ('k', ctypes.c_int32),
                ('ignore_index', ctypes.c_int32), ('dtype', ctypes.c_int32), ('stride_row', ctypes.c_int64),
                ('stride_c', ctypes.c_int64), ('stride_p', ctypes.c_int64)]


class PlanDims(ctypes.Structure):
    """struct stp3_plan_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('B', 'N', 'T', 'H', 'W', 'K0', 'KL')] +
                [(k, ctypes.c_float) for k in ('dx0', 'dx1', 'bx0', 'bx1', 'safety', 'headway', 'lrdivider', 'comfort',
                                               'progress', 'volume', 'rule', 'w0', 'w1', 'headway_dist', 'lr_dist')])


class SceneDims(ctypes.Structure):
    """struct stp3_scene_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('B', 'S', 'T', 'H', 'W', 'Cs', 'Cp', 'first', 'seg_dtype', 'ped_dtype', 'hd_dtype')] +
                [('seg_stride', ctypes.c_int64 * 5), ('ped_stride', ctypes.c_int64 * 5), ('hd_stride', ctypes.c_int64 * 4)])


class DriveDims(ctypes.Structure):
    """struct stp3_drive_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('Hs', 'traj_cols', 'cv_dtype', 'h0_dtype')] +
                [(k, ctypes.c_int64) for k in ('traj_batch_stride', 'traj_row_stride', 'traj_point_stride', 'cv_batch_stride')] +
                [('weights', ctypes.c_void_p)])


class SamplerDims(ctypes.Structure):
    """struct stp3_sampler_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('B', 'M', 'n_left', 'n_straight', 'n_right', 'n_future')] +
                [('dt', ctypes.c_double), ('sort', ctypes.c_int32)])


class ImageDims(ctypes.Structure):
    """struct stp3_image_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('N', 'H', 'W', 'Wr', 'Hr', 'left', 'top', 'Wo', 'Ho', 'ksize_h', 'ksize_v',
                                               'out_dtype')] + [('mean', ctypes.c_float * 3), ('std', ctypes.c_float * 3)])


class AugmentImage(ctypes.Structure):
    """struct stp3_augment_image (include/stp3_hip.h): 16 int32."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('Wr', 'Hr', 'left', 'top', 'flip')] + [('rot', ctypes.c_int32 * 6)] +
                [(k, ctypes.c_int32) for k in ('kk_h', 'bounds_h', 'kk_v', 'bounds_v', 'reserved')])


class AugmentDims(ctypes.Structure):
    """struct stp3_augment_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('N', 'H', 'W', 'Wo', 'Ho', 'cols', 'ksize', 'strip_rows', 'rotate', 'coef_len',
                                               'out_dtype')] + [('mean', ctypes.c_float * 3), ('std', ctypes.c_float * 3)])


class JpegHeader(ctypes.Structure):
    """struct stp3_jpeg_header (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('width', 'height', 'components', 'hs', 'vs', 'mcus_x', 'mcus_y')] +
                [('blocks_x', ctypes.c_int32 * 3), ('blocks_y', ctypes.c_int32 * 3), ('restart_interval', ctypes.c_int32),
                 ('coef_count', ctypes.c_int32)])


class JpegDims(ctypes.Structure):
    """struct stp3_jpeg_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'width', 'height', 'components', 'hs', 'vs')]


class JpegHuffTable(ctypes.Structure):
    """struct stp3_jpeg_huff_table (include/stp3_hip.h)."""
    _fields_ = [('look', ctypes.c_uint16 * 512), ('maxcode', ctypes.c_int32 * 18), ('valptr', ctypes.c_int32 * 17),
                ('vals', ctypes.c_uint8 * 256)]


class JpegScanDesc(ctypes.Structure):
    """struct stp3_jpeg_scan_desc (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('nsub', 'nseg', 'seg_offset', 'scan_offset', 'subseg_offset', 'used_bytes', 'components',
                                               'hs', 'vs', 'mcus_x', 'mcus_y', 'restart_interval', 'coef_count')] +
                [('dc_table', ctypes.c_int32 * 3), ('ac_table', ctypes.c_int32 * 3), ('quant', ctypes.c_uint16 * 64 * 3),
                 ('dc', JpegHuffTable * 2), ('ac', JpegHuffTable * 2)])


class JpegHuffDims(ctypes.Structure):
    """struct stp3_jpeg_huff_dims (include/stp3_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'width', 'height', 'components', 'hs', 'vs', 'scan_stride', 'max_subs', 'max_segs')]


STP3_JPEG_IRREGULAR, STP3_JPEG_NOT_CONVERGED = 10011, 10012                 # include/stp3_hip.h
JPEG_SUB_BYTES, JPEG_SUB_THREADS = 128, 256                                 # STP3_JPEG_SUB_BYTES, STP3_JPEG_SUB_THREADS


class Poly(ctypes.Structure):
    """struct stp3_poly (include/stp3_hip.h)."""
    _fields_ = [('map', ctypes.c_int32), ('nv', ctypes.c_int32), ('value', ctypes.c_float), ('reserved', ctypes.c_int32),
                ('xy', ctypes.c_int32 * 16)]


class DepthAxis(ctypes.Structure):
    """struct stp3_depth_axis (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_void_p) for k in ('tap', 'weight', 'slot_src', 'src_slot')] +
                [(k, ctypes.c_int32) for k in ('n_out', 'n_slot', 'n_src', 'reserved')])


class DepthDims(ctypes.Structure):
    """struct stp3_depth_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('F', 'N', 'n_total', 'out_kind')] +
                [('d_lo', ctypes.c_float), ('d_hi', ctypes.c_float), ('y', DepthAxis), ('x', DepthAxis)])


class AugmentDepthAxis(ctypes.Structure):
    """struct stp3_augment_depth_axis (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_void_p) for k in ('tap', 'weight', 'slot_src')] +
                [(k, ctypes.c_int32) for k in ('entries', 'slots')])


class AugmentDepthDims(ctypes.Structure):
    """struct stp3_augment_depth_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('F', 'N', 'n_total', 'out_kind')] +
                [('d_lo', ctypes.c_float), ('d_hi', ctypes.c_float)] +
                [(k, ctypes.c_int32) for k in ('H', 'W', 'Ho', 'Wo', 'stride', 'separable')] +
                [('records', ctypes.c_void_p), ('y', AugmentDepthAxis), ('x', AugmentDepthAxis)])


class EvalDims(ctypes.Structure):
    """struct stp3_eval_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('B', 'S', 'H', 'W', 'Cs', 'Cp', 'E', 'n_classes', 'first', 'seg_dtype', 'ped_dtype',
                                               'hd_dtype')] +
                [('seg_stride', ctypes.c_int64 * 5), ('ped_stride', ctypes.c_int64 * 5), ('hd_stride', ctypes.c_int64 * 4)])


class EvalPlanDims(ctypes.Structure):
    """struct stp3_eval_plan_dims (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('B', 'T', 'S', 'H', 'W', 'K', 'first_future')] +
                [(k, ctypes.c_float) for k in ('dx0', 'dx1', 'bx0', 'bx1')] +
                [('traj_stride', ctypes.c_int64 * 2), ('gt_stride', ctypes.c_int64 * 2)])


class WindowJob(ctypes.Structure):
    """struct stp3_window_job (include/stp3_hip.h)."""
    _fields_ = [('src', ctypes.c_void_p), ('window', ctypes.c_void_p), ('stride_image', ctypes.c_int64),
                ('stride_channel', ctypes.c_int64), ('stride_pixel', ctypes.c_int64), ('channels', ctypes.c_int32),
                ('dtype', ctypes.c_int32)]


class OptimBucket(ctypes.Structure):
    """struct stp3_optim_bucket (include/stp3_hip.h)."""
    _fields_ = [('grad', ctypes.c_void_p), ('param', ctypes.c_void_p), ('exp_avg', ctypes.c_void_p),
                ('exp_avg_sq', ctypes.c_void_p), ('numel', ctypes.c_int64), ('first_block', ctypes.c_int64)]


class VisMap(ctypes.Structure):
    """struct stp3_vis_map (include/stp3_hip.h)."""
    _fields_ = ([('ptr', ctypes.c_void_p)] + [(k, ctypes.c_int64) for k in ('stride_t', 'stride_c', 'stride_h', 'stride_w')] +
                [('dtype', ctypes.c_int32), ('reserved', ctypes.c_int32)])


class VisPlan(ctypes.Structure):
    """struct stp3_vis_plan (include/stp3_hip.h)."""
    _fields_ = ([('hdmap', ctypes.c_void_p)] + [(k, ctypes.c_int64) for k in ('hd_stride_c', 'hd_stride_h', 'hd_stride_w')] +
                [('traj', ctypes.c_void_p), ('traj_stride_p', ctypes.c_int64), ('traj_stride_c', ctypes.c_int64),
                 ('hd_dtype', ctypes.c_int32), ('n_points', ctypes.c_int32)])


class VisDesc(ctypes.Structure):
    """struct stp3_vis_desc (include/stp3_hip.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('T', 'H', 'W', 'panels')] +
                [(k, VisMap * 2) for k in ('seg', 'ped', 'inst', 'center', 'offset', 'flow')] + [('plan', VisPlan * 2)] +
                [(k, ctypes.c_void_p) for k in ('ego_cells', 'palette', 'jet', 'wheel')] + [('n_ego', ctypes.c_int32)] +
                [(k, ctypes.c_float) for k in ('dx0', 'dx1', 'bx0', 'bx1')] + [('reserved', ctypes.c_int32)])


DTYPE_F32 = 0
DTYPE_BF16 = 1
VIS_DTYPE_I64 = 2
VIS_INSTANCE, VIS_FLOW, VIS_PEDESTRIAN, VIS_PLAN_LABELS, VIS_PLAN_PRED = 1, 2, 4, 8, 16
DEPTH_OUT_F32, DEPTH_OUT_F64, DEPTH_OUT_LABELS = 0, 1, 2
CARLA_OUT_F32, CARLA_OUT_F64, CARLA_OUT_I64 = 0, 1, 2

WINDOW_JOBS_MAX = 4
VOX_REFERENCE = 0
VOX_PIXELMAJOR = 1
BEV_CHANNELS_FIRST = 0
BEV_CHANNELS_LAST = 1
BEV_CHANNELS_LAST_BF16 = 2

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2
ACT_GELU = 3                  # stp3_layernorm_* only
RES_NONE, RES_BEFORE_ACT, RES_AFTER_ACT = 0, 1, 2

_DIMS_P = ctypes.POINTER(LiftDims)
_BN_P = ctypes.POINTER(BnDims)
c_double = ctypes.c_double
_DW_P = ctypes.POINTER(DwConvDims)
_LN_P = ctypes.POINTER(LayerNormDims)
_GRU_P = ctypes.POINTER(GruDims)

# name -> (restype, argtypes); mirrors include/stp3_hip.h one to one
SIGNATURES = {
    'stp3_version': (ctypes.c_char_p, []),
    'stp3_voxel_index': (c_int, [_DIMS_P] + [c_void_p] * 9 + [c_int, c_void_p, c_void_p, c_void_p]),
    'stp3_lift_plan_bytes': (c_int, [_DIMS_P, ctypes.POINTER(c_size_t)]),
    'stp3_lift_plan_build': (c_int, [_DIMS_P] + [c_void_p] * 12 + [c_size_t, c_void_p]),
    'stp3_depth_softmax': (c_int, [_DIMS_P, c_void_p, c_void_p, c_void_p]),
    'stp3_lift_workspace_bytes': (c_int, [_DIMS_P, ctypes.POINTER(c_size_t)]),
    'stp3_lift_splat_fwd': (c_int, [_DIMS_P, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_size_t,
                                    c_void_p, c_void_p, c_void_p]),
    'stp3_lift_bwd_needs_prob': (c_int, [_DIMS_P, ctypes.POINTER(c_int)]),
    'stp3_lift_splat_bwd': (c_int, [_DIMS_P, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_float, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    'stp3_gru_reset_cat_fwd': (c_int, [_GRU_P, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_gru_output_fwd': (c_int, [_GRU_P, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_gru_output_bwd': (c_int, [_GRU_P, c_void_p, ctypes.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_gru_reset_cat_bwd': (c_int, [_GRU_P, c_void_p, ctypes.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_layernorm_fwd': (c_int, [_LN_P, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_layernorm_bwd_workspace': (c_int, [_LN_P, ctypes.POINTER(c_size_t)]),
    'stp3_layernorm_bwd': (c_int, [_LN_P] + [c_void_p] * 8 + [c_size_t, c_void_p]),
    'stp3_dwconv2d_fwd': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_dwconv2d_fwd_bias': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_dwconv2d_bwd_data': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_dwconv2d_bwd_weight_workspace': (c_int, [_DW_P, ctypes.POINTER(c_size_t)]),
    'stp3_dwconv2d_bwd_weight': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_dwconv2d_bwd_weight_oihw': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_bn_workspace_bytes': (c_int, [_BN_P, ctypes.POINTER(c_size_t)]),
    'stp3_bn_stats': (c_int, [_BN_P, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'stp3_bn_apply_fwd': (c_int, [_BN_P] + [c_void_p] * 5 + [c_double, c_void_p, c_void_p, c_float, c_float]
                          + [c_void_p] * 6),
    'stp3_bn_bwd_reduce': (c_int, [_BN_P] + [c_void_p] * 10 + [c_size_t, c_void_p, c_void_p, c_void_p]),
    'stp3_bn_apply_bwd': (c_int, [_BN_P] + [c_void_p] * 10 + [c_double, c_void_p, c_void_p, c_void_p]),
    'stp3_bn_fwd_train': (c_int, [_BN_P] + [c_void_p] * 6 + [c_float, c_float] + [c_void_p] * 4 + [c_size_t, c_void_p,
                                                                                                 c_void_p]),
    'stp3_bn_bwd_train': (c_int, [_BN_P] + [c_void_p] * 10 + [c_size_t] + [c_void_p] * 4),
    'stp3_bn_dsbias': (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_sum_n': (c_int, [c_int32, ctypes.c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    'stp3_linear_fwd': (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    'stp3_linear_bwd': (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                c_void_p]),
    'stp3_sum_n_plane': (c_int, [c_int32, ctypes.c_int64, c_int32, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_void_p, c_void_p]),
    'stp3_conv2d_fwd_workspace': (c_int, [ctypes.POINTER(ConvDims), ctypes.POINTER(c_size_t)]),
    'stp3_conv2d_fwd': (c_int, [ctypes.POINTER(ConvDims)] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    'stp3_conv2d_fwd_add': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_conv2d_fwd_stats': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_conv2d_fwd_bnact': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_conv2d_bn_bwd_reduce': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_conv2d_bn_bwd_apply': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                         c_void_p, c_double, c_void_p, c_void_p]),
    'stp3_se_workspace_bytes': (c_int, [ctypes.POINTER(SeDims), ctypes.POINTER(c_size_t)]),
    'stp3_se_pool': (c_int, [ctypes.POINTER(SeDims), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'stp3_se_scale': (c_int, [ctypes.POINTER(SeDims), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_conv2d_bn_bwd_apply_dx': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                            ctypes.c_double, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    'stp3_conv2d_wgrad_workspace': (c_int, [ctypes.POINTER(ConvDims), ctypes.POINTER(c_size_t)]),
    'stp3_conv2d_wgrad': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_conv2d_wgrad_partials': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
                                           ctypes.POINTER(c_int32), c_void_p]),
    'stp3_conv2d_fwd_pre': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_conv2d_wgrad_pre': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    'stp3_conv2d_wgrad_reduce_batch': (c_int, [c_int32, ctypes.POINTER(WgradJob), c_void_p]),
    'stp3_conv2d_prep_weights': (c_int, [c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    'stp3_conv2d_scatter_weight_grads': (c_int, [c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    'stp3_se_mlp_fwd': (c_int, [c_void_p] * 9),
    'stp3_se_mlp_bwd': (c_int, [c_void_p] * 15),
    'stp3_optim_workspace_bytes': (c_int, [ctypes.c_int64, ctypes.POINTER(c_size_t)]),
    'stp3_optim_clip_adam': (c_int, [c_void_p, c_int32, ctypes.c_int64] + [c_float] * 6 + [c_void_p, c_void_p, c_size_t,
                                                                                          c_void_p]),
    'stp3_causal_pair_fwd': (c_int, [ctypes.POINTER(PairDims), c_void_p, c_void_p, c_void_p]),
    'stp3_causal_pair_bwd': (c_int, [ctypes.POINTER(PairDims), c_void_p, c_void_p, c_void_p]),
    'stp3_upsample_bilinear_fwd': (c_int, [ctypes.POINTER(UpsampleDims), c_void_p, c_void_p, c_void_p]),
    'stp3_upsample_bilinear_bwd': (c_int, [ctypes.POINTER(UpsampleDims), c_void_p, c_void_p, c_void_p]),
    'stp3_dwconv2d_fwd_stats_workspace': (c_int, [_DW_P, ctypes.POINTER(c_size_t)]),
    'stp3_dwconv2d_fwd_stats': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_bn_finalize': (c_int, [c_void_p, c_int32, c_double, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    'stp3_mbconv_workspace_bytes': (c_int, [ctypes.POINTER(SeDims), ctypes.POINTER(c_size_t)]),
    'stp3_se_pool_act': (c_int, [ctypes.POINTER(SeDims), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p,
                                 c_void_p]),
    'stp3_mbconv_scale_act': (c_int, [ctypes.POINTER(SeDims), c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                      c_void_p, c_void_p]),
    'stp3_mbconv_bwd_reduce': (c_int, [ctypes.POINTER(SeDims), c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_size_t, c_void_p, c_void_p]),
    'stp3_mbconv_bwd_coef': (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_mbconv_bwd_apply': (c_int, [ctypes.POINTER(SeDims), c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                      c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    'stp3_dwconv2d_fwd_stats_bn': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_float,
                                           c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'stp3_ce_topk_workspace_bytes': (c_int, [ctypes.POINTER(CeDims), ctypes.POINTER(c_size_t)]),
    'stp3_ce_topk_fwd': (c_int, [ctypes.POINTER(CeDims)] + [c_void_p] * 6 + [c_double, c_int32, c_void_p, c_void_p, c_size_t,
                                                                           c_void_p]),
    'stp3_ce_topk_bwd': (c_int, [ctypes.POINTER(CeDims)] + [c_void_p] * 7 + [c_double, c_void_p, c_void_p]),
    'stp3_reg_loss_workspace_bytes': (c_int, [ctypes.POINTER(c_size_t)]),
    'stp3_reg_loss_fwd': (c_int, [c_int32] * 4 + [c_float, c_int32] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    'stp3_reg_loss_bwd': (c_int, [c_int32] * 4 + [c_float, c_int32] + [c_void_p] * 7),
    'stp3_warp_nearest': (c_int, [c_int32] * 4 + [c_void_p] * 5),
    'stp3_traj_cost_fwd': (c_int, [ctypes.POINTER(PlanDims)] + [c_void_p] * 14),
    'stp3_traj_cost_bwd': (c_int, [ctypes.POINTER(PlanDims)] + [c_void_p] * 5),
    'stp3_plan_scene': (c_int, [ctypes.POINTER(SceneDims)] + [c_void_p] * 7),
    'stp3_plan_drive': (c_int, [ctypes.POINTER(PlanDims), ctypes.POINTER(DriveDims)] + [c_void_p] * 14),
    'stp3_traj_sample': (c_int, [ctypes.POINTER(SamplerDims)] + [c_void_p] * 6),
    'stp3_instance_segment': (c_int, [c_int32] * 3 + [c_float] + [c_void_p] * 7),
    'stp3_instance_track': (c_int, [c_int32] * 4 + [c_float] + [c_void_p] * 5),
    'stp3_eval_semantic': (c_int, [ctypes.POINTER(EvalDims)] + [c_void_p] * 8),
    'stp3_eval_planning': (c_int, [ctypes.POINTER(EvalPlanDims)] + [c_void_p] * 10),
    'stp3_eval_panoptic_workspace_bytes': (c_int, [c_int32] * 3 + [ctypes.POINTER(c_size_t)]),
    'stp3_eval_panoptic': (c_int, [c_int32] * 7 + [c_void_p] * 3 + [c_size_t] + [c_void_p] * 3),
    'stp3_image_prep_rows_per_workgroup': (c_int, []),
    'stp3_image_prep_lds_bytes': (c_int, [ctypes.POINTER(ImageDims), c_int32, ctypes.POINTER(c_size_t)]),
    'stp3_image_prep': (c_int, [ctypes.POINTER(ImageDims)] + [c_void_p] * 5 + [c_int32, c_void_p, c_void_p]),
    'stp3_image_augment_workspace_bytes': (c_int, [ctypes.POINTER(AugmentDims), ctypes.POINTER(c_size_t)]),
    'stp3_image_augment': (c_int, [ctypes.POINTER(AugmentDims)] + [c_void_p] * 4 + [c_size_t, c_void_p, c_void_p]),
    'stp3_jpeg_info': (c_int, [c_void_p, c_size_t, ctypes.POINTER(JpegHeader)]),
    'stp3_jpeg_entropy': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, ctypes.POINTER(JpegHeader)]),
    'stp3_jpeg_strip_rows': (c_int, [c_int32]),
    'stp3_jpeg_reconstruct': (c_int, [ctypes.POINTER(JpegDims), c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_jpeg_scan_bytes': (c_size_t, [ctypes.POINTER(JpegHeader), c_size_t]),
    'stp3_jpeg_scan_prepare': (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    'stp3_jpeg_entropy_workspace_bytes': (c_int, [ctypes.POINTER(JpegHuffDims), c_int32, ctypes.POINTER(c_size_t)]),
    'stp3_jpeg_entropy_device': (c_int, [ctypes.POINTER(JpegHuffDims)] + [c_void_p] * 5 + [c_size_t, c_int32, c_void_p]),
    'stp3_fill_polygons': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    'stp3_instance_labels_workspace_bytes': (c_int, [c_int32, c_int32, ctypes.POINTER(c_size_t)]),
    'stp3_instance_labels': (c_int, [c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                     c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    'stp3_depth_project': (c_int, [c_int32] * 5 + [c_void_p] * 3 + [c_int32] + [c_void_p] * 5),
    'stp3_depth_workspace_bytes': (c_int, [ctypes.POINTER(DepthDims), ctypes.POINTER(c_size_t)]),
    'stp3_depth_from_pixels': (c_int, [ctypes.POINTER(DepthDims)] + [c_void_p] * 5 + [c_size_t, c_void_p, c_void_p]),
    'stp3_depth_from_lidar': (c_int, [ctypes.POINTER(DepthDims)] + [c_void_p] * 3 + [c_int32] + [c_void_p] * 2 +
                              [c_size_t, c_void_p, c_void_p]),
    'stp3_depth_labels_bands': (c_int, [ctypes.POINTER(DepthDims), c_int32, ctypes.POINTER(c_int32)]),
    'stp3_depth_labels_from_lidar': (c_int, [ctypes.POINTER(DepthDims)] + [c_void_p] * 3 + [c_int32, c_void_p, c_int32,
                                                                                         c_void_p, c_void_p]),
    'stp3_depth_from_maps': (c_int, [ctypes.POINTER(DepthDims), c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_augment_depth_workspace_bytes': (c_int, [ctypes.POINTER(AugmentDepthDims), ctypes.POINTER(c_size_t)]),
    'stp3_augment_depth_from_lidar': (c_int, [ctypes.POINTER(AugmentDepthDims)] + [c_void_p] * 3 + [c_int32] + [c_void_p] * 2 +
                                      [c_size_t, c_void_p, c_void_p]),
    'stp3_augment_depth_from_maps': (c_int, [ctypes.POINTER(AugmentDepthDims), c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_voxels_sum_fwd': (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    'stp3_voxels_sum_bwd': (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    'stp3_bn_eval_coefs': (c_int, [c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    'stp3_conv2d_fwd_affine': (c_int, [ctypes.POINTER(ConvDims), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                       c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    'stp3_linear_fwd_affine': (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                       c_void_p, c_void_p]),
    'stp3_dwconv2d_fwd_affine': (c_int, [_DW_P, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    'stp3_window_push': (c_int, [c_int32] * 5 + [ctypes.POINTER(WindowJob), c_void_p]),
    'stp3_vis_workspace_bytes': (c_int, [ctypes.POINTER(VisDesc), ctypes.POINTER(c_size_t)]),
    'stp3_vis_render': (c_int, [ctypes.POINTER(VisDesc), c_void_p, c_void_p, c_void_p]),
    'stp3_carla_frames': (c_int, [c_int32] * 6 + [ctypes.POINTER(ctypes.c_float)] * 2 + [c_int32] + [c_void_p] * 3),
    'stp3_carla_depth': (c_int, [c_int32] * 6 + [c_double] * 2 + [c_void_p] * 3),
    'stp3_carla_hdmap': (c_int, [c_int32] * 5 + [c_void_p] * 3),
    'stp3_carla_topdown': (c_int, [c_int32] * 6 + [c_void_p] * 2 + [c_int32] + [c_void_p] * 4),
    'stp3_png_unfilter': (c_int, [c_void_p] + [c_int32] * 4 + [c_void_p] * 2),
}

_lib = None
_timed = None


class Stp3HipError(RuntimeError):
    pass


def _not_exported(name):
    def call(*args):
        raise Stp3HipError(f'{LIB_PATH} does not export {name}')
    return call


def lib():
    """Load libstp3hip.so once; fail loudly if it is absent or incomplete."""
    global _lib, _timed
    if _lib is not None:
        if profiling.ENABLED:                 # bench.py's roofline steps: every call bracketed by stream events
            if _timed is None:
                _timed = profiling.TimedLib(_lib)
            return _timed
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Stp3HipError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'(or `make -C st-p3_amd/csrc`).  There is no fallback path.')
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            if LIB_PATH == _PRODUCT_LIB_PATH:
                raise Stp3HipError(f'libstp3hip.so does not export {name}') from e
            # a library put in the product's place (the host stand-in of tests/hipcpu, built from some of the sources):
            # what it lacks is an error when it is called, not when the rest is loaded
            setattr(handle, name, _not_exported(name))
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return _lib


STP3_EINVAL, STP3_EUNSUP, STP3_ENOSPACE = -10001, -10002, -10003          # include/stp3_hip.h

_ERRORS = {-10001: 'STP3_EINVAL (bad dimension / null pointer)',
           -10002: 'STP3_EUNSUP (unsupported configuration)',
           -10003: 'STP3_ENOSPACE (workspace too small)'}


def check(rc, what):
    if rc != 0:
        raise Stp3HipError(f'{what} failed: {_ERRORS.get(rc, f"hipError {-rc}")}')
