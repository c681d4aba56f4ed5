/*
 * stp3_hip.h -- C ABI of libstp3hip.so: the MI355X (gfx950) implementation of ST-P3's
 * LSS camera->BEV lifting hot path.
 *
 * Boundary.  The reference is pure Python; the operator boundary this library replaces is
 *   - stp3/utils/geometry.py:299-330   VoxelsSumming.apply(x, geometry, ranks)
 * and, one level up, the code that feeds it:
 *   - stp3/models/stp3.py:186-201      STP3.get_geometry
 *   - stp3/models/stp3.py:215-221      softmax(depth) (x) feature outer product
 *   - stp3/models/stp3.py:226-301      STP3.projection_to_birds_eye_view (ego alignment,
 *                                      voxel index, sort, per-voxel sum, discounted accumulate)
 * The Python host (st-p3_amd/stp3_amd/ops.py) binds these entry points with ctypes and wraps
 * them in torch.autograd.Functions; INTEGRATION.md shows the stub a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - every pointer except `dims` is a DEVICE pointer into caller-owned memory that must stay
 *     valid until the work enqueued on `stream` has completed; the library allocates nothing;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only enqueue,
 *     they never synchronise, so they can be captured into a hipGraph;
 *   - return value: 0 on success, a negative hipError_t on a launch failure, or one of the
 *     STP3_E* codes for rejected arguments.  Nothing throws, nothing exits;
 *   - re-entrant: no global mutable state, no environment variables: every choice is an argument.
 *
 * Layouts ("pixel-major" = channels-last memory of the corresponding NCHW tensor)
 *   pix   = (n*fH + h)*fW + w                      camera pixel index inside one (b,t) frame
 *   feat  [B*T][N*fH*fW][C]     float32            encoder features   (stp3.py:208, x)
 *   depth [B*T][N*fH*fW][D]     float32            depth logits (and their gradient)
 *   prob_cm / vox_cm [B*T][N*fW][D][fH]            depth probabilities / voxel ids, column-major: (camera, column),
 *                                                  depth bin, image row
 *   vox   int32 voxel id = ix*(Y*Z) + iy*Z + iz, or -1 if the point falls outside the grid
 *   bev   [B][T][C][X][Y]       float32            reference layout (stp3.py:230-232)
 */
#ifndef STP3_HIP_H
#define STP3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STP3_OK          0
#define STP3_EINVAL   (-10001)  /* bad dimension / null pointer */
#define STP3_EUNSUP   (-10002)  /* valid request this build does not support (e.g. Z != 1 for pooling) */
#define STP3_ENOSPACE (-10003)  /* workspace too small */

/* element types of activation / gradient tensors */
#define STP3_DTYPE_F32  0
#define STP3_DTYPE_BF16 1

/* Problem shape.  P = N*D*fH*fW frustum points per (b,t); V = X*Y*Z voxels. */
typedef struct stp3_lift_dims {
    int32_t B, T, N;      /* batch, frames (time receptive field), cameras           */
    int32_t D, fH, fW;    /* depth bins, feature-map height/width                     */
    int32_t C;            /* feature channels (cfg.MODEL.ENCODER.OUT_CHANNELS)        */
    int32_t X, Y, Z;      /* BEV grid (geometry.py:56-57)                             */
} stp3_lift_dims;

/* order of the voxel-id array written by stp3_voxel_index */
#define STP3_VOX_REFERENCE  0   /* [B*T][N][D][fH][fW] -- the reference's flatten order (stp3.py:284) */
#define STP3_VOX_PIXELMAJOR 1   /* [B*T][N*fH*fW][D]   -- what the pooling kernels consume           */

/* library / build identification: returns a static string such as "stp3hip 0.1 gfx950" */
const char* stp3_version(void);

/*
 * stp3_voxel_index -- frustum point -> voxel id, bit-exact with the reference's CPU arithmetic.
 * Replaces stp3.py:192-198 (get_geometry), :270-277 (ego alignment), :287-289 (index),
 * :239-255 (range mask + rank).  Float32, one rounding per operation, left-to-right
 * ((m0*x + m1*y) + m2*z) + t, true division, truncation toward zero.
 *
 *   cam_m  [B*T*N][9]  R . K^-1 per camera (row-major 3x3), built by the host with torch CPU ops
 *   cam_t  [B*T*N][3]  camera translation in the ego frame
 *   ego_r  [B*T][9], ego_t [B*T][3]   pose_vec2mat(future_egomotion) (geometry.py:158-172);
 *          frame k of sample b is mapped by ego[b][k], ego[b][k+1], ..., ego[b][T-2] in turn
 *   xs [fW], ys [fH], ds [D]          the separable frustum (stp3.py:111-130)
 *   bev_offset [3] = bev_start - bev_res/2 (float32), bev_res [3]
 *   vox  [B*T*P] int32 out, in `order`
 *   counts [B*T*V] int32 or NULL: if non-NULL it must be zero-filled by the caller; the kernel
 *          adds the number of points per voxel (a diagnostic histogram; the plan does not need it).
 */
int stp3_voxel_index(const stp3_lift_dims* dims,
                     const float* cam_m, const float* cam_t,
                     const float* ego_r, const float* ego_t,
                     const float* xs, const float* ys, const float* ds,
                     const float* bev_offset, const float* bev_res,
                     int order, int32_t* vox, int32_t* counts, void* stream);

/*
 * Pooling plan: the geometry-only structure that the forward kernel consumes.  It replaces the
 * reference's get_geometry + ego alignment + index + boolean mask + argsort (stp3.py:192-198,
 * :270-277, :287-289, :239-257) and depends only on the camera / ego poses, so it can be built on a
 * side stream while the image encoder is running.
 *
 * Along an image column (camera n, feature column w, depth bin d) consecutive rows h fall into
 * the same BEV cell most of the time; a RUN is a maximal set of consecutive h with one voxel
 * id >= 0.  The forward pass sums every run once (pass 1, per image column) into the run's SLOT and
 * then every voxel over its runs (pass 2); the plan numbers the runs (slot = position in the
 * enumeration frame, column, last row, depth bin) and lists them per voxel in ascending order, so
 * that every voxel is summed in ONE fixed order.
 *
 *   stp3_lift_plan_bytes : size of the plan buffer for `dims`
 *   stp3_lift_plan_build : geometry inputs exactly as for stp3_voxel_index; writes
 *                            vox_cm [B*T][N*fW][D][fH] int32  voxel ids in COLUMN-MAJOR order (the same ids
 *                                                            stp3_voxel_index computes; the rows h of an image column
 *                                                            and depth bin are contiguous -- the order the backward
 *                                                            kernel walks them in)
 *                            plan   sections, each 256-byte aligned, in this order:
 *                                   vox_off  [B*T][V+1] int32   exclusive scan of runs per voxel, per frame
 *                                   masks    [B*T][N*fW][fH] 2 x uint64: bit d of word 0 = a run of depth bin d ENDS
 *                                            at this row, bit d of word 1 = point (d, h) lies inside the BEV grid
 *                                   col_cnt  [B*T*N*fW] int32   runs per column (scratch)
 *                                   col_off  [B*T*N*fW + 1] int32  exclusive scan over all frames: slot of the
 *                                            column's first run; col_off[bt*N*fW] = first slot of frame bt; the
 *                                            last entry = total number of runs
 *                                   tmp      [B*T*P] int32      (scratch)
 *                                   vox_runs [B*T*P] int32      slots of voxel v of frame bt, ascending, at
 *                                            col_off[bt*N*fW] + vox_off[bt][v] .. + vox_off[bt][v+1]
 *                                   run_desc [B*T*P] uint32     per slot: depth bin | first row << 8 | last row << 16
 *                                   run_vox  [B*T*P] int32      per slot: the run's voxel
 *                          counts = int32 [B*T][V] scratch that must be ZERO on entry (the caller zero-fills
 *                          it once; every build leaves it zero again).
 *   Launches: columns (ids, masks, counts), scan of the columns, scan of the voxels, fill, per-voxel order.
 *   Limits: Z == 1, C % 4 == 0, C <= 64, D <= 64, fH <= 128, N*fW < 4096, B*T*N*fH*fW*max(C,D)*4 < 2^32,
 *   else STP3_EUNSUP.
 */
int stp3_lift_plan_bytes(const stp3_lift_dims* dims, size_t* bytes);
int stp3_lift_plan_build(const stp3_lift_dims* dims,
                         const float* cam_m, const float* cam_t,
                         const float* ego_r, const float* ego_t,
                         const float* xs, const float* ys, const float* ds,
                         const float* bev_offset, const float* bev_res,
                         int32_t* vox_cm, int32_t* counts, void* plan, size_t plan_bytes, void* stream);

/* stp3_depth_softmax -- softmax over the D depth bins of every pixel (stp3.py:215).
 * logits [B*T][N*fH*fW][D] float32 (pixel-major) -> prob_cm [B*T][N*fW][D][fH] float32 (column-major; must not
 * alias logits).  stp3_lift_splat_fwd computes the same values on the fly; this entry point is the stand-alone
 * operator. */
int stp3_depth_softmax(const stp3_lift_dims* dims, const float* logits, float* prob, void* stream);

/* memory layout of the BEV tensor handed to / produced by the pooling calls */
#define STP3_BEV_CHANNELS_FIRST 0   /* [B][T][C][X][Y]  the reference's layout (stp3.py:230-232, :297-299)          */
#define STP3_BEV_CHANNELS_LAST  1   /* [B][T][X][Y][C]  = channels-last memory of the same (B,T,C,X,Y) tensor: what the */
                                    /* NHWC convolutions of the temporal model consume; no transpose pass             */
#define STP3_BEV_CHANNELS_LAST_BF16 2 /* (forward output only) the same layout, every value rounded ONCE to bf16: what  */
                                    /* a bf16 temporal model makes of the float32 BEV in its first operator anyway --  */
                                    /* half the bytes written and no cast pass in the consumer                         */

/*
 * stp3_lift_splat_fwd -- out[b][t] = sum_{k<=t} discount^(t-k) Pool_k,
 *   Pool_k[c][v] = sum over points p of frame k with vox(p) == v of softmax_D(logits)[p] * feat[pix(p)][c].
 * Replaces stp3.py:215 (depth softmax), :216-221 (outer product, never materialised), geometry.py:302-318
 * (VoxelsSumming.forward) and stp3.py:279-299 (scatter, discount, permute).  Two kernels:
 *   pass 1  per image column; the column's logits and features go global -> LDS directly and every feature and logit
 *           is read from memory exactly once.  Columns of at most 32 rows with C == 64 (lift_column_mma_kernel): ONE
 *           WORKGROUP of four waves per column -- the waves share the staged column, split the rows of the softmax
 *           (in place in LDS) and deal out the 32-run tiles; the run sums are a matrix product  masked probabilities
 *           [runs x rows] x features [rows x C]  on the matrix cores (v_mfma_f32_32x32x2_f32), 32 runs = 32 slots per
 *           tile; this path does NOT write prob_cm (its backward recomputes the probabilities from the logits).
 *           Other shapes (lift_column_kernel): one wave per column, lane = channel, ONE walk over the rows with an
 *           accumulator per depth bin (v_fmac_f32 with a DPP row broadcast of the probability); a finished run's
 *           C-vector goes to its slot; the probabilities are written to prob_cm for the general backward
 *   pass 2  16 lanes per voxel add the voxel's slots (ascending) and carry the discounted state through the T
 *           frames in registers; every BEV row (256 bytes) is written once
 * Deterministic (fixed summation order, no atomics).
 *   feat    [B*T][N*fH*fW][C] float32, logits [B*T][N*fH*fW][D] float32 (pixel-major)
 *   prob_cm [B*T][N*fW][D][fH] float32 out, or NULL (needed by the backward only when stp3_lift_bwd_needs_prob says so)
 *   workspace  stp3_lift_workspace_bytes(dims): one slot per possible run (B*T*P*C floats -- the geometry decides how
 *              many are touched: ~7 % for nuScenes-like rigs) + one BEV-sized buffer
 *   bev_layout STP3_BEV_CHANNELS_LAST : pass 2 writes bev directly
 *              STP3_BEV_CHANNELS_FIRST: pass 2 writes into the workspace and a transpose pass produces bev
 *   bev: B*T*C*X*Y float32, fully overwritten (empty voxels get 0).
 */
int stp3_lift_workspace_bytes(const stp3_lift_dims* dims, size_t* bytes);
int stp3_lift_splat_fwd(const stp3_lift_dims* dims, const float* feat, const float* logits,
                        const void* plan, float discount, int bev_layout,
                        void* workspace, size_t workspace_bytes, float* prob_cm, void* bev, void* stream);

/*
 * stp3_lift_splat_bwd -- gradients of stp3_lift_splat_fwd (softmax included).
 * Replaces autograd through stp3.py:215-301 and VoxelsSumming.backward (geometry.py:320-330).  No atomics.
 *   grad_bev   in `bev_layout` and `grad_dtype` (channels-last float32 / bfloat16, channels-first float32)
 * Columns of at most 32 rows with C == 64 (stp3_lift_bwd_needs_prob -> 0): ONE kernel, one workgroup per image column,
 * the adjoint of the forward's matrix product on the matrix cores,
 *       dM[run][h] = sum_c G[run][c] feat[h][c],    dfeat[h][c] = sum_run M[run][h] G[run][c],
 *   G[run] = the gradient row of the run's voxel, G_t = sum_{t' >= t} discount^(t'-t) grad_bev[b][t'] summed on the fly
 *   over the frames of a channels-last gradient (a channels-first gradient goes through an import pass that transposes
 *   and sums it into `workspace`); probabilities recomputed from `logits` exactly as in the forward; softmax backward
 *   fused.  Reads `logits` and `plan`; prob_cm / vox_cm are not used and may be NULL.
 * Other shapes (stp3_lift_bwd_needs_prob -> 1): import pass (layout / dtype conversion carrying the recurrence,
 *   voxel-major [B*T][V][C] float32 into `workspace`) + a gather kernel, one image pixel per lane pair, walking the depth
 *   bins 8 at a time with the run table and gradient rows staged in LDS.  Reads prob_cm (written by the forward) and
 *   vox_cm; logits / plan are not used and may be NULL.
 *   workspace  stp3_lift_workspace_bytes(dims), always required
 *   grad_feat  [B*T][N*fH*fW][C], grad_logits [B*T][N*fH*fW][D]   outputs, fully overwritten
 */
int stp3_lift_bwd_needs_prob(const stp3_lift_dims* dims, int* needs);
int stp3_lift_splat_bwd(const stp3_lift_dims* dims, const void* grad_bev, int bev_layout, int grad_dtype,
                        const float* feat, const float* logits, const float* prob_cm, const int32_t* vox_cm,
                        const void* plan, float discount,
                        void* workspace, size_t workspace_bytes,
                        float* grad_feat, float* grad_logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise 2-D convolution of the EfficientNet trunk (MBConv blocks), channels-last.
 * Replaces the groups == channels Conv2dStaticSamePadding calls that the reference's Encoder drives
 * (stp3/models/encoder.py:62-70 -> efficientnet_pytorch MBConvBlock._depthwise_conv; forward and the
 * two gradients autograd derives from it).
 *   x  [N][H][W][C], y / dy [N][Ho][Wo][C]   dtype = STP3_DTYPE_F32 or STP3_DTYPE_BF16 (C % 4 / C % 8 == 0)
 *   w  [K*K][C] float32 (tap-major), dw same layout, float32
 *   K in {3,5}, stride in {1,2}; pad_top / pad_left = leading zero padding (the trailing padding is
 *   implied by Ho, Wo: "static same" padding is asymmetric on stride-2 layers)
 *   K = 7 at stride 1: the 7x7 depthwise layer of the ConvNeXt blocks of the prediction stage
 *   (stp3/layers/convolutions.py:309-345 `Block.dwconv`, nn.Conv2d(dim, dim, 7, padding=3, groups=dim) WITH a bias:
 *   stp3_dwconv2d_fwd_bias adds bias[C] float32 (NULL: none); its gradient is the per-channel sum of dy)
 * bwd_weight is deterministic (two-stage reduction through `workspace`, no atomics).
 */
typedef struct stp3_dwconv_dims {
    int32_t N, H, W, C;          /* input  (channels-last)            */
    int32_t Ho, Wo;              /* output spatial size               */
    int32_t K, stride;           /* square kernel, stride             */
    int32_t pad_top, pad_left;   /* leading zero padding              */
    int32_t dtype;               /* STP3_DTYPE_*  of x / y / dy / dx  */
} stp3_dwconv_dims;

int stp3_dwconv2d_fwd(const stp3_dwconv_dims* dims, const void* x, const float* w, void* y, void* stream);
int stp3_dwconv2d_fwd_bias(const stp3_dwconv_dims* dims, const void* x, const float* w, const float* bias, void* y,
                           void* stream);
int stp3_dwconv2d_bwd_data(const stp3_dwconv_dims* dims, const void* dy, const float* w, void* dx, void* stream);
int stp3_dwconv2d_bwd_weight_workspace(const stp3_dwconv_dims* dims, size_t* bytes);
int stp3_dwconv2d_bwd_weight(const stp3_dwconv_dims* dims, const void* x, const void* dy, float* dw,
                             void* workspace, size_t workspace_bytes, void* stream);
/* the same with dw in the layout of the nn.Conv2d parameter, [C][1][K][K] (what autograd hands to the optimizer as it is;
 * stp3_dwconv2d_bwd_weight writes the tap-major [K*K][C] the kernels read their weights in) */
int stp3_dwconv2d_bwd_weight_oihw(const stp3_dwconv_dims* dims, const void* x, const void* dy, float* dw,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise half of the convolutional GRU cells of the prediction stage.  Replaces, around
 * the three convolutions of `SpatialGRU.gru_cell` (stp3/layers/temporal.py:42-56) and `Dual_GRU.gru_cell_1 / _2`
 * (:118-145):  update, reset = sigmoid(conv([x, state]) + bias_init);  tilde = conv([x, (1 - reset) * state]);
 * out = (1 - update) * state + update * tilde  -- and the gradients autograd derives from them.
 *   rows = N * H * W pixels, channels-last.  xs, xs2, dxs2, acc [rows][Cx + C] = [x | state];
 *   gates, dgates [rows][2C] = [update | reset] PRE-activations (the two gate convolutions run as one with 2C outputs);
 *   tilde, dtilde, out [rows][C];  dout [rows][ld_dout >= C].  dtype STP3_DTYPE_F32 / _BF16 (float32 arithmetic, one
 *   rounding per result); Cx, C multiples of 16 bytes of elements, 16-byte aligned pointers (STP3_EUNSUP otherwise).
 *   reset_cat_fwd : xs2 = [x | (1 - r) state]                       (the operand of the tilde convolution)
 *   output_fwd    : out = (1 - u) state + u tilde
 *   output_bwd    : dtilde = dout u;  dgates[:, :C] = dout (tilde - state) u (1 - u)
 *   reset_cat_bwd : acc = [dxs2_x | dout (1 - u) + dxs2_state (1 - r)];  dgates[:, C:] = -dxs2_state state r (1 - r)
 *                   (the caller adds the data gradient of the gate convolution to acc: d[x | state])
 */
typedef struct stp3_gru_dims {
    int64_t rows;
    int32_t Cx, C;               /* channels of x and of the state              */
    int32_t dtype;               /* STP3_DTYPE_*                                */
    float bias_init;             /* gru_bias_init of the reference (default 0)  */
} stp3_gru_dims;

int stp3_gru_reset_cat_fwd(const stp3_gru_dims* dims, const void* xs, const void* gates, void* xs2, void* stream);
int stp3_gru_output_fwd(const stp3_gru_dims* dims, const void* gates, const void* xs, const void* tilde, void* out,
                        void* stream);
int stp3_gru_output_bwd(const stp3_gru_dims* dims, const void* dout, int32_t ld_dout, const void* gates, const void* xs,
                        const void* tilde, void* dtilde, void* dgates, void* stream);
int stp3_gru_reset_cat_bwd(const stp3_gru_dims* dims, const void* dout, int32_t ld_dout, const void* gates, const void* xs,
                           const void* dxs2, void* acc, void* dgates, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the channels of every pixel (+ GELU), channels-last rows -- the prediction stage (SURVEY.md section 8 row
 * f2).  Replaces `LayerNorm` of stp3/layers/convolutions.py:283-307 (F.layer_norm over C in its channels_last form, the
 * hand-written mean / variance over dim 1 in its channels_first form: the same normalisation) and the nn.GELU() that
 * follows it in `Bottleblock` (:347-380); `Block` (:309-345) uses it without the activation.
 *   x, dx [rows][ldx >= C], y / dy [rows][ldy >= C]   dtype STP3_DTYPE_F32 / _BF16, float32 arithmetic, one rounding
 *   y = act((x - mean_c) / sqrt(var_c + eps) * gamma + beta), biased variance; gamma / beta [C] float32 (NULL: 1 / 0)
 *   act = STP3_ACT_NONE or STP3_ACT_GELU (defined with the other activations below; exact: 0.5 v (1 + erf(v / sqrt 2)))
 *   C / (16 bytes of elements) must be a power of two in 4 .. 64, ld multiples of the vector, 16-byte aligned pointers (STP3_EUNSUP
 *   otherwise: the caller keeps torch's operator)
 * bwd recomputes the row statistics from x; dgamma / dbeta [C] float32 (either may be NULL) through a two-stage
 * deterministic reduction in `workspace` (stp3_layernorm_bwd_workspace bytes).
 */
typedef struct stp3_layernorm_dims {
    int64_t rows;                /* pixels: N * H * W                         */
    int32_t C, ldx, ldy;         /* channels, row strides (elements)          */
    int32_t dtype;               /* STP3_DTYPE_*                              */
    int32_t act;                 /* STP3_ACT_NONE | STP3_ACT_GELU             */
    float eps;
} stp3_layernorm_dims;

int stp3_layernorm_fwd(const stp3_layernorm_dims* dims, const void* x, const float* gamma, const float* beta, void* y,
                       void* stream);
int stp3_layernorm_bwd_workspace(const stp3_layernorm_dims* dims, size_t* bytes);
int stp3_layernorm_bwd(const stp3_layernorm_dims* dims, const void* dy, const void* x, const float* gamma,
                       const float* beta, void* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused BatchNorm (+ per-sample bias) + activation (+ residual), channels-last, forward / backward.
 * Replaces the nn.BatchNorm2d/3d -> ReLU / swish (-> "+ skip") chains of
 * stp3/layers/convolutions.py:183-280, stp3/layers/temporal.py:252-273,315-325,426-489,
 * stp3/models/decoder.py:22-140 and of the EfficientNet MBConv blocks driven by
 * stp3/models/encoder.py:57-97; the statistics are handed back between the two passes so the host
 * can all-reduce them over RCCL (train.py:47 sync_batchnorm=True).
 *
 *   x, y, res, dy, dx, dres : [N][rows][C] with row strides ldx (x, dx), ldy (y, dy), ldr (res, dres)
 *                             elements, dtype STP3_DTYPE_F32 / _BF16 (16-byte vector path when C, the
 *                             strides and the pointers allow it, scalar path otherwise)
 *   sbias  [N][C] float32    optional per-sample bias added to x before the normalisation (the ASPP
 *                             image-pooling branch and the pyramid-pooling branch are spatially
 *                             constant: convolutions.py:242-270, temporal.py:375-423)
 *   oscale [N]    float32    optional per-sample scale of the activated output (drop-connect)
 *   forward : y = act(BN(x + sbias) [+ res if BEFORE_ACT]) * oscale [+ res if AFTER_ACT]
 *   sums   [2][C] float32    sum and sum of squares of (x + sbias) over the `count` elements per
 *                             channel they cover (N*rows locally; the host may add other ranks' sums)
 *   stp3_bn_apply_fwd : sums != NULL -> training mode (batch statistics; writes save_mean /
 *                       save_invstd [C]; updates running_mean / running_var with `momentum` and the
 *                       unbiased variance when they are non-NULL); sums == NULL -> inference mode
 *                       (running statistics).
 *   stp3_bn_bwd_reduce: sample_sums [N][3][C] and sums [3][C] = sums of g, g * xhat and xhat, where
 *                       g = dy * oscale * act'(.) is the gradient at the BatchNorm output
 *                       (dbeta = sums[0], dgamma = sums[1]; the per-sample sums give the sbias gradient
 *                        gamma*invstd*(Sg_n - rows*sums[0]/count - Sxhat_n*sums[1]/count));
 *                       sample_sums is written only when has_sbias is set -- its one consumer)
 *   stp3_bn_apply_bwd : dx = gamma * invstd * (g - sums[0]/count - xhat * sums[1]/count)
 *                       (sums == NULL: inference-mode BatchNorm, dx = gamma * invstd * g);
 *                       dres (BEFORE_ACT only, may be NULL) = g.  For AFTER_ACT dres is dy itself.
 *   workspace: stp3_bn_workspace_bytes(dims) bytes.  Deterministic (no atomics).
 */
#define STP3_ACT_NONE  0
#define STP3_ACT_RELU  1
#define STP3_ACT_SWISH 2
#define STP3_ACT_GELU  3   /* stp3_layernorm_* only */
#define STP3_RES_NONE       0
#define STP3_RES_BEFORE_ACT 1
#define STP3_RES_AFTER_ACT  2
#define STP3_BN_MAX_ROW_BLOCKS 128

typedef struct stp3_bn_dims {
    int32_t N, rows, C;        /* samples, rows (H*W) per sample, channels          */
    int32_t ldx, ldy, ldr;     /* row strides in elements                            */
    int32_t dtype;             /* STP3_DTYPE_*                                       */
    int32_t act, res_mode;     /* STP3_ACT_*, STP3_RES_*                             */
    int32_t has_sbias, has_oscale;
    int32_t cpad;              /* 0, or the padded channel count of ZERO-PADDED ROWS: C <= cpad <= ldx, ldy (, ldr), cpad a
                                  multiple of 8.  Lanes [C, cpad) of every row of x / res / dy are read as zero whatever
                                  they hold, and the kernels write zeros there in y / dx / dres: a 35-channel layer
                                  lives in 40-lane rows that the MFMA convolutions (Cin, Cout % 8 == 0) consume and
                                  produce in place, and it runs on the 16-byte vector path.  The per-channel arrays
                                  keep C entries.                                                                  */
} stp3_bn_dims;

int stp3_bn_workspace_bytes(const stp3_bn_dims* dims, size_t* bytes);
int stp3_bn_stats(const stp3_bn_dims* dims, const void* x, const float* sbias, void* workspace,
                  size_t workspace_bytes, float* sums, void* stream);
int stp3_bn_apply_fwd(const stp3_bn_dims* dims, const void* x, const float* sbias, const void* res,
                      const float* oscale, const float* sums, double count, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, float* save_mean, float* save_invstd, void* y, void* stream);
int stp3_bn_bwd_reduce(const stp3_bn_dims* dims, const void* dy, const void* x, const float* sbias,
                       const void* res, const float* oscale, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, void* workspace, size_t workspace_bytes,
                       float* sample_sums, float* sums, void* stream);
int stp3_bn_apply_bwd(const stp3_bn_dims* dims, const void* dy, const void* x, const float* sbias,
                      const void* res, const float* oscale, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, const float* sums, double count, void* dx,
                      void* dres, void* stream);
/* Single-process composites (no cross-replica exchange between the passes; same kernels, one call):
 *   stp3_bn_fwd_train : stats + apply.  stat_buf [4][C] float32 receives sum, sum of squares, mean, invstd.
 *   stp3_bn_bwd_train : reduce + apply. dres as in stp3_bn_apply_bwd; mean / invstd from the forward;
 *                       sum_buf [N+1][3][C] float32 receives the per-sample sums and, last, their totals. */
int stp3_bn_fwd_train(const stp3_bn_dims* dims, const void* x, const float* sbias, const void* res,
                      const float* oscale, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* stat_buf, void* workspace,
                      size_t workspace_bytes, void* y, void* stream);
int stp3_bn_bwd_train(const stp3_bn_dims* dims, const void* dy, const void* x, const float* sbias,
                      const void* res, const float* oscale, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, void* workspace, size_t workspace_bytes,
                      float* sum_buf, void* dx, void* dres, void* stream);

/* stp3_bn_dsbias -- gradient of the per-sample bias (the spatially constant branches folded into a BatchNorm: the ASPP
 * image-pooling branch, stp3/layers/convolutions.py:242-270, the pyramid pooling and the ego-motion planes of the
 * temporal blocks, stp3/layers/temporal.py:380-489, stp3/models/stp3.py:145-152) from the sums of stp3_bn_bwd_reduce:
 *   dsbias[n][c] = gamma[c] invstd[c] (S0[n][c] - rows gsums[0][c] / count - S2[n][c] gsums[1][c] / count)
 *   gsums NULL (evaluation mode, running statistics are constants): gamma invstd S0[n][c].
 *   sample_sums [N][3][C], gsums [3][C] (possibly summed over ranks, count = elements over all ranks), dsbias [N][C].
 * stp3_sum_n -- y = src[0] + ... + src[n-1], n <= 8 dense tensors of numel elements (f32 / bf16) in ONE pass, float32
 *   accumulation in input order, one rounding: the gradients of a tensor with several consumers (the reference's
 *   autograd adds them pairwise: stp3/layers/convolutions.py:256-266 ASPP branches, stp3/models/decoder.py:112-126
 *   heads, stp3/layers/temporal.py:470-489 temporal-block paths).  src: HOST array of n device pointers. */
int stp3_bn_dsbias(int32_t N, int32_t C, int32_t rows, const float* sample_sums, const float* gsums, double count,
                   const float* gamma, const float* invstd, float* dsbias, void* stream);
int stp3_sum_n(int32_t n, int64_t numel, int32_t dtype, const void* const* src, void* y, void* stream);
/* stp3_sum_n_plane -- stp3_sum_n plus one addend that is constant over the plane of every (sample, channel): the gradient of a
 *   whole-plane mean (the ASPP image pooling of stp3/layers/convolutions.py:229-240, the pyramid pooling of
 *   stp3/layers/temporal.py:380-424), which torch materialises as a full tensor before adding it.  The dense tensors are
 *   channels-last [N][H*W][C] (per_sample = H*W*C elements per sample); plane [N][C] in the tensors' type; added last. */
int stp3_sum_n_plane(int32_t n, int64_t numel, int32_t dtype, const void* const* src, const void* plane, int64_t per_sample,
                     int32_t C, void* y, void* stream);

/* stp3_linear_fwd / _bwd -- y [M][N] = x [M][K] w[N][K]^T + b[N] (b may be NULL), float32, for the pooled descriptors of the BEV
 *   networks: 1x1 convolutions of maps that are constant over the plane (ASPP image pooling, stp3/layers/convolutions.py:229-240;
 *   pyramid pooling, stp3/layers/temporal.py:380-424; the ego-motion planes, stp3/models/stp3.py:145-152) are products of a few
 *   rows whose time is launch latency -- one launch forward, ONE backward for dx [M][K], dw [N][K] and db [N] (each may be NULL:
 *   not needed).  Deterministic: every sum is split over 16 lanes in a fixed way and finished by a fixed tree.
 *   ldw / lddw: row strides (in floats, >= K) of w and dw -- the weight may be a run of COLUMNS of a wider parameter (the columns
 *   of ASPP's projection that multiply the pooled vector, of a temporal block's 1x1x1 kernel that multiply the ego-motion
 *   planes), read in place, and its gradient written straight into the same columns of the parameter's gradient. */
int stp3_linear_fwd(int32_t M, int32_t K, int32_t N, const float* x, const float* w, int32_t ldw, const float* b, float* y,
                    void* stream);
int stp3_linear_bwd(int32_t M, int32_t K, int32_t N, const float* dy, const float* x, const float* w, int32_t ldw, float* dx,
                    float* dw, int32_t lddw, float* db, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense 2-D convolution, bf16 MFMA implicit GEMM, NHWC (csrc/stp3_conv.hip).
 * Replaces the nn.Conv2d (and frame-folded nn.Conv3d) contractions of stp3/layers/convolutions.py:183-280,
 * stp3/layers/temporal.py:252-273,315-325, stp3/models/decoder.py:22-140 and the stem / 1x1 expand / project
 * convolutions of the MBConv blocks driven by stp3/models/encoder.py:57-97 (groups == 1).
 *   x [N][H][W][ldx >= Cin]  bf16 (row stride ldx lets the kernel read a channel-slice / concat view)
 *   w [Cout][KH][KW][Cin]    bf16 (= channels-last memory of the (Cout, Cin, KH, KW) parameter)
 *   bias [Cout] float32 or NULL
 *   y [N][Ho][Wo][ldy >= Cout]  out_dtype = STP3_DTYPE_BF16 or STP3_DTYPE_F32, float32 accumulation
 *   y[n][ho][wo][co] = bias[co] + sum_{kh,kw,ci} x[n][ho*stride - pad_h + kh*dil_h][wo*stride - pad_w + kw*dil_w][ci]
 *                                                 * w[co][kh][kw][ci]           (zero padding)
 *   sums [2][Cout] float32 or NULL (bf16 outputs only): per-channel sum and sum of squares of the ROUNDED outputs over
 *        all N*Ho*Wo pixels -- the BatchNorm statistics, taken in the epilogue (the result feeds stp3_bn_apply_fwd
 *        directly, no stp3_bn_stats pass over the convolution output); needs `workspace` of
 *        stp3_conv2d_fwd_workspace(dims) bytes (one partial row per 128-pixel workgroup; deterministic)
 * Workgroup tile 128 pixels x 128 (Cout > 64) or 64 output channels, K steps of 64 staged through LDS,
 * v_mfma_f32_32x32x16_bf16.  Requires Cin % 8 == 0, ldx % 8 == 0, 16-byte aligned x / w / y,
 * N*H*W*ldx < 2^31.  The data gradient of a stride-1 convolution is the same call on dy with the taps flipped and
 * Cin / Cout swapped (the host prepares that weight).
 */
typedef struct stp3_conv_dims {
    int32_t N, H, W, Cin;
    int32_t Ho, Wo, Cout;
    int32_t KH, KW, stride;
    int32_t pad_h, pad_w, dil_h, dil_w;
    int32_t ldx, ldy;
    int32_t out_dtype, has_bias;
} stp3_conv_dims;

int stp3_conv2d_fwd_workspace(const stp3_conv_dims* dims, size_t* bytes);
int stp3_conv2d_fwd(const stp3_conv_dims* dims, const void* x, const void* w, const float* bias, void* y,
                    float* sums, void* workspace, size_t workspace_bytes, void* stream);

/* Convolution -> BatchNorm -> activation with the convolution output NEVER in memory (csrc/stp3_conv.hip, epilogue
 * modes): for layers whose convolution is cheap next to the tensor it produces -- the 1x1 expand convolutions of the
 * EfficientNet MBConv blocks driven by stp3/models/encoder.py:57-97 (24..160 -> 144..960 channels: the expanded tensor is
 * 6x the block input) -- the forward runs the convolution twice and the BatchNorm backward recomputes the output tiles
 * from the input instead of reading a stored copy:
 *   stp3_conv2d_fwd_stats     sums [2][Cout] = per-channel sum / sum of squares of the bf16-ROUNDED outputs; nothing stored
 *   stp3_conv2d_fwd_bnact     y = act(scale * e0 + shift), e0 = the rounded convolution output, coef = [scale | shift |
 *                             mean | invstd][Cout] as stp3_bn_finalize writes them
 *   stp3_conv2d_bn_bwd_reduce sums [2][Cout] = sum g, sum g * xhat with g = dz * act'(scale * e0 + shift),
 *                             xhat = (e0 - mean) * invstd; dz [M][ldz] bf16 = the gradient at the activation output
 *   stp3_conv2d_bn_bwd_apply  dy = scale * (g - gsums[0] / count - xhat * gsums[1] / count): the gradient at the convolution
 *                             output (what stp3_bn_apply_bwd writes), gsums possibly summed over ranks
 * dims / x / w as stp3_conv2d_fwd (bf16, no bias, out_dtype bf16; Cout, ldy, ldz multiples of 8); workspace:
 * stp3_conv2d_fwd_workspace.  Same values as the stored route: every mode rounds the accumulators to bf16 first. */
int stp3_conv2d_fwd_stats(const stp3_conv_dims* dims, const void* x, const void* w, float* sums, void* workspace,
                          size_t workspace_bytes, void* stream);
int stp3_conv2d_fwd_bnact(const stp3_conv_dims* dims, const void* x, const void* w, const float* coef, int32_t act, void* y,
                          void* stream);
int stp3_conv2d_bn_bwd_reduce(const stp3_conv_dims* dims, const void* x, const void* w, const void* dz, int32_t ldz,
                              const float* coef, int32_t act, float* sums, void* workspace, size_t workspace_bytes,
                              void* stream);
int stp3_conv2d_bn_bwd_apply(const stp3_conv_dims* dims, const void* x, const void* w, const void* dz, int32_t ldz,
                             const float* coef, int32_t act, const float* gsums, double count, void* dy, void* stream);
/* stp3_conv2d_bn_bwd_apply_dx -- stp3_conv2d_bn_bwd_apply that ALSO writes the data gradient of the 1x1 convolution,
 * dx[m][ci] = sum_co dy[m][co] w[co][ci] (+ add[m][ci]: the gradient of the block's identity skip, may be NULL), [M][lddx] bf16:
 * the kernel holds the dy tile of its 32 pixels in LDS when it stores it, so the second matrix product reads it there instead
 * of a separate data-gradient convolution reading the 6x larger dy back from memory (the expand convolutions of the MBConv
 * blocks, stp3/models/encoder.py:57-97: 144 / 192 output channels, <= 32 input channels -- the whole-row streaming kernel;
 * anything else: STP3_EUNSUP, the caller keeps the two calls).  dy is still written (the weight gradient reads it). */
int stp3_conv2d_bn_bwd_apply_dx(const stp3_conv_dims* dims, const void* x, const void* w, const void* dz, int32_t ldz,
                                const float* coef, int32_t act, const float* gsums, double count, void* dy, void* dx,
                                int32_t lddx, const void* add, int32_t ldadd, void* stream);

/* stp3_conv2d_fwd_add -- stp3_conv2d_fwd (bf16 output, no statistics) with y = bf16(bf16(conv + bias) + add): the DATA GRADIENT
 * of a block's first convolution written together with the gradient of the block's skip connection (`add` = the gradient at
 * the block output, [N][Ho][Wo][ldadd >= Cout] bf16) -- what torch.autograd does with one more pass over both tensors when a
 * tensor has two consumers (the identity skips of the MBConv blocks, stp3/models/encoder.py:57-97, and of the decoder's
 * ResNet blocks, stp3/models/decoder.py:22-30).  Same bits as the separate addition (it adds the rounded convolution result).
 * Requires Cout % 8 == 0, ldy % 8 == 0, ldadd % 8 == 0 and 16-byte aligned y / add. */
int stp3_conv2d_fwd_add(const stp3_conv_dims* dims, const void* x, const void* w, const float* bias, const void* add,
                        int32_t ldadd, void* y, void* stream);

/* stp3_conv2d_wgrad -- dw[co][kh][kw][ci] = sum_{n,ho,wo} dy[n][ho][wo][co] * x[n][ho*stride-pad_h+kh*dil_h][..][ci]
 * (the weight gradient autograd derives for the convolutions above), float32 output in the weight's own
 * [Cout][KH][KW][Cin] layout.  dy [N][Ho][Wo][ldy >= Cout] and x [N][H][W][ldx >= Cin] are bf16; the pixel
 * contraction is split over workgroups and reduced deterministically through `workspace`
 * (stp3_conv2d_wgrad_workspace(dims) bytes).  Requires Cin % 4 == 0, Cout % 4 == 0, ldx % 4 == 0, ldy % 4 == 0.
 * dims.out_dtype / has_bias are ignored. */
int stp3_conv2d_wgrad_workspace(const stp3_conv_dims* dims, size_t* bytes);
int stp3_conv2d_wgrad(const stp3_conv_dims* dims, const void* dy, const void* x, float* dw, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The same weight gradient in two halves, for callers that can wait for it (the gradient of a LEAF parameter is read by
 * nobody before the optimizer -- torch.autograd's AccumulateGrad only keeps the tensor; reference: the `loss.backward()` /
 * `optimizer.step()` pair PyTorch-Lightning drives for stp3/trainer.py:101-172).
 * stp3_conv2d_wgrad_partials runs the split contraction only: partials[split][Cout][KH][KW][Cin] float32 into caller memory of
 * stp3_conv2d_wgrad_workspace(dims) bytes that must stay untouched until the reduction; *splits receives the split count.
 * stp3_conv2d_wgrad_reduce_batch sums the partials of n such layers in ONE launch per STP3_WGRAD_BATCH_MAX jobs (`jobs` is a
 * HOST array, it travels as the kernel argument): dw[i] = sum_k partials[k][i], the additions in the order of
 * stp3_conv2d_wgrad (bit-identical results).  pre_coef / pre_act: NULL / ignored, or the operand-side BatchNorm of
 * stp3_conv2d_wgrad_pre (below). */
#define STP3_WGRAD_BATCH_MAX 96
typedef struct stp3_wgrad_job {
    const void* partials;   /* device: [splits][numel] float32 */
    float* dw;              /* device: [numel] float32 */
    int64_t numel;          /* Cout * KH * KW * Cin, < 2^32 */
    int32_t splits;
    int32_t reserved;
} stp3_wgrad_job;
int stp3_conv2d_wgrad_partials(const stp3_conv_dims* dims, const void* dy, const void* x, const float* pre_coef,
                               int32_t pre_act, void* partials, size_t partials_bytes, int32_t* splits, void* stream);
int stp3_conv2d_wgrad_reduce_batch(int32_t n, const stp3_wgrad_job* jobs, void* stream);

/* BatchNorm (+ ReLU) applied in the OPERAND LOAD of the 1x1 convolution behind it (csrc/stp3_conv.hip, PRE): for the chains
 * conv -> BatchNorm -> ReLU -> 1x1 conv of stp3/layers/convolutions.py:183-280 (ASPP branches -> projection, DeepLabHead tail)
 * and stp3/models/decoder.py:42-66 (the heads), whose normalised tensor has no reader but that 1x1 convolution.  x is the
 * PRODUCER's convolution output z; the kernels use bf16(act(scale[ci] * z + shift[ci])) in its place -- bit for bit what
 * stp3_bn_apply_fwd (training mode, no skip, no per-sample terms) would have stored -- so that tensor is neither written nor read:
 *   stp3_conv2d_fwd_pre    stp3_conv2d_fwd (no statistics) of that operand; always the LDS-tiled kernel
 *   stp3_conv2d_wgrad_pre  stp3_conv2d_wgrad of that operand (stp3_conv2d_wgrad_partials takes the same two arguments)
 * pre_coef = [scale | shift][Cin] float32 (the first two rows stp3_bn_finalize writes), pre_act = STP3_ACT_NONE / STP3_ACT_RELU.
 * Pieces that stand for padding (rows beyond N * H * W, the channel tail) reach the matrix cores as ZERO, after the transform.
 * 1x1 / stride 1 / no padding, x and w each below 2 GiB, Cin <= 4096 (forward); anything else: STP3_EUNSUP. */
int stp3_conv2d_fwd_pre(const stp3_conv_dims* dims, const void* x, const void* w, const float* bias, const float* pre_coef,
                        int32_t pre_act, void* y, void* stream);
int stp3_conv2d_wgrad_pre(const stp3_conv_dims* dims, const void* dy, const void* x, const float* pre_coef, int32_t pre_act,
                          float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Squeeze-and-excitation data passes (csrc/stp3_se.hip).
 * Replace the pooling, the gate multiply and the elementwise / reduction passes of their backward inside the
 * EfficientNet MBConv blocks driven by stp3/models/encoder.py:57-97.
 *   x, dy, y : [N][rows][ld >= C] channels-last, dtype STP3_DTYPE_F32 / _BF16
 *   stp3_se_pool  : out [N][C] float32 = sum over rows of x (dy == NULL) or of dy * x (dy != NULL); deterministic
 *   stp3_se_scale : y = x * gate[n][c] + add[n][c]   (gate, add [N][C] float32; add may be NULL)
 */
typedef struct stp3_se_dims {
    int32_t N, rows, C, ld;
    int32_t dtype;
} stp3_se_dims;

int stp3_se_workspace_bytes(const stp3_se_dims* dims, size_t* bytes);
int stp3_se_pool(const stp3_se_dims* dims, const void* x, const void* dy, void* workspace, size_t workspace_bytes,
                 float* out, void* stream);
int stp3_se_scale(const stp3_se_dims* dims, const void* x, const float* gate, const float* add, void* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The two fully-connected layers of a squeeze-and-excitation block (csrc/stp3_se_mlp.hip): the MBConv gate
 *     gate = sigmoid(W2 swish(W1 mean_hw(x) + b1) + b2)
 * (efficientnet_pytorch MBConvBlock as driven by stp3/models/encoder.py:57-97) and its backward, float32.
 *   pooled_sum [N][C] : sum over the map (stp3_se_pool); the mean is pooled_sum * inv_rows
 *   w1 [S][C], b1 [S], w2 [C][S], b2 [C]
 *   fwd : z1 [N][S] (pre-activation, kept for the backward), gate [N][C]
 *   bwd : dgate [N][C] = sum_hw dy * x (stp3_se_pool with dy)  ->  dpooled [N][C] (gradient at pooled_sum... of the
 *         MEAN, already scaled by inv_rows, i.e. what stp3_se_scale adds per pixel), dw1 [S][C], db1 [S], dw2 [C][S],
 *         db2 [C]; dz2 [N][C] and dz1 [N][S] are caller-provided scratch.  Samples are reduced in ascending order.
 * Limits: S <= 8192; the weight-gradient kernel keeps 16 N + 8704 floats in LDS (N <= 480 samples per call); S * C < 2^31; else STP3_EUNSUP. */
typedef struct stp3_se_mlp_dims {
    int32_t N, C, S;
    float inv_rows;
} stp3_se_mlp_dims;

int stp3_se_mlp_fwd(const stp3_se_mlp_dims* dims, const float* pooled_sum, const float* w1, const float* b1,
                    const float* w2, const float* b2, float* z1, float* gate, void* stream);
int stp3_se_mlp_bwd(const stp3_se_mlp_dims* dims, const float* dgate, const float* gate, const float* pooled_sum,
                    const float* z1, const float* w1, const float* w2, float* dz2, float* dz1, float* dpooled,
                    float* dw1, float* db1, float* dw2, float* db2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MBConv block passes (csrc/stp3_mbconv.hip, csrc/stp3_dwconv.hip): the EfficientNet block that
 * stp3/models/encoder.py:57-97 drives 22 times per image,
 *     E0 = expand(x) -> E1 = swish(BN0(E0)) -> E2 = depthwise(E1) -> S = swish(BN1(E2))
 *     -> gate = sigmoid(MLP(mean_hw S)) -> A = S * gate -> y = BN2(project(A)) (+ x),
 * with BatchNorm-1, its swish and the squeeze-excite gate applied where the data is consumed instead of in passes of
 * their own over the expanded tensor (the tensor `S` is never written), forward and backward.
 *
 *   stp3_dwconv2d_fwd_stats : stp3_dwconv2d_fwd + sums [2][C] = per-channel sum / sum of squares of the ROUNDED outputs
 *                             (the statistics of BN1; no stp3_bn_stats pass over E2).  workspace:
 *                             stp3_dwconv2d_fwd_stats_workspace(dims) bytes; deterministic.
 *   stp3_bn_finalize        : sums [2][C] over `count` elements -> coef [4][C] = scale (= gamma * invstd), shift
 *                             (= beta - mean * scale), mean, invstd; updates running_mean / running_var (momentum, unbiased
 *                             variance) when non-NULL -- the arithmetic of stp3_bn_apply_fwd's training mode, bit for bit.
 *   stp3_se_pool_act        : out [N][C] = sum over rows of act(scale[c] * x + shift[c])    (the squeeze of S from E2)
 *   stp3_mbconv_scale_act   : y = act(scale[c] * x + shift[c]) * gate[n][c]                  (A from E2; gate may be NULL)
 *   stp3_mbconv_bwd_reduce  : ONE pass over (da = dL/dA, x = E2): sums5 [5][N][C] (quantity-major) =
 *                               [0] sum da*S  (the gate's gradient, input of stp3_se_mlp_bwd)
 *                               [1] sum da*S'   [2] sum da*S'*xhat   [3] sum S'   [4] sum S'*xhat
 *                             with S = act(pre), S' = act'(pre), pre = scale*x + shift, xhat = (x - mean) * invstd.
 *   stp3_mbconv_bwd_coef    : gsums [2][C]:  sum g = sum_n gate*[1] + dpooled*[3],  sum g*xhat = sum_n gate*[2] + dpooled*[4]
 *                             where g = (da*gate + dpooled) * S' is the gradient at the BatchNorm-1 output
 *                             (dbeta1 = gsums[0], dgamma1 = gsums[1]); the host may all-reduce gsums over ranks.
 *   stp3_mbconv_bwd_apply   : dx = scale * (g - gsums[0]/count - xhat * gsums[1]/count)   (= dL/dE2), same dtype as x
 *   x, da, dx, y : [N][rows][ld] channels-last, dims.dtype (bf16: C, ld multiples of 8; f32: of 4; 16-byte aligned),
 *   dims.ld = row stride of x; ldg / ldy = row stride of da and dx / of y.  coef as written by stp3_bn_finalize.
 *   gate, dpooled [N][C] float32 (dpooled: the per-pixel term stp3_se_mlp_bwd returns).  workspace:
 *   stp3_mbconv_workspace_bytes(dims).  Deterministic, no atomics.
 */
int stp3_dwconv2d_fwd_stats_workspace(const stp3_dwconv_dims* dims, size_t* bytes);
int stp3_dwconv2d_fwd_stats(const stp3_dwconv_dims* dims, const void* x, const float* w, void* y, float* sums,
                            void* workspace, size_t workspace_bytes, void* stream);
int stp3_bn_finalize(const float* sums, int32_t C, double count, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, float* coef, void* stream);
int stp3_mbconv_workspace_bytes(const stp3_se_dims* dims, size_t* bytes);
int stp3_se_pool_act(const stp3_se_dims* dims, const void* x, const float* scale, const float* shift, int32_t act,
                     void* workspace, size_t workspace_bytes, float* out, void* stream);
int stp3_mbconv_scale_act(const stp3_se_dims* dims, int32_t ldy, const void* x, const float* scale, const float* shift,
                          int32_t act, const float* gate, void* y, void* stream);
int stp3_mbconv_bwd_reduce(const stp3_se_dims* dims, int32_t ldg, const void* da, const void* x, const float* coef,
                           int32_t act, void* workspace, size_t workspace_bytes, float* sums5, void* stream);
int stp3_mbconv_bwd_coef(int32_t N, int32_t C, const float* sums5, const float* gate, const float* dpooled,
                         float* gsums, void* stream);
int stp3_mbconv_bwd_apply(const stp3_se_dims* dims, int32_t ldg, const void* da, const void* x, const float* coef,
                          int32_t act, const float* gate, const float* dpooled, const float* gsums, double count,
                          void* dx, void* stream);

/* stp3_dwconv2d_fwd_stats_bn -- (depthwise convolution -> BatchNorm-1 of an MBConv block, stp3/models/encoder.py:57-97)
 * stp3_dwconv2d_fwd_stats + stp3_bn_finalize in the launches of the former (one process: nothing
 * happens between the statistics and their use, so the final reduction finishes its own channels -- coef [4][C] = scale |
 * shift | mean | invstd, running statistics updated; the additions keep the order of the stand-alone reduction and the
 * constants stp3_bn_finalize's arithmetic: bit-identical).  count = elements per channel. */
int stp3_dwconv2d_fwd_stats_bn(const stp3_dwconv_dims* dims, const void* x, const float* w, void* y, float* sums, double count,
                               const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                               float* running_var, float* coef, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training losses of the perception path and the label warp (csrc/stp3_loss.hip).
 *
 * stp3_ce_topk_fwd / _bwd -- weighted cross-entropy with ignore_index, per-row scale (future discount) and the mean of
 * the k largest per-pixel losses of every row: stp3/losses.py:43-83 (SegmentationLoss: rows = B*S), :85-114 (HDmapLoss,
 * one call per map element: rows = B), :116-134 (DepthLoss: k = 0, no selection).
 *   logits  element (row, c, p) at logits[row*stride_row + c*stride_c + p*stride_p], dims.dtype f32 / bf16
 *   labels  [rows][P] int64;  class_weights [C] float32 or NULL;  row_scale [rows] float32 or NULL
 *   loss_px [rows][P] float32 out: scale[row] * w[y] * (logsumexp(z) - z[y]), 0 for ignored pixels (kept for the backward)
 *   sel     [rows][2] float32 out: tau = the k-th largest loss of the row (found by a radix select on the float bits; the
 *           reference sorts the row, losses.py:76-81) and the share of the elements EQUAL to tau in the top k
 *   out[0]  = (accumulate ? out[0] : 0) + out_scale * sum_rows sum_{k largest} loss      (out_scale = weight / (rows*k))
 *   bwd     dlogits (same strides / dtype as logits) = gout[0] * out_scale * take * scale[row] * w[y] * (softmax - onehot),
 *           take = 1 above tau, the tie share at tau, 0 below: ties at the threshold share their part of the gradient
 *           equally (torch.topk picks arbitrary ones; the loss value and the total gradient mass are the same)
 *   k <= 0 or k >= P: no selection (mean over all pixels: out_scale = weight / (rows*P)).
 * stp3_reg_loss_fwd / _bwd -- stp3/losses.py:6-40 SpatialRegressionLoss: pred, target [rows][C][P] contiguous;
 *   out[0] = sum over pixels with target[row][0][p] != ignore_value of scale[row] * sum_c |d| (norm 1) or d^2 (norm 2),
 *   divided by the number of such pixels (0 when there are none); out[1] = that number.  bwd: stat = out of the forward.
 * stp3_warp_nearest -- stp3/utils/geometry.py:196-238 warp_features with mode='nearest' on label maps
 *   (F.affine_grid + F.grid_sample, zeros padding, align_corners=False): x, y [frames][C][H][W] float32, theta [frames][6]
 *   (row-major 2x3), identity [frames] int32 or NULL (non-zero: the frame is copied unchanged).
 * Deterministic; float32 arithmetic; workspaces: stp3_ce_topk_workspace_bytes / stp3_reg_loss_workspace_bytes.
 */
typedef struct stp3_ce_dims {
    int32_t rows, P, C, k;
    int32_t ignore_index, dtype;
    int64_t stride_row, stride_c, stride_p;
} stp3_ce_dims;

int stp3_ce_topk_workspace_bytes(const stp3_ce_dims* dims, size_t* bytes);
int stp3_ce_topk_fwd(const stp3_ce_dims* dims, const void* logits, const int64_t* labels, const float* class_weights,
                     const float* row_scale, float* loss_px, float* sel, double out_scale, int32_t accumulate, float* out,
                     void* workspace, size_t workspace_bytes, void* stream);
int stp3_ce_topk_bwd(const stp3_ce_dims* dims, const void* logits, const int64_t* labels, const float* class_weights,
                     const float* row_scale, const float* loss_px, const float* sel, const float* gout, double out_scale,
                     void* dlogits, void* stream);
int stp3_reg_loss_workspace_bytes(size_t* bytes);
int stp3_reg_loss_fwd(int32_t rows, int32_t C, int32_t P, int32_t norm, float ignore_value, int32_t dtype, const void* pred,
                      const float* target, const float* row_scale, float* out, void* workspace, size_t workspace_bytes,
                      void* stream);
int stp3_reg_loss_bwd(int32_t rows, int32_t C, int32_t P, int32_t norm, float ignore_value, int32_t dtype, const void* pred,
                      const float* target, const float* row_scale, const float* stat, const float* gout, void* dpred,
                      void* stream);
int stp3_warp_nearest(int32_t frames, int32_t C, int32_t H, int32_t W, const float* x, const float* theta,
                      const int32_t* identity, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 shadow copies of all convolution weights in ONE launch (csrc/stp3_wprep.hip).  Replaces the per-layer cast / flip / transpose / re-layout the host would
 * otherwise redo after every optimizer step for the operands of stp3_conv2d_fwd (forward: [Cout][KH][KW][Cin];
 * data gradient: [Cin][KH][KW][Cout] with the taps flipped).
 *   table : n_entries structs in DEVICE memory, sorted by first_block
 *   src   : fp32 master weight, element (co, ci, r, s) at src[co*stride_co + ci*stride_ci + r*stride_kh + s*stride_kw]
 *   fwd / flip : bf16 destinations (either may be NULL)
 *   first_block : exclusive scan over the table of ceil(cout*cin*kh*kw / 256); total_blocks = the scan's total
 * Rounding: to nearest even, as torch's .to(bfloat16). */
typedef struct stp3_wprep_entry {
    const float* src;
    void* fwd;
    void* flip;
    int64_t stride_co, stride_ci, stride_kh, stride_kw;
    int64_t first_block;
    int32_t cout, cin, kh, kw;
    /* a PIECE of an assembled weight: the block lands at channel offsets (co_off, ci_off) of destinations with dst_cout x
     * dst_cin channels (fwd [dst_cout][KH][KW][dst_cin], flip [dst_cin][KH][KW][dst_cout]); dst_cout == 0: the entry is the
     * whole weight (dst = cout x cin, offsets 0).  Elements no piece covers are not written. */
    int32_t dst_cout, dst_cin, co_off, ci_off;
    int32_t fwd_f32;       /* 1: fwd receives float32 (the tap-major [KH*KW][C] weights of stp3_dwconv2d_*: cout = 1, cin = C) */
    int32_t reserved;
} stp3_wprep_entry;

int stp3_conv2d_prep_weights(const stp3_wprep_entry* table, int32_t n_entries, int64_t total_blocks, void* stream);

/* The way back: the float32 gradient of an assembled weight ([dst_cout][KH][KW][dst_cin], what stp3_conv2d_wgrad writes) cut
 * into its pieces, each stored into its parameter's gradient -- same table layout, with ``src`` = the (writable) destination
 * inside the parameter's gradient, read through the entry's strides, and ``fwd`` = the assembled gradient.  One launch for
 * every assembled weight of a backward pass.  Replaces the backward of the reference's weight plumbing (torch autograd of
 * the slices / pads / concatenations around stp3/layers/temporal.py:8-37 CausalConv3d, stp3/layers/convolutions.py ASPP.project,
 * stp3/models/decoder.py:96-140 heads): slice_backward, constant_pad_nd, cat and add kernels per layer. */
int stp3_conv2d_scatter_weight_grads(const stp3_wprep_entry* table, int32_t n_entries, int64_t total_blocks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-norm clipping + Adam on flat fp32 buckets in three launches (csrc/stp3_optim.hip).  Replaces, for the flat buckets of stp3_amd/parallel.py, the reference's
 * gradient_clip_val (train.py:48, torch clip_grad_norm_ semantics: scale = min(max_norm / (norm + 1e-6), 1)) and
 * torch.optim.Adam step (trainer.py:456-462: L2 weight decay folded into the gradient, bias correction, no amsgrad).
 *   table : n_buckets structs in DEVICE memory, sorted by first_block; grad / param / exp_avg / exp_avg_sq are
 *           float32 arrays of numel elements; first_block = exclusive scan of ceil(numel / 4096)
 *   state : 5 floats in device memory, [0] = step count (in/out, incremented by the call), out: [1] clip scale,
 *           [2] lr / (1 - beta1^t), [3] sqrt(1 - beta2^t), [4] total gradient norm before clipping
 *   max_norm <= 0 : no clipping.  The clipped gradient is written back to grad (as clip_grad_norm_ does).
 *   workspace : stp3_optim_workspace_bytes(total_blocks) bytes.  No host synchronisation; deterministic. */
typedef struct stp3_optim_bucket {
    float* grad;
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int64_t first_block;
} stp3_optim_bucket;

int stp3_optim_workspace_bytes(int64_t total_blocks, size_t* bytes);
int stp3_optim_clip_adam(const stp3_optim_bucket* table, int32_t n_buckets, int64_t total_blocks, float max_norm,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float* state,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Causal two-frame channel pairing of the frame-folded BEV sequence (csrc/stp3_temporal.hip): the operand of the
 * (2,3,3) convolution of CausalConv3d, stp3/layers/temporal.py:252-273 (time padded on the left by one frame:
 * y[t] = W[:, :, 0] * x[t-1] + W[:, :, 1] * x[t], x[-1] = 0), as ONE 2-D convolution over 2C channels.
 *   x  [frames][rows][ldx >= C]  bf16 / float32, channels-last; frames = B*T, the T frames of a sample consecutive
 *   y  [frames][rows][2C] : y[n][r][0:C] = x[n-1][r][0:C] (zero when n % T == 0) ; y[n][r][C:2C] = x[n][r][0:C]
 *   bwd: dy [frames][rows][2C] -> dx [frames][rows][C] (dense),
 *        dx[n][r][c] = dy[n][r][C + c] + (dy[n+1][r][c] unless n % T == T - 1)      (float32 add, rounded once)
 * C and ldx multiples of 16 bytes (8 bf16 / 4 float32), 16-byte aligned pointers (STP3_EUNSUP otherwise). */
typedef struct stp3_pair_dims {
    int32_t frames, T, rows, C, ldx, dtype;
} stp3_pair_dims;
int stp3_causal_pair_fwd(const stp3_pair_dims* dims, const void* x, void* y, void* stream);
int stp3_causal_pair_bwd(const stp3_pair_dims* dims, const void* dy, void* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bilinear up-sampling by an integer factor, align_corners = False (csrc/stp3_upsample.hip): nn.Upsample(scale_factor=2,
 * mode='bilinear') of UpsamplingConcat / UpsamplingAdd, stp3/layers/convolutions.py:183-215 (encoder merge and the three
 * BEV decoder stages).
 *   x  [N][H][W][ldx >= C]            bf16 / float32, channels-last (ldx: a channel slice is read in place)
 *   y  [N][H*scale][W*scale][ldy >= C] same type (ldy: the result may be written into a slice of a concatenation)
 *   y[oh][ow] = l0h * (l0w * x[h0][w0] + l1w * x[h0][w1]) + l1h * (l0w * x[h1][w0] + l1w * x[h1][w1]),
 *       src = max((o + 0.5) / scale - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, size - 1), l1 = src - i0, l0 = 1 - l1
 *       (float32 arithmetic in this order -- torch's -- then one rounding to the element type)
 *   bwd: dy [N][H*scale][W*scale][ldy] -> dx [N][H][W][ldx]: every input pixel gathers the gradients of the outputs
 *        that read it (float32 accumulation, deterministic, no atomics)
 * scale 1..4; C, ldx, ldy multiples of 16 bytes; 16-byte aligned pointers; < 2^31 vectors (STP3_EUNSUP otherwise). */
typedef struct stp3_upsample_dims {
    int32_t N, H, W, C, scale, ldx, ldy, dtype;
} stp3_upsample_dims;
int stp3_upsample_bilinear_fwd(const stp3_upsample_dims* dims, const void* x, void* y, void* stream);
int stp3_upsample_bilinear_bwd(const stp3_upsample_dims* dims, const void* dy, void* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Planner: trajectory-cost evaluation (csrc/stp3_plan.hip) -- the reference's Cost_Function.forward, stp3/cost.py:26-47,
 * with its seven terms (SafetyCost :210-241, HeadwayCost :244-272, LR_divider :274-315, Comfort :318-372, Progress
 * :374-392, Rule :183-207, Cost_Volume :166-181) in one launch.  Called by Planning.select / Planning.loss
 * (stp3/models/planning_model.py:43-88) once for the N sampled trajectories and once for the expert trajectory (N = 1).
 *   trajs        [B][N][T][2] float32   (lateral, forward) metres in the ego frame, UNflipped (the kernel applies the
 *                                       reference's (-1, 1) flip, cost.py:35)
 *   cost_volume  [B][T][H][W] float32   the decoder's cost-volume head, raw (clamped to [0, 1000] inside)
 *   occupancy    [B][T][H][W] float32   0 / 1 (labels in training, argmax of the prediction in evaluation)
 *   drivable     [B][H][W]    float32   drivable-area mask AFTER the reference's preprocessing (labels as they are;
 *                                       logits: softmax, entries < 0.5 zeroed -- cost.py:196-201; host side, three operators)
 *   lane         [B][H][W]    float32   lane-divider mask after the same preprocessing (:289-294); != 0 is a divider
 *   target       [B][2] float32 ; target_sum [1] float32 = sum of `target` (progress drops its goal term when the sum
 *                                       over the batch is < 0.5, :386 -- a device scalar, no host synchronisation)
 *   footprint0 / footprint_lambda  [K0][2] / [KL][2] int32  (row, column) cells of the ego box and of the box inflated
 *                                       by LAMBDA, as BaseCost.get_origin_points builds them (:70-83; 32 / 192 cells)
 *   cost_fc [B][N] float32 = comfort + progress ; cost_fo [B][N][T] float32 = safety + headway + lane + volume + rule,
 *                                       every term clamped as in :36-42
 *   cv_cell [B][N][T] int32 / cv_scale [B][N][T] float32: (optional, both or neither) the cost-volume cell each cost
 *                                       read and d cost_fo / d cost_volume[cell] -- what the backward needs
 *   bwd: grad_cost_volume [B][T][H][W] float32, written completely (zeros where nothing was read); contributions of
 *        several trajectories to one cell are added in ascending trajectory order (deterministic, no atomics).
 * Limits: B*N*T and B*T*H*W < 2^31; backward N <= 20 480 (STP3_EUNSUP). */
typedef struct stp3_plan_dims {
    int32_t B, N, T, H, W, K0, KL;
    float dx0, dx1, bx0, bx1;                     /* BEV resolution / first cell centre, (x = forward, y = side) */
    float safety, headway, lrdivider, comfort, progress, volume, rule;   /* COST_FUNCTION factors; rule = 5 */
    float w0, w1;                                 /* SafetyCost.w */
    float headway_dist, lr_dist;                  /* 10 m, 1 m */
} stp3_plan_dims;
int stp3_traj_cost_fwd(const stp3_plan_dims* dims, const float* trajs, const float* cost_volume, const float* occupancy,
                       const float* drivable, const float* lane, const float* target, const float* target_sum,
                       const int32_t* footprint0, const int32_t* footprint_lambda, float* cost_fc, float* cost_fo,
                       int32_t* cv_cell, float* cv_scale, void* stream);
int stp3_traj_cost_bwd(const stp3_plan_dims* dims, const float* grad_cost_fo, const int32_t* cv_cell,
                       const float* cv_scale, float* grad_cost_volume, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Planner: the tail of an inference call (csrc/stp3_plan.hip) -- what the reference's callers run after the forward
 * (evaluate.py:96-132, carla_agent.py:397-462) as two launches that a hipGraph can hold: nothing in them depends on the host.
 *
 * stp3_plan_scene -- the planner's view of the scene from the decoder's heads, one launch over the BEV grid: replaces
 * evaluate.py:96-106,122 (argmax of the segmentation and pedestrian heads, logical_or) and the head of Rule / HeadwayCost /
 * LR_divider.forward (stp3/cost.py:196-201, :258-263, :289-294: softmax of a logit pair, threshold).
 *   segmentation [B][S][Cs][H][W], pedestrian [B][S][Cp][H][W] (Cp = 0: NULL), hdmap [B][4][H][W]: logits, float32 or bf16, any
 *                element strides (channels-last included); float32 arithmetic after widening
 *   occupancy [B][T][H][W] float32 = 1 where the argmax class of either head at frame first + t is != 0 (the first maximal
 *                class wins a tie, a NaN counts as the maximum: torch.argmax), else 0
 *   lane     [B][H][W] float32 = softmax probability of class 1 of channels 0:2, 0 where it is <= 0.5
 *   drivable [B][H][W] float32 = softmax probability of class 1 of channels 2:4, 0 where it is <  0.5
 * STP3_EINVAL: a null pointer, a size < 1, first < 0 or first + T > S; STP3_EUNSUP: another dtype, B or T + 1 > 65 535.
 *
 * stp3_plan_drive -- select and refine, one launch, one workgroup per sample: replaces the eval path of Planning.forward
 * (stp3/models/planning_model.py:101-145: the command's third of the samples :103-115, Planning.select :47-64 with
 * Cost_Function :26-47, the GRUCell / decoder loop :121-132).
 *   dims, cost_volume (the sample stride given apart), occupancy, drivable, lane, target, footprint tables: as for
 *   stp3_traj_cost_fwd, whose arithmetic scores the candidates (one shared device function); the batch's target sum is taken
 *   inside.  trajs: N rows of T points per sample, float32, (lateral, forward[, heading ...]) with the strides of `drive`.
 *   command [B] int32: 0 LEFT, 1 FORWARD, 2 RIGHT select the rows [k N / 3, (k + 1) N / 3), anything else all N rows; each
 *   DISTINCT row is scored once.  total = cost_fc + (sum over t ascending of cost_fo[t]); the smallest total wins, the lowest
 *   row index on an exact tie (a fixed-order reduction inside the workgroup).
 *   cost_volume and h0 may be float32 or bf16 (drive->cv_dtype / h0_dtype; widened to float32 where they are read).
 *   h0 [B][Hs]: the GRU state (the reduced front-camera features).  Per step x = [previous point (0 first), selected
 *   point, target], torch.nn.GRUCell (gates r, z, n; n = tanh(W_in x + b_in + r (W_hn h + b_hn))), Linear - ReLU - Linear.
 *   float32, every dot product one fused-multiply-add chain in ascending k (the last layer: 64 interleaved chains and a fixed
 *   butterfly): bit-reproducible run to run.
 *   final_traj [B][T][3] (third column 0), selected_traj [B][T][3] (the chosen row's first 3 columns; 0 where it has 2),
 *   selected_index [B] int32 (a row of the N given).
 * STP3_EINVAL: a null pointer, invalid dims, N % 3 != 0, Hs < 1, traj_cols < 2, a point stride below traj_cols, a negative
 * stride.  STP3_EUNSUP: Hs not a multiple of 64 or > 512; more than 160 KB of LDS (4 (N (T + 1) + 8 Hs + 2056) bytes); 3 T > 1024;
 * a stride of 2^31 elements or more; another dtype; a device ordinal >= 64.
 * Both are answered before anything touches the GPU. */
typedef struct stp3_scene_dims {
    int32_t B, S, T, H, W;
    int32_t Cs, Cp;                               /* classes of the two heads; Cp = 0: no pedestrian head */
    int32_t first;                                /* first frame used: the model's receptive field */
    int32_t seg_dtype, ped_dtype, hd_dtype;       /* STP3_DTYPE_* */
    int64_t seg_stride[5], ped_stride[5];         /* elements: sample, frame, class, row, column */
    int64_t hd_stride[4];                         /* elements: sample, channel, row, column */
} stp3_scene_dims;
int stp3_plan_scene(const stp3_scene_dims* dims, const void* segmentation, const void* pedestrian, const void* hdmap,
                    float* occupancy, float* lane, float* drivable, void* stream);
typedef struct stp3_drive_dims {
    int32_t Hs;                                   /* GRU state size: a multiple of 64, <= 512 */
    int32_t traj_cols;                            /* columns of a trajectory point (>= 2) */
    int32_t cv_dtype, h0_dtype;                   /* STP3_DTYPE_* of cost_volume and h0 (bf16 is widened inside) */
    int64_t traj_batch_stride, traj_row_stride, traj_point_stride;   /* floats */
    int64_t cv_batch_stride;                      /* floats between the cost volumes of two samples ([T][H][W] is dense) */
    const float* weights;                         /* one buffer of 4 Hs Hs + 27 Hs + 2 floats: GRUCell.weight_ih [3 Hs][6],
                                                     bias_ih [3 Hs], weight_hh TRANSPOSED [Hs][3 Hs], bias_hh [3 Hs],
                                                     decoder[0].weight TRANSPOSED [Hs][Hs], decoder[0].bias [Hs],
                                                     decoder[2].weight [2][Hs], decoder[2].bias [2] */
} stp3_drive_dims;
int stp3_plan_drive(const stp3_plan_dims* dims, const stp3_drive_dims* drive, const float* trajs, const void* cost_volume,
                    const float* occupancy, const float* drivable, const float* lane, const float* target,
                    const int32_t* command, const int32_t* footprint0, const int32_t* footprint_lambda, const void* h0,
                    float* final_traj, float* selected_traj, int32_t* selected_index, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Planner: the candidate set (csrc/stp3_sampler.hip) -- the reference's trajectory sampler, stp3/utils/sampler.py:8-146, as
 * its loaders call it (stp3/datas/NuscenesData.py:389-437: T0 = (0, 1), N0 = (1, 0) for kappa <= 0 else (-1, 0), frames
 * dt = 0.5 s apart, [:, ::10]): M trajectories per sample -- straight lines (:47-49), arcs about the curvature clamped to
 * |kappa| >= 0.01 (:53-66) and clothoids through the Fresnel integrals (:72-104) around the measured speed (:28-37), one
 * curve block mirrored depending on the sign of kappa (:129-140) -- evaluated at the n_future + 1 frame times only, ordered by
 * the lateral position of the last pose (:143-144).  One launch per batch, one workgroup per sample, nothing allocated.
 *   v0, kappa  [B] float64              initial speed (m/s), curvature (1/m, positive: left)
 *   draws      [B][3 M + 2 Mc] float64  uniforms in [0, 1), Mc = n_left + n_right, in the order the reference consumes its
 *                                       random stream: accelerations [M], velocity candidates [M], velocity selection [M]
 *                                       (< 0.2 keeps v0), clothoid scales [Mc], arc-or-clothoid pick [Mc] (< 0.2: arc)
 *   trajs      [B][M][n_future + 1][3] float32  (x lateral, y forward, heading); float64 arithmetic, rounded on the store
 *   order      [B][M] int32, optional (NULL): the generation index of each output row -- its row in the reference's array
 *                                       before the sort, [left | lines | right] (:142)
 *   sort != 0: rows in ascending order of the STORED (float32) x of the last pose, equal keys in ascending generation index
 *              (the reference's argsort is not stable and its straight lines all tie at 0); sort == 0: generation order.
 * STP3_EINVAL: B, M or n_future < 1, a negative count, n_left + n_straight + n_right != M, dt <= 0, a null pointer (order
 * excepted).  Limit: M <= 8 192 (the keys of a sample, 8 bytes each, in 64 KB of one workgroup's LDS); else STP3_EUNSUP.
 * Both are answered before anything touches the GPU. */
typedef struct stp3_sampler_dims {
    int32_t B, M;
    int32_t n_left, n_straight, n_right;          /* int(M p) of the reference's possibility = (0.4, 0.2, 0.4), :24-26 */
    int32_t n_future;
    double dt;                                    /* 0.5 s */
    int32_t sort;
} stp3_sampler_dims;
int stp3_traj_sample(const stp3_sampler_dims* dims, const double* v0, const double* kappa, const double* draws,
                     float* trajs, int32_t* order, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vehicle instances from the centerness / offset / flow heads (csrc/stp3_instance.hip) -- the reference's post-processing,
 * stp3/utils/instance.py:80-269, as its validation step and evaluate.py call it (predict_instance_segmentation_and_
 * trajectories, :272-306).  The same rules as torch code: st-p3_amd/stp3_amd/instance.py.
 *
 * stp3_instance_segment -- get_instance_segmentation_and_centers (:116-144: find_instance_centers :80-91, group_pixels
 * :94-113, make_instance_seg_consecutive :165-170) for N = B * S frames in one launch, one workgroup per frame.
 *   center      [N][H][W] float32      centerness
 *   offset      [N][2][H][W] float32   (row, column) offset to the instance centre
 *   foreground  [N][H][W] uint8        non-zero: the pixel's class is the vehicle class
 *   seg         [N][H][W] int32        instance ids
 *   centers     [N][100][2] int32      (row, column) of the centres, zero beyond counts[n]
 *   counts      [N] int32
 *   - a centre: t = (x <= conf_threshold ? -1 : x) is > 0 and equals the maximum of t over the 3x3 neighbourhood inside the
 *     image; every tied pixel of a plateau is one; a NaN in the neighbourhood disqualifies (max_pool2d propagates it);
 *   - centres are numbered in row-major order and cut to the first 100 (max_n_instance_centers);
 *   - a pixel's centre: the k with the lowest float32 sqrt(dr * dr + dc * dc), dr = row_k - (row + offset[0]), without
 *     contraction and with a correctly rounded square root, the lowest k on equal values;
 *   - id = (k + 1) * (foreground != 0), then replaced by its rank among the distinct ids of the frame -- a frame without a
 *     background pixel has no id 0, so its lowest id becomes 0 (the reference's behaviour);
 *   - a frame without centres: all ids 0, count 0 (:130-132).
 *
 * stp3_instance_track -- make_instance_id_temporally_consistent (:173-269) for B samples in one launch, one workgroup per
 * sample, the loop over the S frames inside.
 *   raw    [B][S][H][W] int32      ids of stp3_instance_segment: per frame 0..n, every value present, n <= 100
 *   flow   [B][S][2][H][W] float32 (row, column) displacement to the next frame; NULL: zero flow
 *   out    [B][S][H][W] int32      consistent ids; frame 0 is raw frame 0
 *   err    [4] int32, zeroed by the caller: word k is set to 1 when  0: the assignment hit its iteration bound,  1: a raw
 *          frame's ids are not 0..n <= 100 with every value present (an offending pixel counts as background),  2: a frame
 *          has no background pixel,  3: a flow value of an instance pixel is not finite or >= 32768 in magnitude (taken as
 *          0).  The kernel always runs to its end.
 *   Per step t: rows = the ids of the consistent frame t, ascending, at the mean of (row, col) + flow[t] over their pixels;
 *   columns = ids 1..n of raw frame t + 1 at their pixel means; means are exact sums (integer coordinates, flow rounded to
 *   2^-20 pixel) divided in float64 and rounded to float32; float32 Euclidean distances; minimum-cost assignment by
 *   shortest augmenting paths over the smaller side in float64 (the method of scipy's linear_sum_assignment, its tie rule
 *   included); pairs with distance < matching_threshold keep the row's id; every other id of frame t + 1 gets
 *   ++largest_instance_id IN ASCENDING ORDER OF ITS OLD ID (the reference hands them out in the iteration order of a Python
 *   set, :257-264, which is not an order: results agree up to a renaming of ids created at the same step).  No instance at t
 *   or none at t + 1: the raw frame is taken over (:211-214, :228-231); largest_instance_id starts at the maximum of frame
 *   0 and is carried across.
 * Both: STP3_EINVAL for a count or side < 1 or a null pointer (flow excepted); STP3_EUNSUP for H or W > 1024 or
 * H * W >= 2^24.  Answered before anything touches the GPU. */
int stp3_instance_segment(int32_t N, int32_t H, int32_t W, float conf_threshold, const float* center, const float* offset,
                          const uint8_t* foreground, int32_t* seg, int32_t* centers, int32_t* counts, void* stream);
int stp3_instance_track(int32_t B, int32_t S, int32_t H, int32_t W, float matching_threshold, const int32_t* raw,
                        const float* flow, int32_t* out, int32_t* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation scorer (csrc/stp3_eval.hip) -- the metric updates of the reference's evaluation loop, evaluate.py:95-137, as
 * launches on the caller's stream with nothing in them that waits for the host: a hipGraph can hold them.  The states are
 * ADDED TO, never overwritten; the caller zeroes them (and `err`) once.  The host side: st-p3_amd/stp3_amd/evaluation.py.
 *
 * stp3_eval_semantic -- evaluate.py:95-119 (argmax of every semantic head) and IntersectionOverUnion.update
 * (stp3/metrics.py:37-43, stat_scores_multiple_classes) for all heads of an update in ONE launch.
 *   segmentation [B][S][Cs][H][W], pedestrian [B][S][Cp][H][W] (Cp = 0: NULL), hdmap [B][2 E][H][W] (E = 0: NULL): logits,
 *                float32 or bf16, any non-negative element strides (channels-last included)
 *   segmentation_label, pedestrian_label [B][S][1][H][W], hdmap_label [B][E][H][W]: int64, dense
 *   counts       int64 [2 + E][n_classes][4]: tp, fp, fn, support per class of the heads segmentation, pedestrian (left alone
 *                when Cp = 0), hd-map element 0 .. E - 1 (the logit pair 2 e, 2 e + 1)
 *   Frames first .. S - 1 of the two temporal heads are scored; the hd-map has no time axis.  Per pixel: the arg-max class
 *   (the first maximal class wins a tie, a NaN counts as the maximum: torch.argmax, the rule of stp3_plan_scene); class c
 *   counts tp when prediction and label are both c, fp when only the prediction is, fn when only the label is, support
 *   when the label is.  A label (or prediction) outside [0, n_classes), such as 255, is no class of its own but still makes
 *   the other side's class a false positive / negative.  Integer sums: exact and the same in every run.
 * STP3_EINVAL: a null pointer (a head that is switched off excepted, and then required to be NULL), a size < 1, first
 * outside [0, S); STP3_EUNSUP: Cs or Cp > 16, n_classes > 8, H or W > 1024, another dtype, a stride of 2^31 elements or
 * more, more than 65 535 planes (B (S - first) per temporal head + B E).
 *
 * stp3_eval_planning -- PlanningMetric.update (stp3/metrics.py:292-389; evaluate.py:122-137) in one launch of one workgroup.
 *   trajs, gt_trajs [B][T][>= 2] float32 (lateral, forward, ...), sample and point strides in floats
 *   the label maps of stp3_eval_semantic ([B][S][1][H][W] int64; pedestrian_label may be NULL): the true occupancy of step t
 *   is `segmentation label != 0 or pedestrian label != 0` at frame first_future + t, evaluated where it is read
 *   footprint [K][2] int32: the (row, column) cell offsets of the ego box (cost.BaseCost.footprint(0))
 *   obj_col, obj_box_col int64 [T], total int64 [1], l2 float64 [T]
 *   Per step, in float32 without contraction: distance = sqrtf(dx dx + dy dy); x is negated (the BEV flip); a box cell is
 *   trunc(y / dx0 + row) / trunc(x / dx1 + column) clamped into the grid; the point's cell trunc((y - bx0) / dx0),
 *   trunc((x - bx1) / dx1) counts only inside the grid; steps at which the EXPERT's box collides are not counted.  The
 *   distances are added to l2 in ascending sample order by one thread per step; total += B.
 * STP3_EINVAL: a null pointer (pedestrian_label excepted), a size < 1, first_future < 0 or first_future + T > S, a cell size
 * <= 0, a negative stride; STP3_EUNSUP: B T > 1024, H or W > 1024.
 *
 * stp3_eval_panoptic -- PanopticMetric.update (stp3/metrics.py:94-261) for n_classes = 2, vehicles_id = 1: one workgroup per
 * sample with the loop over its frames inside, then a one-workgroup launch that finishes.
 *   pred, gt   [B][S][H][W] int32 (wide_ids = 0) or int64 (wide_ids != 0) instance ids, 0 = background; frames first .. S - 1
 *   workspace  stp3_eval_panoptic_workspace_bytes: the per-frame results [B (S - first)][4][2] float32 (iou, true positive,
 *              false positive, false negative; class 0 = background, 1 = vehicle) stay there for the caller to read
 *   state      float32 [4][2]
 *   err        [4] int32, zeroed by the caller: word k is set to 1 when  0: an id lies outside [0, 2^20) (the pixel counts as
 *              background),  1: no ground-truth pixel of the update is background,  2: a frame has more distinct (gt id,
 *              predicted id) pairs than the table holds -- STP3_EVAL_PANOPTIC_PAIRS - 1 besides (background, background) --
 *              or a sample matched more than STP3_EVAL_PANOPTIC_PAIRS distinct gt ids (the frame's result is then
 *              meaningless);  3: reserved, never set.  The kernels always run to their end.
 *   Per frame: the distinct pairs with their pixel counts and the areas per id; in ascending (gt id, predicted id): IoU =
 *   (n + 1e-9f) / (area_gt + area_pred - n + 1e-9f) in float32; a match needs IoU > 0.5 and both sides background or both
 *   vehicles; with temporally_consistent != 0 a matched vehicle whose gt id was last matched (in an earlier frame of the
 *   sample) to ANOTHER predicted id counts as one false negative plus one false positive instead; ids with pixels and no
 *   match candidate count as false negative (gt) / false positive (predicted).  The frames are added in update order
 *   (sample-major, frame ascending) into a zero total, which is added to `state`: one update of a zero state has the
 *   reference's bits.
 * STP3_EINVAL: a null pointer, a size < 1, first outside [0, S); STP3_EUNSUP: H or W > 1024, H W >= 2^24, B > 65 535;
 * STP3_ENOSPACE: the workspace is too small.
 * All are answered before anything touches the GPU. */
#define STP3_EVAL_PANOPTIC_PAIRS 1024
typedef struct stp3_eval_dims {
    int32_t B, S, H, W;
    int32_t Cs, Cp, E;                            /* classes of the two temporal heads (Cp = 0: none), hd-map elements */
    int32_t n_classes;                            /* classes counted per head */
    int32_t first;                                /* first frame scored: the model's receptive field - 1 */
    int32_t seg_dtype, ped_dtype, hd_dtype;       /* STP3_DTYPE_* */
    int64_t seg_stride[5], ped_stride[5];         /* elements: sample, frame, class, row, column */
    int64_t hd_stride[4];                         /* elements: sample, channel, row, column */
} stp3_eval_dims;
int stp3_eval_semantic(const stp3_eval_dims* dims, const void* segmentation, const void* pedestrian, const void* hdmap,
                       const int64_t* segmentation_label, const int64_t* pedestrian_label, const int64_t* hdmap_label,
                       int64_t* counts, void* stream);
typedef struct stp3_eval_plan_dims {
    int32_t B, T, S, H, W;
    int32_t K;                                    /* footprint cells */
    int32_t first_future;                         /* frame of step 0: the model's receptive field */
    float dx0, dx1, bx0, bx1;                     /* cell size and first cell centre, (forward, lateral) */
    int64_t traj_stride[2], gt_stride[2];         /* floats: sample, point */
} stp3_eval_plan_dims;
int stp3_eval_planning(const stp3_eval_plan_dims* dims, const float* trajs, const float* gt_trajs,
                       const int64_t* segmentation_label, const int64_t* pedestrian_label, const int32_t* footprint,
                       int64_t* obj_col, int64_t* obj_box_col, int64_t* total, double* l2, void* stream);
int stp3_eval_panoptic_workspace_bytes(int32_t B, int32_t S, int32_t first, size_t* bytes);
int stp3_eval_panoptic(int32_t B, int32_t S, int32_t H, int32_t W, int32_t first, int32_t temporally_consistent,
                       int32_t wide_ids, const void* pred, const void* gt, void* workspace, size_t workspace_bytes,
                       float* state, int32_t* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Camera images: decoded bytes -> network input (csrc/stp3_image.hip).  The per-image chain of the reference's loader,
 * stp3/datas/NuscenesData.py:236-244: resize_and_crop_image (stp3/utils/geometry.py:9-13: PIL resize BILINEAR + crop)
 * followed by torchvision ToTensor + Normalize (:68-72), for all N images of a batch in one launch.
 *   images   [N][H][W][3] uint8 (RGB, as PIL decodes them)
 *   kk_h / bounds_h  [Wr][ksize_h] int32 / [Wr][2] int32: Pillow's horizontal resampling coefficients in its 22-bit fixed
 *            point and (first source column, count) per resized column; kk_v / bounds_v the same for the rows.  Built on
 *            the host exactly as Pillow builds them (stp3_amd.datas.pil_bilinear_coefficients); configuration-only.
 *   out      [N][3][Ho][Wo] float32 or bf16 = ((byte / 255) - mean[c]) / std[c], byte = the resized image at
 *            (top + r, left + x); window positions outside the resized image are PIL's zero padding.
 *   strip_rows: the largest number of source rows the vertical taps of the output rows of one workgroup span (host:
 *            from bounds_v; stp3_image_prep_rows_per_workgroup() returns how many rows that is); sizes the LDS strip.
 * The resized bytes equal PIL.Image.resize(..., BILINEAR) bit for bit (both passes, byte rounding between them). */
typedef struct stp3_image_dims {
    int32_t N, H, W;              /* source */
    int32_t Wr, Hr;               /* resize_dims */
    int32_t left, top, Wo, Ho;    /* crop window in the resized image */
    int32_t ksize_h, ksize_v;
    int32_t out_dtype;            /* STP3_DTYPE_F32 | STP3_DTYPE_BF16 */
    float mean[3], std[3];
} stp3_image_dims;
int stp3_image_prep_rows_per_workgroup(void);
int stp3_image_prep_lds_bytes(const stp3_image_dims* dims, int32_t strip_rows, size_t* bytes);
int stp3_image_prep(const stp3_image_dims* dims, const uint8_t* images, const int32_t* kk_h, const int32_t* bounds_h,
                    const int32_t* kk_v, const int32_t* bounds_v, int32_t strip_rows, void* out, void* stream);

/* Camera images with a PER-IMAGE augmentation (csrc/stp3_image.hip): the Lift-Splat step the reference carries as
 * img_transform, stp3/utils/tools.py:122-146 -- resize, crop, horizontal flip, in-plane rotation -- with the loader's
 * resize filter (resize_and_crop_image, stp3/utils/geometry.py:9-13: BILINEAR) and ToTensor + Normalize behind it:
 *     Image.resize(resize_dims_i, BILINEAR) -> .crop(crop_i) -> [.transpose(FLIP_LEFT_RIGHT)] -> .rotate(rotate_i)
 * byte-exact with Pillow for all N images of a call.  All crops of a call have the size Wo x Ho.
 *   images   [N][H][W][3] uint8
 *   table    [N] stp3_augment_image IN DEVICE MEMORY (a captured graph is replayed with new parameters by rewriting it):
 *            resize_dims (Wr, Hr), the crop origin (left, top) in the resized image, flip, the six 16.16 fixed-point
 *            integers of Pillow's Image.rotate (NEAREST, no expand, centre (Wo / 2, Ho / 2), zero fill; the host computes
 *            them in float64 as Pillow does, stp3_amd.datas.pil_rotate_fixed; 65536, 0, 32768, 0, 65536, 32768 is the
 *            identity), and where the image's coefficient tables start in `coef`, in int32 elements.
 *   coef     [coef_len] int32 in device memory: per distinct (source size, resized size) of an axis the table
 *            kk [resized][ksize] followed anywhere by bounds [resized][2] of stp3_image_prep, every kk row padded with
 *            zeros to the call's largest tap count `ksize` (one value for both axes).
 *   strip_rows  as for stp3_image_prep, the largest over the images of the call.
 *   cols     the LDS strip and coefficient rows hold only the window columns that lie inside the resized image (a contiguous
 *            range, mirrored by the flip): the largest count over the images of the call (Wo always fits).
 *   rotate   0: no image of the call is rotated; the rotation integers are not read, `workspace` may be NULL and the call is
 *            ONE launch.  1: TWO launches -- the resampler writes the images whose rotation is not the identity as cropped
 *            and flipped bytes [N][Ho][Wo][3] into `workspace` (the others directly into `out`), and a nearest gather
 *            reads them at Pillow's slanted integer addresses and normalises.
 *   out      [N][3][Ho][Wo] float32 or bf16.
 * The kernels clamp every address a table entry produces (rows to the source, table offsets to coef_len, strip rows to
 * strip_rows): an image whose entry is malformed is left unwritten, it cannot make the kernels read or write outside the
 * buffers.  Enqueues on `stream` only, allocates nothing, does not synchronise (capturable).
 * STP3_EINVAL: a null pointer, a size < 1, Wo or Ho above 8192 (Pillow's 32-bit accumulation is not reproduced past it),
 * rotate with a workspace smaller than stp3_image_augment_workspace_bytes;  STP3_EUNSUP: another out_dtype, N > 65 535,
 * more LDS than a workgroup has. */
typedef struct stp3_augment_image {
    int32_t Wr, Hr;               /* resize_dims of this image */
    int32_t left, top;            /* crop origin in the resized image */
    int32_t flip;                 /* 0 | 1 */
    int32_t rot[6];               /* a0 a1 a2 a3 a4 a5: xin = (a2 + x a0 + y a1) >> 16, yin = (a5 + x a3 + y a4) >> 16 */
    int32_t kk_h, bounds_h, kk_v, bounds_v;     /* offsets into coef */
    int32_t reserved;
} stp3_augment_image;
typedef struct stp3_augment_dims {
    int32_t N, H, W;              /* source */
    int32_t Wo, Ho;               /* crop size, the same for every image */
    int32_t cols;                 /* 1 .. Wo: the most window columns of one image that lie inside its resized image */
    int32_t ksize, strip_rows, rotate, coef_len;
    int32_t out_dtype;            /* STP3_DTYPE_F32 | STP3_DTYPE_BF16 */
    float mean[3], std[3];
} stp3_augment_dims;
int stp3_image_augment_workspace_bytes(const stp3_augment_dims* dims, size_t* bytes);
int stp3_image_augment(const stp3_augment_dims* dims, const uint8_t* images, const stp3_augment_image* table,
                       const int32_t* coef, void* workspace, size_t workspace_bytes, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG camera frames (csrc/stp3_jpeg_entropy.h, csrc/stp3_jpeg.hip): a baseline decode split where it is serial.  The
 * Huffman bit stream is decoded on the HOST into quantised coefficients; dequantisation, inverse DCT, chroma up-sampling
 * and colour conversion run in ONE kernel whose output is the `images` of stp3_image_prep / stp3_image_augment, byte for
 * byte what Pillow (libjpeg-turbo, default settings) decodes.  Restated from libjpeg's published source: jidctint.c
 * (jpeg_idct_islow), jdsample.c (h2v1 / h2v2 fancy up-sampling and its replication fall-back for chroma widths <= 2,
 * reproduced), jdmainct.c (edge context rows), jdcolor.c (ycc_rgb_convert), jdmaster.c (the range-limit table), jdapimin.c
 * (how the colour space is guessed), jdhuff.c (look-ahead Huffman decoding).
 *
 * Host (plain C++, no GPU call; allocates nothing persistent, keeps no state, throws nothing):
 *   stp3_jpeg_info     parses the markers up to the scan and fills the header, so that the caller can size its buffers.
 *   stp3_jpeg_entropy  decodes the scan.  coef: header.coef_count int16 (room for coef_capacity ELEMENTS), component after
 *                      component, each [blocks_y][blocks_x][64] in NATURAL (de-zigzagged, row-major) order, every block of
 *                      the MCU grid, padding blocks included (blocks_x = mcus_x * h factor, blocks_y = mcus_y * v factor).
 *                      quant: [3][64] uint16 in natural order, one table per component (grey: three copies).
 *   Streams: SOF0 / SOF1, 8-bit samples, Huffman, ONE scan; one component (grey; decoded 1x1) or Y Cb Cr with luma
 *   sampling 1x1, 2x1 or 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0); restart intervals; 8- and 16-bit quantisation tables;
 *   sides up to 16 384.  STP3_EUNSUP, decided before anything is written: progressive, arithmetic, lossless, 12-bit, four
 *   components (CMYK / YCCK), RGB streams (Adobe transform 0, or ids 'R','G','B' without JFIF), other sampling factors, a
 *   scan that holds only part of the components.  STP3_EINVAL: a null pointer, a malformed or truncated stream (a code no
 *   table assigns, a run past coefficient 63, a table the scan names but no segment defined, a missing RSTn or EOI, data
 *   that ends early, a coefficient whose dequantised value |coefficient * quantiser| exceeds 32 767 -- no 8-bit encoder
 *   writes one, libjpeg-turbo's SIMD IDCT holds 16 bits there, and the byte equality with Pillow is claimed inside that
 *   bound), a buffer smaller than coef_count.  Bytes that are no marker in front of an RSTn or of EOI are skipped, as
 *   libjpeg skips them with a warning.  Every read is checked against len, every write against the buffer.
 *
 * Device: stp3_jpeg_reconstruct, all N images of a call at once; they share width, height, components and sampling.
 *   coef   [N][coef_count] int16 in device memory, as stp3_jpeg_entropy wrote them
 *   quant  [N][3][64] uint16 IN DEVICE MEMORY, per image (a captured graph is replayed on new images by rewriting both)
 *   out    [N][height][width][3] uint8 RGB (grey: the sample three times, as Image.convert('RGB'))
 *   A workgroup owns stp3_jpeg_strip_rows(vs) pixel rows of one image (whole MCU rows) and keeps their samples in LDS.
 * Enqueues on `stream` only, allocates nothing, does not synchronise (capturable).  STP3_EINVAL: a null pointer, a size < 1,
 * components / sampling outside the list above;  STP3_EUNSUP: N > 65 535, a side above 16 384, a strip wider than LDS (about
 * 2 500 pixels). */
typedef struct stp3_jpeg_header {
    int32_t width, height;
    int32_t components;           /* 1 | 3 */
    int32_t hs, vs;               /* luma sampling factors (chroma is 1 x 1) */
    int32_t mcus_x, mcus_y;
    int32_t blocks_x[3], blocks_y[3];
    int32_t restart_interval;     /* MCUs, 0: none */
    int32_t coef_count;           /* int16 elements of one image */
} stp3_jpeg_header;
typedef struct stp3_jpeg_dims {
    int32_t N, width, height, components, hs, vs;
} stp3_jpeg_dims;
int stp3_jpeg_info(const uint8_t* data, size_t len, stp3_jpeg_header* header);
int stp3_jpeg_entropy(const uint8_t* data, size_t len, int16_t* coef, size_t coef_capacity, uint16_t* quant,
                      stp3_jpeg_header* header);
int stp3_jpeg_strip_rows(int32_t vs);
int stp3_jpeg_reconstruct(const stp3_jpeg_dims* dims, const int16_t* coef, const uint16_t* quant, uint8_t* out,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG camera frames, the Huffman scan ON THE DEVICE (csrc/stp3_jpeg_entropy.h: stp3_jpeg_scan_prepare;
 * csrc/stp3_jpeg_huff.hip): a second way to the coefficient and table buffers of stp3_jpeg_reconstruct, equal to what
 * stp3_jpeg_entropy writes element for element, padding blocks included.  The host decoder stays the statement of the
 * result; this path never guesses -- whatever it does not decode cleanly is reported and belongs to stp3_jpeg_entropy.
 * Restated from published sources: jdhuff.c (the look-ahead tables and the symbol decode, as above) and, for the parallel
 * scheme, Klein & Wiseman, "Parallel Huffman decoding with applications to JPEG files" (The Computer Journal 46(5), 2003:
 * a decoder started at a wrong bit falls into step with the right one after a few codes) and Weissenberger & Schmidt,
 * "Massively parallel Huffman decoding on GPUs" (ICPP 2018: subsequences, one thread each, overflow into the neighbours
 * until the recorded state repeats, a prefix sum for the output positions, a second decode that writes).
 *
 * Host: stp3_jpeg_scan_prepare parses the headers exactly as stp3_jpeg_info does (the same STP3_EUNSUP / STP3_EINVAL),
 *   then walks the entropy-coded bytes ONCE (memchr for 0xFF, block copies) and writes into `scan_out` (room for
 *   scan_capacity bytes; stp3_jpeg_scan_bytes(header, len) is an upper bound):
 *     [seg_offset]     nseg x {first subsequence, bit length, first MCU} int32 -- one SEGMENT per restart interval (a
 *                      stream without restart markers: one), in stream order
 *     [scan_offset]    nsub subsequences of STP3_JPEG_SUB_BYTES bytes: the scan WITHOUT byte stuffing and without the
 *                      markers, every segment padded with zeros to whole subsequences (at least one)
 *     [subseg_offset]  nsub int32: the segment of every subsequence
 *   and fills `desc`: those offsets and counts, the look-ahead tables as the host decoder builds them (at most two DC and
 *   two AC tables), the table index per component, the quantisers in ZIGZAG order (for the 16-bit bound) and the MCU
 *   layout.  quant: [3][64] uint16 in natural order, as stp3_jpeg_entropy writes it.  STP3_JPEG_IRREGULAR (not an error:
 *   the caller gives the stream to stp3_jpeg_entropy): a marker in the scan other than the RSTn expected in sequence, no
 *   EOI, fill bytes (0xFF 0xFF) or an 0xFF at the very end, a segment count that differs from what restart_interval and
 *   the MCU count give, more than two tables of a class, more than 65 536 segments or 2^27 bytes.  (Junk bytes in front
 *   of a marker are indistinguishable from data here: the device decode reports such a stream, see below.)  STP3_EINVAL
 *   also for a null pointer or a scan_capacity too small.  Every read is checked against len, every write against
 *   scan_capacity; nothing is allocated, no state is kept.
 *
 * Device: stp3_jpeg_entropy_device, all N images of one geometry per call.
 *   scans   [N][scan_stride] bytes in device memory, image n as stp3_jpeg_scan_prepare wrote it (scan_stride: a multiple
 *           of 4, at least every image's used_bytes)
 *   descs   [N] stp3_jpeg_scan_desc in device memory
 *   coef    [N][coef_count] int16, as stp3_jpeg_entropy writes them (cleared first by the call)
 *   status  [N] int32: 0 decoded; STP3_JPEG_NOT_CONVERGED the subsequences had not fallen into step after `sync_rounds`
 *           further launches; STP3_EINVAL a code no table assigns, a run past coefficient 63, a coefficient or a running DC
 *           whose dequantised value leaves 16 bits, a bit consumed behind a segment's end, a segment that does not end
 *           inside its last byte with exactly its MCUs, or a descriptor that does not fit scan_stride / max_subs /
 *           max_segs.  The coefficients of an image whose status is not 0 are unspecified: decode it with stp3_jpeg_entropy.
 *   workspace  stp3_jpeg_entropy_workspace_bytes(dims, sync_rounds, &bytes) bytes of device memory.  Its first
 *           N x (sync_rounds + 3) int32 are per image: [0 .. sync_rounds] whether launch r of the synchronisation still
 *           changed a state another workgroup had consumed (the first zero: the rounds used), [sync_rounds + 1] the error
 *           flag, [sync_rounds + 2] how many subsequences decoded more than one further subsequence before their state
 *           repeated.
 *   Passes: synchronise (one thread per subsequence, STP3_JPEG_SUB_THREADS subsequences per workgroup: decode from the
 *   assumed state "first block of an MCU, DC expected", run on into the following subsequences until the state recorded
 *   there repeats; across workgroups in at most sync_rounds further launches of the same step), a prefix sum of the blocks
 *   completed per subsequence, a second decode that stores AC values and DC DIFFERENCES, an ordered scan of the DC
 *   differences per component and segment, the status.  Every loop has a bound fixed by the host, no workgroup waits for
 *   another, every store index is compared with coef_count.  Enqueues on `stream` only, allocates nothing, does not
 *   synchronise.  STP3_EINVAL: a null pointer, dims outside what stp3_jpeg_reconstruct takes, scan_stride / max_subs /
 *   max_segs < 1, sync_rounds outside [0, 64];  STP3_ENOSPACE: workspace_bytes too small. */
#define STP3_JPEG_IRREGULAR      10011   /* stp3_jpeg_scan_prepare: a stream for the host decoder */
#define STP3_JPEG_NOT_CONVERGED  10012   /* status word of stp3_jpeg_entropy_device */
#define STP3_JPEG_SUB_BYTES      128     /* S: bytes of a subsequence */
#define STP3_JPEG_SUB_THREADS    256     /* G: subsequences (threads) of a workgroup */
typedef struct stp3_jpeg_huff_table {       /* csrc/stp3_jpeg_entropy.h: Huff */
    uint16_t look[512];
    int32_t maxcode[18];
    int32_t valptr[17];
    uint8_t vals[256];
} stp3_jpeg_huff_table;
typedef struct stp3_jpeg_scan_desc {
    int32_t nsub, nseg;
    int32_t seg_offset, scan_offset, subseg_offset, used_bytes;   /* bytes, inside the image's scan buffer */
    int32_t components, hs, vs, mcus_x, mcus_y, restart_interval, coef_count;
    int32_t dc_table[3], ac_table[3];       /* per component: index into dc[] / ac[] */
    uint16_t quant[3][64];                  /* per component, zigzag order */
    stp3_jpeg_huff_table dc[2], ac[2];
} stp3_jpeg_scan_desc;
typedef struct stp3_jpeg_huff_dims {
    int32_t N, width, height, components, hs, vs;
    int32_t scan_stride;                    /* bytes between the scan buffers of two images */
    int32_t max_subs, max_segs;             /* the largest nsub / nseg of the call */
} stp3_jpeg_huff_dims;
size_t stp3_jpeg_scan_bytes(const stp3_jpeg_header* header, size_t len);
int stp3_jpeg_scan_prepare(const uint8_t* data, size_t len, uint8_t* scan_out, size_t scan_capacity,
                           stp3_jpeg_scan_desc* desc, uint16_t* quant);
int stp3_jpeg_entropy_workspace_bytes(const stp3_jpeg_huff_dims* dims, int32_t sync_rounds, size_t* bytes);
int stp3_jpeg_entropy_device(const stp3_jpeg_huff_dims* dims, const uint8_t* scans, const stp3_jpeg_scan_desc* descs,
                             int16_t* coef, int32_t* status, void* workspace, size_t workspace_bytes, int32_t sync_rounds,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone voxel summing (csrc/stp3_voxsum.hip): the operator-level twin of the reference's
 * VoxelsSumming.forward / .backward (stp3/utils/geometry.py:302-318 / :320-330) for callers that hold the
 * rank-sorted row matrix; the fused path above never builds it.
 *   x        [M][channels] float32, rows sorted by voxel rank
 *   seg_off  [n_segments + 1] int32, ascending, seg_off[0] = 0, seg_off[n_segments] = M: voxel s owns the rows
 *            [seg_off[s], seg_off[s+1])  (the host derives it from ranks[1:] != ranks[:-1], geometry.py:308-309)
 *   fwd: out [n_segments][channels] = per-voxel row sums, rows added in ascending order (deterministic; no
 *        running sum over the whole matrix, so no cancellation against preceding voxels)
 *   bwd: grad_x [M][channels], every row receives its voxel's grad_out row (geometry.py:326-328)
 * n_segments == 0 is a no-op. */
int stp3_voxels_sum_fwd(const float* x, const int32_t* seg_off, int32_t n_segments, int32_t channels, float* out,
                        void* stream);
int stp3_voxels_sum_bwd(const float* grad_out, const int32_t* seg_off, int32_t n_segments, int32_t channels,
                        float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BEV labels of the data loader (csrc/stp3_labels.hip).
 *
 * stp3_fill_polygons -- cv2.fillPoly of integer polygons, in order, a later one overwriting an earlier one: what
 *   stp3/datas/NuscenesData.py:303-338 (get_birds_eye_view_label: instance / segmentation / pedestrian maps from the
 *   annotation boxes) and :520-564 (road polygons of voxelize_hd_map) call.  OpenCV is a third-party dependency that is
 *   not vendored under the reference: restated from its published algorithm (8-connected Bresenham outline drawn left to
 *   right + scanlines between pairs of active edges, ceil(left) .. floor(right), 16.16 fixed-point edge positions with the
 *   slope truncated), PARITY UNPINNED; cross-checked against an edge-walking restatement and against Pillow.
 *   polys [n_poly] in paint order: `map` = which of the n_maps [H][W] float32 images, nv <= 8 vertices xy = (column, row)
 *   as cv2 takes them, `value` painted.  The maps are painted over what they hold (zero them for fresh labels).
 * stp3_instance_labels -- stp3/utils/instance.py:12-77 convert_instance_mask_to_center_and_offset_label:
 *   instance [T][H][W] int64 ids (0 = background, 1..K instances); warped [T][H][W] float32 = frame t's instance map warped
 *   into frame t-1 (warp_features(..., mode='nearest'), frame 0 unused) or NULL (no displacement labels);
 *   center [T][1][H][W] = max over the frame's instances of exp(-((xc - x)^2 + (yc - y)^2) / sigma^2), (xc, yc) = rounded
 *   mean pixel of the instance; offset [T][2][H][W] = (xc - x, yc - y) on the instance's pixels, ignore_index elsewhere;
 *   flow [T][2][H][W] = (rounded mean pixel of the instance's WARPED next-frame mask) - (xc, yc) on the instance's
 *   pixels when the instance is in the next frame too and its warped mask is not empty, ignore_index elsewhere.
 *   workspace: stp3_instance_labels_workspace_bytes(T, K) (integer moments; zeroed by the call).  Deterministic.
 */
typedef struct stp3_poly {
    int32_t map, nv;
    float value;
    int32_t reserved;
    int32_t xy[16];
} stp3_poly;

int stp3_fill_polygons(const stp3_poly* polys, int32_t n_poly, int32_t n_maps, int32_t H, int32_t W, float* maps,
                       void* stream);
int stp3_instance_labels_workspace_bytes(int32_t T, int32_t K, size_t* bytes);
int stp3_instance_labels(int32_t T, int32_t H, int32_t W, int32_t K, float ignore_index, float sigma,
                         const int64_t* instance, const float* warped, void* workspace, size_t workspace_bytes,
                         float* center, float* offset, float* flow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference: convolution -> eval BatchNorm -> activation (+ skip) in ONE pass over the layer's tensor (csrc/stp3_conv.hip,
 * csrc/stp3_dwconv.hip, csrc/stp3_bnact.hip).  What they serve: the eval forward the reference runs per validation sample
 * (evaluate.py:88-91) and per simulator tick -- stp3/models/stp3.py:132-184 (forward), encoder.py:57-97 (EfficientNet
 * trunk + heads), decoder.py:91-140 (ResNet-18 BEV decoder + heads) -- with every BatchNorm on its running statistics.
 * The stored route is  stp3_conv2d_fwd / stp3_dwconv2d_fwd  (bf16 tensor written)  then  stp3_bn_apply_fwd  in eval mode
 * (tensor read back, written again); the entry points below KEEP ITS ROUNDING POINTS -- the float32 accumulator (+ bias) is
 * rounded to bf16, then  t = fma(v, scale, shift);  [t += res];  t = act(t);  [t += res]  in float32 as the eval branch of
 * stp3_bn_apply_fwd evaluates it, one rounding at the end -- so their results are BIT-EQUAL to the two operators'.
 *
 * stp3_bn_eval_coefs -- the per-channel constants of every eval BatchNorm of a model, one table-driven launch (as
 *   stp3_conv2d_prep_weights): entry e writes  out[0 .. lanes) = scale, out[lanes .. 2 lanes) = shift  with
 *   invstd = 1 / sqrt(running_var + eps), scale = gamma * invstd, shift = beta - running_mean * scale  (gamma / beta NULL: 1 /
 *   0) -- the device expression of stp3_bn_apply_fwd's eval branch -- and ZERO in the lanes [channels, lanes) (zero-padded
 *   channel lanes: 35 channels in 40 lanes).  first_block: exclusive scan of ceil(lanes / 256) over the entries.
 * stp3_conv2d_fwd_affine -- stp3_conv2d_fwd (same kernels, same tiles, same accumulation order for the same dims) with that
 *   epilogue.  coef = [scale | shift][Cout] float32; channels <= Cout = the BatchNorm's channel count, Cout = channels
 *   rounded up to 8 (the lanes beyond are written as zeros); res NULL or [N][Ho][Wo][ldres] bf16 added before or after
 *   the activation (res_mode STP3_RES_*); y [N][Ho][Wo][ldy] bf16 with ldy >= Cout (a channel slice of a wider tensor).
 *   sbias NULL or [N][channels] float32, a per-sample bias in front of the BatchNorm (the folded image-pooling branch of an
 *   ASPP projection): shift = fma(sbias, scale, shift) per sample, as stp3_bn_apply_fwd folds it; taken by the tiled kernel
 *   only (layers the streaming pointwise kernels run -- 1x1, Cin <= 128, Cout >= 64 -- answer STP3_EUNSUP with an sbias).
 *   STP3_EUNSUP unless: bf16 output, Cout / ldy / ldres multiples of 8, y / res 16-byte aligned.
 * stp3_dwconv2d_fwd_affine -- stp3_dwconv2d_fwd (bf16; 3x3 / 5x5, stride 1 / 2) with the same epilogue, no skip:
 *   coef = [scale | shift][C].
 * stp3_linear_fwd_affine -- stp3_linear_fwd with the eval BatchNorm + activation of a pooled descriptor (ASPP image pooling,
 *   stp3/layers/convolutions.py:229-240) applied to the float32 value it would have stored: scale = coef[n],
 *   shift = coef[ldcoef + n].
 */
typedef struct stp3_bn_coef_entry {
    const float* running_mean;  /* [channels] */
    const float* running_var;
    const float* gamma;         /* NULL: 1 */
    const float* beta;          /* NULL: 0 */
    float* out;                 /* [2][lanes] */
    int64_t first_block;
    int32_t channels, lanes;
    float eps;
    int32_t reserved;
} stp3_bn_coef_entry;

int stp3_bn_eval_coefs(const stp3_bn_coef_entry* table, int32_t n_entries, int64_t total_blocks, void* stream);
int stp3_conv2d_fwd_affine(const stp3_conv_dims* dims, const void* x, const void* w, const float* bias, const float* coef,
                           const float* sbias, int32_t channels, int32_t act, const void* res, int32_t ldres, int32_t res_mode,
                           void* y, void* stream);
int stp3_linear_fwd_affine(int32_t M, int32_t K, int32_t N, const float* x, const float* w, int32_t ldw, const float* b,
                           const float* coef, int32_t ldcoef, int32_t act, float* y, void* stream);
int stp3_dwconv2d_fwd_affine(const stp3_dwconv_dims* dims, const void* x, const float* w, const float* coef, int32_t act,
                             void* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming inference: the sliding window of the closed-loop forward (csrc/stp3_window.hip).  What it serves: the simulator
 * tick, carla_agent.py:408-432 + :445 -- the newest camera frame joins a buffer of T and the model is handed the whole window
 * again.  In eval mode the image encoder (stp3/models/encoder.py:57-97) couples no two images, so the encoder outputs of the
 * T - 1 older frames are kept between ticks, in the layout stp3_lift_splat_fwd reads:
 *   window [B][T][N * pixels][channels] float32, pixel-major (pixels = fH * fW) -- feat_pm and logits_pm.
 * stp3_window_push advances up to STP3_WINDOW_JOBS_MAX such windows by one frame, IN PLACE, in ONE launch (`jobs` is a HOST
 * array, it travels as the kernel argument): per sample  window[t] = window[t + 1]  for t < T - 1, then  window[T - 1] = src,
 * the encoder head's new output -- a logical [B * N][channels][pixels] tensor of dtype STP3_DTYPE_F32 / _BF16 read through its
 * three ELEMENT strides (NCHW-contiguous: pixels * channels, pixels, 1; channels-last: pixels * channels, 1, channels), every
 * value widened exactly.  One thread owns one 16-byte channel vector position of the frame in all T frames, so the shift needs
 * no second buffer and no order between workgroups; src must not overlap a window.
 * STP3_EINVAL: B, T, N, pixels or channels < 1, a null pointer, a negative stride;  STP3_EUNSUP: channels % 4 != 0, a window
 * that is not 16-byte aligned or holds 2^32 bytes or more, another dtype, more than STP3_WINDOW_JOBS_MAX jobs. */
#define STP3_WINDOW_JOBS_MAX 4
typedef struct stp3_window_job {
    const void* src;            /* device: the newest frame, [B * N][channels][pixels] through the strides below */
    float* window;              /* device: [B][T][N * pixels][channels] float32 */
    int64_t stride_image, stride_channel, stride_pixel;     /* of src, in elements */
    int32_t channels;
    int32_t dtype;              /* STP3_DTYPE_* of src */
} stp3_window_job;
int stp3_window_push(int32_t B, int32_t T, int32_t N, int32_t pixels, int32_t n_jobs, const stp3_window_job* jobs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth labels from LiDAR points (csrc/stp3_depth.hip): batch['depths'] of LIFT.GT_DEPTH.
 *
 * What is restated (the header of csrc/stp3_depth.hip gives the arithmetic):
 *   (a) projection: NuScenesExplorer.map_pointcloud_to_image of the nuScenes devkit -- third-party, restated from its
 *       published source, PARITY UNPINNED;
 *   (b) scatter, last point wins: stp3/datas/NuscenesData.py:291-293;
 *   (c) bilinear resample (align_corners=False) of the whole map, crop, round half to even: :294-299 and :261-266;
 *   (d) class ids: stp3/trainer.py:269-276.
 * Inputs of a batch of F frames x N cameras:
 *   points      [n_total][3] float32, the sweeps of all frames one after the other
 *   offsets     [F + 1] int32 ON THE DEVICE, ascending inside [0, n_total]: frame f owns points [offsets[f], offsets[f+1]);
 *               a frame whose pair is not ordered inside that range is treated as empty (checked on the device)
 *   steps       [F][N][4][12] float64: per rigid step the rotation (row-major) and the translation
 *   before      bit s set: step s translates before it rotates (the devkit: 0b1100)
 *   intrinsics  [F][N][3][3] float64
 * Geometry of the resample (stp3_depth_axis per image axis; configuration-only, built on the host as ATen builds its
 * indices and weights -- stp3_amd.datas.DepthLabeller): the source rows / columns that are taps of a kept output row /
 * column are numbered in ascending order ("slots");
 *   tap      [n_out][2] int32   slots of i0 and i1 of every output index
 *   weight   [n_out][2] float64 1 - lambda, lambda (for float32 maps: the float32 values, held in doubles)
 *   slot_src [n_slot] int32     source index of a slot;   src_slot [n_src] int32  slot of a source index or -1
 * An output map is [F][N][y.n_out][x.n_out]; out_kind chooses float32 / float64 values (integers, exact in both) or int64
 * class ids  (int64)(min(max(v, d_lo), d_hi) - d_lo)  in float32 (the tables then describe the label rows and columns).
 *
 * stp3_depth_project            (a): pixels [n_total][N][2] int32 (u, v truncated; 0 where not kept), depth [n_total][N]
 *                               float64 (the float32 z), keep [n_total][N] uint8
 * stp3_depth_from_pixels        (b) + (c) on given pixels / depth / keep (the pinned entry)
 * stp3_depth_from_lidar         (a) - (c) [- (d)]: winners by integer atomic max into the workspace
 *                               (stp3_depth_workspace_bytes: the winner table, zeroed by the call, and 4 bytes per point
 *                               and camera for the depths of the pairs that reached it)
 * stp3_depth_labels_from_lidar  (a) - (d) in ONE launch without global scratch: a workgroup per image and band of label rows,
 *                               winner table in LDS.  bands: at least that many bands (0: as few as fit);
 *                               stp3_depth_labels_bands tells how many are used, STP3_EUNSUP if one label row's slots exceed LDS
 * stp3_depth_from_maps          (c) [- (d)] of stored dense maps [F][N][y.n_src][x.n_src], float64 or float32 (map_dtype:
 *                               STP3_DEPTH_OUT_F32 | _F64), arithmetic in the map's dtype
 * All entries only enqueue on `stream`, allocate nothing and are deterministic (no floating-point atomics). */
#define STP3_DEPTH_OUT_F32 0
#define STP3_DEPTH_OUT_F64 1
#define STP3_DEPTH_OUT_LABELS 2

typedef struct stp3_depth_axis {
    const int32_t* tap;
    const double* weight;
    const int32_t* slot_src;
    const int32_t* src_slot;
    int32_t n_out, n_slot, n_src, reserved;
} stp3_depth_axis;

typedef struct stp3_depth_dims {
    int32_t F, N, n_total, out_kind;
    float d_lo, d_hi;
    stp3_depth_axis y, x;
} stp3_depth_dims;

int stp3_depth_project(int32_t F, int32_t N, int32_t n_total, int32_t H, int32_t W, const float* points,
                       const int32_t* offsets, const double* steps, int32_t before, const double* intrinsics,
                       int32_t* pixels, double* depth, uint8_t* keep, void* stream);
int stp3_depth_workspace_bytes(const stp3_depth_dims* dims, size_t* bytes);
int stp3_depth_from_pixels(const stp3_depth_dims* dims, const int32_t* pixels, const double* depth, const uint8_t* keep,
                           const int32_t* offsets, void* workspace, size_t workspace_bytes, void* out, void* stream);
int stp3_depth_from_lidar(const stp3_depth_dims* dims, const float* points, const int32_t* offsets, const double* steps,
                          int32_t before, const double* intrinsics, void* workspace, size_t workspace_bytes, void* out,
                          void* stream);
int stp3_depth_labels_bands(const stp3_depth_dims* dims, int32_t bands, int32_t* used);
int stp3_depth_labels_from_lidar(const stp3_depth_dims* dims, const float* points, const int32_t* offsets,
                                 const double* steps, int32_t before, const double* intrinsics, int32_t bands,
                                 int64_t* labels, void* stream);
int stp3_depth_from_maps(const stp3_depth_dims* dims, const void* maps, int32_t map_dtype, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth labels under the per-image augmentation of the camera images (csrc/stp3_depth_augment.hip): batch['depths'] for the
 * parameter sets of stp3_image_augment -- a resize, crop, flip and in-plane rotation PER IMAGE.  The composition is this
 * project's (the reference never combines img_transform with its depth branch); every step is the reference's statement:
 *   (a), (b) projection and scatter as stp3_depth_from_lidar (stp3/datas/NuscenesData.py:291-293), LiDAR route only;
 *   (c) F.interpolate over the whole map in the map's dtype, per image: :295 (recompute_scale_factor=True: taps from
 *       n_src / n_out) for the LiDAR route, :262 (taps from 1 / resize) for stored maps; torch.round, :299 / :266;
 *   (e) stp3/utils/tools.py:127-130 on the rounded map: .crop (zero fill outside the resized map, negative origins allowed),
 *       .transpose(FLIP_LEFT_RIGHT), .rotate (NEAREST, no expand, zero fill, Pillow's six 16.16 fixed-point integers);
 *   (d) class ids of window rows and columns 0, stride, 2 stride, ...: stp3/trainer.py:269-276.
 * Every per-image quantity is read from device memory (nothing per image is a launch argument), so a captured call replays
 * with rewritten tables.  Per axis the host lists, image after image, one ENTRY per window row / column in the order the
 * rotation addresses them (columns after the flip); entry k of an image stands for window coordinate k (separable = 0) or
 * k stride (separable = 1: no image rotates, so only the label rows and columns are listed):
 *   tap      [entries][2] int32    the image's slots of i0 and i1, -1 where the row / column lies outside the resized map
 *   weight   [entries][2] float64  1 - lambda, lambda (for float32 maps: the float32 values, held in doubles)
 *   slot_src [slots] int32         per image an ASCENDING list of the source indices that are taps
 *   records  [F N][16] int32       0-5 the rotation's integers a0 .. a5 (source of window pixel (x, y):
 *                                  ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16)); 6, 7 first entry of the image's rows /
 *                                  columns; 8, 9 first element of its slot lists (y, x); 10, 11 their lengths; 12-15 zero
 * n = Ho (Wo), or ceil(Ho / stride) (ceil(Wo / stride)) when separable, entries of an image per axis; its winner table is
 * 2 n_y x 2 n_x words whatever its lists hold.  A record or a table entry that points outside its arrays makes the image's
 * pixels zero and its points skipped (checked on the device); it never reaches memory outside the buffers.
 * Output [F][N][ceil(Ho / stride)][ceil(Wo / stride)] of out_kind (STP3_DEPTH_OUT_*); stride > 1 samples the window.
 *
 * stp3_augment_depth_from_lidar  (a) - (e) [- (d)]: clear, scatter (slot of a pixel by binary search in the image's lists,
 *                                integer atomic max), output.  Workspace (stp3_augment_depth_workspace_bytes): the winner
 *                                tables and 4 bytes per point and camera.
 * stp3_augment_depth_from_maps   (c) - (e) [- (d)] of stored dense maps [F][N][H][W], float64 or float32 (map_dtype:
 *                                STP3_DEPTH_OUT_F32 | _F64), arithmetic in the map's dtype: one kernel
 * Both only enqueue kernels on `stream`, allocate nothing and are deterministic (no floating-point atomics). */
typedef struct stp3_augment_depth_axis {
    const int32_t* tap;
    const double* weight;
    const int32_t* slot_src;
    int32_t entries, slots;              /* room of tap / weight (in entries) and of slot_src */
} stp3_augment_depth_axis;

typedef struct stp3_augment_depth_dims {
    int32_t F, N, n_total, out_kind;
    float d_lo, d_hi;
    int32_t H, W;                        /* source map */
    int32_t Ho, Wo;                      /* crop window: at most 8192 a side (Pillow's rotation) */
    int32_t stride, separable;
    const int32_t* records;
    stp3_augment_depth_axis y, x;
} stp3_augment_depth_dims;

int stp3_augment_depth_workspace_bytes(const stp3_augment_depth_dims* dims, size_t* bytes);
int stp3_augment_depth_from_lidar(const stp3_augment_depth_dims* dims, const float* points, const int32_t* offsets,
                                  const double* steps, int32_t before, const double* intrinsics, void* workspace,
                                  size_t workspace_bytes, void* out, void* stream);
int stp3_augment_depth_from_maps(const stp3_augment_depth_dims* dims, const void* maps, int32_t map_dtype, void* out,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * The training video (csrc/stp3_vis.hip): stp3/utils/visualisation.py:208-322 (visualise_output) of ONE sample, painted on the
 * device.  video [T][3][7 H][2 W] uint8, planar; rows of panels top to bottom: instance, future flow, segmentation,
 * centerness, offset, pedestrian, planning; left column labels, right column predictions.  Every panel shows cell
 * (H - 1 - r, W - 1 - c) at its pixel (r, c) and, when enabled, carries a one-pixel black border; a disabled panel is zero.
 * The arithmetic of every panel is stated in the header of csrc/stp3_vis.hip; the planning panel is this project's own
 * (DESIGN.md section 4.15), everything else is the reference's byte for byte up to the rounding of atan2.
 *
 * A source (stp3_vis_map) is the map of frame 0 of the sample with strides in ELEMENTS: frames, channels, rows, columns.
 * [0] of every pair belongs to the labels, [1] to the predictions.
 *   seg, ped      labels: int64 (1 is the class that is drawn); predictions: float32 | bf16 logits of 2 channels, class 1 where
 *                 logit[1] > logit[0]
 *   inst          int64 instance ids (labels; the consistent ids of the instance post-processing)
 *   center        float32 | bf16, 1 channel;   offset, flow: float32 | bf16, 2 channels
 *   plan          hdmap: labels int64 values of 2 channels, predictions float32 | bf16 logits of 4 channels (two pairs);
 *                 traj: n_points float32 (x, y) in metres
 *   ego_cells     [n_ego][2] int32 (row, column) of the ego box;   dx / bx: resolution and first cell centre of rows and columns
 *   palette [70][3], jet [256][3], wheel [55][3]: uint8 colour tables (stp3_amd/visualisation.py owns them)
 * stp3_vis_render enqueues two kernels on `stream` -- one that copies the descriptor into `workspace` (stp3_vis_workspace_bytes,
 * 8-byte aligned) and, with STP3_VIS_INSTANCE, computes the per-frame scalars there (min / max of the two centre maps, smallest
 * id of the two instance maps: one workgroup per scalar pair), then the painter -- allocates nothing, does not synchronise and is
 * deterministic (no floating-point atomics).
 * STP3_EINVAL: null descriptor / video / workspace / required source, T < 1, H or W < 3, unknown dtype, n_points or n_ego < 0;
 * STP3_EUNSUP: 2 W * 7 H * 3 * T >= 2^31 or 7 T > 65535. */
#define STP3_VIS_DTYPE_I64 2            /* beside STP3_DTYPE_F32 / STP3_DTYPE_BF16 */
#define STP3_VIS_INSTANCE     1        /* instance, centerness and offset rows */
#define STP3_VIS_FLOW         2
#define STP3_VIS_PEDESTRIAN   4
#define STP3_VIS_PLAN_LABELS  8
#define STP3_VIS_PLAN_PRED   16

typedef struct stp3_vis_map {
    const void* ptr;
    int64_t stride_t, stride_c, stride_h, stride_w;
    int32_t dtype, reserved;
} stp3_vis_map;

typedef struct stp3_vis_plan {
    const void* hdmap;
    int64_t hd_stride_c, hd_stride_h, hd_stride_w;
    const float* traj;
    int64_t traj_stride_p, traj_stride_c;
    int32_t hd_dtype, n_points;
} stp3_vis_plan;

typedef struct stp3_vis_desc {
    int32_t T, H, W, panels;
    stp3_vis_map seg[2], ped[2], inst[2], center[2], offset[2], flow[2];
    stp3_vis_plan plan[2];
    const int32_t* ego_cells;
    const uint8_t* palette;
    const uint8_t* jet;
    const uint8_t* wheel;
    int32_t n_ego;
    float dx0, dx1, bx0, bx1;
    int32_t reserved;
} stp3_vis_desc;

int stp3_vis_workspace_bytes(const stp3_vis_desc* desc, size_t* bytes);
int stp3_vis_render(const stp3_vis_desc* desc, uint8_t* video, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CARLA: recorded samples and simulator ticks from decoded bytes to tensors (csrc/stp3_carla.hip; stp3_amd.carla.CarlaDecoder).
 * One launch per call for all n images; every entry is re-entrant, only enqueues on `stream`, allocates nothing and does not
 * synchronise (it can be captured into a graph).  "The window" of an H x W image and a side c <= min(H, W) is rows
 * H / 2 - c / 2 .. + c and columns W / 2 - c / 2 .. + c (integer divisions): scale_and_crop_image at scale 1,
 * stp3/datas/CarlaData.py:454-464.
 *
 * stp3_carla_frames   camera images: scale_and_crop_image(..., scale=1, crop) + normalise_image, CarlaData.py:377-384,454-464 and
 *                     carla_agent.py:326-329,370-426.  frames [n][Hs][Ws][Cs] uint8, Cs = 3 | 4; bgr = 1 reverses the first three
 *                     channels (cv2.cvtColor(x[:, :, :3], COLOR_BGR2RGB)); a fourth channel is ignored.  out [n][3][crop][crop]
 *                     STP3_DTYPE_F32: (float32(x) / 255 - mean[ch]) / std[ch], two true divisions, bit-equal to the torch
 *                     statements; STP3_DTYPE_BF16: their rounding to nearest even.
 * stp3_carla_depth    the 24-bit depth images: get_depth on the window, CarlaData.py:345-353,387-396.  frames [n][Hs][Ws][3] uint8
 *                     (R, G, B); v = double(R 65536 + G 256 + B) / 16777215.0 * 1000.0 in float64, in that order.  out_kind
 *                     STP3_DEPTH_OUT_F64 / _F32: the metre map [n][crop][crop] (float32: the rounding of v); STP3_DEPTH_OUT_LABELS:
 *                     the class ids of stp3/trainer.py:269-276, [n][ceil(crop / downsample)]^2 int64 =
 *                     (int64)(min(max(v, d_lo), d_hi) - d_lo) in float64 at every downsample-th row and column of the window
 *                     (d_hi: D_BOUND[1] - 1); only those pixels are decoded.
 * stp3_carla_hdmap    get_hdmap at scale 1, CarlaData.py:240-260.  frames [n][Hm][Wm][3] uint8; out [n][2][crop][crop]: channel 0
 *                     lane = pixel == (255, 0, 255), channel 1 drivable = pixel == (54, 52, 46) | lane, both flipped along both
 *                     axes.
 * stp3_carla_topdown  get_labels, CarlaData.py:262-280.  frames [n][Ht][Wt] uint8 class ids; Pillow's NEAREST resize to Hr x Wr
 *                     enters as row_src [Hr] / col_src [Wr] int32 ON THE DEVICE (source row / column of every resized row /
 *                     column; an entry outside the source is clamped); the window is taken of the resized image.  vehicle,
 *                     pedestrian [n][1][crop][crop]: pixel == 10 with window rows 89..111 x columns 96..104 (the ego vehicle)
 *                     cleared, pixel == 4; both flipped along both axes.
 * Maps (hdmap, topdown) are written as 0 / 1 in float32, float64 or int64 (STP3_CARLA_OUT_*).
 * STP3_EINVAL: a null pointer, n or a size < 1, a window larger than its image, Cs not 3 | 4, an unknown out_kind, labels with
 * downsample < 1 or d_lo > d_hi;  STP3_EUNSUP: n > 65 535, crop > 32 768, an image of 2^31 pixels, another out_dtype. */
#define STP3_CARLA_OUT_F32 0
#define STP3_CARLA_OUT_F64 1
#define STP3_CARLA_OUT_I64 2

int stp3_carla_frames(int32_t n, int32_t Hs, int32_t Ws, int32_t Cs, int32_t crop, int32_t bgr, const float* mean,
                      const float* std, int32_t out_dtype, const uint8_t* frames, void* out, void* stream);
int stp3_carla_depth(int32_t n, int32_t Hs, int32_t Ws, int32_t crop, int32_t out_kind, int32_t downsample, double d_lo,
                     double d_hi, const uint8_t* frames, void* out, void* stream);
int stp3_carla_hdmap(int32_t n, int32_t Hm, int32_t Wm, int32_t crop, int32_t out_kind, const uint8_t* frames, void* out,
                     void* stream);
int stp3_carla_topdown(int32_t n, int32_t Ht, int32_t Wt, int32_t Hr, int32_t Wr, int32_t crop, const int32_t* row_src,
                       const int32_t* col_src, int32_t out_kind, const uint8_t* frames, void* vehicle, void* pedestrian,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG scanlines (csrc/stp3_png.hip; stp3_amd.datas.PngDecoder): the Image.open(...) in front of every entry above --
 * get_hdmap / get_labels, stp3/datas/CarlaData.py:240-266, and the camera and depth files of __getitem__, :377-397 -- split
 * where a PNG decode is serial.  The HOST parses the chunks and inflates the IDAT data (Python: struct + zlib, no C of this
 * library); undoing the per-scanline filters runs in ONE kernel for all n images of a geometry, byte for byte what Pillow
 * (or any conforming decoder) returns.  Restated from the PNG specification, section 9 (filter types 0 .. 4).
 *
 * stp3_png_unfilter   rows [n][height][1 + width * bpp] uint8 IN DEVICE MEMORY, as inflate wrote them: per scanline one filter
 *                     byte, then the filtered bytes, no padding (scanlines therefore start at any alignment).  bpp = bytes per
 *                     pixel, 1 .. 4 (8-bit grey or palette index, grey + alpha, RGB, RGBA).  out [n][height][width * bpp] uint8,
 *                     contiguous.  Per byte, with a = the reconstructed byte bpp to the left (0 for x < bpp), b = the byte above
 *                     (0 in row 0), c = the byte above-left (0 in row 0 or for x < bpp), all sums modulo 256: 0 None adds 0,
 *                     1 Sub adds a, 2 Up adds b, 3 Average adds (a + b) >> 1 of the 9-bit sum, 4 Paeth adds a if
 *                     |p - a| <= |p - b| and |p - a| <= |p - c| for p = a + b - c, else b if |p - b| <= |p - c|, else c.
 *                     The kernel is TOTAL: a filter byte above 4 (the host refuses such a stream before it gets here) adds 0,
 *                     and no input byte enters an address.  One workgroup of up to 8 waves per image; a wave owns a band of
 *                     64 rows, lane l at pixel s - l in step s, each wave 80 steps behind the wave of the band above; the
 *                     last row of a band reaches the next wave through a ring in LDS, the last row of 512 rows waits in
 *                     LDS (4 bytes per pixel) for the next pass.  Waves meet at __syncthreads only, nothing spins.  Width
 *                     and height limit: 16 384 (the carry row is 64 KB of LDS there, 104 KB in all for an RGBA image of
 *                     449 rows or more; the limit of dynamic LDS is raised once per device to that, so calls from several
 *                     host threads do not disturb each other); there is no narrower limit of the design.
 * Re-entrant, only enqueues on `stream`, allocates nothing, reads nothing from the host and does not synchronise: it can be
 * captured, and a replay after both buffers were rewritten decodes the new images.
 * STP3_EINVAL: a null pointer, n or a size < 1, bpp outside 1 .. 4;  STP3_EUNSUP: a side above 16 384 (any n is taken: one
 * workgroup per image). */
int stp3_png_unfilter(const uint8_t* rows, int32_t n, int32_t height, int32_t width, int32_t bpp, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STP3_HIP_H */
