// stp3_depth.hip -- depth labels from LiDAR points (LIFT.GT_DEPTH): the loader-side producer of batch['depths'] for gfx950.
//
// Replaces, behind stp3_depth_*, what the reference's loader computes per camera and frame on the host:
//   (a) NuScenesExplorer.map_pointcloud_to_image of the nuScenes devkit (third-party, not vendored under the reference):
//       the float32 sweep through four rigid steps -- sensor -> ego at the sweep time, ego -> global, global -> ego at the
//       image time, ego -> camera --, each a LidarPointCloud.rotate / .translate pair applied to the float32 array in place,
//       depth = z, view_points(..., normalize=True) with the 3 x 3 intrinsics, keep = depth > 1, 1 < u < W - 1,
//       1 < v < H - 1.  Restated from the devkit's published source, PARITY UNPINNED.  This project's definition of the
//       arithmetic: every rotate component is ((r0 x) + (r1 y)) + (r2 z) in float64, every translate component x + t in
//       float64, each stored back to float32; the projection ((k0 x) + (k1 y)) + (k2 z) per row in float64 and the two
//       quotients by the third row (z for a pinhole matrix).  The library is built with -ffp-contract=off, so these are the
//       roundings of the elementwise torch statements of stp3_amd.datas.DepthLabeller.reference_project, bit for bit.
//   (b) stp3/datas/NuscenesData.py:291-293 (get_depth_from_lidar): pixel = (u, v) truncated toward zero, map[v, u] = depth
//       into a zeroed ORIGINAL_HEIGHT x ORIGINAL_WIDTH float64 image; where several points hit a pixel the LAST in point
//       order wins (numpy's assignment rule).  Here: the winner is an integer -- the highest point index of the frame + 1, by
//       an integer atomic max (global memory or LDS) -- so the result does not depend on scheduling; there is no
//       floating-point atomic in this file.
//   (c) :294-299 and :261-266 (get_input_data, stored maps): F.interpolate(scale_factor=RESIZE_SCALE, mode='bilinear',
//       align_corners=False) over the whole map in the map's dtype, the crop [top:bottom, left:right], torch.round (half to
//       even).  Taps and weights per output row / column are configuration-only: the host builds them as ATen does
//       (source = max(0, (1 / s) (o + 0.5) - 0.5), i0 = trunc, i1 = min(i0 + 1, n - 1), weights 1 - lambda, lambda) and the
//       kernels evaluate  hy0 (wx0 A + wx1 B) + hy1 (wx0 C + wx1 D)  without contraction.  The rounded map is what is pinned.
//   (d) stp3/trainer.py:269-276: every DOWNSAMPLE-th row and column, clamp(D_BOUND[0], D_BOUND[1] - 1) - D_BOUND[0], int64:
//       the same kernels on the tables of those rows and columns, the clamp in float32 as torch applies it to the float32 map.
//
// The full-resolution image is never built.  Only source pixels that are taps of kept output pixels can matter: the host
// numbers those source rows and columns ("slots", ascending) and the winner table is n_slot_y x n_slot_x words per image.
//   full map:     depth_clear_kernel, depth_scatter_kernel (one thread per point and camera: project, slot look-up, atomic max
//                 into the table in the workspace, the float32 depth of a pair that reached the table beside it: 4 bytes per
//                 point and camera) then depth_resample_kernel (one thread per output pixel: four winners and their depths)
//   labels only:  depth_labels_kernel, ONE launch, no global scratch: a workgroup per image and band of label rows keeps the
//                 band's winner table in LDS (28 x 60 labels: 56 x 120 words), walks the frame's points, then writes the
//                 class ids of its rows
//   stored maps:  depth_resample_kernel reading the dense map at the slots' source rows and columns.
// Device-side guards make every index that comes from a table or from `offsets` safe (a frame whose offsets are not
// monotone inside [0, n_total] is treated as empty; a slot or source index outside its range is skipped).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stp3_hip.h"

#include "stp3_depth_point.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLabelThreads = 1024;          // one workgroup per image and band: 4 waves per SIMD walk the frame's points
constexpr size_t kLdsLimit = 64 * 1024;      // dynamic LDS without an attribute

struct Axis {
    const int* tap;                          // [n_out][2]
    const double* weight;                    // [n_out][2]
    const int* slot_src;                     // [n_slot]
    const int* src_slot;                     // [n_src]
    int n_out, n_slot, n_src;
};

struct Geo {
    Axis y, x;
    int F, N, n_total, out_kind;
    float d_lo, d_hi;
};

__global__ __launch_bounds__(kThreads) void depth_project_kernel(Cloud c, int F, int N, int n_total, int H, int W,
                                                                 int* __restrict__ pixels, double* __restrict__ depth,
                                                                 uint8_t* __restrict__ keep) {
    const int p = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;      // one camera per workgroup: its steps are uniform
    if (p >= n_total) return;
    const int64_t gid = (int64_t)p * N + n;
    const int f = frame_of(c.offsets, F, n_total, p);
    Hit h;
    h.px = h.py = 0; h.depth = 0.f; h.keep = false;
    if (f >= 0) {
        const size_t cam = (size_t)f * N + n;
        h = project_point(c.points + 3 * (size_t)p, c.steps + cam * 48, c.before, c.intrinsics + cam * 9, H, W);
    }
    pixels[2 * gid] = h.px;
    pixels[2 * gid + 1] = h.py;
    depth[gid] = (double)h.depth;
    keep[gid] = h.keep ? 1 : 0;
}

// slot of a kept pixel in the winner table of its image, or -1
__device__ __forceinline__ bool slots_of(const Geo& g, int px, int py, int& sy, int& sx) {
    if ((unsigned)px >= (unsigned)g.x.n_src || (unsigned)py >= (unsigned)g.y.n_src) return false;
    sx = g.x.src_slot[px];
    sy = g.y.src_slot[py];
    return (unsigned)sx < (unsigned)g.x.n_slot && (unsigned)sy < (unsigned)g.y.n_slot;
}

template <bool kPixels>
__global__ __launch_bounds__(kThreads) void depth_scatter_kernel(Geo g, Cloud c, const int* __restrict__ pixels,
                                                                 const uint8_t* __restrict__ keep, int* __restrict__ win,
                                                                 float* __restrict__ zbuf) {
    const int p = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;
    if (p >= g.n_total) return;
    const int f = frame_of(c.offsets, g.F, g.n_total, p);
    if (f < 0) return;
    const size_t cam = (size_t)f * g.N + n;
    int px, py;
    float z = 0.f;
    const size_t e = (size_t)p * g.N + n;
    if (kPixels) {
        if (!keep[e]) return;
        px = pixels[2 * e];
        py = pixels[2 * e + 1];
    } else {
        const Hit h = project_point(c.points + 3 * (size_t)p, c.steps + cam * 48, c.before, c.intrinsics + cam * 9,
                                    g.y.n_src, g.x.n_src);
        if (!h.keep) return;
        px = h.px;
        py = h.py;
        z = h.depth;
    }
    int sy, sx;
    if (!slots_of(g, px, py, sy, sx)) return;
    atomicMax(&win[(cam * g.y.n_slot + sy) * g.x.n_slot + sx], p - c.offsets[f] + 1);
    if (!kPixels) zbuf[e] = z;                       // read back for winners only: every winner has written its entry
}

// zeroes the winner table (a kernel of the stream like the two around it, so that a captured call is a plain chain of kernels)
__global__ __launch_bounds__(kThreads) void depth_clear_kernel(int* __restrict__ win, size_t words) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += stride) win[i] = 0;
}

enum { kSrcPixels = 0, kSrcLidar = 1, kSrcMapF64 = 2, kSrcMapF32 = 3 };

struct Taps {
    int sy0, sy1, sx0, sx1;
    double hy0, hy1, wx0, wx1;
    bool ok;
};

__device__ __forceinline__ Taps taps_of(const Geo& g, int oy, int ox) {
    Taps t;
    t.sy0 = g.y.tap[2 * oy]; t.sy1 = g.y.tap[2 * oy + 1];
    t.sx0 = g.x.tap[2 * ox]; t.sx1 = g.x.tap[2 * ox + 1];
    t.hy0 = g.y.weight[2 * oy]; t.hy1 = g.y.weight[2 * oy + 1];
    t.wx0 = g.x.weight[2 * ox]; t.wx1 = g.x.weight[2 * ox + 1];
    t.ok = (unsigned)t.sy0 < (unsigned)g.y.n_slot && (unsigned)t.sy1 < (unsigned)g.y.n_slot &&
           (unsigned)t.sx0 < (unsigned)g.x.n_slot && (unsigned)t.sx1 < (unsigned)g.x.n_slot;
    return t;
}

// the depth a winner word stands for: 0 for an empty pixel, else the z of that point of the frame in this camera
__device__ __forceinline__ double winner_depth(const Geo& g, const Cloud& c, int w, int start, size_t cam) {
    if (w <= 0) return 0.0;
    const int64_t p = (int64_t)start + w - 1;
    if (p < 0 || p >= g.n_total) return 0.0;
    return (double)transform_point(c.points + 3 * (size_t)p, c.steps + cam * 48, c.before).z;
}

template <typename T>
__device__ __forceinline__ T blend(const Taps& t, T a, T b, T cc, T d) {
    const T hy0 = (T)t.hy0, hy1 = (T)t.hy1, wx0 = (T)t.wx0, wx1 = (T)t.wx1;
    return hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * cc + wx1 * d);
}

__device__ __forceinline__ double round_even(double v) { return rint(v); }
__device__ __forceinline__ float round_even(float v) { return rintf(v); }

__device__ __forceinline__ int64_t class_id(const Geo& g, float x) {
    x = fminf(fmaxf(x, g.d_lo), g.d_hi) - g.d_lo;          // torch.clamp(depth, D0, D1 - 1) - D0 on the float32 map
    return (int64_t)x;
}

__device__ __forceinline__ void store_value(const Geo& g, void* __restrict__ out, int64_t idx, double v) {
    if (g.out_kind == STP3_DEPTH_OUT_F32) ((float*)out)[idx] = (float)v;
    else if (g.out_kind == STP3_DEPTH_OUT_F64) ((double*)out)[idx] = v;
    else ((int64_t*)out)[idx] = class_id(g, (float)v);
}

template <int kSrc>
__global__ __launch_bounds__(kThreads) void depth_resample_kernel(Geo g, Cloud c, const double* __restrict__ depth,
                                                                  const float* __restrict__ zbuf,
                                                                  const int* __restrict__ win, const void* __restrict__ maps,
                                                                  void* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t per_image = (int64_t)g.y.n_out * g.x.n_out;
    if (idx >= per_image * g.F * g.N) return;
    const int ox = (int)(idx % g.x.n_out), oy = (int)((idx / g.x.n_out) % g.y.n_out);
    const size_t cam = (size_t)(idx / per_image);
    const Taps t = taps_of(g, oy, ox);
    double v = 0.0;
    if (t.ok) {
        if (kSrc == kSrcPixels || kSrc == kSrcLidar) {
            const int f = (int)(cam / g.N), n = (int)(cam % g.N);
            const int start = c.offsets[f];
            const int* w = win + cam * g.y.n_slot * g.x.n_slot;
            const int sy[2] = {t.sy0, t.sy1}, sx[2] = {t.sx0, t.sx1};
            double tap[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int word = w[(size_t)sy[i >> 1] * g.x.n_slot + sx[i & 1]];
                const int64_t p = (int64_t)start + word - 1;
                const bool hit = word > 0 && p >= 0 && p < g.n_total;
                if (kSrc == kSrcLidar) tap[i] = hit ? (double)zbuf[(size_t)p * g.N + n] : 0.0;
                else tap[i] = hit ? depth[(size_t)p * g.N + n] : 0.0;
            }
            v = round_even(blend<double>(t, tap[0], tap[1], tap[2], tap[3]));
        } else {
            const int y0 = g.y.slot_src[t.sy0], y1 = g.y.slot_src[t.sy1], x0 = g.x.slot_src[t.sx0], x1 = g.x.slot_src[t.sx1];
            if ((unsigned)y0 < (unsigned)g.y.n_src && (unsigned)y1 < (unsigned)g.y.n_src && (unsigned)x0 < (unsigned)g.x.n_src &&
                (unsigned)x1 < (unsigned)g.x.n_src) {
                const size_t base = cam * g.y.n_src * g.x.n_src, r0 = base + (size_t)y0 * g.x.n_src, r1 = base + (size_t)y1 * g.x.n_src;
                if (kSrc == kSrcMapF64) {
                    const double* m = (const double*)maps;
                    v = round_even(blend<double>(t, m[r0 + x0], m[r0 + x1], m[r1 + x0], m[r1 + x1]));
                } else {
                    const float* m = (const float*)maps;
                    v = (double)round_even(blend<float>(t, m[r0 + x0], m[r0 + x1], m[r1 + x0], m[r1 + x1]));
                }
            }
        }
    }
    store_value(g, out, idx, v);
}

// labels only, from the points, in one launch: grid (F N, bands); `rows` label rows per band
__global__ __launch_bounds__(kLabelThreads) void depth_labels_kernel(Geo g, Cloud c, int rows, int64_t* __restrict__ out) {
    extern __shared__ int win[];
    const int tid = threadIdx.x;
    const size_t cam = blockIdx.x;
    const int f = (int)(cam / g.N);
    const int r0 = blockIdx.y * rows, r1 = min(r0 + rows, g.y.n_out);
    if (r0 >= r1) return;
    // the band's slots: taps ascend with the output row
    const int lo = g.y.tap[2 * r0], hi = g.y.tap[2 * (r1 - 1) + 1] + 1;
    const int n_rows = hi - lo, nsx = g.x.n_slot;
    const bool sane = lo >= 0 && hi <= g.y.n_slot && n_rows >= 1 && n_rows <= 2 * rows;
    const int words = sane ? n_rows * nsx : 0;
    for (int i = tid; i < words; i += kLabelThreads) win[i] = 0;
    __syncthreads();
    int start = c.offsets[f], end = c.offsets[f + 1];
    if (start < 0 || end < start || end > g.n_total || !sane) start = end = 0;
    const double* st = c.steps + cam * 48;
    const double* k = c.intrinsics + cam * 9;
    for (int p = start + tid; p < end; p += kLabelThreads) {
        const Hit h = project_point(c.points + 3 * (size_t)p, st, c.before, k, g.y.n_src, g.x.n_src);
        if (!h.keep) continue;
        int sy, sx;
        if (!slots_of(g, h.px, h.py, sy, sx) || sy < lo || sy >= hi) continue;
        atomicMax(&win[(sy - lo) * nsx + sx], p - start + 1);
    }
    __syncthreads();
    const int wo = g.x.n_out;
    for (int o = tid; o < (r1 - r0) * wo; o += kLabelThreads) {
        const int oy = r0 + o / wo, ox = o % wo;
        const Taps t = taps_of(g, oy, ox);
        double v = 0.0;
        if (t.ok && sane && t.sy0 >= lo && t.sy1 < hi) {
            const int sy[2] = {t.sy0 - lo, t.sy1 - lo}, sx[2] = {t.sx0, t.sx1};
            double tap[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) tap[i] = winner_depth(g, c, win[sy[i >> 1] * nsx + sx[i & 1]], start, cam);
            v = round_even(blend<double>(t, tap[0], tap[1], tap[2], tap[3]));
        }
        out[(cam * g.y.n_out + oy) * wo + ox] = class_id(g, (float)v);
    }
}

bool axis_ok(const stp3_depth_axis& a) {
    return a.tap && a.weight && a.slot_src && a.src_slot && a.n_out >= 1 && a.n_slot >= 1 && a.n_src >= 1 &&
           a.n_slot <= 2 * (int64_t)a.n_out && a.n_slot <= a.n_src;
}

bool dims_ok(const stp3_depth_dims* d) {
    return d && d->F >= 1 && d->N >= 1 && d->n_total >= 0 && axis_ok(d->y) && axis_ok(d->x) &&
           (d->out_kind == STP3_DEPTH_OUT_F32 || d->out_kind == STP3_DEPTH_OUT_F64 || d->out_kind == STP3_DEPTH_OUT_LABELS) &&
           (int64_t)d->F * d->N * d->y.n_out * d->x.n_out < ((int64_t)1 << 31) * kThreads &&
           (int64_t)d->F * d->N <= 0x7fffffff && d->N <= 65535;
}

Axis axis_of(const stp3_depth_axis& a) {
    Axis o;
    o.tap = a.tap; o.weight = a.weight; o.slot_src = a.slot_src; o.src_slot = a.src_slot;
    o.n_out = a.n_out; o.n_slot = a.n_slot; o.n_src = a.n_src;
    return o;
}

Geo geo_of(const stp3_depth_dims* d) {
    Geo g;
    g.y = axis_of(d->y); g.x = axis_of(d->x);
    g.F = d->F; g.N = d->N; g.n_total = d->n_total; g.out_kind = d->out_kind;
    g.d_lo = d->d_lo; g.d_hi = d->d_hi;
    return g;
}

Cloud cloud_of(const float* points, const int32_t* offsets, const double* steps, int32_t before, const double* intrinsics) {
    Cloud c;
    c.points = points; c.offsets = offsets; c.steps = steps; c.intrinsics = intrinsics; c.before = before;
    return c;
}

size_t table_bytes(const stp3_depth_dims* d) {
    return (size_t)d->F * d->N * d->y.n_slot * d->x.n_slot * sizeof(int);
}

// the winner table, then the float32 depth of every (point, camera) that reached it
size_t workspace_bytes(const stp3_depth_dims* d) { return table_bytes(d) + (size_t)d->n_total * d->N * sizeof(float); }

int last_error() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

void clear_table(const stp3_depth_dims* d, void* workspace, void* stream) {
    const size_t words = table_bytes(d) / sizeof(int);
    const size_t blocks = (words + 4 * kThreads - 1) / (4 * kThreads);                 // four words a thread, at most 64k blocks
    hipLaunchKernelGGL(depth_clear_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kThreads), 0,
                       (hipStream_t)stream, (int*)workspace, words);
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// rows per band of the labels kernel: the fewest bands whose table fits in LDS, at least `bands`
int label_rows(const stp3_depth_dims* d, int bands) {
    const size_t row_bytes = 2 * (size_t)d->x.n_slot * sizeof(int);      // a label row has at most two slot rows
    if (row_bytes > kLdsLimit) return 0;
    const int fit = (int)(kLdsLimit / row_bytes);
    int rows = (d->y.n_out + (bands < 1 ? 1 : bands) - 1) / (bands < 1 ? 1 : bands);
    if (rows > fit) rows = fit;
    return rows < 1 ? 1 : rows;
}

}  // namespace

extern "C" {

int stp3_depth_project(int32_t F, int32_t N, int32_t n_total, int32_t H, int32_t W, const float* points,
                       const int32_t* offsets, const double* steps, int32_t before, const double* intrinsics,
                       int32_t* pixels, double* depth, uint8_t* keep, void* stream) {
    if (F < 1 || N < 1 || n_total < 0 || H < 3 || W < 3 || (before & ~15) || !offsets || !steps || !intrinsics ||
        (n_total > 0 && (!points || !pixels || !depth || !keep)) || N > 65535)
        return STP3_EINVAL;
    if (n_total == 0) return STP3_OK;
    hipLaunchKernelGGL(depth_project_kernel, dim3(blocks_for(n_total), N), dim3(kThreads), 0, (hipStream_t)stream,
                       cloud_of(points, offsets, steps, before, intrinsics), F, N, n_total, H, W, pixels, depth, keep);
    return last_error();
}

int stp3_depth_workspace_bytes(const stp3_depth_dims* dims, size_t* bytes) {
    if (!dims_ok(dims) || !bytes) return STP3_EINVAL;
    *bytes = workspace_bytes(dims);
    return STP3_OK;
}

int stp3_depth_from_pixels(const stp3_depth_dims* dims, const int32_t* pixels, const double* depth, const uint8_t* keep,
                           const int32_t* offsets, void* workspace, size_t workspace_bytes, void* out, void* stream) {
    if (!dims_ok(dims) || !offsets || !workspace || !out || (dims->n_total > 0 && (!pixels || !depth || !keep)))
        return STP3_EINVAL;
    if (workspace_bytes < ::workspace_bytes(dims)) return STP3_ENOSPACE;
    const Geo g = geo_of(dims);
    const Cloud c = cloud_of(nullptr, offsets, nullptr, 0, nullptr);
    clear_table(dims, workspace, stream);
    if (g.n_total > 0)
        hipLaunchKernelGGL(depth_scatter_kernel<true>, dim3(blocks_for(g.n_total), g.N), dim3(kThreads), 0, (hipStream_t)stream,
                           g, c, pixels, keep, (int*)workspace, (float*)nullptr);
    hipLaunchKernelGGL(depth_resample_kernel<kSrcPixels>, dim3(blocks_for((int64_t)g.F * g.N * g.y.n_out * g.x.n_out)),
                       dim3(kThreads), 0, (hipStream_t)stream, g, c, depth, (const float*)nullptr, (const int*)workspace,
                       (const void*)nullptr, out);
    return last_error();
}

int stp3_depth_from_lidar(const stp3_depth_dims* dims, const float* points, const int32_t* offsets, const double* steps,
                          int32_t before, const double* intrinsics, void* workspace, size_t workspace_bytes, void* out,
                          void* stream) {
    if (!dims_ok(dims) || (before & ~15) || !offsets || !steps || !intrinsics || !workspace || !out ||
        (dims->n_total > 0 && !points))
        return STP3_EINVAL;
    if (workspace_bytes < ::workspace_bytes(dims)) return STP3_ENOSPACE;
    const Geo g = geo_of(dims);
    const Cloud c = cloud_of(points, offsets, steps, before, intrinsics);
    float* zbuf = (float*)((char*)workspace + table_bytes(dims));
    clear_table(dims, workspace, stream);
    if (g.n_total > 0)
        hipLaunchKernelGGL(depth_scatter_kernel<false>, dim3(blocks_for(g.n_total), g.N), dim3(kThreads), 0, (hipStream_t)stream,
                           g, c, (const int*)nullptr, (const uint8_t*)nullptr, (int*)workspace, zbuf);
    hipLaunchKernelGGL(depth_resample_kernel<kSrcLidar>, dim3(blocks_for((int64_t)g.F * g.N * g.y.n_out * g.x.n_out)),
                       dim3(kThreads), 0, (hipStream_t)stream, g, c, (const double*)nullptr, (const float*)zbuf,
                       (const int*)workspace, (const void*)nullptr, out);
    return last_error();
}

int stp3_depth_labels_bands(const stp3_depth_dims* dims, int32_t bands, int32_t* used) {
    if (!dims_ok(dims) || !used || bands < 0) return STP3_EINVAL;
    const int rows = label_rows(dims, bands);
    if (rows == 0) return STP3_EUNSUP;
    *used = (dims->y.n_out + rows - 1) / rows;
    return STP3_OK;
}

int stp3_depth_labels_from_lidar(const stp3_depth_dims* dims, const float* points, const int32_t* offsets,
                                 const double* steps, int32_t before, const double* intrinsics, int32_t bands,
                                 int64_t* labels, void* stream) {
    if (!dims_ok(dims) || dims->out_kind != STP3_DEPTH_OUT_LABELS || (before & ~15) || bands < 0 || !offsets || !steps ||
        !intrinsics || !labels || (dims->n_total > 0 && !points))
        return STP3_EINVAL;
    const int rows = label_rows(dims, bands);
    if (rows == 0) return STP3_EUNSUP;
    const int used = (dims->y.n_out + rows - 1) / rows;
    if (used > 65535) return STP3_EUNSUP;
    const Geo g = geo_of(dims);
    hipLaunchKernelGGL(depth_labels_kernel, dim3((unsigned)(g.F * g.N), used), dim3(kLabelThreads),
                       2 * (size_t)rows * g.x.n_slot * sizeof(int), (hipStream_t)stream, g,
                       cloud_of(points, offsets, steps, before, intrinsics), rows, labels);
    return last_error();
}

int stp3_depth_from_maps(const stp3_depth_dims* dims, const void* maps, int32_t map_dtype, void* out, void* stream) {
    if (!dims_ok(dims) || !maps || !out || (map_dtype != STP3_DEPTH_OUT_F32 && map_dtype != STP3_DEPTH_OUT_F64))
        return STP3_EINVAL;
    const Geo g = geo_of(dims);
    const Cloud c = cloud_of(nullptr, nullptr, nullptr, 0, nullptr);
    const dim3 grid(blocks_for((int64_t)g.F * g.N * g.y.n_out * g.x.n_out));
    if (map_dtype == STP3_DEPTH_OUT_F64)
        hipLaunchKernelGGL(depth_resample_kernel<kSrcMapF64>, grid, dim3(kThreads), 0, (hipStream_t)stream, g, c,
                           (const double*)nullptr, (const float*)nullptr, (const int*)nullptr, maps, out);
    else
        hipLaunchKernelGGL(depth_resample_kernel<kSrcMapF32>, grid, dim3(kThreads), 0, (hipStream_t)stream, g, c,
                           (const double*)nullptr, (const float*)nullptr, (const int*)nullptr, maps, out);
    return last_error();
}

}  // extern "C"
