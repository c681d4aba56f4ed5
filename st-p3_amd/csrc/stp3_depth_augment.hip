// stp3_depth_augment.hip -- depth labels (LIFT.GT_DEPTH) under the per-image augmentation of the camera images, for gfx950:
// batch['depths'] for the parameter sets of stp3_image_augment, from the LiDAR sweep or from stored maps.
//
// The composition is this project's -- the reference never combines img_transform with its depth branch --, every step the
// reference's own statement (include/stp3_hip.h lists the lines):
//   scatter (last point of a source pixel wins: an integer, by integer atomic max; no floating-point atomic in this file)
//   -> F.interpolate(scale_factor=resize_i, 'bilinear') over the whole map in the map's dtype  -> torch.round
//   -> Image.crop(crop_i) with zero fill -> [FLIP_LEFT_RIGHT] -> Image.rotate(rotate_i) NEAREST  [-> class ids].
// torch.round commutes with the three gathers that follow it, so an output pixel is: its address carried back through the
// rotation's fixed-point integers into the window, the window row and column looked up in the image's tables (built on the
// host as ATen builds its indices and weights; the flip is the order of the column entries, the crop origin and the resized
// size decide which entries carry taps), then  rint(hy0 (wx0 A + wx1 B) + hy1 (wx0 C + wx1 D))  without contraction (the
// library is built with -ffp-contract=off) of the four winners' depths, or zero.
// As in stp3_depth.hip the full-resolution map is never built: only source pixels that are taps matter, the host numbers
// them per image and axis ("slots", ascending) and an image's winner table is 2 n_y x 2 n_x words.  A point finds the slot of
// its pixel by binary search in the image's two ascending lists (at most 2 n entries each, read from the image's record).
//   LiDAR:  depth_augment_clear_kernel, depth_augment_scatter_kernel (one thread per point and camera),
//           depth_augment_output_kernel<0> (one thread per output pixel or label)
//   maps:   depth_augment_output_kernel<1 | 2> reading the dense float64 | float32 map at the slots' source rows and columns.
// Everything per image comes from device memory, and every index derived from a record, a table entry or `offsets` is
// checked against the room the launch was given: an impossible value zeroes the image's pixels or skips the point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stp3_hip.h"

#include "stp3_depth_point.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 8192;               // Pillow accumulates the rotation's addresses in 32-bit integers
constexpr int kRecord = 16;                  // words of a record

struct Axis {
    const int* tap;                          // [entries][2]
    const double* weight;                    // [entries][2]
    const int* slot_src;                     // [slots]
    int n, entries, slots, n_src;            // n: entries of one image
};

struct Geo {
    Axis y, x;
    const int* records;                      // [F N][16]
    int F, N, n_total, out_kind;
    int Ho, Wo, stride, separable, out_h, out_w;
    float d_lo, d_hi;
};

// an image's record, checked: where its entries and its slot lists lie
struct Image {
    int tab_y, tab_x, slot_y, slot_x, nsy, nsx;
    bool ok;
};

__device__ __forceinline__ bool range_ok(int first, int count, int most, int room) {
    return first >= 0 && count >= 0 && count <= most && (int64_t)first + count <= (int64_t)room;
}

__device__ __forceinline__ Image image_of(const Geo& g, size_t img) {
    const int* r = g.records + kRecord * img;
    Image im;
    im.tab_y = r[6]; im.tab_x = r[7]; im.slot_y = r[8]; im.slot_x = r[9]; im.nsy = r[10]; im.nsx = r[11];
    im.ok = range_ok(im.tab_y, g.y.n, g.y.n, g.y.entries) && range_ok(im.tab_x, g.x.n, g.x.n, g.x.entries) &&
            range_ok(im.slot_y, im.nsy, 2 * g.y.n, g.y.slots) && range_ok(im.slot_x, im.nsx, 2 * g.x.n, g.x.slots);
    return im;
}

// index of `v` in the ascending list[0 .. n), or -1; reads inside the list whatever it holds
__device__ __forceinline__ int find_slot(const int* __restrict__ list, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && list[lo] == v) ? lo : -1;
}

__global__ __launch_bounds__(kThreads) void depth_augment_clear_kernel(int* __restrict__ win, size_t words) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += stride) win[i] = 0;
}

__global__ __launch_bounds__(kThreads) void depth_augment_scatter_kernel(Geo g, Cloud c, int* __restrict__ win,
                                                                         float* __restrict__ zbuf) {
    const int p = blockIdx.x * kThreads + threadIdx.x, n = blockIdx.y;      // one camera per workgroup: its steps are uniform
    if (p >= g.n_total) return;
    const int f = frame_of(c.offsets, g.F, g.n_total, p);
    if (f < 0) return;
    const size_t cam = (size_t)f * g.N + n;
    const Hit h = project_point(c.points + 3 * (size_t)p, c.steps + cam * 48, c.before, c.intrinsics + cam * 9, g.y.n_src,
                                g.x.n_src);
    if (!h.keep) return;
    const Image im = image_of(g, cam);
    if (!im.ok) return;
    const int sx = find_slot(g.x.slot_src + im.slot_x, im.nsx, h.px);
    if (sx < 0) return;
    const int sy = find_slot(g.y.slot_src + im.slot_y, im.nsy, h.py);
    if (sy < 0) return;
    atomicMax(&win[(cam * 2 * g.y.n + sy) * 2 * g.x.n + sx], p - c.offsets[f] + 1);
    zbuf[(size_t)p * g.N + n] = h.depth;              // read back for winners only: every winner has written its entry
}

enum { kSrcLidar = 0, kSrcMapF64 = 1, kSrcMapF32 = 2 };

template <typename T>
__device__ __forceinline__ T blend(double hy0, double hy1, double wx0, double wx1, T a, T b, T cc, T d) {
    return (T)hy0 * ((T)wx0 * a + (T)wx1 * b) + (T)hy1 * ((T)wx0 * cc + (T)wx1 * d);
}

__device__ __forceinline__ void store_value(const Geo& g, void* __restrict__ out, int64_t idx, double v) {
    if (g.out_kind == STP3_DEPTH_OUT_F32) ((float*)out)[idx] = (float)v;
    else if (g.out_kind == STP3_DEPTH_OUT_F64) ((double*)out)[idx] = v;
    else {
        const float x = fminf(fmaxf((float)v, g.d_lo), g.d_hi) - g.d_lo;   // torch.clamp(depth, D0, D1 - 1) - D0 on the float32 map
        ((int64_t*)out)[idx] = (int64_t)x;
    }
}

template <int kSrc>
__global__ __launch_bounds__(kThreads) void depth_augment_output_kernel(Geo g, Cloud c, const float* __restrict__ zbuf,
                                                                        const int* __restrict__ win,
                                                                        const void* __restrict__ maps, void* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t per_image = (int64_t)g.out_h * g.out_w;
    if (idx >= per_image * g.F * g.N) return;
    const int ox = (int)(idx % g.out_w), oy = (int)((idx / g.out_w) % g.out_h);
    const size_t cam = (size_t)(idx / per_image);
    const Image im = image_of(g, cam);
    // the entries of this pixel's window row and column
    int ky = oy, kx = ox;
    bool inside = im.ok;
    if (!g.separable) {
        const int* r = g.records + kRecord * cam;
        const int64_t x = (int64_t)ox * g.stride, y = (int64_t)oy * g.stride;
        const int64_t xin = ((int64_t)r[2] + x * r[0] + y * r[1]) >> 16, yin = ((int64_t)r[5] + x * r[3] + y * r[4]) >> 16;
        inside = inside && xin >= 0 && xin < g.Wo && yin >= 0 && yin < g.Ho;
        kx = (int)xin;
        ky = (int)yin;
    }
    double v = 0.0;
    if (inside) {
        const size_t ey = (size_t)im.tab_y + ky, ex = (size_t)im.tab_x + kx;          // inside the tables: image_of, k < n
        const int sy0 = g.y.tap[2 * ey], sy1 = g.y.tap[2 * ey + 1], sx0 = g.x.tap[2 * ex], sx1 = g.x.tap[2 * ex + 1];
        if ((unsigned)sy0 < (unsigned)im.nsy && (unsigned)sy1 < (unsigned)im.nsy && (unsigned)sx0 < (unsigned)im.nsx &&
            (unsigned)sx1 < (unsigned)im.nsx) {
            const double hy0 = g.y.weight[2 * ey], hy1 = g.y.weight[2 * ey + 1], wx0 = g.x.weight[2 * ex], wx1 = g.x.weight[2 * ex + 1];
            if (kSrc == kSrcLidar) {
                const int f = (int)(cam / g.N), n = (int)(cam % g.N);
                const int start = c.offsets[f];
                const size_t row = 2 * (size_t)g.x.n;
                const int* w = win + cam * 2 * g.y.n * row;
                const int word[4] = {w[sy0 * row + sx0], w[sy0 * row + sx1], w[sy1 * row + sx0], w[sy1 * row + sx1]};
                double tap[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t p = (int64_t)start + word[i] - 1;
                    tap[i] = (word[i] > 0 && p >= 0 && p < g.n_total) ? (double)zbuf[(size_t)p * g.N + n] : 0.0;
                }
                v = rint(blend<double>(hy0, hy1, wx0, wx1, tap[0], tap[1], tap[2], tap[3]));
            } else {
                const int y0 = g.y.slot_src[im.slot_y + sy0], y1 = g.y.slot_src[im.slot_y + sy1];
                const int x0 = g.x.slot_src[im.slot_x + sx0], x1 = g.x.slot_src[im.slot_x + sx1];
                if ((unsigned)y0 < (unsigned)g.y.n_src && (unsigned)y1 < (unsigned)g.y.n_src && (unsigned)x0 < (unsigned)g.x.n_src &&
                    (unsigned)x1 < (unsigned)g.x.n_src) {
                    const size_t base = cam * g.y.n_src * g.x.n_src, r0 = base + (size_t)y0 * g.x.n_src, r1 = base + (size_t)y1 * g.x.n_src;
                    if (kSrc == kSrcMapF64) {
                        const double* m = (const double*)maps;
                        v = rint(blend<double>(hy0, hy1, wx0, wx1, m[r0 + x0], m[r0 + x1], m[r1 + x0], m[r1 + x1]));
                    } else {
                        const float* m = (const float*)maps;
                        v = (double)rintf(blend<float>(hy0, hy1, wx0, wx1, m[r0 + x0], m[r0 + x1], m[r1 + x0], m[r1 + x1]));
                    }
                }
            }
        }
    }
    store_value(g, out, idx, v);
}

int per_image(int side, const stp3_augment_depth_dims* d) { return d->separable ? (side + d->stride - 1) / d->stride : side; }

bool axis_ok(const stp3_augment_depth_axis& a, int n) {
    return a.tap && a.weight && a.slot_src && a.entries >= n && a.slots >= 0;
}

bool dims_ok(const stp3_augment_depth_dims* d) {
    if (!d || d->F < 1 || d->N < 1 || d->N > 65535 || d->n_total < 0 || d->H < 3 || d->W < 3 || d->Ho < 1 || d->Wo < 1 ||
        d->Ho > kMaxSide || d->Wo > kMaxSide || d->stride < 1 || (d->separable != 0 && d->separable != 1) || !d->records ||
        (d->out_kind != STP3_DEPTH_OUT_F32 && d->out_kind != STP3_DEPTH_OUT_F64 && d->out_kind != STP3_DEPTH_OUT_LABELS))
        return false;
    return (int64_t)d->F * d->N <= 0x7fffffff / kRecord && axis_ok(d->y, per_image(d->Ho, d)) && axis_ok(d->x, per_image(d->Wo, d));
}

Geo geo_of(const stp3_augment_depth_dims* d) {
    Geo g;
    g.y.tap = d->y.tap; g.y.weight = d->y.weight; g.y.slot_src = d->y.slot_src;
    g.y.n = per_image(d->Ho, d); g.y.entries = d->y.entries; g.y.slots = d->y.slots; g.y.n_src = d->H;
    g.x.tap = d->x.tap; g.x.weight = d->x.weight; g.x.slot_src = d->x.slot_src;
    g.x.n = per_image(d->Wo, d); g.x.entries = d->x.entries; g.x.slots = d->x.slots; g.x.n_src = d->W;
    g.records = d->records;
    g.F = d->F; g.N = d->N; g.n_total = d->n_total; g.out_kind = d->out_kind;
    g.Ho = d->Ho; g.Wo = d->Wo; g.stride = d->stride; g.separable = d->separable;
    g.out_h = (d->Ho + d->stride - 1) / d->stride; g.out_w = (d->Wo + d->stride - 1) / d->stride;
    g.d_lo = d->d_lo; g.d_hi = d->d_hi;
    return g;
}

size_t table_bytes(const stp3_augment_depth_dims* d) {
    return (size_t)d->F * d->N * 2 * per_image(d->Ho, d) * 2 * per_image(d->Wo, d) * sizeof(int);
}

// the winner tables, then the float32 depth of every (point, camera) that reached one
size_t workspace_bytes(const stp3_augment_depth_dims* d) { return table_bytes(d) + (size_t)d->n_total * d->N * sizeof(float); }

int last_error() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" {

int stp3_augment_depth_workspace_bytes(const stp3_augment_depth_dims* dims, size_t* bytes) {
    if (!dims_ok(dims) || !bytes) return STP3_EINVAL;
    *bytes = workspace_bytes(dims);
    return STP3_OK;
}

int stp3_augment_depth_from_lidar(const stp3_augment_depth_dims* dims, const float* points, const int32_t* offsets,
                                  const double* steps, int32_t before, const double* intrinsics, void* workspace,
                                  size_t workspace_bytes, void* out, void* stream) {
    if (!dims_ok(dims) || (before & ~15) || !offsets || !steps || !intrinsics || !workspace || !out ||
        (dims->n_total > 0 && !points))
        return STP3_EINVAL;
    if (workspace_bytes < ::workspace_bytes(dims)) return STP3_ENOSPACE;
    const Geo g = geo_of(dims);
    const int64_t outputs = (int64_t)g.F * g.N * g.out_h * g.out_w;
    if (outputs >= ((int64_t)1 << 31) * kThreads) return STP3_EINVAL;
    Cloud c;
    c.points = points; c.offsets = offsets; c.steps = steps; c.intrinsics = intrinsics; c.before = before;
    const size_t words = table_bytes(dims) / sizeof(int);
    const size_t clear_blocks = (words + 4 * kThreads - 1) / (4 * kThreads);             // four words a thread, at most 64k blocks
    float* zbuf = (float*)((char*)workspace + table_bytes(dims));
    hipLaunchKernelGGL(depth_augment_clear_kernel, dim3((unsigned)(clear_blocks < 65536 ? clear_blocks : 65536)), dim3(kThreads), 0,
                       (hipStream_t)stream, (int*)workspace, words);
    if (g.n_total > 0)
        hipLaunchKernelGGL(depth_augment_scatter_kernel, dim3(blocks_for(g.n_total), g.N), dim3(kThreads), 0, (hipStream_t)stream,
                           g, c, (int*)workspace, zbuf);
    hipLaunchKernelGGL(depth_augment_output_kernel<kSrcLidar>, dim3(blocks_for(outputs)), dim3(kThreads), 0, (hipStream_t)stream,
                       g, c, (const float*)zbuf, (const int*)workspace, (const void*)nullptr, out);
    return last_error();
}

int stp3_augment_depth_from_maps(const stp3_augment_depth_dims* dims, const void* maps, int32_t map_dtype, void* out,
                                 void* stream) {
    if (!dims_ok(dims) || !maps || !out || (map_dtype != STP3_DEPTH_OUT_F32 && map_dtype != STP3_DEPTH_OUT_F64))
        return STP3_EINVAL;
    const Geo g = geo_of(dims);
    const int64_t outputs = (int64_t)g.F * g.N * g.out_h * g.out_w;
    if (outputs >= ((int64_t)1 << 31) * kThreads) return STP3_EINVAL;
    Cloud c;
    c.points = nullptr; c.offsets = nullptr; c.steps = nullptr; c.intrinsics = nullptr; c.before = 0;
    if (map_dtype == STP3_DEPTH_OUT_F64)
        hipLaunchKernelGGL(depth_augment_output_kernel<kSrcMapF64>, dim3(blocks_for(outputs)), dim3(kThreads), 0,
                           (hipStream_t)stream, g, c, (const float*)nullptr, (const int*)nullptr, maps, out);
    else
        hipLaunchKernelGGL(depth_augment_output_kernel<kSrcMapF32>, dim3(blocks_for(outputs)), dim3(kThreads), 0,
                           (hipStream_t)stream, g, c, (const float*)nullptr, (const int*)nullptr, maps, out);
    return last_error();
}

}  // extern "C"
