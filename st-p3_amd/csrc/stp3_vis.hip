// stp3_vis.hip -- the training video (stp3/utils/visualisation.py:208-322, visualise_output) of one sample for gfx950.
//
// The reference pulls about fourteen tensors per frame to the host and colours them with numpy; here one launch paints
// video [T][3][7 H][2 W] (uint8, planar) from the device-resident labels and head outputs.  Rows of panels, top to bottom:
// instance, future flow, segmentation, centerness, offset, pedestrian, planning; labels left, predictions right.  A panel shows
// cell (H - 1 - r, W - 1 - c) at pixel (r, c) (the reference's [::-1, ::-1]), an enabled panel then gets make_contour's
// one-pixel black border, a disabled one is zero.  The arithmetic, panel by panel (the library is built with -ffp-contract=off
// and correctly rounded float32 division and square root, so every statement rounds where numpy rounds):
//   segmentation, pedestrian   semantic_colours: 1 is black, everything else white; a prediction is class 1 where
//                 logit[1] > logit[0] (argmax takes the first maximum)
//   instance      palette[id mod 70], except the frame's SMALLEST id, which stays white whether it is the background or not
//                 (the reference drops unique()[0]); the smallest id comes from vis_prepare_kernel
//   centerness    heatmap_image: v = (x - min) / (max - min, or 1 when that is 0) in float32, matplotlib's index
//                 trunc(v * 256) in float32 with 256 -> 255 (below 0 -> 0, above -> 255, NaN -> black), the jet byte table;
//                 min and max of the frame come from vis_prepare_kernel
//   offset, flow  compute_color in the reference's mixed precision: vectors of cells whose segmentation (labels: the label,
//                 predictions: the predicted class) is not 1 are zeroed first, which paints them white; rad = sqrt(u u + v v)
//                 and a = atan2(-v, -u) / pi in float32, fk = (a + 1) / 2 * 54 + 1 in float32, k0 = floor(fk), f = fk - k0 in
//                 float64, col = (1 - f) wheel[k0 - 1] / 255 + f wheel[k1 - 1] / 255 in float64, rad <= 1: 1 - rad (1 - col),
//                 else 0.75 col; the byte is trunc(255 col).  A NaN component gives a black pixel.  atan2 is evaluated in
//                 float64 and rounded to float32 (numpy's float32 arctan2 may differ from that by an ulp: the one place where a
//                 byte can differ from the reference's, by 1)
//   planning      NOT the reference's matplotlib canvas (anti-aliased, not reproducible): white; cells with hd_map[0] != 0
//                 (255, 230, 220); cells with hd_map[1] != 0 (230, 216, 227), painted later; the ego box cells (118, 185, 0);
//                 then the trajectory (31, 119, 180): between the cells of consecutive points -- row = trunc((y - bx0) / dx0),
//                 column = trunc((-x - bx1) / dx1) in float32, clipped to the map: what the cost function reads -- the cells
//                 (r0 + round(i dr / n), c0 + round(i dc / n)), i = 0..n, n = max(|dr|, |dc|), round(a / n) =
//                 floor((2 a + n) / (2 n)): a one-pixel, 8-connected line.  A prediction's hd map is the argmax of each
//                 channel pair of the logits.
// Launches: vis_prepare_kernel (grid (T, 1 | 5): the descriptor's copy into the workspace and, with the instance rows, one
// workgroup per frame and scalar pair -- a fixed tree in LDS, no atomics) and vis_paint_kernel (a workgroup stays inside one
// panel of one frame; a thread paints four neighbouring pixels of a video row and stores one 32-bit word per colour plane;
// with an odd W or an unaligned video the rows are not word aligned and it stores bytes, the last group of a row is then a
// two-pixel tail).  Lanes walk a row of the video left to right, so the mirrored source cells are read at descending consecutive
// addresses: whole cache lines per wave.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stp3_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPanelRows = 7;
constexpr int kPalette = 70, kWheel = 55;
enum { kRowInstance = 0, kRowFlow, kRowSeg, kRowCenter, kRowOffset, kRowPed, kRowPlan };

struct Scalars {                              // per frame, [0] labels, [1] predictions
    float cmin[2], cmax[2];
    long long idmin[2];
};

// a float32 value, or a bf16 one widened exactly
__device__ __forceinline__ float load_logit(const void* p, int dtype, long long off) {
    if (dtype == STP3_DTYPE_BF16) return __uint_as_float((uint32_t)((const uint16_t*)p)[off] << 16);
    return ((const float*)p)[off];
}

__device__ __forceinline__ float load_real(const stp3_vis_map& m, long long off) { return load_logit(m.ptr, m.dtype, off); }

__device__ __forceinline__ long long cell_offset(const stp3_vis_map& m, int t, int y, int x) {
    return t * m.stride_t + y * m.stride_h + x * m.stride_w;
}

// class 1 at a cell: the value of an int64 label map, the argmax of two logits
__device__ __forceinline__ bool is_class1(const stp3_vis_map& m, int t, int y, int x) {
    const long long off = cell_offset(m, t, y, x);
    if (m.dtype == STP3_VIS_DTYPE_I64) return ((const long long*)m.ptr)[off] == 1;
    return load_real(m, off + m.stride_c) > load_real(m, off);
}

__device__ __forceinline__ uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
constexpr uint32_t kWhite = 0xffffffu, kBlack = 0u;

__device__ __forceinline__ uint32_t table_rgb(const uint8_t* __restrict__ table, int i) {
    return rgb(table[3 * i], table[3 * i + 1], table[3 * i + 2]);
}

constexpr int kDescWords = sizeof(stp3_vis_desc) / 4;
static_assert(sizeof(stp3_vis_desc) % 4 == 0 && kDescWords <= kThreads, "one thread per word of the descriptor");

// grid (T, 1 | 5).  Row 0 (its first workgroup) copies the descriptor into the workspace: the painter reads it from there with
// scalar loads where it needs a field, instead of holding all 194 words of a by-value argument in registers.  Rows 1..4 are
// the per-frame scalars: min and max of the centre map of the labels / the predictions, smallest id of their instance maps.
__global__ __launch_bounds__(kThreads) void vis_prepare_kernel(stp3_vis_desc d, Scalars* __restrict__ ws,
                                                               uint32_t* __restrict__ copy) {
    __shared__ float s_lo[kThreads], s_hi[kThreads];
    __shared__ long long s_id[kThreads];
    const int tid = threadIdx.x, t = blockIdx.x;
    if (blockIdx.y == 0) {
        if (t == 0 && tid < kDescWords) copy[tid] = ((const uint32_t*)&d)[tid];
        return;
    }
    const int side = (blockIdx.y - 1) & 1;
    const bool ids = blockIdx.y >= 3;
    const stp3_vis_map& m = ids ? (side ? d.inst[1] : d.inst[0]) : (side ? d.center[1] : d.center[0]);
    float lo = INFINITY, hi = -INFINITY;
    long long id = INT64_MAX;
    for (int i = tid; i < d.H * d.W; i += kThreads) {
        const long long off = cell_offset(m, t, i / d.W, i % d.W);
        if (ids) {
            const long long v = ((const long long*)m.ptr)[off];
            id = v < id ? v : id;
        } else {
            const float v = load_real(m, off);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    s_lo[tid] = lo; s_hi[tid] = hi; s_id[tid] = id;
    __syncthreads();
    for (int n = kThreads / 2; n > 0; n >>= 1) {
        if (tid < n) {
            s_lo[tid] = fminf(s_lo[tid], s_lo[tid + n]);
            s_hi[tid] = fmaxf(s_hi[tid], s_hi[tid + n]);
            s_id[tid] = s_id[tid + n] < s_id[tid] ? s_id[tid + n] : s_id[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (ids) ws[t].idmin[side] = s_id[0];
        else { ws[t].cmin[side] = s_lo[0]; ws[t].cmax[side] = s_hi[0]; }
    }
}

__device__ __forceinline__ uint32_t centre_colour(const stp3_vis_desc& d, float x, float lo, float hi) {
    float delta = hi - lo;
    if (delta == 0.f) delta = 1.f;
    float s = (x - lo) / delta * 256.f;
    if (s != s) return kBlack;                                   // matplotlib's "bad" entry
    if (s == 256.f) s = 255.f;
    const int i = s < 0.f ? 0 : (s >= 256.f ? 255 : (int)s);
    return table_rgb(d.jet, i);
}

__device__ __forceinline__ uint32_t flow_colour(const stp3_vis_desc& d, float u, float v) {
    if (u != u || v != v) return kBlack;
    const float rad = sqrtf(u * u + v * v);
    const float a = (float)atan2((double)-v, (double)-u) / 3.14159274f;
    const float fk = (a + 1.f) / 2.f * (float)(kWheel - 1) + 1.f;
    int k0 = (int)floorf(fk);
    k0 = k0 < 1 ? 1 : (k0 > kWheel ? kWheel : k0);
    const int k1 = k0 == kWheel ? 1 : k0 + 1;
    const double f = (double)fk - (double)k0;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double c0 = (double)d.wheel[3 * (k0 - 1) + i] / 255.0, c1 = (double)d.wheel[3 * (k1 - 1) + i] / 255.0;
        double col = (1.0 - f) * c0 + f * c1;
        if (rad <= 1.f) col = 1.0 - (double)rad * (1.0 - col);
        else col *= 0.75;
        out |= (uint32_t)(uint8_t)(col * 255.0) << (8 * i);
    }
    return out;
}

__device__ __forceinline__ uint32_t flow_panel(const stp3_vis_desc& d, const stp3_vis_map& m, const stp3_vis_map& seg, int t,
                                               int y, int x) {
    if (!is_class1(seg, t, y, x)) return kWhite;                 // a zeroed vector: rad = 0 whitens whatever the angle
    const long long off = cell_offset(m, t, y, x);
    return flow_colour(d, load_real(m, off), load_real(m, off + m.stride_c));
}

// the cell the cost function reads for trajectory point i, clipped to the map
__device__ __forceinline__ void traj_cell(const stp3_vis_desc& d, const stp3_vis_plan& p, int i, int& r, int& c) {
    const float x = -p.traj[i * p.traj_stride_p], y = p.traj[i * p.traj_stride_p + p.traj_stride_c];
    const float fr = (y - d.bx0) / d.dx0, fc = (x - d.bx1) / d.dx1;
    r = (int)fminf(fmaxf(fr, 0.f), (float)(d.H - 1));            // (a NaN becomes 0; clamping first keeps the cast in range)
    c = (int)fminf(fmaxf(fc, 0.f), (float)(d.W - 1));
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// is (y, x) one of the cells (r0 + round(i dr / n), c0 + round(i dc / n)), i = 0..n ?
__device__ __forceinline__ bool on_line(int r0, int c0, int r1, int c1, int y, int x) {
    const int dr = r1 - r0, dc = c1 - c0, ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc;
    const int n = ar > ac ? ar : ac;
    if (n == 0) return y == r0 && x == c0;
    if (ac >= ar) {
        const int i = dc < 0 ? c0 - x : x - c0;
        return i >= 0 && i <= n && y == r0 + (int)floor_div(2ll * i * dr + n, 2ll * n);
    }
    const int i = dr < 0 ? r0 - y : y - r0;
    return i >= 0 && i <= n && x == c0 + (int)floor_div(2ll * i * dc + n, 2ll * n);
}

__device__ __forceinline__ uint32_t plan_panel(const stp3_vis_desc& d, const stp3_vis_plan& p, int y, int x) {
    uint32_t colour = kWhite;
    const long long off = y * p.hd_stride_h + x * p.hd_stride_w, sc = p.hd_stride_c;
    bool lane, area;
    if (p.hd_dtype == STP3_VIS_DTYPE_I64) {
        lane = ((const long long*)p.hdmap)[off] != 0;
        area = ((const long long*)p.hdmap)[off + sc] != 0;
    } else {
        lane = load_logit(p.hdmap, p.hd_dtype, off + sc) > load_logit(p.hdmap, p.hd_dtype, off);
        area = load_logit(p.hdmap, p.hd_dtype, off + 3 * sc) > load_logit(p.hdmap, p.hd_dtype, off + 2 * sc);
    }
    if (lane) colour = rgb(255, 230, 220);
    if (area) colour = rgb(230, 216, 227);
    for (int i = 0; i < d.n_ego; ++i)
        if (d.ego_cells[2 * i] == y && d.ego_cells[2 * i + 1] == x) colour = rgb(118, 185, 0);
    int r0 = 0, c0 = 0;
    for (int i = 0; i < p.n_points; ++i) {
        int r1, c1;
        traj_cell(d, p, i, r1, c1);
        if (i == 0 ? (y == r1 && x == c1) : on_line(r0, c0, r1, c1, y, x)) colour = rgb(31, 119, 180);
        r0 = r1; c0 = c1;
    }
    return colour;
}

// the colour of pixel (r, col) of panel row `panel` of frame t, packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t paint(const stp3_vis_desc& d, const Scalars* __restrict__ ws, int t, int panel, int r, int col) {
    const int side = col >= d.W ? 1 : 0, c = col - side * d.W;
    bool on = true;
    if (panel == kRowInstance || panel == kRowCenter || panel == kRowOffset) on = d.panels & STP3_VIS_INSTANCE;
    else if (panel == kRowFlow) on = d.panels & STP3_VIS_FLOW;
    else if (panel == kRowPed) on = d.panels & STP3_VIS_PEDESTRIAN;
    else if (panel == kRowPlan) on = d.panels & (side ? STP3_VIS_PLAN_PRED : STP3_VIS_PLAN_LABELS);
    if (!on || r == 0 || r == d.H - 1 || c == 0 || c == d.W - 1) return kBlack;
    const int y = d.H - 1 - r, x = d.W - 1 - c;
    const stp3_vis_map& seg = side ? d.seg[1] : d.seg[0];
    switch (panel) {
    case kRowInstance: {
        const stp3_vis_map& m = side ? d.inst[1] : d.inst[0];
        const long long id = ((const long long*)m.ptr)[cell_offset(m, t, y, x)];
        if (id == ws[t].idmin[side]) return kWhite;
        return table_rgb(d.palette, (int)((id % kPalette + kPalette) % kPalette));
    }
    case kRowFlow: return flow_panel(d, side ? d.flow[1] : d.flow[0], seg, t, y, x);
    case kRowSeg: return is_class1(seg, t, y, x) ? kBlack : kWhite;
    case kRowCenter: {
        const stp3_vis_map& m = side ? d.center[1] : d.center[0];
        return centre_colour(d, load_real(m, cell_offset(m, t, y, x)), ws[t].cmin[side], ws[t].cmax[side]);
    }
    case kRowOffset: return flow_panel(d, side ? d.offset[1] : d.offset[0], seg, t, y, x);
    case kRowPed: return is_class1(side ? d.ped[1] : d.ped[0], t, y, x) ? kBlack : kWhite;
    default: return plan_panel(d, side ? d.plan[1] : d.plan[0], y, x);
    }
}

__global__ __launch_bounds__(kThreads) void vis_paint_kernel(const stp3_vis_desc* __restrict__ desc, const Scalars* __restrict__ ws,
                                                             uint8_t* __restrict__ video, int groups, int words) {
    const stp3_vis_desc& d = *desc;
    // a workgroup stays inside one panel row of one frame: which sources it reads is uniform
    const int idx = blockIdx.x * kThreads + threadIdx.x, panel = blockIdx.y % kPanelRows, t = blockIdx.y / kPanelRows;
    const int rows = kPanelRows * d.H, width = 2 * d.W;
    if (idx >= d.H * groups) return;
    const int g = idx % groups, r = idx / groups, row = panel * d.H + r;
    const int col0 = 4 * g, n = width - col0 < 4 ? width - col0 : 4;
    uint32_t plane[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < n) {
            const uint32_t colour = paint(d, ws, t, panel, r, col0 + k);
            plane[0] |= (colour & 255u) << (8 * k);
            plane[1] |= ((colour >> 8) & 255u) << (8 * k);
            plane[2] |= ((colour >> 16) & 255u) << (8 * k);
        }
    }
    const long long plane_bytes = (long long)rows * width;
    uint8_t* out = video + (long long)t * 3 * plane_bytes + (long long)row * width + col0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (words) {
            *(uint32_t*)(out + ch * plane_bytes) = plane[ch];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) out[ch * plane_bytes + k] = (uint8_t)(plane[ch] >> (8 * k));
        }
    }
}

bool real_dtype(int dtype) { return dtype == STP3_DTYPE_F32 || dtype == STP3_DTYPE_BF16; }

bool ids_ok(const stp3_vis_map& m) { return m.ptr && m.dtype == STP3_VIS_DTYPE_I64; }
bool real_ok(const stp3_vis_map& m) { return m.ptr && real_dtype(m.dtype); }

int desc_check(const stp3_vis_desc* d) {
    if (!d || d->T < 1 || d->H < 3 || d->W < 3 || d->n_ego < 0 || (d->panels & ~31)) return STP3_EINVAL;
    if (!ids_ok(d->seg[0]) || !real_ok(d->seg[1])) return STP3_EINVAL;
    if (d->panels & STP3_VIS_PEDESTRIAN)
        if (!ids_ok(d->ped[0]) || !real_ok(d->ped[1])) return STP3_EINVAL;
    if (d->panels & STP3_VIS_INSTANCE) {
        if (!ids_ok(d->inst[0]) || !ids_ok(d->inst[1]) || !d->palette || !d->jet || !d->wheel) return STP3_EINVAL;
        for (int s = 0; s < 2; ++s)
            if (!real_ok(d->center[s]) || !real_ok(d->offset[s])) return STP3_EINVAL;
    }
    if (d->panels & STP3_VIS_FLOW)
        if (!real_ok(d->flow[0]) || !real_ok(d->flow[1]) || !d->wheel) return STP3_EINVAL;
    for (int s = 0; s < 2; ++s) {
        if (!(d->panels & (s ? STP3_VIS_PLAN_PRED : STP3_VIS_PLAN_LABELS))) continue;
        const stp3_vis_plan& p = d->plan[s];
        if (!p.hdmap || p.n_points < 0 || (p.n_points > 0 && !p.traj) || (d->n_ego > 0 && !d->ego_cells) ||
            !(p.hd_dtype == STP3_VIS_DTYPE_I64 || real_dtype(p.hd_dtype)))
            return STP3_EINVAL;
    }
    if ((int64_t)2 * d->W * kPanelRows * d->H * 3 * d->T >= ((int64_t)1 << 31) || d->T * kPanelRows > 65535) return STP3_EUNSUP;
    return STP3_OK;
}

int last_error() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // namespace

extern "C" {

int stp3_vis_workspace_bytes(const stp3_vis_desc* desc, size_t* bytes) {
    const int rc = desc_check(desc);
    if (rc != STP3_OK) return rc;
    if (!bytes) return STP3_EINVAL;
    *bytes = (size_t)desc->T * sizeof(Scalars) + sizeof(stp3_vis_desc);      // the scalars, then the descriptor's copy
    return STP3_OK;
}

int stp3_vis_render(const stp3_vis_desc* desc, uint8_t* video, void* workspace, void* stream) {
    const int rc = desc_check(desc);
    if (rc != STP3_OK) return rc;
    if (!video || !workspace || ((uintptr_t)workspace & 7)) return STP3_EINVAL;
    const stp3_vis_desc d = *desc;
    stp3_vis_desc* copy = (stp3_vis_desc*)((Scalars*)workspace + d.T);
    hipLaunchKernelGGL(vis_prepare_kernel, dim3(d.T, (d.panels & STP3_VIS_INSTANCE) ? 5 : 1), dim3(kThreads), 0,
                       (hipStream_t)stream, d, (Scalars*)workspace, (uint32_t*)copy);
    // rows of 2 W bytes are word aligned in every plane when W is even and the video is
    const int words = d.W % 2 == 0 && ((uintptr_t)video & 3) == 0;
    const int groups = (2 * d.W + 3) / 4;
    const long long threads = (long long)d.H * groups;             // of one panel row of one frame
    hipLaunchKernelGGL(vis_paint_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads), d.T * kPanelRows), dim3(kThreads), 0,
                       (hipStream_t)stream, (const stp3_vis_desc*)copy, (const Scalars*)workspace, video, groups, words);
    return last_error();
}

}  // extern "C"
