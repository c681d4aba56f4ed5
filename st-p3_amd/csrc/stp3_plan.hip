// stp3_plan.hip -- the planner's trajectory-cost evaluation for gfx950.
//
// Replaces, behind stp3_traj_cost_fwd / _bwd, the reference's Cost_Function (stp3/cost.py:10-47) and its seven terms
// (SafetyCost :210-241, HeadwayCost :244-272, LR_divider :274-315, Comfort :318-372, Progress :374-392, Rule :183-207,
// Cost_Volume :166-181), which the reference evaluates with ~150 small tensor operators and, for every term that looks
// at the ego footprint, a materialised (B, N, T, K) gather (K = 32 cells of the ego box, 192 of the inflated one).
// Here one thread owns one (sample, trajectory, time step): it walks the footprint tables once, reading the three BEV
// maps (occupancy, drivable area, lane dividers) and the cost volume where they lie -- an L2-resident gather workload:
// the maps of one sample are 4 x 160 KB.  Nothing is materialised; the trajectory-level terms (comfort, progress) are
// evaluated by the thread of the first time step.
//
// Arithmetic: float32, one operation per reference operation in the reference's order (no contraction: the library is
// built with -ffp-contract=off, divisions and square roots correctly rounded), truncating float -> integer conversions and
// clamps as the reference's `.long()` / `torch.clamp`.  Lane dividers: the reference takes the minimum distance to ALL
// divider cells and then drops everything beyond L = 1 m; only cells within ceil(L / resolution) of the trajectory
// point can matter, so the kernel looks at that window -- the same value, not an approximation.
//
// Backward: the trajectories, maps and target are data; the only differentiable input is the cost volume (the decoder's
// cost-volume head).  Its gradient is a scatter of the (B, N, T) cost gradients into the cells the forward read; cells
// hit by several trajectories are summed in ascending trajectory order by the thread of the FIRST of them -- no
// floating-point atomics, bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "stp3_hip.h"

namespace {

struct PlanDims {
    int B, N, T, H, W, K0, KL;
    float dx0, dx1, bx0, bx1;
    float safety, headway, lrdivider, comfort, progress, volume, rule;
    float w0, w1, headway_dist, lr_dist;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }   // NaN -> lo

// torch: x.long() then clamp(0, n - 1).  Values beyond the int range (and NaN, which .long() sends to INT64_MIN) end up
// at the same clamp bound either way.
__device__ __forceinline__ int cell_of(float v, int n) {
    if (!(v > -1.0f)) return 0;                            // trunc(v) <= 0, or NaN
    if (v >= (float)n) return n - 1;
    return (int)v;                                         // truncation toward zero
}

// sum over the footprint of  map_a[cell] (* map_b[cell] when map_b != nullptr; == 0 when `negate`)
template <bool kProduct, bool kNegate>
__device__ __forceinline__ float footprint_sum(const PlanDims& d, const float* __restrict__ a, const float* __restrict__ b,
                                               const int2* __restrict__ rc, int K, float fy, float fx) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) {
        const int2 o = rc[k];
        const int r = cell_of(fy + (float)o.x, d.H), c = cell_of(fx + (float)o.y, d.W);
        float v = a[r * d.W + c];
        if (kNegate) v = v == 0.f ? 1.f : 0.f;
        if (kProduct) v = v * b[r * d.W + c];
        s += v;
    }
    return s;
}

// element i of a float32 or bf16 tensor, in float32: what utils.hp does to a bf16 tensor
__device__ __forceinline__ float logit_at(const void* __restrict__ p, long long i, int bf16) {
    if (bf16) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(p)[i] << 16);
    return reinterpret_cast<const float*>(p)[i];
}

// The five per-step terms of one trajectory point: `tr` is the trajectory (point stride `ts` floats), `occ_t` / `cv_t` the
// occupancy and cost-volume planes of its sample AND time step (the latter float32 or bf16, widened), `drv` / `ln` the sample's masks.  Shared by traj_cost_kernel
// and plan_drive_kernel: one operation per reference operation, in the reference's order.  `cell`, `cv`, `term`: what the
// backward of the cost volume needs.
__device__ __forceinline__ float point_cost(const PlanDims& d, const float* __restrict__ tr, int ts, int t,
                                            const void* __restrict__ cv_t, int cv_bf16, const float* __restrict__ occ,
                                            const float* __restrict__ drv, const float* __restrict__ ln,
                                            const int2* __restrict__ rc0, const int2* __restrict__ rcl, int& cell, float& cv,
                                            float& term) {
    // the reference flips the lateral axis first (cost.py:35)
    const float x = tr[ts * t] * -1.0f, y = tr[ts * t + 1];
    const float xp = t ? tr[ts * (t - 1)] * -1.0f : 0.f, yp = t ? tr[ts * (t - 1) + 1] : 0.f;
    const float ddx = t ? x - xp : x, ddy = t ? y - yp : y;
    const float vel = sqrtf(ddx * ddx + ddy * ddy) / 0.5f;
    const float fy = y / d.dx1, fx = x / d.dx0;            // get_points: trajs / dx, then rows <- y, columns <- x

    // safety (cost.py:210-241): occupied cells under the box + occupied cells under the inflated box x speed
    const float a0 = footprint_sum<false, false>(d, occ, nullptr, rc0, d.K0, fy, fx);
    const float al = footprint_sum<false, false>(d, occ, nullptr, rcl, d.KL, fy, fx);
    const float safety = clampf((a0 * d.w0 + (al * vel) * d.w1) * d.safety, 0.f, 100.f);
    // headway (:244-272): occupied AND drivable cells under the box moved L metres ahead
    const float fyh = (y + d.headway_dist) / d.dx1;
    const float headway = clampf(footprint_sum<true, false>(d, occ, drv, rc0, d.K0, fyh, fx) * d.headway, 0.f, 100.f);
    // rule (:183-207): non-drivable cells under the box
    const float rule = clampf(footprint_sum<false, true>(d, drv, nullptr, rc0, d.K0, fy, fx) * d.rule, 0.f, 100.f);
    // the trajectory point's own cell (discretize, :131-147)
    const int yi = cell_of((y - d.bx0) / d.dx0, d.H), xi = cell_of((x - d.bx1) / d.dx1, d.W);
    // lane dividers (:274-315)
    float lr = 0.f;
    {
        const float res = fminf(d.dx0, d.dx1);
        const int rad = (int)ceilf(d.lr_dist / res);
        float best = INFINITY;
        for (int r = max(yi - rad, 0); r <= min(yi + rad, d.H - 1); ++r)
            for (int c = max(xi - rad, 0); c <= min(xi + rad, d.W - 1); ++c)
                if (ln[r * d.W + c] != 0.f) {
                    const float ey = (float)(yi - r) * d.dx1, ex = (float)(xi - c) * d.dx0;   // reversed(dx)
                    best = fminf(best, sqrtf(ey * ey + ex * ex));
                }
        if (!(best > d.lr_dist)) {
            const float g = d.lr_dist - best;
            lr = g * g;
        }
        lr = clampf(lr * d.lrdivider, 0.f, 100.f);
    }
    // cost volume (:166-181)
    cell = yi * d.W + xi;
    cv = logit_at(cv_t, cell, cv_bf16);
    term = clampf(cv, 0.f, 1000.f) * d.volume;
    const float volume = clampf(term, 0.f, 100.f);
    return (((safety + headway) + lr) + volume) + rule;
}

// The trajectory-level terms: comfort (:318-372) + progress (:374-392).  `tgt`: the sample's target point.
__device__ __forceinline__ float trajectory_cost(const PlanDims& d, const float* __restrict__ tr, int ts,
                                                 const float* __restrict__ tgt, float target_sum) {
    float lat_acc = 0.f, lon_acc = 0.f, jerk = 0.f, ymax = -INFINITY;
    float px = 0.f, py = 0.f, plat = 0.f, plon = 0.f, pvel = 0.f, pacc = 0.f, lx = 0.f, ly = 0.f;
    for (int i = 0; i < d.T; ++i) {
        const float cx = tr[ts * i] * -1.0f, cy = tr[ts * i + 1];
        const float sx = i ? cx - px : cx, sy = i ? cy - py : cy;
        const float lat = sx / 0.5f, lon = sy / 0.5f;
        const float v = sqrtf(sx * sx + sy * sy) / 0.5f;
        float acc = 0.f;
        if (i >= 1) {
            lat_acc = fmaxf(lat_acc, fabsf((lat - plat) / 0.5f));
            lon_acc = fmaxf(lon_acc, fabsf((lon - plon) / 0.5f));
            acc = (v - pvel) / 0.5f;
        }
        if (i >= 2) jerk = fmaxf(jerk, fabsf((acc - pacc) / 0.5f));
        ymax = fmaxf(ymax, cy);
        px = cx; py = cy; plat = lat; plon = lon; pvel = v; pacc = acc; lx = cx; ly = cy;
    }
    float comfort = 0.f;
    { const float a = clampf(lat_acc - 3.f, 0.f, 30.f); comfort += a * a; }
    { const float a = clampf(lon_acc - 3.f, 0.f, 30.f); comfort += a * a; }
    { const float a = clampf(jerk - 1.f, 0.f, 20.f); comfort += a * a; }
    comfort = clampf(comfort * d.comfort, 0.f, 100.f);
    float goal = 0.f;
    if (!(target_sum < 0.5f)) {                             // the reference tests the sum over the WHOLE batch (:386)
        const float ex = lx - tgt[0], ey = ly - tgt[1];
        goal = ex * ex + ey * ey;
    }
    const float progress = clampf((goal - ymax) * d.progress, -100.f, 100.f);
    return comfort + progress;
}

__global__ __launch_bounds__(256) void traj_cost_kernel(PlanDims d, const float* __restrict__ trajs,
                                                        const float* __restrict__ cost_volume,
                                                        const float* __restrict__ occupancy,
                                                        const float* __restrict__ drivable, const float* __restrict__ lane,
                                                        const float* __restrict__ target, const float* __restrict__ target_sum,
                                                        const int2* __restrict__ rc0, const int2* __restrict__ rcl,
                                                        float* __restrict__ cost_fc, float* __restrict__ cost_fo,
                                                        int* __restrict__ cv_cell, float* __restrict__ cv_scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= d.B * d.N * d.T) return;
    const int t = idx % d.T, bn = idx / d.T, b = bn / d.N;
    const float* tr = trajs + (size_t)bn * d.T * 2;
    const size_t plane = (size_t)d.H * d.W;
    int cell;
    float cv, term;
    cost_fo[idx] = point_cost(d, tr, 2, t, cost_volume + ((size_t)b * d.T + t) * plane, 0,
                              occupancy + ((size_t)b * d.T + t) * plane, drivable + (size_t)b * plane,
                              lane + (size_t)b * plane, rc0, rcl, cell, cv, term);
    if (cv_cell) {
        cv_cell[idx] = cell;
        // torch.clamp passes the gradient where min <= x <= max
        cv_scale[idx] = (cv >= 0.f && cv <= 1000.f && term >= 0.f && term <= 100.f) ? d.volume : 0.f;
    }
    if (t) return;
    // ---- trajectory-level terms, by the thread of the first step
    cost_fc[bn] = trajectory_cost(d, tr, 2, target + 2 * b, target_sum[0]);
}

// d cost_volume[b, t, cell] = sum over the trajectories n that read the cell of g[b, n, t] * scale[b, n, t], in ascending n.
// The (t, b) plane's N (cell, weighted gradient) pairs sit in LDS; one THREAD per trajectory scans the list (all lanes read
// the same entry: an LDS broadcast), and the first reader of a cell adds up all of them and writes the cell.  The plane
// was zero-filled by the launcher; gridDim.z workgroups share the trajectories of a plane.
__global__ __launch_bounds__(256) void traj_cost_bwd_kernel(PlanDims d, const float* __restrict__ g_fo,
                                                            const int* __restrict__ cv_cell,
                                                            const float* __restrict__ cv_scale,
                                                            float* __restrict__ d_cost_volume) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int* cells = reinterpret_cast<int*>(smem);
    float* g = reinterpret_cast<float*>(smem) + d.N;
    const int t = blockIdx.x, b = blockIdx.y;
    float* out = d_cost_volume + ((size_t)b * d.T + t) * d.H * d.W;
    for (int n = threadIdx.x; n < d.N; n += 256) {
        const size_t i = ((size_t)b * d.N + n) * d.T + t;
        cells[n] = cv_cell[i];
        g[n] = g_fo[i] * cv_scale[i];
    }
    __syncthreads();
    const int n = blockIdx.z * 256 + threadIdx.x;
    if (n >= d.N) return;
    const int c = cells[n];
    for (int m = 0; m < n; ++m)
        if (cells[m] == c) return;                         // an earlier trajectory owns this cell
    float s = g[n];
    for (int m = n + 1; m < d.N; ++m)
        if (cells[m] == c) s += g[m];
    out[c] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// The planner tail of an inference call (include/stp3_hip.h: stp3_plan_scene, stp3_plan_drive).

struct SceneDims {
    int B, T, H, W, Cs, Cp, first, seg_bf16, ped_bf16, hd_bf16;
    long long seg_st[5], ped_st[5], hd_st[4];              // element strides (batch, frame, class, row, column)
};

// torch.argmax over the classes != 0: the FIRST maximal class wins a tie, a NaN counts as the maximum
__device__ __forceinline__ bool foreground(const void* __restrict__ p, long long base, long long cstride, int C, int bf16) {
    float bv = logit_at(p, base, bf16);
    int best = 0;
    for (int c = 1; c < C; ++c) {
        const float v = logit_at(p, base + c * cstride, bf16);
        if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
    }
    return best != 0;
}

// softmax probability of class 1 of the logit pair (l0, l1), as torch.softmax evaluates it in float32
__device__ __forceinline__ float pair_probability(float l0, float l1) {
    const float m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    return e1 / (e0 + e1);
}

// grid (cells / 256, T + 1, B): planes 0 .. T-1 write the occupancy of frame first + t, plane T the two hd-map masks
__global__ __launch_bounds__(256) void plan_scene_kernel(SceneDims d, const void* __restrict__ seg, const void* __restrict__ ped,
                                                         const void* __restrict__ hd, float* __restrict__ occupancy,
                                                         float* __restrict__ lane, float* __restrict__ drivable) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= d.H * d.W) return;
    const int r = cell / d.W, c = cell % d.W, t = blockIdx.y, b = blockIdx.z;
    if (t < d.T) {
        const int s = d.first + t;
        bool on = foreground(seg, b * d.seg_st[0] + s * d.seg_st[1] + r * d.seg_st[3] + c * d.seg_st[4], d.seg_st[2], d.Cs,
                             d.seg_bf16);
        if (d.Cp)
            on = on || foreground(ped, b * d.ped_st[0] + s * d.ped_st[1] + r * d.ped_st[3] + c * d.ped_st[4], d.ped_st[2],
                                  d.Cp, d.ped_bf16);
        occupancy[((size_t)b * d.T + t) * d.H * d.W + cell] = on ? 1.f : 0.f;
        return;
    }
    const long long base = b * d.hd_st[0] + r * d.hd_st[2] + c * d.hd_st[3];
    float l[4];
    for (int k = 0; k < 4; ++k) l[k] = logit_at(hd, base + k * d.hd_st[1], d.hd_bf16);
    const float pl = pair_probability(l[0], l[1]), pd = pair_probability(l[2], l[3]);
    lane[(size_t)b * d.H * d.W + cell] = pl <= 0.5f ? 0.f : pl;          // cost.py:289-294
    drivable[(size_t)b * d.H * d.W + cell] = pd < 0.5f ? 0.f : pd;       // cost.py:196-201 / :258-263
}

struct DriveArgs {
    int Hs, cols, cv_bf16, h0_bf16;                        // GRU state size; floats per trajectory point copied out (2 | 3)
    int traj_b, traj_n, traj_t, cv_b;                      // element strides: sample, row and point of trajs, sample of cost_volume
    const float* weights;                                  // [w_ih | b_ih | w_hh^T | b_hh | w1^T | b1 | w2 | b2], see stp3_drive_dims
};

constexpr int kDriveThreads = 1024;

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// One workgroup per sample.  (1) every (candidate of the command's range, step) by one thread: point_cost into LDS, the
// trajectory-level terms by the thread of step 0; (2) totals fc + sum_t fo[t] (t ascending) and a fixed-order arg-min, the
// lower index winning an exact tie; (3) T steps of GRUCell + Linear-ReLU-Linear on the winner, the state in LDS, every dot
// product one fmaf chain in ascending k (the output layer: 64 strided chains + a fixed butterfly).  Weights are read
// through transposed copies (whh_t [Hs][3 Hs], w1_t [Hs][Hs]): consecutive threads, consecutive addresses.
__global__ __launch_bounds__(kDriveThreads) void plan_drive_kernel(
    PlanDims d, DriveArgs a, const float* __restrict__ trajs, const void* __restrict__ cost_volume,
    const float* __restrict__ occupancy, const float* __restrict__ drivable, const float* __restrict__ lane,
    const float* __restrict__ target, const int* __restrict__ command, const int2* __restrict__ rc0,
    const int2* __restrict__ rcl, const void* __restrict__ h0, float* __restrict__ final_traj,
    float* __restrict__ selected_traj, int* __restrict__ selected_index) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* fo = reinterpret_cast<float*>(smem);            // [N][T]
    float* fc = fo + (size_t)d.N * d.T;                    // [N]
    float* red_v = fc + d.N;                               // [kDriveThreads]
    int* red_i = reinterpret_cast<int*>(red_v + kDriveThreads);
    float* h = red_v + 2 * kDriveThreads;                  // [Hs]
    float* gi = h + a.Hs;                                  // [3 Hs]
    float* gh = gi + 3 * a.Hs;                             // [3 Hs]
    float* hid = gh + 3 * a.Hs;                            // [Hs]
    float* x = hid + a.Hs;                                 // [8]: previous point, chosen point, target, the new point
    // the cost constants through LDS: as kernel arguments the 22 words stay in scalar registers next to everything the later
    // phases need, more than a wave has
    __shared__ PlanDims dc;
    const int b = blockIdx.x, tid = threadIdx.x, Hs = a.Hs;
    if (tid == 0) dc = d;
    __syncthreads();
    const int code = command[b], third = d.N / 3;
    const int lo = (code >= 0 && code <= 2) ? code * third : 0, hi = (code >= 0 && code <= 2) ? lo + third : d.N;
    const size_t plane = (size_t)d.H * d.W;
    const float* tr_b = trajs + (size_t)b * a.traj_b;
    const char* cv_b = reinterpret_cast<const char*>(cost_volume) + (a.cv_bf16 ? 2 : 4) * ((size_t)b * a.cv_b);
    float target_sum = 0.f;                                // the sum over the WHOLE batch (cost.py:386), ascending
    for (int i = 0; i < 2 * d.B; ++i) target_sum += target[i];

    for (int i = tid; i < (hi - lo) * d.T; i += kDriveThreads) {
        const int n = lo + i / d.T, t = i % d.T;
        const float* tr = tr_b + (size_t)n * a.traj_n;
        int cell;
        float cv, term;
        fo[i] = point_cost(dc, tr, a.traj_t, t, cv_b + (a.cv_bf16 ? 2 : 4) * (t * plane), a.cv_bf16, occupancy + ((size_t)b * d.T + t) * plane,
                           drivable + (size_t)b * plane, lane + (size_t)b * plane, rc0, rcl, cell, cv, term);
        if (t == 0) fc[i / d.T] = trajectory_cost(dc, tr, a.traj_t, target + 2 * b, target_sum);
    }
    for (int j = tid; j < Hs; j += kDriveThreads) h[j] = logit_at(h0, (long long)b * Hs + j, a.h0_bf16);
    __syncthreads();

    float best = INFINITY;
    int best_n = lo;
    for (int n = lo + tid; n < hi; n += kDriveThreads) {
        const float* f = fo + (size_t)(n - lo) * d.T;
        float s = f[0];
        for (int t = 1; t < d.T; ++t) s += f[t];
        const float total = fc[n - lo] + s;
        if (total < best) { best = total; best_n = n; }
    }
    red_v[tid] = best;
    red_i[tid] = best_n;
    __syncthreads();
    for (int s = kDriveThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const float ov = red_v[tid + s];
            const int oi = red_i[tid + s];
            if (ov < red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
    }
    const int win = red_i[0];
    const float* chosen = tr_b + (size_t)win * a.traj_n;
    if (tid < d.T * 3) {
        const int t = tid / 3, c = tid % 3;
        selected_traj[((size_t)b * d.T + t) * 3 + c] = c < a.cols ? chosen[t * a.traj_t + c] : 0.f;
    }
    if (tid == 0) {
        selected_index[b] = win;
        x[6] = 0.f;
        x[7] = 0.f;
    }
    __syncthreads();

    const float* w_ih = a.weights;                         // [3 Hs][6]
    const float* b_ih = w_ih + 18 * Hs;
    const float* whh_t = b_ih + 3 * Hs;                    // [Hs][3 Hs]
    const float* b_hh = whh_t + (size_t)3 * Hs * Hs;
    const float* w1_t = b_hh + 3 * Hs;                     // [Hs][Hs]
    const float* b1 = w1_t + (size_t)Hs * Hs;
    const float* w2 = b1 + Hs;                             // [2][Hs]
    const float* b2 = w2 + 2 * Hs;
    for (int t = 0; t < d.T; ++t) {
        if (tid < 6) x[tid] = tid < 2 ? x[6 + tid] : tid < 4 ? chosen[t * a.traj_t + tid - 2] : target[2 * b + tid - 4];
        __syncthreads();
        for (int j = tid; j < 3 * Hs; j += kDriveThreads) {
            float vi = b_ih[j], vh = b_hh[j];
            for (int k = 0; k < 6; ++k) vi = fmaf(w_ih[j * 6 + k], x[k], vi);
#pragma unroll 8
            for (int k = 0; k < Hs; ++k) vh = fmaf(whh_t[(size_t)k * 3 * Hs + j], h[k], vh);
            gi[j] = vi;
            gh[j] = vh;
        }
        __syncthreads();
        for (int j = tid; j < Hs; j += kDriveThreads) {    // torch.nn.GRUCell: gates r, z, n
            const float r = sigmoidf(gi[j] + gh[j]), z = sigmoidf(gi[Hs + j] + gh[Hs + j]);
            const float n = tanhf(gi[2 * Hs + j] + r * gh[2 * Hs + j]);
            h[j] = n + z * (h[j] - n);
        }
        __syncthreads();
        for (int j = tid; j < Hs; j += kDriveThreads) {
            float v = b1[j];
#pragma unroll 8
            for (int k = 0; k < Hs; ++k) v = fmaf(w1_t[(size_t)k * Hs + j], h[k], v);
            hid[j] = fmaxf(v, 0.f);
        }
        __syncthreads();
        if (tid < 128) {                                   // waves 0 and 1: the two output coordinates
            const int c = tid >> 6, l = tid & 63;
            float p = 0.f;
            for (int k = l; k < Hs; k += 64) p = fmaf(w2[c * Hs + k], hid[k], p);
            for (int m = 32; m > 0; m >>= 1) p += __shfl_xor(p, m);
            if (l == 0) {
                const float o = p + b2[c];
                x[6 + c] = o;
                final_traj[((size_t)b * d.T + t) * 3 + c] = o;
                if (c == 0) final_traj[((size_t)b * d.T + t) * 3 + 2] = 0.f;
            }
        }
        __syncthreads();
    }
}

bool valid(const stp3_plan_dims* p) {
    return p && p->B > 0 && p->N > 0 && p->T > 0 && p->H > 0 && p->W > 0 && p->K0 >= 0 && p->KL >= 0 && p->dx0 > 0.f &&
           p->dx1 > 0.f && p->lr_dist >= 0.f && (int64_t)p->B * p->N * p->T < (1LL << 31) &&
           (int64_t)p->B * p->T * p->H * p->W < (1LL << 31);
}

PlanDims convert(const stp3_plan_dims* p) {
    PlanDims d;
    d.B = p->B; d.N = p->N; d.T = p->T; d.H = p->H; d.W = p->W; d.K0 = p->K0; d.KL = p->KL;
    d.dx0 = p->dx0; d.dx1 = p->dx1; d.bx0 = p->bx0; d.bx1 = p->bx1;
    d.safety = p->safety; d.headway = p->headway; d.lrdivider = p->lrdivider; d.comfort = p->comfort;
    d.progress = p->progress; d.volume = p->volume; d.rule = p->rule;
    d.w0 = p->w0; d.w1 = p->w1; d.headway_dist = p->headway_dist; d.lr_dist = p->lr_dist;
    return d;
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // namespace

extern "C" {

int stp3_traj_cost_fwd(const stp3_plan_dims* p, const float* trajs, const float* cost_volume, const float* occupancy,
                       const float* drivable, const float* lane, const float* target, const float* target_sum,
                       const int32_t* footprint0, const int32_t* footprint_lambda, float* cost_fc, float* cost_fo,
                       int32_t* cv_cell, float* cv_scale, void* stream) {
    if (!valid(p) || !trajs || !cost_volume || !occupancy || !drivable || !lane || !target || !target_sum || !cost_fc ||
        !cost_fo || (p->K0 && !footprint0) || (p->KL && !footprint_lambda) || (!cv_cell != !cv_scale))
        return STP3_EINVAL;
    const int total = p->B * p->N * p->T;
    hipLaunchKernelGGL(traj_cost_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, convert(p), trajs,
                       cost_volume, occupancy, drivable, lane, target, target_sum, (const int2*)footprint0,
                       (const int2*)footprint_lambda, cost_fc, cost_fo, cv_cell, cv_scale);
    return status();
}

int stp3_traj_cost_bwd(const stp3_plan_dims* p, const float* grad_cost_fo, const int32_t* cv_cell, const float* cv_scale,
                       float* grad_cost_volume, void* stream) {
    if (!valid(p) || !grad_cost_fo || !cv_cell || !cv_scale || !grad_cost_volume) return STP3_EINVAL;
    const size_t lds = (size_t)p->N * 8;
    if (lds > 160 * 1024 || p->B > 65535 || p->N > 65535 * 256) return STP3_EUNSUP;   // 20 480 trajectories per sample
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&traj_cost_bwd_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return -(int)e;
    e = hipMemsetAsync(grad_cost_volume, 0, (size_t)p->B * p->T * p->H * p->W * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(traj_cost_bwd_kernel, dim3(p->T, p->B, (p->N + 255) / 256), dim3(256), lds, (hipStream_t)stream,
                       convert(p), grad_cost_fo, cv_cell, cv_scale, grad_cost_volume);
    return status();
}

int stp3_plan_scene(const stp3_scene_dims* p, const void* segmentation, const void* pedestrian, const void* hdmap,
                    float* occupancy, float* lane, float* drivable, void* stream) {
    if (!p || !segmentation || !hdmap || !occupancy || !lane || !drivable || p->B < 1 || p->S < 1 || p->T < 1 || p->H < 1 ||
        p->W < 1 || p->Cs < 1 || p->Cp < 0 || (p->Cp && !pedestrian) || p->first < 0 || (int64_t)p->first + p->T > p->S ||
        (int64_t)p->B * p->T * p->H * p->W >= (1LL << 31))
        return STP3_EINVAL;
    auto known = [](int dtype) { return dtype == STP3_DTYPE_F32 || dtype == STP3_DTYPE_BF16; };
    if (!known(p->seg_dtype) || (p->Cp && !known(p->ped_dtype)) || !known(p->hd_dtype)) return STP3_EUNSUP;
    if (p->B > 65535 || p->T + 1 > 65535) return STP3_EUNSUP;
    SceneDims d;
    d.B = p->B; d.T = p->T; d.H = p->H; d.W = p->W; d.Cs = p->Cs; d.Cp = p->Cp; d.first = p->first;
    d.seg_bf16 = p->seg_dtype == STP3_DTYPE_BF16; d.ped_bf16 = p->ped_dtype == STP3_DTYPE_BF16;
    d.hd_bf16 = p->hd_dtype == STP3_DTYPE_BF16;
    for (int i = 0; i < 5; ++i) { d.seg_st[i] = p->seg_stride[i]; d.ped_st[i] = p->ped_stride[i]; }
    for (int i = 0; i < 4; ++i) d.hd_st[i] = p->hd_stride[i];
    hipLaunchKernelGGL(plan_scene_kernel, dim3((p->H * p->W + 255) / 256, p->T + 1, p->B), dim3(256), 0, (hipStream_t)stream, d,
                       segmentation, pedestrian, hdmap, occupancy, lane, drivable);
    return status();
}

int stp3_plan_drive(const stp3_plan_dims* p, const stp3_drive_dims* q, const float* trajs, const void* cost_volume,
                    const float* occupancy, const float* drivable, const float* lane, const float* target,
                    const int32_t* command, const int32_t* footprint0, const int32_t* footprint_lambda, const void* h0,
                    float* final_traj, float* selected_traj, int32_t* selected_index, void* stream) {
    if (!valid(p) || !q || !trajs || !cost_volume || !occupancy || !drivable || !lane || !target || !command || !h0 ||
        !final_traj || !selected_traj || !selected_index || (p->K0 && !footprint0) || (p->KL && !footprint_lambda) ||
        !q->weights || p->N % 3 != 0 ||
        q->Hs < 1 || q->traj_cols < 2 || q->traj_point_stride < q->traj_cols || q->traj_row_stride < 0 ||
        q->traj_batch_stride < 0 || q->cv_batch_stride < 0)
        return STP3_EINVAL;
    if (q->traj_batch_stride >= (1LL << 31) || q->traj_row_stride >= (1LL << 31) || q->traj_point_stride >= (1LL << 31) ||
        q->cv_batch_stride >= (1LL << 31))
        return STP3_EUNSUP;
    auto known = [](int dtype) { return dtype == STP3_DTYPE_F32 || dtype == STP3_DTYPE_BF16; };
    if (!known(q->cv_dtype) || !known(q->h0_dtype)) return STP3_EUNSUP;
    if (q->Hs % 64 != 0 || q->Hs > 512 || p->B > 65535 || p->T * 3 > kDriveThreads) return STP3_EUNSUP;
    const size_t lds = ((size_t)p->N * (p->T + 1) + 2 * kDriveThreads + 8 * (size_t)q->Hs + 8) * sizeof(float);
    if (lds + 128 > 160 * 1024) return STP3_EUNSUP;      // (+ the kernel's static constants)
    // the dynamic-LDS limit of the kernel, raised ONCE per device to the largest size this entry accepts: the first call on a
    // device is an eager one (the engine warms up before it captures), so the attribute is never set inside a stream capture
    static std::atomic<bool> granted[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return -(int)e;
    if (dev < 0 || dev >= 64) return STP3_EUNSUP;
    if (!granted[dev].load()) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&plan_drive_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 128);
        if (e != hipSuccess) return -(int)e;
        granted[dev].store(true);
    }
    DriveArgs a;
    a.Hs = q->Hs; a.cols = q->traj_cols < 3 ? q->traj_cols : 3;
    a.cv_bf16 = q->cv_dtype == STP3_DTYPE_BF16; a.h0_bf16 = q->h0_dtype == STP3_DTYPE_BF16;
    a.traj_b = (int)q->traj_batch_stride; a.traj_n = (int)q->traj_row_stride; a.traj_t = (int)q->traj_point_stride;
    a.cv_b = (int)q->cv_batch_stride;
    a.weights = q->weights;
    hipLaunchKernelGGL(plan_drive_kernel, dim3(p->B), dim3(kDriveThreads), lds, (hipStream_t)stream, convert(p), a, trajs,
                       cost_volume, occupancy, drivable, lane, target, command, (const int2*)footprint0,
                       (const int2*)footprint_lambda, h0, final_traj, selected_traj, selected_index);
    return status();
}

}  // extern "C"
