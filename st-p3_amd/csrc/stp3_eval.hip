// Evaluation scorer (include/stp3_hip.h: stp3_eval_semantic, stp3_eval_planning, stp3_eval_panoptic): the metric updates of
// the reference's evaluation loop (evaluate.py:95-137 with stp3/metrics.py) as launches that a hipGraph can hold.
//   stp3_eval_semantic   arg-max of the segmentation / pedestrian / hd-map logits and the tp / fp / fn / support counts of
//                        IntersectionOverUnion.update, all heads in one launch
//   stp3_eval_planning   PlanningMetric.update: L2, point and box collisions per future step, one workgroup
//   stp3_eval_panoptic   PanopticMetric.update: one workgroup per sample with the loop over its frames inside, then a
//                        one-workgroup launch that adds the frames in update order into the state
// Everything that is accumulated by atomics is an integer, so the results do not depend on the order of the additions; the
// float sums (IoU of the matched segments, L2) are added by ONE thread in the reference's order.  Every loop has a bound
// known before it starts; an input that breaks the panoptic contract sets a word of `err` and the kernel runs to its end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_hip.h"

namespace {

constexpr int kMaxSide = 1024;

// element i of a float32 or bf16 tensor, in float32
__device__ __forceinline__ float logit_at(const void* __restrict__ p, long long i, int bf16) {
    if (bf16) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(p)[i] << 16);
    return reinterpret_cast<const float*>(p)[i];
}

// torch.argmax over C classes: the FIRST maximal class wins a tie, a NaN counts as the maximum (the first NaN stays)
__device__ __forceinline__ int argmax_class(const void* __restrict__ p, long long base, long long cstride, int C, int bf16) {
    float bv = logit_at(p, base, bf16);
    int best = 0;
    for (int c = 1; c < C; ++c) {
        const float v = logit_at(p, base + c * cstride, bf16);
        if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
    }
    return best;
}

// ----------------------------------------------------------------------------------------------------------------------
// semantic heads
// ----------------------------------------------------------------------------------------------------------------------
constexpr int kSemThreads = 256;
constexpr int kSemPerThread = 8;
constexpr int kSemTile = kSemThreads * kSemPerThread;     // pixels of one plane per workgroup
constexpr int kMaxClasses = 8;
constexpr int kMaxLogits = 16;

struct SemDims {
    int B, S, H, W, Cs, Cp, E, n, first, seg_bf16, ped_bf16, hd_bf16;
    long long seg_st[5], ped_st[5], hd_st[4];
};

// grid (tiles of a plane, planes): planes = B (S - first) frames of the segmentation head, the same of the pedestrian head
// (Cp > 0), B E hd-map elements.  counts[head][class][tp, fp, fn, support] += ...
__global__ __launch_bounds__(kSemThreads) void semantic_kernel(SemDims d, const void* __restrict__ seg, const void* __restrict__ ped,
                                                               const void* __restrict__ hd, const long long* __restrict__ seg_label,
                                                               const long long* __restrict__ ped_label,
                                                               const long long* __restrict__ hd_label,
                                                               unsigned long long* __restrict__ counts) {
    __shared__ int s_cnt[kMaxClasses * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int P = d.H * d.W, Sf = d.S - d.first, frames = d.B * Sf;
    int plane = blockIdx.y, head, C, bf16;
    const void* logits;
    const long long* label;
    long long base, cstride, rstride, xstride;
    if (plane < frames || (d.Cp > 0 && plane < 2 * frames)) {
        const bool is_ped = plane >= frames;
        if (is_ped) plane -= frames;
        const int b = plane / Sf, s = d.first + plane % Sf;
        const long long* st = is_ped ? d.ped_st : d.seg_st;
        head = is_ped ? 1 : 0;
        C = is_ped ? d.Cp : d.Cs;
        bf16 = is_ped ? d.ped_bf16 : d.seg_bf16;
        logits = is_ped ? ped : seg;
        label = (is_ped ? ped_label : seg_label) + ((size_t)b * d.S + s) * P;
        base = b * st[0] + s * st[1];
        cstride = st[2]; rstride = st[3]; xstride = st[4];
    } else {
        plane -= d.Cp > 0 ? 2 * frames : frames;
        const int b = plane / d.E, e = plane % d.E;
        head = 2 + e;
        C = 2;
        bf16 = d.hd_bf16;
        logits = hd;
        label = hd_label + ((size_t)b * d.E + e) * P;
        base = b * d.hd_st[0] + 2 * e * d.hd_st[1];
        cstride = d.hd_st[1]; rstride = d.hd_st[2]; xstride = d.hd_st[3];
    }
    if (tid < kMaxClasses * 3) s_cnt[tid] = 0;
    __syncthreads();

    int mine = 0;                                 // lane 3 c + k keeps counter k (tp, fp, fn) of class c of this wave
#pragma unroll 1
    for (int it = 0; it < kSemPerThread; ++it) {  // (the trip count is the same for every thread: the ballots below need it)
        const int p = blockIdx.x * kSemTile + it * kSemThreads + tid;
        const bool valid = p < P;
        int pred = -1;
        long long tgt = -1;
        if (valid) {
            const int r = p / d.W, x = p - r * d.W;
            pred = argmax_class(logits, base + r * rstride + x * xstride, cstride, C, bf16);
            tgt = label[p];
        }
#pragma unroll 1
        for (int c = 0; c < d.n; ++c) {           // metrics.py:37-43: a label outside [0, n) is no class of its own ...
            const bool is_p = valid && pred == c, is_t = valid && tgt == (long long)c;
            const int tp = __popcll(__ballot(is_p && is_t));
            const int fp = __popcll(__ballot(is_p && !is_t));         // ... but makes the other side's class a false positive
            const int fn = __popcll(__ballot(is_t && !is_p));         // ... or a false negative
            const int k = lane - 3 * c;
            mine += k == 0 ? tp : k == 1 ? fp : k == 2 ? fn : 0;
        }
    }
    if (lane < 3 * d.n && mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    if (tid < d.n * 4) {                          // one 64-bit atomic per counter per workgroup
        const int c = tid >> 2, k = tid & 3;
        const int v = k < 3 ? s_cnt[c * 3 + k] : s_cnt[c * 3 + 0] + s_cnt[c * 3 + 2];     // support = tp + fn
        if (v) atomicAdd(&counts[((size_t)head * d.n + c) * 4 + k], (unsigned long long)v);
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// planning
// ----------------------------------------------------------------------------------------------------------------------
constexpr int kPlanThreads = 1024;

struct PlanEvalDims {
    int B, T, S, H, W, K, first;
    float dx0, dx1, bx0, bx1;
    long long traj_st[2], gt_st[2];
};

// torch: x.to(int) then clamp(0, n - 1).  Values beyond the integer range (and NaN) end up at a clamp bound either way.
__device__ __forceinline__ int cell_of(float v, int n) {
    if (!(v > -1.0f)) return 0;                   // trunc(v) <= 0, or NaN
    if (v >= (float)n) return n - 1;
    return (int)v;                                // truncation toward zero
}

__device__ __forceinline__ bool occupied(const long long* __restrict__ seg, const long long* __restrict__ ped, int cell) {
    return seg[cell] != 0 || (ped && ped[cell] != 0);
}

// PlanningMetric.box_collisions (metrics.py:89-97): does the ego box at the flipped point (x, y) touch an occupied cell
__device__ __forceinline__ bool box_collides(const PlanEvalDims& d, const int2* __restrict__ rc, const long long* __restrict__ seg,
                                             const long long* __restrict__ ped, float x, float y) {
    const float fy = y / d.dx0, fx = x / d.dx1;
    bool any = false;
    for (int k = 0; k < d.K; ++k) {
        const int2 o = rc[k];
        const int r = cell_of(fy + (float)o.x, d.H), c = cell_of(fx + (float)o.y, d.W);
        any = any || occupied(seg, ped, r * d.W + c);
    }
    return any;
}

__global__ __launch_bounds__(kPlanThreads) void planning_kernel(PlanEvalDims d, const float* __restrict__ trajs,
                                                                const float* __restrict__ gt_trajs,
                                                                const long long* __restrict__ seg_label,
                                                                const long long* __restrict__ ped_label,
                                                                const int2* __restrict__ footprint, long long* __restrict__ obj_col,
                                                                long long* __restrict__ obj_box_col, long long* __restrict__ total,
                                                                double* __restrict__ l2) {
    __shared__ float s_l2[kPlanThreads];
    __shared__ unsigned char s_col[kPlanThreads], s_box[kPlanThreads];
    const int tid = threadIdx.x, n = d.B * d.T;
    if (tid < n) {
        const int b = tid / d.T, t = tid - b * d.T;
        const float* pt = trajs + b * d.traj_st[0] + t * d.traj_st[1];
        const float* gt = gt_trajs + b * d.gt_st[0] + t * d.gt_st[1];
        const float px = pt[0], py = pt[1], gx = gt[0], gy = gt[1];
        const float ex = px - gx, ey = py - gy;
        s_l2[tid] = sqrtf(ex * ex + ey * ey);     // metrics.py:103
        const size_t plane = ((size_t)b * d.S + d.first + t) * d.H * d.W;
        const long long* seg = seg_label + plane;
        const long long* ped = ped_label ? ped_label + plane : nullptr;
        const float fx = -px, fgx = -gx;          // the x flip (:104-105)
        const bool clean = !box_collides(d, footprint, seg, ped, fgx, gy);
        const float vy = (py - d.bx0) / d.dx0, vx = (fx - d.bx1) / d.dx1;             // :107-108, .long() truncates
        const bool inside = vy > -1.0f && vy < (float)d.H && vx > -1.0f && vx < (float)d.W;
        const bool hit = occupied(seg, ped, cell_of(vy, d.H) * d.W + cell_of(vx, d.W));
        s_col[tid] = hit && inside && clean;
        s_box[tid] = box_collides(d, footprint, seg, ped, fx, py) && clean;
    }
    __syncthreads();
    if (tid < d.T) {                              // one thread per step, the samples in ascending order
        double sum = l2[tid];
        long long col = 0, box = 0;
        for (int b = 0; b < d.B; ++b) {
            sum += (double)s_l2[b * d.T + tid];
            col += s_col[b * d.T + tid];
            box += s_box[b * d.T + tid];
        }
        l2[tid] = sum;
        obj_col[tid] += col;
        obj_box_col[tid] += box;
    }
    if (tid == 0) total[0] += d.B;
}

// ----------------------------------------------------------------------------------------------------------------------
// panoptic
// ----------------------------------------------------------------------------------------------------------------------
constexpr int kPanThreads = 1024;
constexpr int kPairs = STP3_EVAL_PANOPTIC_PAIRS;  // rows of the pair table of one frame; one thread per row
constexpr int kSlots = 2 * kPairs;                // hash slots
constexpr int kLast = kPairs;                     // entries of the last_match table of a sample
constexpr int kIdLimit = 1 << 20;
constexpr unsigned long long kEmpty = ~0ull;

enum { kErrIds = 0, kErrNoBackground = 1, kErrTable = 2 };

__device__ __forceinline__ int id_at(const void* __restrict__ p, size_t i, int wide) {
    const long long v = wide ? reinterpret_cast<const long long*>(p)[i] : (long long)reinterpret_cast<const int*>(p)[i];
    return (v < 0 || v >= kIdLimit) ? -1 : (int)v;
}

// workspace: float frames[B * Sf][8] (iou, tp, fp, fn of class 0 and 1, interleaved as [4][2]), then int has_background[B]
__global__ __launch_bounds__(kPanThreads) void panoptic_kernel(int S, int H, int W, int first, int consistent, int wide,
                                                               const void* __restrict__ pred, const void* __restrict__ gt,
                                                               float* __restrict__ frames, int* __restrict__ has_background,
                                                               int* __restrict__ err) {
    __shared__ unsigned long long s_key[kSlots];  // gt id << 20 | predicted id
    __shared__ int s_count[kSlots];               // pixels of the slot's pair; also the claim: the first to add owns the slot
    __shared__ int s_g[kPairs], s_p[kPairs], s_n[kPairs];
    __shared__ float s_iou[kPairs];               // IoU of the true positives of class 1 by rank, 0 elsewhere
    __shared__ unsigned char s_cand[kPairs];
    __shared__ int s_last_g[kLast], s_last_p[kLast];
    __shared__ int s_wait[3], s_over[3];
    __shared__ int s_rows, s_bg, s_pairs, s_nlast, s_tp[2], s_fp, s_fn, s_hasbg, s_err[4];
    __shared__ float s_iou0;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int P = H * W, Sf = S - first, chunks = (P + kPanThreads - 1) / kPanThreads;
    volatile unsigned long long* key = s_key;
    if (tid < 3) { s_wait[tid] = 0; s_over[tid] = 0; }
    if (tid < 4) s_err[tid] = 0;
    if (tid == 0) { s_nlast = 0; s_hasbg = 0; }
    int round = 0;                                // counts the votes of the whole kernel: the same value in every thread

    for (int f = 0; f < Sf; ++f) {
        for (int k = tid; k < kSlots; k += kPanThreads) { s_key[k] = kEmpty; s_count[k] = 0; }
        if (tid == 0) { s_rows = 0; s_bg = 0; s_pairs = 0; s_tp[0] = 0; s_tp[1] = 0; s_fp = 0; s_fn = 0; s_iou0 = 0.0f; }
        __syncthreads();
        const size_t at = ((size_t)b * S + first + f) * P;

        // ---- the distinct (gt id, predicted id) pairs with their pixel counts: an LDS hash, integer adds only ----
        int bg = 0;                               // (background, background) pixels seen by this wave
        bool overflow = false;
#pragma unroll 1
        for (int ch = 0; ch < chunks && !overflow; ++ch) {
            const int px = ch * kPanThreads + tid;
            int g = 0, p = 0;
            if (px < P) {
                g = id_at(gt, at + px, wide);
                p = id_at(pred, at + px, wide);
                if (g < 0 || p < 0) { s_err[kErrIds] = 1; g = g < 0 ? 0 : g; p = p < 0 ? 0 : p; }
            }
            const bool both_bg = px < P && g == 0 && p == 0;
            bg += __popcll(__ballot(both_bg));
            const unsigned long long mine = ((unsigned long long)g << 20) | (unsigned long long)p;
            unsigned h = ((unsigned)g * 2654435761u + (unsigned)p * 40503u) >> 7 & (kSlots - 1);
            // 0: looking for a slot, 1: added to a slot whose key is not visible yet, 2: done
            int state = (px < P && !both_bg) ? 0 : 2;
            for (;;) {
                while (state == 0) {
                    const unsigned long long k = key[h];
                    if (k == mine) { atomicAdd(&s_count[h], 1); state = 2; }
                    else if (k != kEmpty) h = (h + 1) & (kSlots - 1);
                    else if (atomicAdd(&s_count[h], 1) == 0) {                  // the slot is this thread's
                        key[h] = mine;
                        if (atomicAdd(&s_pairs, 1) >= kPairs - 1) s_over[round % 3] = 1;
                        state = 2;
                    } else state = 1;             // its owner publishes the key before the next barrier
                }
                if (state == 1) s_wait[round % 3] = 1;
                if (tid == 0) { s_wait[(round + 1) % 3] = 0; s_over[(round + 1) % 3] = 0; }
                __syncthreads();
                const bool again = s_wait[round % 3] != 0;
                overflow = s_over[round % 3] != 0;
                ++round;
                if (overflow || !again) break;
                if (state == 1) {
                    if (key[h] == mine) state = 2;                              // (already counted)
                    else { atomicAdd(&s_count[h], -1); h = (h + 1) & (kSlots - 1); state = 0; }
                }
            }
        }
        if (lane == 0 && bg) atomicAdd(&s_bg, bg);
        if (overflow && tid == 0) s_err[kErrTable] = 1;
        __syncthreads();
        // ---- the table's rows, one per thread (their order does not matter: every row finds its own rank) ----
        if (!overflow)
            for (int k = tid; k < kSlots; k += kPanThreads)
                if (s_count[k] > 0) {
                    const int i = atomicAdd(&s_rows, 1);
                    const unsigned long long kk = s_key[k];
                    s_g[i] = (int)(kk >> 20); s_p[i] = (int)(kk & (kIdLimit - 1)); s_n[i] = s_count[k];
                }
        __syncthreads();
        if (tid == 0 && !overflow && s_bg > 0) { const int i = s_rows; s_g[i] = 0; s_p[i] = 0; s_n[i] = s_bg; s_rows = i + 1; }
        __syncthreads();
        const int m = overflow ? 0 : s_rows;      // <= kPairs
        const bool row = tid < m;
        const int g = row ? s_g[tid] : 0, p = row ? s_p[tid] : 0, n = row ? s_n[tid] : 0;
        int rank = 0;
        bool first_g = true, first_p = true, cand = false;
        float iou = 0.0f;
        if (row) {
            int area_g = 0, area_p = 0;
#pragma unroll 1
            for (int j = 0; j < m; ++j) {
                const int gj = s_g[j], pj = s_p[j], nj = s_n[j];
                const bool before = gj < g || (gj == g && pj < p);
                if (gj == g) { area_g += nj; if (before) first_g = false; }
                if (pj == p) { area_p += nj; if (before) first_p = false; }
                rank += before;
            }
            iou = ((float)n + 1e-9f) / ((float)(area_g + area_p - n) + 1e-9f);      // metrics.py:195
            cand = iou > 0.5f && (g == 0) == (p == 0);
            s_cand[tid] = cand;
            s_iou[tid] = 0.0f;
            if (g == 0) s_hasbg = 1;
        }
        __syncthreads();
        // ---- matches (IoU > 0.5: at most one per id on either side, so the rows decide independently) ----
        int known = -1;                           // this gt id's entry of last_match
        if (row) {
            bool matched_g = false, matched_p = false;
#pragma unroll 1
            for (int j = 0; j < m; ++j)
                if (s_cand[j]) {
                    if (s_g[j] == g) matched_g = true;
                    if (s_p[j] == p) matched_p = true;
                }
            if (first_g && g > 0 && !matched_g) atomicAdd(&s_fn, 1);            // :209
            if (first_p && p > 0 && !matched_p) atomicAdd(&s_fp, 1);            // :210
            if (cand && g > 0 && consistent) {
                const int nlast = s_nlast;
#pragma unroll 1
                for (int k = 0; k < nlast; ++k)
                    if (s_last_g[k] == g) known = k;
            }
        }
        __syncthreads();
        if (cand) {
            const int cls = g == 0 ? 0 : 1;
            bool counted = true;
            if (cls == 1 && consistent) {
                if (known >= 0) {
                    if (s_last_p[known] != p) { atomicAdd(&s_fn, 1); atomicAdd(&s_fp, 1); s_last_p[known] = p; counted = false; }   // :201-205
                } else {
                    const int k = atomicAdd(&s_nlast, 1);
                    if (k < kLast) { s_last_g[k] = g; s_last_p[k] = p; }
                    else s_err[kErrTable] = 1;
                }
            }
            if (counted) {
                atomicAdd(&s_tp[cls], 1);
                if (cls == 0) s_iou0 = iou;       // (the only row of class 0 that can match)
                else s_iou[rank] = iou;
            }
        }
        __syncthreads();
        if (tid == 0) {
            if (s_nlast > kLast) s_nlast = kLast;
            float sum = 0.0f;                     // the reference's order: ascending (gt id, predicted id)
#pragma unroll 1
            for (int j = 0; j < m; ++j) sum += s_iou[j];
            float* out = frames + ((size_t)b * Sf + f) * 8;
            out[0] = s_iou0; out[1] = sum;
            out[2] = (float)s_tp[0]; out[3] = (float)s_tp[1];
            out[4] = 0.0f; out[5] = (float)s_fp;
            out[6] = 0.0f; out[7] = (float)s_fn;
        }
        __syncthreads();
    }
    if (tid == 0) has_background[b] = s_hasbg;
    if (tid < 4 && s_err[tid]) err[tid] = 1;      // (every writer stores the same value)
}

// state[4][2] += the frames added in update order (sample-major, frame ascending) into a zero total: PanopticMetric.update
__global__ __launch_bounds__(64) void panoptic_finish_kernel(int B, int nframes, const float* __restrict__ frames,
                                                             const int* __restrict__ has_background, float* __restrict__ state,
                                                             int* __restrict__ err) {
    const int tid = threadIdx.x;
    if (tid < 8) {
        float total = 0.0f;
        for (int f = 0; f < nframes; ++f) total += frames[(size_t)f * 8 + tid];
        state[tid] += total;
    } else if (tid == 8) {
        int any = 0;
        for (int b = 0; b < B; ++b) any |= has_background[b];
        if (!any) err[kErrNoBackground] = 1;
    }
}

bool known_dtype(int dtype) { return dtype == STP3_DTYPE_F32 || dtype == STP3_DTYPE_BF16; }

bool strides_fit(const int64_t* st, int n) {
    for (int k = 0; k < n; ++k)
        if (st[k] < 0 || st[k] >= (1ll << 31)) return false;
    return true;
}

}  // namespace

extern "C" {

int stp3_eval_semantic(const stp3_eval_dims* p, const void* segmentation, const void* pedestrian, const void* hdmap,
                       const int64_t* segmentation_label, const int64_t* pedestrian_label, const int64_t* hdmap_label,
                       int64_t* counts, void* stream) {
    if (!p || !segmentation || !segmentation_label || !counts) return STP3_EINVAL;
    if (p->B < 1 || p->S < 1 || p->H < 1 || p->W < 1 || p->Cs < 1 || p->Cp < 0 || p->E < 0 || p->n_classes < 1) return STP3_EINVAL;
    if (p->first < 0 || p->first >= p->S) return STP3_EINVAL;
    if ((p->Cp > 0) != (pedestrian != nullptr) || (p->Cp > 0) != (pedestrian_label != nullptr)) return STP3_EINVAL;
    if ((p->E > 0) != (hdmap != nullptr) || (p->E > 0) != (hdmap_label != nullptr)) return STP3_EINVAL;
    if (p->Cs > kMaxLogits || p->Cp > kMaxLogits || p->n_classes > kMaxClasses) return STP3_EUNSUP;
    if (p->H > kMaxSide || p->W > kMaxSide || (int64_t)p->H * p->W >= (1 << 24)) return STP3_EUNSUP;
    if (!known_dtype(p->seg_dtype) || (p->Cp > 0 && !known_dtype(p->ped_dtype)) || (p->E > 0 && !known_dtype(p->hd_dtype)))
        return STP3_EUNSUP;
    if (!strides_fit(p->seg_stride, 5) || (p->Cp > 0 && !strides_fit(p->ped_stride, 5)) || (p->E > 0 && !strides_fit(p->hd_stride, 4)))
        return STP3_EUNSUP;
    const int64_t frames = (int64_t)p->B * (p->S - p->first);
    const int64_t planes = frames * (p->Cp > 0 ? 2 : 1) + (int64_t)p->B * p->E;
    if (planes > 65535) return STP3_EUNSUP;
    SemDims d;
    d.B = p->B; d.S = p->S; d.H = p->H; d.W = p->W; d.Cs = p->Cs; d.Cp = p->Cp; d.E = p->E; d.n = p->n_classes; d.first = p->first;
    d.seg_bf16 = p->seg_dtype == STP3_DTYPE_BF16; d.ped_bf16 = p->ped_dtype == STP3_DTYPE_BF16; d.hd_bf16 = p->hd_dtype == STP3_DTYPE_BF16;
    for (int k = 0; k < 5; ++k) { d.seg_st[k] = p->seg_stride[k]; d.ped_st[k] = p->Cp > 0 ? p->ped_stride[k] : 0; }
    for (int k = 0; k < 4; ++k) d.hd_st[k] = p->E > 0 ? p->hd_stride[k] : 0;
    const int tiles = (p->H * p->W + kSemTile - 1) / kSemTile;
    hipLaunchKernelGGL(semantic_kernel, dim3(tiles, (unsigned)planes), dim3(kSemThreads), 0, (hipStream_t)stream, d, segmentation,
                       pedestrian, hdmap, (const long long*)segmentation_label, (const long long*)pedestrian_label,
                       (const long long*)hdmap_label, (unsigned long long*)counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

int stp3_eval_planning(const stp3_eval_plan_dims* p, const float* trajs, const float* gt_trajs, const int64_t* segmentation_label,
                       const int64_t* pedestrian_label, const int32_t* footprint, int64_t* obj_col, int64_t* obj_box_col,
                       int64_t* total, double* l2, void* stream) {
    if (!p || !trajs || !gt_trajs || !segmentation_label || !footprint || !obj_col || !obj_box_col || !total || !l2) return STP3_EINVAL;
    if (p->B < 1 || p->T < 1 || p->S < 1 || p->H < 1 || p->W < 1 || p->K < 1) return STP3_EINVAL;
    if (p->first_future < 0 || (int64_t)p->first_future + p->T > p->S) return STP3_EINVAL;
    if (!(p->dx0 > 0.0f) || !(p->dx1 > 0.0f)) return STP3_EINVAL;
    for (int k = 0; k < 2; ++k)
        if (p->traj_stride[k] < 0 || p->gt_stride[k] < 0) return STP3_EINVAL;
    if ((int64_t)p->B * p->T > kPlanThreads) return STP3_EUNSUP;
    if (p->H > kMaxSide || p->W > kMaxSide || (int64_t)p->H * p->W >= (1 << 24)) return STP3_EUNSUP;
    PlanEvalDims d;
    d.B = p->B; d.T = p->T; d.S = p->S; d.H = p->H; d.W = p->W; d.K = p->K; d.first = p->first_future;
    d.dx0 = p->dx0; d.dx1 = p->dx1; d.bx0 = p->bx0; d.bx1 = p->bx1;
    for (int k = 0; k < 2; ++k) { d.traj_st[k] = p->traj_stride[k]; d.gt_st[k] = p->gt_stride[k]; }
    hipLaunchKernelGGL(planning_kernel, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, d, trajs, gt_trajs,
                       (const long long*)segmentation_label, (const long long*)pedestrian_label, (const int2*)footprint,
                       (long long*)obj_col, (long long*)obj_box_col, (long long*)total, l2);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

int stp3_eval_panoptic_workspace_bytes(int32_t B, int32_t S, int32_t first, size_t* bytes) {
    if (!bytes || B < 1 || S < 1 || first < 0 || first >= S) return STP3_EINVAL;
    *bytes = (size_t)B * (S - first) * 8 * sizeof(float) + (size_t)B * sizeof(int32_t);
    return STP3_OK;
}

int stp3_eval_panoptic(int32_t B, int32_t S, int32_t H, int32_t W, int32_t first, int32_t temporally_consistent, int32_t wide_ids,
                       const void* pred, const void* gt, void* workspace, size_t workspace_bytes, float* state, int32_t* err,
                       void* stream) {
    size_t need = 0;
    if (B < 1 || S < 1 || H < 1 || W < 1 || !pred || !gt || !workspace || !state || !err) return STP3_EINVAL;
    if (stp3_eval_panoptic_workspace_bytes(B, S, first, &need) != STP3_OK) return STP3_EINVAL;
    if (H > kMaxSide || W > kMaxSide || (int64_t)H * W >= (1 << 24) || B > 65535) return STP3_EUNSUP;
    if (workspace_bytes < need) return STP3_ENOSPACE;
    float* frames = (float*)workspace;
    int* has_background = (int*)(frames + (size_t)B * (S - first) * 8);
    hipLaunchKernelGGL(panoptic_kernel, dim3(B), dim3(kPanThreads), 0, (hipStream_t)stream, S, H, W, first,
                       temporally_consistent != 0, wide_ids != 0, pred, gt, frames, has_background, err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(panoptic_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, B, B * (S - first), (const float*)frames,
                       (const int*)has_background, state, err);
    e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
