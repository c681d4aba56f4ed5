// Vehicle instance post-processing (stp3/utils/instance.py:80-269 of the reference) for a whole batch:
//   stp3_instance_segment   centerness / offset / foreground of N = B * S frames -> instance ids, one workgroup per frame
//   stp3_instance_track     raw ids + flow of B samples -> temporally consistent ids, one workgroup per sample, the loop over
//                           time inside the kernel
// The rules (what counts as a centre, which distance is compared, how ids are renumbered and handed out) are written down in
// include/stp3_hip.h and, as torch code, in stp3_amd/instance.py; the two are compared bit for bit by the tests.
// Everything that is accumulated is an integer (pixel coordinates, the flow in 2^-20 fixed point), so LDS atomics give the
// same sums in any order.  Every loop has a bound known before it starts; when one is hit, or an input breaks the
// contract, a word of `err` is set and the kernel runs on to its end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_hip.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = 100;                        // max_n_instance_centers (instance.py:122)
constexpr int kMaxSide = 1024;
constexpr float kFlowScale = 1048576.0f;          // 2^20
constexpr float kFlowLimit = 32768.0f;

enum { kErrBound = 0, kErrIds = 1, kErrNoBackground = 2, kErrFlow = 3 };

// F.threshold(x, thr, -1): x <= thr ? -1 : x (a NaN stays a NaN)
__device__ __forceinline__ float thresholded(float x, float thr) { return x <= thr ? -1.0f : x; }

__global__ __launch_bounds__(kThreads) void segment_kernel(int H, int W, float thr, const float* __restrict__ center,
                                                           const float* __restrict__ offset,
                                                           const uint8_t* __restrict__ foreground, int* __restrict__ seg,
                                                           int* __restrict__ centers, int* __restrict__ counts) {
    __shared__ int s_cr[kMaxC], s_cc[kMaxC];
    __shared__ int s_wave[kWaves];
    __shared__ int s_present[kMaxC + 1], s_rank[kMaxC + 1];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = H * W;
    const float* cen = center + (size_t)f * P;
    const float* off = offset + (size_t)f * 2 * P;
    const uint8_t* fg = foreground + (size_t)f * P;
    int* out = seg + (size_t)f * P;
    if (tid <= kMaxC) s_present[tid] = 0;
    __syncthreads();

    // ---- centres: row-major order, the first kMaxC (instance.py:80-91, 134-136) ----
    int base = 0;                                 // candidates before this chunk: the same value in every thread
    const int chunks = (P + kThreads - 1) / kThreads;
    for (int ch = 0; ch < chunks && base < kMaxC; ++ch) {
        const int p = ch * kThreads + tid;
        const int r = p / W, c = p - r * W;
        bool cand = false;
        if (p < P) {
            const float t = thresholded(cen[p], thr);
            if (t > 0.0f) {
                float m = t;
                bool nan = false;
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc) {
                        const int rr = r + dr, cc = c + dc;
                        if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
                        const float v = thresholded(cen[rr * W + cc], thr);
                        if (v != v) nan = true;
                        else if (v > m) m = v;
                    }
                cand = !nan && t == m;
            }
        }
        const unsigned long long votes = __ballot(cand);
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            const int n = s_wave[w];
            if (w < wave) before += n;
            total += n;
        }
        if (cand) {
            const int k = before + __popcll(votes & ((1ull << lane) - 1ull));
            if (k < kMaxC) { s_cr[k] = r; s_cc[k] = c; }
        }
        base += total;
        __syncthreads();
    }
    const int K = base < kMaxC ? base : kMaxC;
    if (tid < kMaxC) {
        centers[((size_t)f * kMaxC + tid) * 2] = tid < K ? s_cr[tid] : 0;
        centers[((size_t)f * kMaxC + tid) * 2 + 1] = tid < K ? s_cc[tid] : 0;
    }
    if (tid == 0) counts[f] = K;
    if (K == 0) {                                 // instance.py:130-132
        for (int p = tid; p < P; p += kThreads) out[p] = 0;
        return;
    }

    // ---- nearest centre of pixel + offset, float32 sqrt(dr * dr + dc * dc), lowest k on equal values (:94-113, :139) ----
    for (int p = tid; p < P; p += kThreads) {
        const int r = p / W, c = p - r * W;
        const float lr = (float)r + off[p], lc = (float)c + off[P + p];
        float best = 0.0f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float dr = (float)s_cr[k] - lr, dc = (float)s_cc[k] - lc;
            const float d = sqrtf(dr * dr + dc * dc);
            if (k == 0 || d < best) { best = d; arg = k; }
        }
        const int id = fg[p] ? arg + 1 : 0;
        out[p] = id;
        s_present[id] = 1;                        // (every writer stores the same value)
    }
    __syncthreads();
    // ---- make_instance_seg_consecutive (:165-170): the rank among the distinct values of the masked map ----
    if (tid <= kMaxC) {
        int below = 0;
        for (int v = 0; v <= tid; ++v) below += s_present[v];
        s_rank[tid] = below - 1;                  // (only read for present values: >= 0)
    }
    __syncthreads();
    for (int p = tid; p < P; p += kThreads) out[p] = s_rank[out[p]];      // (each thread re-reads its own stores)
}

// ----------------------------------------------------------------------------------------------------------------------
// tracking
// ----------------------------------------------------------------------------------------------------------------------
struct FrameStats {                               // keyed by the raw id 0..kMaxC of a frame
    int cnt[kMaxC + 1];
    unsigned long long sr[kMaxC + 1], sc[kMaxC + 1], fr[kMaxC + 1], fc[kMaxC + 1];      // two's complement sums
};

struct Solver {                                   // stp3_amd.instance.lsap, the same names
    double u[kMaxC], v[kMaxC], spc[kMaxC];
    int path[kMaxC], col4row[kMaxC], row4col[kMaxC], rem[kMaxC];
    unsigned char in_sr[kMaxC], in_sc[kMaxC];
};

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

// Minimum-cost assignment of dist[nrows][ncols] (row stride kMaxC) by ONE wave, lanes across the columns of the problem
// after the smaller side has been made its rows.  Afterwards col4row[i] (i < min side) is the partner on the larger side or
// -1.  Returns false when a bound was hit.
__device__ bool assign(Solver& s, const float* dist, int nrows, int ncols, int lane) {
    const bool transposed = ncols < nrows;
    const int nr = transposed ? ncols : nrows, nc = transposed ? nrows : ncols;
    for (int k = lane; k < kMaxC; k += 64) {
        s.u[k] = 0.0; s.v[k] = 0.0; s.col4row[k] = -1; s.row4col[k] = -1;
    }
    wave_sync();
    bool ok = true;
    for (int cur = 0; cur < nr && ok; ++cur) {
        for (int k = lane; k < nc; k += 64) {
            s.spc[k] = __builtin_inf(); s.path[k] = -1; s.rem[k] = nc - 1 - k; s.in_sc[k] = 0;
        }
        for (int k = lane; k < nr; k += 64) s.in_sr[k] = 0;
        wave_sync();
        double min_val = 0.0;
        int i = cur, sink = -1, nrem = nc;
        for (int step = 0; step < nc && sink < 0; ++step) {
            if (lane == 0) s.in_sr[i] = 1;
            const double ui = s.u[i];
            double best = __builtin_inf();
            int key = -1;                         // position << 1 | unassigned; -1: nothing yet
            for (int it = lane; it < nrem; it += 64) {
                const int j = s.rem[it];
                const double c = (double)(transposed ? dist[j * kMaxC + i] : dist[i * kMaxC + j]);
                const double r = min_val + c - ui - s.v[j];
                if (r < s.spc[j]) { s.spc[j] = r; s.path[j] = i; }
                const double val = s.spc[j];
                const int unassigned = s.row4col[j] < 0 ? 1 : 0;
                if (key < 0 || val < best || (val == best && unassigned)) { best = val; key = (it << 1) | unassigned; }
            }
            // the sequential scan's choice: the lowest value; among equals the LAST unassigned column, else the FIRST
#pragma unroll 1
            for (int m = 1; m < 64; m <<= 1) {
                const double ob = __shfl_xor(best, m);
                const int ok2 = __shfl_xor(key, m);
                bool take = false;
                if (ok2 >= 0) {
                    if (key < 0 || ob < best) take = true;
                    else if (ob == best) {
                        const int mine = key & 1, theirs = ok2 & 1;
                        if (theirs != mine) take = theirs == 1;
                        else take = theirs ? ok2 > key : ok2 < key;
                    }
                }
                if (take) { best = ob; key = ok2; }
            }
            if (key < 0) { ok = false; break; }   // (nrem >= 1 here, so this does not happen)
            min_val = best;
            const int index = key >> 1;
            const int j = s.rem[index], last = s.rem[nrem - 1], owner = s.row4col[j];
            wave_sync();
            if (lane == 0) { s.in_sc[j] = 1; s.rem[index] = last; }
            --nrem;
            wave_sync();
            if (owner < 0) sink = j;
            else i = owner;
        }
        if (sink < 0) { ok = false; break; }
        // dual variables
        for (int k = lane; k < nr; k += 64)
            if (k == cur) s.u[k] += min_val;
            else if (s.in_sr[k]) s.u[k] += min_val - s.spc[s.col4row[k]];
        for (int k = lane; k < nc; k += 64)
            if (s.in_sc[k]) s.v[k] -= min_val - s.spc[k];
        wave_sync();
        // augment along the path (one lane; at most nr rows change their partner)
        if (lane == 0) {
            int j = sink, steps = 0;
            for (; steps <= nr; ++steps) {
                const int r = s.path[j];
                if (r < 0) { steps = nr + 1; break; }     // (a column without a predecessor: cannot happen with finite costs)
                s.row4col[j] = r;
                const int prev = s.col4row[r];
                s.col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
            if (steps > nr) s.in_sr[0] = 2;       // (marks the failure for the other lanes)
        }
        wave_sync();
        if (s.in_sr[0] == 2) ok = false;
        wave_sync();
    }
    return ok;
}

__global__ __launch_bounds__(kThreads) void track_kernel(int S, int H, int W, float thr, const int* __restrict__ raw,
                                                         const float* __restrict__ flow, int* __restrict__ out,
                                                         int* __restrict__ err) {
    __shared__ float s_dist[kMaxC * kMaxC];
    __shared__ FrameStats s_stats[2];
    __shared__ Solver s_solver;
    __shared__ int s_newid[2][kMaxC + 1];         // raw id -> consistent id, of the frames t and t + 1
    __shared__ int s_rowid[kMaxC];                // the rows of the cost matrix: consistent ids of frame t, ascending
    __shared__ float s_wr[kMaxC], s_wc[kMaxC], s_ar[kMaxC], s_ac[kMaxC];
    __shared__ int s_nrows, s_largest, s_err[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int P = H * W;
    const int* raw_b = raw + (size_t)b * S * P;
    int* out_b = out + (size_t)b * S * P;
    if (tid < 4) s_err[tid] = 0;

    for (int f = 0; f < S; ++f) {
        // ---- per raw id of frame f: pixel count, coordinate sums and (frames that are warped: all but the last) flow sums ----
        FrameStats& st = s_stats[f & 1];
        for (int k = tid; k <= kMaxC; k += kThreads) { st.cnt[k] = 0; st.sr[k] = 0; st.sc[k] = 0; st.fr[k] = 0; st.fc[k] = 0; }
        __syncthreads();
        const int* ids = raw_b + (size_t)f * P;
        const float* fl = (flow && f + 1 < S) ? flow + ((size_t)b * S + f) * 2 * P : nullptr;
#pragma unroll 1
        for (int p = tid; p < P; p += kThreads) {
            int id = ids[p];
            if (id < 0 || id > kMaxC) { s_err[kErrIds] = 1; id = 0; }
            if (id == 0) { if (st.cnt[0] == 0) st.cnt[0] = 1; continue; }     // (only "is there background" is needed)
            const int r = p / W, c = p - r * W;
            atomicAdd(&st.cnt[id], 1);
            atomicAdd(&st.sr[id], (unsigned long long)r);
            atomicAdd(&st.sc[id], (unsigned long long)c);
            if (fl) {
                float a = fl[p], d = fl[P + p];
                if (!(fabsf(a) < kFlowLimit) || !(fabsf(d) < kFlowLimit)) { s_err[kErrFlow] = 1; a = 0.0f; d = 0.0f; }
                atomicAdd(&st.fr[id], (unsigned long long)llrintf(a * kFlowScale));
                atomicAdd(&st.fc[id], (unsigned long long)llrintf(d * kFlowScale));
            }
        }
        __syncthreads();
        int n = 0;                                // the largest raw id of frame f (instance.py:226), every thread the same
#pragma unroll 1
        for (int k = 1; k <= kMaxC; ++k)
            if (st.cnt[k] > 0) n = k;
        if (tid == 0 && st.cnt[0] == 0) s_err[kErrNoBackground] = 1;
        if (tid >= 1 && tid <= n && st.cnt[tid] == 0) s_err[kErrIds] = 1;
        int* newid = s_newid[f & 1];
        if (f == 0) {                             // instance.py:194-195: taken over, through the relabelling pass below
            for (int k = tid; k <= kMaxC; k += kThreads) newid[k] = k;
            if (tid == 0) s_largest = n;
        } else {
            // ---- step t = f - 1 -> f ----
            const FrameStats& sp = s_stats[(f - 1) & 1];
            const int* previd = s_newid[(f - 1) & 1];
            if (tid == 0) s_nrows = 0;
            __syncthreads();
            // rows: the instances of the consistent frame t in ascending id, warped by the flow (:201-219)
            if (tid >= 1 && tid <= kMaxC && sp.cnt[tid] > 0) {
                int row = 0;
#pragma unroll 1
                for (int k = 1; k <= kMaxC; ++k)
                    if (sp.cnt[k] > 0 && previd[k] < previd[tid]) ++row;
                const double cnt = (double)sp.cnt[tid];
                const double sr = (double)(long long)sp.sr[tid] + (double)(long long)sp.fr[tid] * (1.0 / 1048576.0);
                const double sc = (double)(long long)sp.sc[tid] + (double)(long long)sp.fc[tid] * (1.0 / 1048576.0);
                s_rowid[row] = previd[tid];
                s_wr[row] = (float)(sr / cnt);
                s_wc[row] = (float)(sc / cnt);
                atomicAdd(&s_nrows, 1);
            }
            // columns: ids 1..n of the raw frame t + 1 (:226-236)
            if (tid >= 1 && tid <= n) {
                const double cnt = (double)(st.cnt[tid] > 0 ? st.cnt[tid] : 1);
                s_ar[tid - 1] = (float)((double)(long long)st.sr[tid] / cnt);
                s_ac[tid - 1] = (float)((double)(long long)st.sc[tid] / cnt);
            }
            __syncthreads();
            const int nrows = s_nrows;
            const bool take_over = nrows == 0 || n == 0;      // :211-214, :228-231 (block-uniform)
            if (take_over) {
                for (int k = tid; k <= kMaxC; k += kThreads) newid[k] = k;
            } else {
                for (int e = tid; e < nrows * n; e += kThreads) {
                    const int i = e / n, j = e - i * n;
                    const float dr = s_ar[j] - s_wr[i], dc = s_ac[j] - s_wc[i];
                    s_dist[i * kMaxC + j] = sqrtf(dr * dr + dc * dc);                  // :239
                }
                for (int k = tid; k <= kMaxC; k += kThreads) newid[k] = 0;
                __syncthreads();
                if (tid < 64) {
                    if (!assign(s_solver, s_dist, nrows, n, lane)) s_err[kErrBound] = 1;
                    wave_sync();
                    const bool transposed = n < nrows;
                    const int nr = transposed ? n : nrows;
                    for (int k = lane; k < nr; k += 64) {
                        const int partner = s_solver.col4row[k];
                        if (partner < 0) continue;
                        const int i = transposed ? partner : k, j = transposed ? k : partner;
                        if (s_dist[i * kMaxC + j] < thr) newid[j + 1] = s_rowid[i];    // :253-254
                    }
                    wave_sync();
                    // fresh ids in ascending order of the old id (include/stp3_hip.h; the reference: set order, :257-264)
                    int largest = s_largest;
                    for (int k0 = 1; k0 <= n; k0 += 64) {
                        const int k = k0 + lane;
                        const bool fresh = k <= n && st.cnt[k] > 0 && newid[k] == 0;
                        const unsigned long long votes = __ballot(fresh);
                        if (fresh) newid[k] = largest + 1 + __popcll(votes & ((1ull << lane) - 1ull));
                        largest += __popcll(votes);
                    }
                    wave_sync();
                    if (lane == 0) s_largest = largest;
                }
            }
        }
        __syncthreads();
        int* dst = out_b + (size_t)f * P;
        for (int p = tid; p < P; p += kThreads) {                                   // :266
            const int id = ids[p];
            dst[p] = (id < 0 || id > kMaxC) ? 0 : newid[id];
        }
    }
    __syncthreads();
    if (tid < 4 && s_err[tid]) err[tid] = 1;      // (every writer stores the same value)
}

}  // namespace

extern "C" {

int stp3_instance_segment(int32_t N, int32_t H, int32_t W, float conf_threshold, const float* center, const float* offset,
                          const uint8_t* foreground, int32_t* seg, int32_t* centers, int32_t* counts, void* stream) {
    if (N < 1 || H < 1 || W < 1 || !center || !offset || !foreground || !seg || !centers || !counts) return STP3_EINVAL;
    if (H > kMaxSide || W > kMaxSide || (int64_t)H * W >= (1 << 24)) return STP3_EUNSUP;
    hipLaunchKernelGGL(segment_kernel, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, H, W, conf_threshold, center, offset,
                       foreground, seg, centers, counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

int stp3_instance_track(int32_t B, int32_t S, int32_t H, int32_t W, float matching_threshold, const int32_t* raw,
                        const float* flow, int32_t* out, int32_t* err, void* stream) {
    if (B < 1 || S < 1 || H < 1 || W < 1 || !raw || !out || !err) return STP3_EINVAL;
    if (H > kMaxSide || W > kMaxSide || (int64_t)H * W >= (1 << 24)) return STP3_EUNSUP;
    hipLaunchKernelGGL(track_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, S, H, W, matching_threshold, raw, flow,
                       out, err);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
