// stp3_window.hip -- the sliding window of the closed-loop forward on gfx950: advance the cached encoder outputs by one frame.
//
// Reference: the simulator tick, carla_agent.py:408-432 -- the newest camera frame is appended to a buffer and the model is
// handed all T frames again (:445), two of which it encoded on the previous tick.  In eval mode the image encoder
// (stp3/models/encoder.py:57-97) couples no two images, so its outputs of the older frames can be kept:
//     window [B][T][N * fH * fW][C] float32, pixel-major -- exactly what stp3_lift_splat_fwd reads (feat_pm, logits_pm).
// A push is, per sample,  window[t] = window[t + 1]  for t < T - 1  and  window[T - 1] = the encoder head's new output, a logical
// (B * N, C, fH, fW) tensor in bf16 or float32 read through three element strides (image, channel, pixel: NCHW-contiguous and
// channels-last memory alike), widened exactly.  torch would take 2 (T - 1) + 2 copy launches and a second buffer for the same.
//
// IN PLACE, ONE LAUNCH, NO ORDER BETWEEN WORKGROUPS.  A thread owns one 16-byte channel vector POSITION (sample b, pixel, channel
// group) of the frame and is the only thread of the launch that reads or writes that position in ANY of the T frames: it walks
// t = 0 .. T - 2 (load frame t + 1, store frame t -- the value a step overwrites was copied by the step before, in this thread's
// program order) and then stores the new value into frame T - 1.  Two threads never touch the same window address, so no
// barrier, no second buffer and no ordering between threads, waves or workgroups is needed; the source is only read (the caller
// keeps it outside the window).  Both caches -- up to STP3_WINDOW_JOBS_MAX windows -- go in one launch: blockIdx.y is the job.
// HBM-bound streaming kernel: 16-byte accesses along the channel axis on the window side, (T - 1) loads + T stores per thread.
// The SOURCE read streams for channels-last memory only (stride_channel == 1: one 8 / 16-byte load per thread, neighbouring threads
// adjacent -- what the encoder heads emit under to_channels_last); an NCHW source is read with four scalar loads `pixels` elements
// apart, neighbouring threads 4 * pixels apart: correct, not coalesced.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kJobs = STP3_WINDOW_JOBS_MAX;

struct WindowJob {
    const void* src;
    float4* window;
    int64_t s_img, s_ch, s_pix;     // element strides of src
    uint32_t positions;             // B * npix * cv: the 16-byte vectors of ONE frame of all samples
    uint32_t cv;                    // channels / 4
    int bf16;
    int vec;                        // s_ch == 1 and every 4-channel group of src is aligned to its vector load
};

struct WindowJobs {
    WindowJob job[kJobs];
    uint32_t T, N, pixels;          // frames per window, images per sample, fH * fW
};

__device__ __forceinline__ float4 widen4(uint32_t lo, uint32_t hi) {
    return make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                       __uint_as_float(hi & 0xffff0000u));
}

__global__ __launch_bounds__(kThreads) void window_push_kernel(WindowJobs jobs) {
    // (blockIdx.y is uniform: the job's fields are scalar loads from the kernel argument)
    const WindowJob j = jobs.job[blockIdx.y];
    const uint32_t T = jobs.T, npix = jobs.N * jobs.pixels;
    const uint32_t per_sample = npix * j.cv;                               // vectors of one frame of one sample
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < j.positions; i += gridDim.x * kThreads) {
        const uint32_t b = i / per_sample, r = i - b * per_sample;
        const uint32_t pix = r / j.cv, c = (r - pix * j.cv) * 4;
        const uint32_t n = pix / jobs.pixels, p = pix - n * jobs.pixels;
        const int64_t at = (int64_t)(b * jobs.N + n) * j.s_img + (int64_t)p * j.s_pix + (int64_t)c * j.s_ch;
        float4 v;
        if (j.bf16) {
            const uint16_t* s = (const uint16_t*)j.src + at;
            if (j.vec) {
                const uint2 w = *reinterpret_cast<const uint2*>(s);
                v = widen4(w.x, w.y);
            } else {
                v = make_float4(__uint_as_float((uint32_t)s[0] << 16), __uint_as_float((uint32_t)s[j.s_ch] << 16),
                                __uint_as_float((uint32_t)s[2 * j.s_ch] << 16), __uint_as_float((uint32_t)s[3 * j.s_ch] << 16));
            }
        } else {
            const float* s = (const float*)j.src + at;
            if (j.vec) v = *reinterpret_cast<const float4*>(s);
            else v = make_float4(s[0], s[j.s_ch], s[2 * j.s_ch], s[3 * j.s_ch]);
        }
        // this thread's position in frame 0 of sample b; frame t is t * per_sample vectors further (< 2^28 vectors in all)
        float4* w = j.window + ((size_t)b * T * per_sample + r);
        for (uint32_t t = 0; t + 1 < T; ++t) w[(size_t)t * per_sample] = w[(size_t)(t + 1) * per_sample];
        w[(size_t)(T - 1) * per_sample] = v;
    }
}

inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // namespace

extern "C" {

int stp3_window_push(int32_t B, int32_t T, int32_t N, int32_t pixels, int32_t n_jobs, const stp3_window_job* jobs, void* stream) {
    if (B < 1 || T < 1 || N < 1 || pixels < 1 || n_jobs < 0 || (n_jobs > 0 && !jobs)) return STP3_EINVAL;
    if (n_jobs > kJobs) return STP3_EUNSUP;
    if (n_jobs == 0) return STP3_OK;
    WindowJobs t;
    t.T = (uint32_t)T; t.N = (uint32_t)N; t.pixels = (uint32_t)pixels;
    int64_t most = 0;
    for (int k = 0; k < kJobs; ++k) {
        WindowJob& d = t.job[k];
        if (k >= n_jobs) {
            d = WindowJob{nullptr, nullptr, 0, 0, 0, 0u, 1u, 0, 0};
            continue;
        }
        const stp3_window_job& q = jobs[k];
        if (!q.src || !q.window || q.channels < 1) return STP3_EINVAL;
        if (q.dtype != STP3_DTYPE_F32 && q.dtype != STP3_DTYPE_BF16) return STP3_EUNSUP;
        if (q.channels % 4 || ((uintptr_t)q.window & 15)) return STP3_EUNSUP;
        if (q.stride_image < 0 || q.stride_channel < 0 || q.stride_pixel < 0) return STP3_EINVAL;
        // (each factor is below 2^31: the products below cannot wrap an int64 before they are compared)
        const int64_t frame = (int64_t)N * pixels * q.channels;             // elements of one frame of one sample
        if (frame >= (1LL << 30) || (int64_t)B * T >= (1LL << 30)) return STP3_EUNSUP;
        if ((int64_t)B * T * frame * 4 >= (1LL << 32)) return STP3_EUNSUP;  // window bytes: 32-bit vector indices
        const int esize = q.dtype == STP3_DTYPE_BF16 ? 2 : 4;
        const int64_t mask = 4 - 1;                                         // a 4-element group: 8 (bf16) / 16 (float32) bytes
        d.src = q.src;
        d.window = (float4*)q.window;
        d.s_img = q.stride_image; d.s_ch = q.stride_channel; d.s_pix = q.stride_pixel;
        d.positions = (uint32_t)((int64_t)B * frame / 4);
        d.cv = (uint32_t)(q.channels / 4);
        d.bf16 = q.dtype == STP3_DTYPE_BF16;
        d.vec = q.stride_channel == 1 && !(q.stride_image & mask) && !(q.stride_pixel & mask) &&
                !((uintptr_t)q.src & (uintptr_t)(4 * esize - 1));
        if (d.positions > most) most = d.positions;
    }
    // one resident round of the chip's 256 CUs at 8 workgroups each, shared by the jobs; grid-stride beyond
    const int64_t want = (most + kThreads - 1) / kThreads, cap = 256 * 8 / n_jobs;
    const unsigned gx = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(window_push_kernel, dim3(gx, (unsigned)n_jobs), dim3(kThreads), 0, (hipStream_t)stream, t);
    return status();
}

}  // extern "C"
