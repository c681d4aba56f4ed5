// stp3_carla.hip -- the CARLA loader and agent from decoded bytes to tensors (stp3/datas/CarlaData.py, carla_agent.py) for gfx950.
//
// Replaces, behind stp3_carla_*, what the reference computes per image on the host once the PNG decoder (or the simulator's
// sensor) has handed over bytes -- ONE launch per kind for all frames and cameras of a call:
//   frames   scale_and_crop_image(..., scale=1, crop=c) + normalise_image (CarlaData.py:377-384,454-464; carla_agent.py:326-329,
//            370-426): the centre window rows Hs/2 - c/2 .., columns Ws/2 - c/2 .., ToTensor (float32 x / 255) and
//            Normalize ((x - mean) / std), both TRUE divisions (the library is built without contraction): the float32 output is
//            bit-equal to those statements, the bf16 output is their rounding.  Sources of 3 or 4 channels; with the BGR flag
//            the first three channels are reversed and a fourth is ignored (cv2.cvtColor(x[:, :, :3], COLOR_BGR2RGB)).
//   depth    get_depth (CarlaData.py:345-353,387-396) on the same window: v = double(R 65536 + G 256 + B) / 16777215.0 * 1000.0 in
//            float64 in that order -> the metre map (float64, or float32: the rounding of the float64 value), or directly the
//            trainer's class ids (stp3/trainer.py:269-276) of every `downsample`-th row and column of the window:
//            int64(min(max(v, d_lo), d_hi) - d_lo) in float64 -- only the kept pixels are decoded.
//   hdmap    get_hdmap (CarlaData.py:240-260) at scale 1: lane = pixel == (255, 0, 255), drivable = pixel == (54, 52, 46) | lane,
//            both flipped along both axes; out [n][2][c][c], channel 0 the lane.
//   topdown  get_labels (CarlaData.py:262-280): Pillow's NEAREST resize as two index tables built on the host (source row of every
//            resized row, source column of every resized column: configuration only), the centre window of the resized image,
//            vehicle = (pixel == 10) with the fixed ego box rows 89..111 x columns 96..104 of the window cleared (clipped to the
//            window as a numpy slice clips it), pedestrian = (pixel == 4), both flipped along both axes.
// Byte-wide sources: a window starts at an arbitrary byte (300 x 400 RGB: 216; 11 x 13: 9) and its rows have arbitrary pitch,
// so every pixel is read with byte loads -- except a 4-channel source on a 4-byte aligned base, whose pixel is one aligned
// dword.  The work is bandwidth-trivial (four 300 x 400 BGRA frames: 1.9 MB in, 3.1 MB out); one thread per output pixel,
// consecutive threads on consecutive columns, so the planar stores are coalesced.  A table entry outside the source is
// clamped on the device.  All entries only enqueue on `stream`, allocate nothing and do not synchronise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_cdna.h"
#include "stp3_hip.h"

namespace {

constexpr int kThreads = 256;

struct Window {
    int n, Hs, Ws, Cs, c, y0, x0;
};

struct Norm {
    float mean[3], std[3];
};

template <typename T>
__device__ __forceinline__ void store_flag(void* out, size_t o, bool v) {
    reinterpret_cast<T*>(out)[o] = v ? (T)1 : (T)0;
}

__device__ __forceinline__ void store_map(void* out, size_t o, bool v, int kind) {
    if (kind == STP3_CARLA_OUT_F32) store_flag<float>(out, o, v);
    else if (kind == STP3_CARLA_OUT_F64) store_flag<double>(out, o, v);
    else store_flag<int64_t>(out, o, v);
}

__global__ __launch_bounds__(kThreads) void carla_frames_kernel(Window w, Norm nm, int bgr, int out_bf16, int dword_ok,
                                                                 const uint8_t* __restrict__ frames, void* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.c * w.c) return;
    const int n = blockIdx.y;
    const int r = i / w.c, x = i - r * w.c;
    const size_t px = ((size_t)n * w.Hs + (w.y0 + r)) * w.Ws + (w.x0 + x);
    int v[3];
    if (dword_ok) {                                            // Cs == 4, 4-byte aligned base: the pixel is one dword
        const uint32_t q = reinterpret_cast<const uint32_t*>(frames)[px];
        v[0] = q & 0xffu; v[1] = (q >> 8) & 0xffu; v[2] = (q >> 16) & 0xffu;
    } else {
        const uint8_t* p = frames + px * w.Cs;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
    if (bgr) { const int t = v[0]; v[0] = v[2]; v[2] = t; }
    const size_t plane = (size_t)w.c * w.c;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float f = ((float)v[ch] / 255.0f - nm.mean[ch]) / nm.std[ch];
        const size_t o = ((size_t)n * 3 + ch) * plane + i;
        if (out_bf16) reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)(pack_bf16(f, 0.f) & 0xffffu);
        else reinterpret_cast<float*>(out)[o] = f;
    }
}

// `side` output rows and columns per image; output (r, x) is window pixel (r step, x step)
__global__ __launch_bounds__(kThreads) void carla_depth_kernel(Window w, int side, int step, int kind, double d_lo, double d_hi,
                                                                const uint8_t* __restrict__ frames, void* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= side * side) return;
    const int n = blockIdx.y;
    const int r = i / side, x = i - r * side;
    const uint8_t* p = frames + (((size_t)n * w.Hs + (w.y0 + r * step)) * w.Ws + (w.x0 + x * step)) * 3;
    const int code = (int)p[0] * 65536 + (int)p[1] * 256 + (int)p[2];
    const double v = (double)code / 16777215.0 * 1000.0;
    const size_t o = (size_t)n * side * side + i;
    if (kind == STP3_DEPTH_OUT_F64) reinterpret_cast<double*>(out)[o] = v;
    else if (kind == STP3_DEPTH_OUT_F32) reinterpret_cast<float*>(out)[o] = (float)v;
    else reinterpret_cast<int64_t*>(out)[o] = (int64_t)(fmin(fmax(v, d_lo), d_hi) - d_lo);
}

__global__ __launch_bounds__(kThreads) void carla_hdmap_kernel(Window w, int kind, const uint8_t* __restrict__ frames,
                                                                void* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.c * w.c) return;
    const int n = blockIdx.y;
    const int r = i / w.c, x = i - r * w.c;
    // output (r, x) shows window pixel (c - 1 - r, c - 1 - x)
    const uint8_t* p = frames + (((size_t)n * w.Hs + (w.y0 + w.c - 1 - r)) * w.Ws + (w.x0 + w.c - 1 - x)) * 3;
    const int p0 = p[0], p1 = p[1], p2 = p[2];
    const bool lane = p0 == 255 && p1 == 0 && p2 == 255;
    const bool drivable = (p0 == 54 && p1 == 52 && p2 == 46) || lane;
    const size_t plane = (size_t)w.c * w.c;
    store_map(out, ((size_t)n * 2) * plane + i, lane, kind);
    store_map(out, ((size_t)n * 2 + 1) * plane + i, drivable, kind);
}

// w.Hs x w.Ws: the SOURCE; (w.y0, w.x0): the window's origin in the RESIZED image of Hr x Wr
__global__ __launch_bounds__(kThreads) void carla_topdown_kernel(Window w, int Hr, int Wr, int kind, const int* __restrict__ row_src,
                                                                  const int* __restrict__ col_src, const uint8_t* __restrict__ frames,
                                                                  void* __restrict__ vehicle, void* __restrict__ pedestrian) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.c * w.c) return;
    const int n = blockIdx.y;
    const int r = i / w.c, x = i - r * w.c;
    const int wr = w.c - 1 - r, wx = w.c - 1 - x;              // the window pixel this output shows
    const int sy = min(max(row_src[w.y0 + wr], 0), w.Hs - 1);
    const int sx = min(max(col_src[w.x0 + wx], 0), w.Ws - 1);
    const int px = frames[((size_t)n * w.Hs + sy) * w.Ws + sx];
    const bool ego = wr >= 89 && wr < 112 && wx >= 96 && wx < 105;
    const size_t o = (size_t)n * w.c * w.c + i;
    store_map(vehicle, o, px == 10 && !ego, kind);
    store_map(pedestrian, o, px == 4, kind);
}

// n images of Hs x Ws whose centre window of c x c is read: STP3_OK, or why not
int window_of(int n, int Hs, int Ws, int Cs, int c, int Hr, int Wr, Window* w) {
    if (n < 1 || Hs < 1 || Ws < 1 || c < 1 || Hr < c || Wr < c) return STP3_EINVAL;
    if (n > 65535 || c > 32768 || (int64_t)Hs * Ws >= (1LL << 31)) return STP3_EUNSUP;
    w->n = n; w->Hs = Hs; w->Ws = Ws; w->Cs = Cs; w->c = c;
    w->y0 = Hr / 2 - c / 2;                                    // >= 0 and y0 + c <= Hr because c <= Hr
    w->x0 = Wr / 2 - c / 2;
    return STP3_OK;
}

dim3 grid_of(int pixels, int n) { return dim3((unsigned)((pixels + kThreads - 1) / kThreads), (unsigned)n); }

int last_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

bool map_kind_ok(int kind) { return kind == STP3_CARLA_OUT_F32 || kind == STP3_CARLA_OUT_F64 || kind == STP3_CARLA_OUT_I64; }

}  // namespace

extern "C" {

int stp3_carla_frames(int32_t n, int32_t Hs, int32_t Ws, int32_t Cs, int32_t crop, int32_t bgr, const float* mean,
                      const float* std, int32_t out_dtype, const uint8_t* frames, void* out, void* stream) {
    if (!frames || !out || !mean || !std || (Cs != 3 && Cs != 4) || (bgr != 0 && bgr != 1)) return STP3_EINVAL;
    if (out_dtype != STP3_DTYPE_F32 && out_dtype != STP3_DTYPE_BF16) return STP3_EUNSUP;
    Window w;
    const int rc = window_of(n, Hs, Ws, Cs, crop, Hs, Ws, &w);
    if (rc != STP3_OK) return rc;
    Norm nm;
    for (int ch = 0; ch < 3; ++ch) { nm.mean[ch] = mean[ch]; nm.std[ch] = std[ch]; }
    const int dword_ok = Cs == 4 && ((uintptr_t)frames & 3) == 0;
    hipLaunchKernelGGL(carla_frames_kernel, grid_of(crop * crop, n), dim3(kThreads), 0, (hipStream_t)stream, w, nm, (int)bgr,
                       (int)(out_dtype == STP3_DTYPE_BF16), dword_ok, frames, out);
    return last_error();
}

int stp3_carla_depth(int32_t n, int32_t Hs, int32_t Ws, int32_t crop, int32_t out_kind, int32_t downsample, double d_lo,
                     double d_hi, const uint8_t* frames, void* out, void* stream) {
    if (!frames || !out) return STP3_EINVAL;
    if (out_kind != STP3_DEPTH_OUT_F32 && out_kind != STP3_DEPTH_OUT_F64 && out_kind != STP3_DEPTH_OUT_LABELS) return STP3_EINVAL;
    const bool labels = out_kind == STP3_DEPTH_OUT_LABELS;
    if (labels && (downsample < 1 || !(d_lo <= d_hi))) return STP3_EINVAL;
    Window w;
    const int rc = window_of(n, Hs, Ws, 3, crop, Hs, Ws, &w);
    if (rc != STP3_OK) return rc;
    const int step = labels ? downsample : 1;
    const int side = (crop + step - 1) / step;                 // rows 0, step, 2 step, .. < crop
    hipLaunchKernelGGL(carla_depth_kernel, grid_of(side * side, n), dim3(kThreads), 0, (hipStream_t)stream, w, side, step,
                       (int)out_kind, d_lo, d_hi, frames, out);
    return last_error();
}

int stp3_carla_hdmap(int32_t n, int32_t Hm, int32_t Wm, int32_t crop, int32_t out_kind, const uint8_t* frames, void* out,
                     void* stream) {
    if (!frames || !out || !map_kind_ok(out_kind)) return STP3_EINVAL;
    Window w;
    const int rc = window_of(n, Hm, Wm, 3, crop, Hm, Wm, &w);
    if (rc != STP3_OK) return rc;
    hipLaunchKernelGGL(carla_hdmap_kernel, grid_of(crop * crop, n), dim3(kThreads), 0, (hipStream_t)stream, w, (int)out_kind, frames,
                       out);
    return last_error();
}

int stp3_carla_topdown(int32_t n, int32_t Ht, int32_t Wt, int32_t Hr, int32_t Wr, int32_t crop, const int32_t* row_src,
                       const int32_t* col_src, int32_t out_kind, const uint8_t* frames, void* vehicle, void* pedestrian,
                       void* stream) {
    if (!frames || !vehicle || !pedestrian || !row_src || !col_src || !map_kind_ok(out_kind)) return STP3_EINVAL;
    Window w;
    const int rc = window_of(n, Ht, Wt, 1, crop, Hr, Wr, &w);
    if (rc != STP3_OK) return rc;
    hipLaunchKernelGGL(carla_topdown_kernel, grid_of(crop * crop, n), dim3(kThreads), 0, (hipStream_t)stream, w, (int)Hr, (int)Wr,
                       (int)out_kind, row_src, col_src, frames, vehicle, pedestrian);
    return last_error();
}

}  // extern "C"
