// stp3_image.hip -- camera images from decoded bytes to network input for gfx950.
//
// Replaces, behind stp3_image_prep, the per-image chain of the reference's loader (stp3/datas/NuscenesData.py:236-244):
//     PIL.Image.resize(resize_dims, BILINEAR)  ->  .crop(crop)  ->  ToTensor (/ 255)  ->  Normalize(mean, std)
// 18 times per sample (6 cameras x 3 frames) on 1600 x 900 x 3 bytes each.  BYTE-EXACT with Pillow's resampler: the same
// two passes (horizontal, then vertical) with its fixed-point arithmetic -- coefficients round(w * 2^22) built on the host
// exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do (stp3_amd/datas.py), accumulators starting at 2^21,
// (sum >> 22) clipped to a byte after EACH pass -- so the network sees the numbers it was trained on.
//
// HBM-bound byte work: 4.3 MB in, 0.43-1.3 MB out per image.  One workgroup owns kRows output rows of one image: the input
// rows its vertical taps need are streamed through LDS (16-byte loads of whole rows), reduced horizontally to bytes -- only
// the columns inside the crop -- into an LDS strip, and the vertical pass + normalisation run from the strip; the output
// is written planar (CHW), coalesced, as float32 or bf16.  Pixels of the crop window that lie outside the resized image
// are PIL's zero padding (crop beyond the border), normalised like any other value.
//
// stp3_image_augment runs the SAME band body (resample_band) with a per-image view -- resized size, crop origin, table
// offsets, a mirrored column index for the horizontal flip -- read from a parameter table in device memory: the Lift-Splat
// augmentation the reference carries as img_transform (stp3/utils/tools.py:122-146) behind the loader's BILINEAR resize
// (stp3/utils/geometry.py:9-13).  The in-plane rotation (Pillow's Image.rotate: a NEAREST gather at 16.16 fixed-point
// addresses) reads window rows far outside a band (+-5.4 degrees across 480 columns: 45 rows), so rotated images leave the
// band kernel as cropped, flipped BYTES in a workspace and a second kernel gathers and normalises them; images whose
// rotation is the identity are written normalised by the band kernel itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_cdna.h"
#include "stp3_hip.h"

namespace {

constexpr int kPrecision = 22;          // Pillow: PRECISION_BITS = 32 - 8 - 2
constexpr int kRows = 4;                // output rows per workgroup
constexpr int kChunk = 4;               // source rows staged per iteration
constexpr int kPre = 5;                 // 16-byte pieces per thread of the chunk in flight (4 x 4 800 bytes: 1 200 pieces)

struct ImageDims {
    int N, H, W, Wr, Hr, left, top, Wo, Ho, ksize_h, ksize_v, out_bf16, strip_rows;
    float mean[3], inv255_unused, std[3];
};

// What one workgroup resamples: the geometry and the tables of ITS image (the same for all images of stp3_image_prep,
// read from the parameter table for stp3_image_augment).
// Only the window columns x0 .. x0 + cols can lie inside the resized image: the LDS strip and coefficient rows hold those
// (all Wo of them for stp3_image_prep; a Lift-Splat resize leaves a third of a 480-wide window outside, and the LDS that
// saves is what lets two workgroups share a compute unit).
struct BandView {
    int H, W, Wr, Hr, left, top, Wo, Ho, ksize_h, ksize_v, strip_rows, flip, x0, cols;
    const int* kk_h;
    const int* bounds_h;
    const int* kk_v;
    const int* bounds_v;
};

__device__ __forceinline__ int clip8(int v) { return min(max(v >> kPrecision, 0), 255); }

// column of the resized image behind window column x (the flip mirrors the window)
__device__ __forceinline__ int resized_column(const BandView& d, int x) { return d.left + (d.flip ? d.Wo - 1 - x : x); }

// The horizontal taps of one pixel come from LDS as dwords when there are at most 9 (the 10/3 down-scale of the stock recipe)
// or at most 13 (down-scales up to 6: the Lift-Splat resize range 0.193 .. 0.225) of them: the row of coefficients is then
// padded to 12 / 16 ints for 16-byte reads.  More taps take the byte loop.
__host__ __device__ inline int dword_taps(int ksize_h) { return ksize_h <= 9 ? 9 : ksize_h <= 13 ? 13 : 0; }
__host__ __device__ inline int coef_stride(int ksize_h) {
    return dword_taps(ksize_h) == 9 ? 12 : dword_taps(ksize_h) == 13 ? 16 : ksize_h;
}

__host__ __device__ inline size_t band_lds_bytes(int W, int Wo, int ksize_h, int strip_rows) {
    return (size_t)kChunk * ((W * 3 + 15) & ~15) + (((size_t)strip_rows * Wo * 3 + 15) & ~(size_t)15) +
           (size_t)Wo * (coef_stride(ksize_h) + 2) * sizeof(int32_t);
}

// kTaps (9 | 13) taps = 3 kTaps consecutive bytes: dword reads, realigned to the first byte with funnel shifts, instead of
// byte reads (the kernel was bound by its LDS instruction count); the coefficients as 16-byte reads.  Taps beyond the
// pixel's count have coefficient 0; their bytes lie inside the staging buffer or the strip behind it.
template <int kTaps>
__device__ __forceinline__ void taps_from_dwords(const uint8_t* rowbuf, int addr, const int* k, int& s0, int& s1, int& s2) {
    constexpr int kWords = (3 * kTaps + 3) / 4;            // dwords holding the bytes once realigned: 7 | 10
    const int sh = (addr & 3) * 8;
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(rowbuf + (addr & ~3));
    uint32_t w[kWords + 1], v[kWords];
#pragma unroll
    for (int j = 0; j < kWords + 1; ++j) w[j] = wp[j];
#pragma unroll
    for (int j = 0; j < kWords; ++j) v[j] = (uint32_t)(((((uint64_t)w[j + 1]) << 32) | w[j]) >> sh);
    int kw[kTaps];
#pragma unroll
    for (int q = 0; q < kTaps / 4; ++q) {
        const uint4 kq = reinterpret_cast<const uint4*>(k)[q];
        kw[4 * q] = (int)kq.x; kw[4 * q + 1] = (int)kq.y; kw[4 * q + 2] = (int)kq.z; kw[4 * q + 3] = (int)kq.w;
    }
    kw[kTaps - 1] = k[kTaps - 1];                          // (kTaps = 4 q + 1)
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const int b0 = 3 * t, b1 = 3 * t + 1, b2 = 3 * t + 2;
        s0 += (int)((v[b0 >> 2] >> (8 * (b0 & 3))) & 0xffu) * kw[t];
        s1 += (int)((v[b1 >> 2] >> (8 * (b1 & 3))) & 0xffu) * kw[t];
        s2 += (int)((v[b2 >> 2] >> (8 * (b2 & 3))) & 0xffu) * kw[t];
    }
}

// The horizontal pass of the window rows r0 .. r0 + rows of one image into the LDS strip; returns the first source row of
// the strip (row y of the source is strip row y - y0).  kGuard: the view comes from device memory -- source rows are
// clamped to the image and strip rows to the strip, so that no table entry can move an access out of its buffer.
template <bool kGuard>
__device__ __forceinline__ int resample_band(const BandView& d, const uint8_t* __restrict__ img, int r0, int rows,
                                             uint8_t* smem) {
    const int row_bytes = d.W * 3;
    const int row_pitch = (row_bytes + 15) & ~15;
    uint8_t* rowbuf = smem;                                // kChunk input rows
    uint8_t* strip = smem + kChunk * row_pitch;            // [strip_rows][cols * 3] horizontally resampled bytes
    // the horizontal coefficients of the window's columns, [cols][ksize_h] + (first source column, count): read once per
    // workgroup -- fetched per tap from global memory they made the kernel bound by its vector-memory issue rate
    const int kstride = coef_stride(d.ksize_h);            // <= 9 | 13 taps: rows padded to 48 | 64 bytes for 16-byte reads
    const int dwords = dword_taps(d.ksize_h);
    int* ck = reinterpret_cast<int*>(strip + ((d.strip_rows * d.cols * 3 + 15) & ~15));
    int* cb = ck + d.cols * kstride;
    const int tid = threadIdx.x;
    // input rows the vertical taps of this workgroup's output rows read
    int y0 = d.H, y1 = 0;
    for (int r = 0; r < rows; ++r) {
        const int yr = d.top + r0 + r;
        if (yr < 0 || yr >= d.Hr) continue;
        const int lo = d.bounds_v[2 * yr], cnt = d.bounds_v[2 * yr + 1];
        y0 = min(y0, lo);
        y1 = max(y1, lo + cnt);
    }
    if (kGuard) {
        y0 = max(y0, 0);
        y1 = min(y1, min(d.H, y0 + d.strip_rows));
    }
    const int strip_pitch = d.cols * 3;
    const bool vec = (row_bytes & 15) == 0 && ((uintptr_t)img & 15) == 0;
    // kChunk source rows at a time: the 16-byte pieces of the NEXT chunk are in flight (registers) while the horizontal
    // pass of the current one runs from LDS -- one row per iteration was latency-bound (0.08 of the HBM rate)
    const int pieces = row_pitch / 16;                     // per row
    uint4 pre[kPre];
    auto fetch = [&](int yc) {                             // pieces tid, tid + 256, ... of the chunk starting at row yc
#pragma unroll
        for (int j = 0; j < kPre; ++j) {
            const int i = tid + 256 * j;
            const int rr = i / pieces, pp = i - rr * pieces;
            pre[j] = make_uint4(0u, 0u, 0u, 0u);
            if (rr < kChunk && yc + rr < y1) pre[j] = reinterpret_cast<const uint4*>(img + (size_t)(yc + rr) * row_bytes)[pp];
        }
    };
    const bool staged = vec && kChunk * pieces <= 256 * kPre;
    if (staged && y0 < y1) fetch(y0);
    for (int i = tid; i < d.cols; i += 256) {              // strip column i is window column x0 + i
        const int xr = resized_column(d, d.x0 + i);
        const bool in = xr >= 0 && xr < d.Wr;
        cb[2 * i] = in ? d.bounds_h[2 * xr] : 0;
        cb[2 * i + 1] = in ? d.bounds_h[2 * xr + 1] : 0;   // outside the resized image: no taps, the byte stays 0
        if (kGuard && (cb[2 * i] < 0 || cb[2 * i + 1] < 0 || cb[2 * i] + cb[2 * i + 1] > d.W)) cb[2 * i] = cb[2 * i + 1] = 0;
        for (int t = 0; t < kstride; ++t) ck[i * kstride + t] = (in && t < d.ksize_h) ? d.kk_h[xr * d.ksize_h + t] : 0;
    }
    for (int yc = y0; yc < y1; yc += kChunk) {
        const int nrows = min(kChunk, y1 - yc);
        if (staged) {
#pragma unroll
            for (int j = 0; j < kPre; ++j) {
                const int i = tid + 256 * j;
                if (i < kChunk * pieces) reinterpret_cast<uint4*>(rowbuf)[i] = pre[j];
            }
            if (yc + kChunk < y1) fetch(yc + kChunk);
        } else {
            for (int rr = 0; rr < nrows; ++rr)
                for (int i = tid; i < row_bytes; i += 256) rowbuf[rr * row_pitch + i] = img[(size_t)(yc + rr) * row_bytes + i];
        }
        __syncthreads();
        for (int i = tid; i < nrows * d.cols; i += 256) {   // one thread per (row, column): the three channels share the taps
            const int rr = i / d.cols, x = i - rr * d.cols;
            const int lo = cb[2 * x], cnt = cb[2 * x + 1];
            const int* k = ck + x * kstride;
            int s0 = 1 << (kPrecision - 1), s1 = s0, s2 = s0;
            if (dwords == 9) {                              // 27 bytes: eight dword reads, three coefficient reads
                taps_from_dwords<9>(rowbuf, rr * row_pitch + lo * 3, k, s0, s1, s2);
            } else if (dwords == 13) {                      // 39 bytes: eleven dword reads, four coefficient reads
                taps_from_dwords<13>(rowbuf, rr * row_pitch + lo * 3, k, s0, s1, s2);
            } else {
                const uint8_t* src = rowbuf + rr * row_pitch + lo * 3;
                for (int t = 0; t < cnt; ++t) {
                    const int w = k[t];
                    s0 += (int)src[3 * t] * w;
                    s1 += (int)src[3 * t + 1] * w;
                    s2 += (int)src[3 * t + 2] * w;
                }
            }
            uint8_t* dst = strip + (yc - y0 + rr) * strip_pitch + 3 * x;
            dst[0] = cnt ? (uint8_t)clip8(s0) : 0;
            dst[1] = cnt ? (uint8_t)clip8(s1) : 0;
            dst[2] = cnt ? (uint8_t)clip8(s2) : 0;
        }
        __syncthreads();
    }
    return y0;
}

// The vertical pass for channel c of the window pixel (row r0 + r, column x) from the strip: the resized byte, 0 outside.
template <bool kGuard>
__device__ __forceinline__ int window_byte(const BandView& d, const uint8_t* strip, int y0, int wr, int x, int c) {
    const int yr = d.top + wr, xr = resized_column(d, x), xs = x - d.x0;
    int v = 0;
    if (yr >= 0 && yr < d.Hr && xr >= 0 && xr < d.Wr && (!kGuard || (xs >= 0 && xs < d.cols))) {
        const int lo = d.bounds_v[2 * yr];
        int cnt = d.bounds_v[2 * yr + 1];
        if (kGuard && (lo < y0 || lo + cnt > y0 + d.strip_rows)) cnt = 0;
        const int* k = d.kk_v + yr * d.ksize_v;
        int ss = 1 << (kPrecision - 1);
        for (int t = 0; t < cnt; ++t) ss += (int)strip[(lo + t - y0) * (d.cols * 3) + xs * 3 + c] * k[t];
        v = clip8(ss);
    }
    return v;
}

// ToTensor + Normalize of one byte into the planar output
__device__ __forceinline__ void store_normalised(void* out, size_t o, int v, float mean, float std, int out_bf16) {
    const float f = ((float)v / 255.0f - mean) / std;
    if (out_bf16) {
        reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)(pack_bf16(f, 0.f) & 0xffffu);
    } else {
        reinterpret_cast<float*>(out)[o] = f;
    }
}

// vertical pass + ToTensor + Normalize of a band; planar output, x fastest
template <bool kGuard>
__device__ __forceinline__ void write_band_planar(const BandView& d, const uint8_t* strip, int y0, int n, int r0, int rows,
                                                  const float* mean, const float* std, int out_bf16, void* out) {
    const int per_plane = rows * d.Wo;
    for (int i = threadIdx.x; i < 3 * per_plane; i += 256) {
        const int c = i / per_plane, rem = i - c * per_plane;
        const int r = rem / d.Wo, x = rem - r * d.Wo;
        const int v = window_byte<kGuard>(d, strip, y0, r0 + r, x, c);
        store_normalised(out, (((size_t)n * 3 + c) * d.Ho + (r0 + r)) * d.Wo + x, v, mean[c], std[c], out_bf16);
    }
}

__global__ __launch_bounds__(256) void image_prep_kernel(ImageDims d, const uint8_t* __restrict__ images,
                                                         const int* __restrict__ kk_h, const int* __restrict__ bounds_h,
                                                         const int* __restrict__ kk_v, const int* __restrict__ bounds_v,
                                                         void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const BandView v = {d.H, d.W, d.Wr, d.Hr, d.left, d.top, d.Wo, d.Ho, d.ksize_h, d.ksize_v, d.strip_rows, 0, 0, d.Wo,
                        kk_h, bounds_h, kk_v, bounds_v};
    const int r0 = blockIdx.x * kRows, n = blockIdx.y;
    const int rows = min(kRows, d.Ho - r0);
    const int y0 = resample_band<false>(v, images + (size_t)n * d.H * (d.W * 3), r0, rows, smem);
    write_band_planar<false>(v, smem + kChunk * ((d.W * 3 + 15) & ~15), y0, n, r0, rows, d.mean, d.std, d.out_bf16, out);
}

struct AugDims {
    int N, H, W, Wo, Ho, cols, ksize, strip_rows, rotate, coef_len, out_bf16;
    float mean[3], std[3];
};

__device__ __forceinline__ bool rotation_is_identity(const stp3_augment_image& t) {
    return t.rot[0] == 65536 && t.rot[1] == 0 && t.rot[2] == 32768 && t.rot[3] == 0 && t.rot[4] == 65536 && t.rot[5] == 32768;
}

// every table of the entry lies inside coef
__device__ __forceinline__ bool entry_is_valid(const AugDims& d, const stp3_augment_image& t) {
    if (t.Wr < 1 || t.Hr < 1 || t.Wr > (1 << 20) || t.Hr > (1 << 20)) return false;
    if (t.left < -(1 << 24) || t.left > (1 << 24) || t.top < -(1 << 24) || t.top > (1 << 24)) return false;
    const long long len = d.coef_len;
    return t.kk_h >= 0 && t.bounds_h >= 0 && t.kk_v >= 0 && t.bounds_v >= 0 && t.kk_h + (long long)t.Wr * d.ksize <= len &&
           t.bounds_h + 2LL * t.Wr <= len && t.kk_v + (long long)t.Hr * d.ksize <= len && t.bounds_v + 2LL * t.Hr <= len;
}

__global__ __launch_bounds__(256) void image_augment_kernel(AugDims d, const uint8_t* __restrict__ images,
                                                            const stp3_augment_image* __restrict__ table,
                                                            const int* __restrict__ coef, uint8_t* __restrict__ window,
                                                            void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int r0 = blockIdx.x * kRows, n = blockIdx.y;
    const stp3_augment_image t = table[n];
    if (!entry_is_valid(d, t)) return;                     // (uniform over the workgroup)
    // the window columns inside the resized image (mirrored by the flip); the host sized `cols` for the widest image
    const int flip = t.flip != 0;
    const int xa = max(0, flip ? t.left + d.Wo - t.Wr : -t.left);
    const int xb = min(d.Wo, flip ? t.left + d.Wo : t.Wr - t.left);
    const BandView v = {d.H, d.W, t.Wr, t.Hr, t.left, t.top, d.Wo, d.Ho, d.ksize, d.ksize, d.strip_rows, flip,
                        min(xa, d.Wo), min(max(xb - xa, 0), d.cols),
                        coef + t.kk_h, coef + t.bounds_h, coef + t.kk_v, coef + t.bounds_v};
    const int rows = min(kRows, d.Ho - r0);
    const bool direct = !d.rotate || rotation_is_identity(t);      // (decided here: one scalar lives through the band, not six)
    const int y0 = resample_band<true>(v, images + (size_t)n * d.H * (d.W * 3), r0, rows, smem);
    const uint8_t* strip = smem + kChunk * ((d.W * 3 + 15) & ~15);
    if (direct) {
        write_band_planar<true>(v, strip, y0, n, r0, rows, d.mean, d.std, d.out_bf16, out);
        return;
    }
    // to be rotated: the cropped, flipped bytes [Ho][Wo][3], channel fastest (consecutive lanes, consecutive bytes)
    uint8_t* dst = window + ((size_t)n * d.Ho + r0) * d.Wo * 3;
    for (int i = threadIdx.x; i < rows * d.Wo * 3; i += 256) {
        const int px = i / 3, c = i - px * 3;
        const int r = px / d.Wo, x = px - r * d.Wo;
        dst[i] = (uint8_t)window_byte<true>(v, strip, y0, r0 + r, x, c);
    }
}

// Pillow's Image.rotate (Geometry.c affine_fixed: NEAREST, 16.16 fixed point, zero fill) of the byte windows + ToTensor +
// Normalize: one lane per output pixel, consecutive lanes consecutive x -- the three planar stores are coalesced, the
// three byte loads of a wave follow one slanted line of the window (322 KB per 224 x 480 image: L2-resident).
__global__ __launch_bounds__(256) void image_rotate_kernel(AugDims d, const stp3_augment_image* __restrict__ table,
                                                           const uint8_t* __restrict__ window, void* __restrict__ out) {
    const int n = blockIdx.y;
    const stp3_augment_image t = table[n];
    if (!entry_is_valid(d, t) || rotation_is_identity(t)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.Ho * d.Wo) return;
    const int y = i / d.Wo, x = i - y * d.Wo;
    // (unsigned: Pillow's int arithmetic, which does not overflow for Wo, Ho <= 8192 and the coefficients Pillow makes)
    const int xin = (int)((uint32_t)t.rot[2] + (uint32_t)x * (uint32_t)t.rot[0] + (uint32_t)y * (uint32_t)t.rot[1]) >> 16;
    const int yin = (int)((uint32_t)t.rot[5] + (uint32_t)x * (uint32_t)t.rot[3] + (uint32_t)y * (uint32_t)t.rot[4]) >> 16;
    const bool in = xin >= 0 && xin < d.Wo && yin >= 0 && yin < d.Ho;
    const uint8_t* src = window + (((size_t)n * d.Ho + (in ? yin : 0)) * d.Wo + (in ? xin : 0)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        store_normalised(out, (((size_t)n * 3 + c) * d.Ho + y) * d.Wo + x, in ? (int)src[c] : 0, d.mean[c], d.std[c], d.out_bf16);
}

}  // namespace

extern "C" {

int stp3_image_prep_lds_bytes(const stp3_image_dims* p, int32_t strip_rows, size_t* bytes) {
    if (!p || !bytes || strip_rows < 0) return STP3_EINVAL;
    *bytes = band_lds_bytes(p->W, p->Wo, p->ksize_h, strip_rows);
    return STP3_OK;
}

int stp3_image_prep(const stp3_image_dims* p, const uint8_t* images, const int32_t* kk_h, const int32_t* bounds_h,
                    const int32_t* kk_v, const int32_t* bounds_v, int32_t strip_rows, void* out, void* stream) {
    if (!p || !images || !kk_h || !bounds_h || !kk_v || !bounds_v || !out) return STP3_EINVAL;
    if (p->N <= 0 || p->H <= 0 || p->W <= 0 || p->Wr <= 0 || p->Hr <= 0 || p->Wo <= 0 || p->Ho <= 0 || p->ksize_h <= 0 ||
        p->ksize_v <= 0 || strip_rows <= 0)
        return STP3_EINVAL;
    if (p->out_dtype != STP3_DTYPE_F32 && p->out_dtype != STP3_DTYPE_BF16) return STP3_EUNSUP;
    if (p->N > 65535 || (int64_t)p->N * p->H * p->W * 3 >= (1LL << 40)) return STP3_EUNSUP;
    size_t lds = 0;
    stp3_image_prep_lds_bytes(p, strip_rows, &lds);
    if (lds > 160 * 1024) return STP3_EUNSUP;              // (a 1600 x 900 source at scale 0.3: 78 KB)
    ImageDims d;
    d.N = p->N; d.H = p->H; d.W = p->W; d.Wr = p->Wr; d.Hr = p->Hr; d.left = p->left; d.top = p->top; d.Wo = p->Wo;
    d.Ho = p->Ho; d.ksize_h = p->ksize_h; d.ksize_v = p->ksize_v; d.out_bf16 = p->out_dtype == STP3_DTYPE_BF16;
    d.strip_rows = strip_rows; d.inv255_unused = 0.f;
    for (int c = 0; c < 3; ++c) { d.mean[c] = p->mean[c]; d.std[c] = p->std[c]; }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&image_prep_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(image_prep_kernel, dim3((p->Ho + kRows - 1) / kRows, p->N), dim3(256), lds, (hipStream_t)stream, d,
                       images, kk_h, bounds_h, kk_v, bounds_v, out);
    e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

int stp3_image_prep_rows_per_workgroup(void) { return kRows; }

int stp3_image_augment_workspace_bytes(const stp3_augment_dims* p, size_t* bytes) {
    if (!p || !bytes || p->N <= 0 || p->Wo <= 0 || p->Ho <= 0 || p->Wo > 8192 || p->Ho > 8192) return STP3_EINVAL;
    *bytes = p->rotate ? (size_t)p->N * p->Ho * p->Wo * 3 : 0;
    return STP3_OK;
}

int stp3_image_augment(const stp3_augment_dims* p, const uint8_t* images, const stp3_augment_image* table,
                       const int32_t* coef, void* workspace, size_t workspace_bytes, void* out, void* stream) {
    if (!p || !images || !table || !coef || !out) return STP3_EINVAL;
    if (p->N <= 0 || p->H <= 0 || p->W <= 0 || p->Wo <= 0 || p->Ho <= 0 || p->ksize <= 0 || p->strip_rows <= 0 ||
        p->coef_len <= 0 || (p->rotate != 0 && p->rotate != 1) || p->cols <= 0 || p->cols > p->Wo)
        return STP3_EINVAL;
    if (p->Wo > 8192 || p->Ho > 8192) return STP3_EINVAL;   // Pillow accumulates the rotation's addresses in 32 bits
    if (p->out_dtype != STP3_DTYPE_F32 && p->out_dtype != STP3_DTYPE_BF16) return STP3_EUNSUP;
    if (p->N > 65535 || (int64_t)p->N * p->H * p->W * 3 >= (1LL << 40) || p->W > (1 << 20) || p->ksize > 4096) return STP3_EUNSUP;
    if (p->rotate && (!workspace || workspace_bytes < (size_t)p->N * p->Ho * p->Wo * 3)) return STP3_EINVAL;
    if ((int64_t)p->strip_rows * p->Wo * 3 > (1 << 20)) return STP3_EUNSUP;
    const size_t lds = band_lds_bytes(p->W, p->cols, p->ksize, p->strip_rows);
    if (lds > 160 * 1024) return STP3_EUNSUP;
    AugDims d;
    d.N = p->N; d.H = p->H; d.W = p->W; d.Wo = p->Wo; d.Ho = p->Ho; d.cols = p->cols; d.ksize = p->ksize;
    d.strip_rows = p->strip_rows;
    d.rotate = p->rotate; d.coef_len = p->coef_len; d.out_bf16 = p->out_dtype == STP3_DTYPE_BF16;
    for (int c = 0; c < 3; ++c) { d.mean[c] = p->mean[c]; d.std[c] = p->std[c]; }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&image_augment_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(image_augment_kernel, dim3((p->Ho + kRows - 1) / kRows, p->N), dim3(256), lds, (hipStream_t)stream, d,
                       images, table, coef, static_cast<uint8_t*>(workspace), out);
    e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    if (p->rotate) {
        hipLaunchKernelGGL(image_rotate_kernel, dim3((p->Ho * p->Wo + 255) / 256, p->N), dim3(256), 0, (hipStream_t)stream, d,
                           table, static_cast<const uint8_t*>(workspace), out);
        e = hipGetLastError();
    }
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
