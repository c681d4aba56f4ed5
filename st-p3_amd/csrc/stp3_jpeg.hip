// stp3_jpeg.hip -- JPEG camera frames: the dense half of a baseline decode on gfx950 (include/stp3_hip.h, "JPEG camera frames").
//
// The Huffman bit stream is serial and stays on the host (stp3_jpeg_entropy.h, wrapped below as stp3_jpeg_info /
// stp3_jpeg_entropy); what follows it -- dequantisation, the 8 x 8 inverse DCT, chroma up-sampling, YCbCr -> RGB -- is integer
// arithmetic over every pixel and runs here, BYTE-EXACT with what Pillow (libjpeg-turbo, its defaults) returns:
//     jidctint.c   jpeg_idct_islow     CONST_BITS 13, PASS1_BITS 2: columns first (descale 11), then rows (descale 18), the
//                                      sample = range_limit[v & 1023] (the clamp of v + 128 for v in [-512, 511]; it wraps)
//     jdsample.c   h2v1 / h2v2 fancy   triangle filter over the component's TRUE size ceil(W / 2) x ceil(H / 2); plain
//                                      replication when that width is 2 or less (libjpeg's own rule, reproduced here)
//     jdmainct.c   context rows        the row above the first and below the last REAL chroma row replicate that row
//     jdcolor.c    ycc_rgb_convert     16-bit scaled tables: 91881, 116130, -22554, -46802, rounding 32768
//
// ONE launch, samples never leave LDS: a workgroup owns kStripMcuRows MCU rows of one image.  Phase 1 reconstructs the
// blocks of the strip into byte planes in LDS -- 8 lanes per block: one column each, an exchange through LDS, one row each
// -- and, for 4:2:0, the last sample row of the chroma block row above and the first of the one below (recomputed: the halo
// of the vertical filter).  Phase 2 up-samples, converts and stores RGB rows: a lane owns 4 consecutive pixels = 12 bytes,
// consecutive lanes consecutive groups.  Traffic is the compulsory 3 B/px in + 3 B/px out plus the halo's coefficients.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_hip.h"
#include "stp3_jpeg_entropy.h"

namespace {

constexpr int kStripMcuRows = 2;        // MCU rows per workgroup (4:2:0: 32 pixel rows; halo: 2 of 6 chroma block rows)
constexpr int kThreads = 1024;          // 128 blocks per pass; one workgroup per CU (1600 px wide 4:2:0: 117 248 bytes of LDS)
constexpr int kBlocksPerPass = kThreads / 8;
// dwords per block in the exchange buffer: 64 + 8, so that the 8 blocks of a wave start 8 banks apart -- at 64 the lanes of
// a column-pass store (block b, row r, column c -> b * kWs + 8 r + c) met 8 to a bank
constexpr int kWs = 72;

struct JpegDims {
    int N, W, H, nc, hs, vs, mcus_x, mcus_y;
    int Wc, Hc;                         // true chroma size
    int fancy;                          // libjpeg: fancy up-sampling only when the chroma width exceeds 2
    int coef_count;
};

__host__ __device__ inline int chroma_lds_rows(int vs) { return kStripMcuRows * 8 + (vs == 2 ? 2 : 0); }

__host__ __device__ inline size_t jpeg_lds_bytes(int nc, int hs, int vs, int mcus_x) {
    size_t b = (size_t)kBlocksPerPass * kWs * sizeof(int32_t) + 192 * sizeof(uint16_t);
    b += (size_t)kStripMcuRows * 8 * vs * mcus_x * hs * 8;
    if (nc == 3) b += 2 * (size_t)chroma_lds_rows(vs) * mcus_x * 8;
    return (b + 15) & ~(size_t)15;
}

// jidctint.c: one 8-point pass of jpeg_idct_islow; DESCALE by `shift`.  The sums are formed in uint32_t -- two's complement
// wrap, the same bits as int32 wherever int32 does not overflow, and defined where it would (the entropy decoder bounds
// |coefficient * quantiser| by 32767, which no legal stream approaches; the bytes are claimed equal to Pillow's inside it).
__device__ __forceinline__ void idct8(const int* in, int* out, int shift) {
    typedef uint32_t u;
    u z2 = (u)in[2], z3 = (u)in[6];
    u z1 = (z2 + z3) * 4433u;
    u tmp2 = z1 - z3 * 15137u;
    u tmp3 = z1 + z2 * 6270u;
    z2 = (u)in[0]; z3 = (u)in[4];
    u tmp0 = (z2 + z3) * 8192u;
    u tmp1 = (z2 - z3) * 8192u;
    const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (u)in[7]; tmp1 = (u)in[5]; tmp2 = (u)in[3]; tmp3 = (u)in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    u z4 = tmp1 + tmp3;
    const u z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995; z3 *= (u)-16069; z4 *= (u)-3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const u half = 1u << (shift - 1);
    out[0] = (int)(tmp10 + tmp3 + half) >> shift; out[7] = (int)(tmp10 - tmp3 + half) >> shift;
    out[1] = (int)(tmp11 + tmp2 + half) >> shift; out[6] = (int)(tmp11 - tmp2 + half) >> shift;
    out[2] = (int)(tmp12 + tmp1 + half) >> shift; out[5] = (int)(tmp12 - tmp1 + half) >> shift;
    out[3] = (int)(tmp13 + tmp0 + half) >> shift; out[4] = (int)(tmp13 - tmp0 + half) >> shift;
}

// jdmaster.c prepare_range_limit_table, as the IDCT indexes it
__device__ __forceinline__ uint32_t range_limit(int v) {
    const int i = v & 1023;
    return (uint32_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

__device__ __forceinline__ int clamp_byte(int v) { return min(max(v, 0), 255); }

// one chroma sample at full resolution: pixel (x, y) of component plane `p` (LDS rows of `pitch` bytes; row_of maps a chroma
// row to its LDS row)
struct ChromaView {
    const uint8_t* p;
    int pitch, row0;                    // LDS row of chroma row r: r - row0
};

__device__ __forceinline__ int chroma_at(const JpegDims& d, const ChromaView& c, int x, int y) {
    if (d.hs == 1) return c.p[(y - c.row0) * c.pitch + x];
    const int i = x >> 1;
    if (!d.fancy) return c.p[((d.vs == 2 ? y >> 1 : y) - c.row0) * c.pitch + i];
    if (d.vs == 1) {                                        // h2v1_fancy_upsample
        const uint8_t* s = c.p + (y - c.row0) * c.pitch;
        if (x & 1) return i == d.Wc - 1 ? s[i] : (3 * s[i] + s[i + 1] + 2) >> 2;
        return i == 0 ? s[0] : (3 * s[i] + s[i - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                  // h2v2_fancy_upsample
    const int fy = min(max((y & 1) ? cy + 1 : cy - 1, 0), d.Hc - 1);
    const uint8_t* s0 = c.p + (cy - c.row0) * c.pitch;
    const uint8_t* s1 = c.p + (fy - c.row0) * c.pitch;
    const int here = 3 * s0[i] + s1[i];
    if (x & 1) return i == d.Wc - 1 ? (4 * here + 7) >> 4 : (3 * here + 3 * s0[i + 1] + s1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * here + 8) >> 4 : (3 * here + 3 * s0[i - 1] + s1[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(kThreads) void jpeg_reconstruct_kernel(JpegDims d, const int16_t* __restrict__ coef,
                                                                    const uint16_t* __restrict__ quant,
                                                                    uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int m0 = blockIdx.x * kStripMcuRows, m1 = min(m0 + kStripMcuRows, d.mcus_y);
    const int bx_y = d.mcus_x * d.hs, bx_c = d.mcus_x;     // blocks per block row
    const int by_y = d.mcus_y * d.vs;
    const int pitch_y = bx_y * 8, pitch_c = bx_c * 8;
    const int crows = chroma_lds_rows(d.vs);
    const int halo = d.vs == 2 ? 1 : 0;                     // LDS row 0 of a chroma plane is chroma row m0 * 8 - halo
    int32_t* ws = reinterpret_cast<int32_t*>(smem);         // [kBlocksPerPass][kWs]: the column pass' results, [8][8] + pad
    uint16_t* q = reinterpret_cast<uint16_t*>(ws + kBlocksPerPass * kWs);   // this image's tables
    uint8_t* plane_y = reinterpret_cast<uint8_t*>(q + 192);
    uint8_t* plane_c = plane_y + kStripMcuRows * 8 * d.vs * pitch_y;       // Cb then Cr, [crows][pitch_c] each

    for (int i = tid; i < 192; i += kThreads) q[i] = quant[(size_t)n * 192 + i];
    __syncthreads();

    // ---- phase 1: blocks -> samples in LDS --------------------------------------------------------------------------
    const int16_t* image = coef + (size_t)n * d.coef_count;
    const int n_y = (m1 - m0) * d.vs * bx_y;                // luma blocks of the strip
    const int n_c = d.nc == 3 ? (m1 - m0) * bx_c : 0;       // blocks of one chroma component
    const bool top = halo && m0 > 0, bottom = halo && m1 < d.mcus_y;
    const int n_top = top ? bx_c : 0, n_bottom = bottom ? bx_c : 0;
    const int total = n_y + 2 * (n_c + n_top + n_bottom);
    const size_t plane_blocks_y = (size_t)bx_y * by_y, plane_blocks_c = (size_t)bx_c * d.mcus_y;
    const int sub = tid >> 3, lane = tid & 7;
    // the task of a block: component, block row and column in its plane, which row to keep (-1: all) and where it goes
    struct Task { int comp, brow, bcol, keep, lds_row; };
    auto locate = [&](int t) {
        Task k = {0, 0, 0, -1, 0};
        if (t < n_y) {
            k.brow = m0 * d.vs + t / bx_y; k.bcol = t % bx_y;
            k.lds_row = (k.brow - m0 * d.vs) * 8;
            return k;
        }
        t -= n_y;
        const int per = n_c + n_top + n_bottom;
        k.comp = 1 + t / per;
        t %= per;
        if (t < n_c) {
            k.brow = m0 + t / bx_c; k.bcol = t % bx_c;
            k.lds_row = (k.brow - m0) * 8 + halo;
        } else if (t < n_c + n_top) {
            k.brow = m0 - 1; k.bcol = t - n_c; k.keep = 7;
            k.lds_row = 0;
        } else {
            k.brow = m1; k.bcol = t - n_c - n_top; k.keep = 0;
            k.lds_row = (m1 - m0) * 8 + 1;
        }
        return k;
    };
    // this lane's column of the block of the NEXT pass: the loads are in flight while the current pass computes and waits at
    // its barriers (one workgroup per CU: nothing else hides their latency)
    int raw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int t) {
        if (t >= total) return;
        const Task k = locate(t);
        const size_t blk = k.comp == 0 ? (size_t)k.brow * bx_y + k.bcol
                                       : plane_blocks_y + (k.comp - 1) * plane_blocks_c + (size_t)k.brow * bx_c + k.bcol;
        const int16_t* src = image + blk * 64;
#pragma unroll
        for (int r = 0; r < 8; ++r) raw[r] = (int)src[r * 8 + lane];
    };
    fetch(sub);
    for (int base = 0; base < total; base += kBlocksPerPass) {
        const int t = base + sub;
        const bool active = t < total;
        const Task k = locate(active ? t : 0);
        const int comp = k.comp, bcol = k.bcol, keep = k.keep, lds_row = k.lds_row;
        int in[8];
        const uint16_t* qc = q + comp * 64;
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = raw[r] * (int)qc[r * 8 + lane];
        fetch(t + kBlocksPerPass);
        if (active) {
            int col[8];
            idct8(in, col, 13 - 2);
#pragma unroll
            for (int r = 0; r < 8; ++r) ws[sub * kWs + r * 8 + lane] = col[r];
        }
        __syncthreads();
        if (active && (keep < 0 || keep == lane)) {         // lane = the row of the block
            int row[8];
            const int4 a = reinterpret_cast<const int4*>(ws + sub * kWs + lane * 8)[0];
            const int4 b = reinterpret_cast<const int4*>(ws + sub * kWs + lane * 8)[1];
            in[0] = a.x; in[1] = a.y; in[2] = a.z; in[3] = a.w; in[4] = b.x; in[5] = b.y; in[6] = b.z; in[7] = b.w;
            idct8(in, row, 13 + 2 + 3);
            uint8_t* plane = comp == 0 ? plane_y : plane_c + (comp - 1) * crows * pitch_c;
            const int pitch = comp == 0 ? pitch_y : pitch_c;
            const int r = keep < 0 ? lds_row + lane : lds_row;
            uint2 v;
            v.x = range_limit(row[0]) | range_limit(row[1]) << 8 | range_limit(row[2]) << 16 | range_limit(row[3]) << 24;
            v.y = range_limit(row[4]) | range_limit(row[5]) << 8 | range_limit(row[6]) << 16 | range_limit(row[7]) << 24;
            *reinterpret_cast<uint2*>(plane + r * pitch + bcol * 8) = v;
        }
        __syncthreads();
    }

    // ---- phase 2: up-sample, convert, store ------------------------------------------------------------------------
    const int y0 = m0 * 8 * d.vs, y1 = min(m1 * 8 * d.vs, d.H);
    const int groups = (d.W + 3) >> 2;
    const ChromaView cb = {plane_c, pitch_c, m0 * 8 - halo};
    const ChromaView cr = {plane_c + crows * pitch_c, pitch_c, m0 * 8 - halo};
    uint8_t* image_out = out + (size_t)n * d.H * d.W * 3;
    const bool words = (d.W & 3) == 0 && ((uintptr_t)out & 3) == 0;
    for (int i = tid; i < (y1 - y0) * groups; i += kThreads) {
        const int y = y0 + i / groups, x0 = (i % groups) * 4;
        uint32_t px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = min(x0 + k, d.W - 1);
            const int luma = plane_y[(y - y0) * pitch_y + x];
            if (d.nc == 1) {
                px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (uint32_t)luma;
            } else {
                const int u = chroma_at(d, cb, x, y) - 128, v = chroma_at(d, cr, x, y) - 128;
                px[3 * k] = (uint32_t)clamp_byte(luma + ((91881 * v + 32768) >> 16));
                px[3 * k + 1] = (uint32_t)clamp_byte(luma + ((-22554 * u + 32768 - 46802 * v) >> 16));
                px[3 * k + 2] = (uint32_t)clamp_byte(luma + ((116130 * u + 32768) >> 16));
            }
        }
        uint8_t* dst = image_out + ((size_t)y * d.W + x0) * 3;
        if (words) {
            uint32_t* w = reinterpret_cast<uint32_t*>(dst);
            w[0] = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
            w[1] = px[4] | px[5] << 8 | px[6] << 16 | px[7] << 24;
            w[2] = px[8] | px[9] << 8 | px[10] << 16 | px[11] << 24;
        } else {
            const int valid = min(4, d.W - x0) * 3;
            for (int k = 0; k < valid; ++k) dst[k] = (uint8_t)px[k];
        }
    }
}

int check_dims(const stp3_jpeg_dims* p, JpegDims* d) {
    if (!p || p->N <= 0 || p->width <= 0 || p->height <= 0) return STP3_EINVAL;
    if (p->components != 1 && p->components != 3) return STP3_EINVAL;
    const bool hv = (p->hs == 1 && p->vs == 1) || (p->components == 3 && p->hs == 2 && (p->vs == 1 || p->vs == 2));
    if (!hv) return STP3_EINVAL;
    if (p->width > stp3_jpeg::kMaxSide || p->height > stp3_jpeg::kMaxSide || p->N > 65535) return STP3_EUNSUP;
    d->N = p->N; d->W = p->width; d->H = p->height; d->nc = p->components; d->hs = p->hs; d->vs = p->vs;
    d->mcus_x = (p->width + 8 * p->hs - 1) / (8 * p->hs);
    d->mcus_y = (p->height + 8 * p->vs - 1) / (8 * p->vs);
    d->Wc = (p->width + p->hs - 1) / p->hs;
    d->Hc = (p->height + p->vs - 1) / p->vs;
    d->fancy = d->Wc > 2;
    const int64_t blocks = (int64_t)d->mcus_x * d->mcus_y * (p->hs * p->vs + (p->components == 3 ? 2 : 0));
    d->coef_count = (int)(blocks * 64);
    return STP3_OK;
}

}  // namespace

extern "C" {

int stp3_jpeg_info(const uint8_t* data, size_t len, stp3_jpeg_header* header) { return stp3_jpeg::info(data, len, header); }

int stp3_jpeg_entropy(const uint8_t* data, size_t len, int16_t* coef, size_t coef_capacity, uint16_t* quant,
                      stp3_jpeg_header* header) {
    return stp3_jpeg::entropy(data, len, coef, coef_capacity, quant, header);
}

int stp3_jpeg_strip_rows(int32_t vs) { return kStripMcuRows * 8 * (vs == 2 ? 2 : 1); }

int stp3_jpeg_reconstruct(const stp3_jpeg_dims* p, const int16_t* coef, const uint16_t* quant, uint8_t* out, void* stream) {
    JpegDims d;
    const int rc = check_dims(p, &d);
    if (rc != STP3_OK) return rc;
    if (!coef || !quant || !out) return STP3_EINVAL;
    const size_t lds = jpeg_lds_bytes(d.nc, d.hs, d.vs, d.mcus_x);
    if (lds > 160 * 1024) return STP3_EUNSUP;               // (about 2 500 pixels wide, whatever the sampling)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&jpeg_reconstruct_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(jpeg_reconstruct_kernel, dim3((d.mcus_y + kStripMcuRows - 1) / kStripMcuRows, d.N), dim3(kThreads), lds,
                       (hipStream_t)stream, d, coef, quant, out);
    e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
