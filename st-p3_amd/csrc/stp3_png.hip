// stp3_png.hip -- PNG images of the CARLA loader: the dense half of a decode on gfx950 (include/stp3_hip.h, "PNG scanlines").
//
// DEFLATE is serial and stays on the host (zlib, stp3_amd.datas.PngDecoder.inflate); what it leaves is one filter byte and
// W * bpp filtered bytes per scanline.  Undoing the filters (PNG specification, section 9: None, Sub, Up, Average, Paeth) is
// integer arithmetic modulo 256 with an exact definition, so the output is BYTE-EXACT with any conforming decoder:
//     a = the reconstructed byte bpp to the left (0 for x < bpp), b = the byte above (0 in row 0), c = the byte above-left
//     None + 0 | Sub + a | Up + b | Average + ((a + b) >> 1) on the 9-bit sum | Paeth + the one of a, b, c nearest to a + b - c
//     (ties: a before b before c)
// Average and Paeth are non-linear recurrences along the row (through a) AND down the image (through b, c): pixel (r, x) needs
// (r, x - 1), (r - 1, x) and (r - 1, x - 1).  The anti-diagonals r + x = const are independent, which is what the kernel uses:
//
// ONE workgroup of up to kMaxWaves waves per image.  A wave owns a band of 64 rows: lane l owns row l of the band and
// reconstructs pixel x = s - l at the wave's step s (all bpp bytes of a pixel in one 32-bit register); b is the previous step's
// result of lane l - 1 (one __shfl_up per step), c is the previous b, a the lane's own previous result.  Wave w works on the
// band below wave w - 1 and runs kLag steps behind it: the last row of the band above reaches its lane 0 through a ring in LDS.
// Time advances in chunks of kChunk steps with workgroup barriers between them; kLag >= kChunk + 63 puts a barrier between
// every write of the ring and its read.  The nw bands of a pass take W + 63 + (nw - 1) kLag steps instead of nw (W + 63); an
// image of more than 64 nw rows takes several passes, the last row of a pass waiting in LDS (one dword per pixel) for wave 0.
// Per chunk a wave stages the 64 x kChunk pixels its lanes will meet -- a parallelogram, row j shifted by j -- through LDS:
// row-contiguous loads and stores for the memory system, one row per lane for the arithmetic, the result written in place.
// The bytes of the next chunk are loaded into registers while the current one is computed.
// Waves depend on each other through __syncthreads only; nothing spins, nothing is read back from global memory.
//
// The kernel is total: the filter byte selects arithmetic only (anything above 4 adds 0, as None), every address is a function
// of n, H, W, bpp and the thread's indices.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "stp3_hip.h"

namespace {

constexpr int kBand = 64;               // rows per wave = lanes
constexpr int kChunk = 16;              // steps between two workgroup barriers
constexpr int kLag = 80;                // steps a wave runs behind the wave above it
constexpr int kRing = 128;              // dwords of the ring between two waves
constexpr int kMaxWaves = 8;
constexpr int kMaxSide = 16384;         // carry row: 4 * 16 384 bytes of LDS
constexpr int kMaxDevices = 64;
// a value written to the ring in one chunk is read in a later one, and is read before the slot is written again
static_assert(kLag >= kChunk + kBand - 1 && kRing >= kLag - (kBand - 1) + kChunk, "ring protocol");

__host__ __device__ constexpr int tile_pitch(int bpp) { return kChunk * bpp + 4; }     // bytes; an odd number of dwords: lanes on distinct banks

__host__ __device__ inline size_t png_lds_bytes(int W, int bpp, int nw) {
    return ((size_t)W + (size_t)nw * kRing) * sizeof(uint32_t) + (size_t)nw * kBand * tile_pitch(bpp);
}

// one channel: the filtered byte `raw` + the predictor of filter type `ft`
__device__ __forceinline__ uint32_t unfilter_byte(int ft, int raw, int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);      // |p - a|, |p - b|, |p - c| for p = a + b - c
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    return (uint32_t)(raw + pred) & 255u;
}

template <int BPP>
__global__ __launch_bounds__(kBand * kMaxWaves) void png_unfilter_kernel(const uint8_t* __restrict__ rows, int H, int W,
                                                                         uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr int kPitch = tile_pitch(BPP), kBytes = kChunk * BPP;           // of one row of the tile
    constexpr int kRows = kBand / kBytes, kIters = kBand / kRows;            // tile rows per instruction, instructions per tile
    static_assert(kBytes <= kBand && kIters % 4 == 0, "a tile row is at most one instruction wide");
    const int lane = threadIdx.x & (kBand - 1), wave = threadIdx.x / kBand, nw = blockDim.x / kBand;
    uint32_t* carry = lds;                                                    // [W]: the last row of the pass before
    uint32_t* ring = carry + W + wave * kRing;                                // [kRing]: the last row of the wave above, by x % kRing
    uint8_t* tile = reinterpret_cast<uint8_t*>(carry + W + nw * kRing) + wave * kBand * kPitch;
    const int line = W * BPP;
    const size_t pitch = 1 + (size_t)line;
    const uint8_t* image = rows + (size_t)blockIdx.x * H * pitch;
    uint8_t* image_out = out + (size_t)blockIdx.x * H * line;

    for (int r0 = 0; r0 < H; r0 += nw * kBand) {
        const int active_waves = (min(nw * kBand, H - r0) + kBand - 1) / kBand;
        const int band = r0 + wave * kBand;                                   // first row of this wave's band
        const bool valid = band + lane < H;
        const int ft = image[(size_t)min(band + lane, H - 1) * pitch];        // (a lane past the image reads the last row's)
        const int total = W + kBand - 1 + (active_waves - 1) * kLag;
        auto busy_at = [&](int s0) { return wave < active_waves && s0 + kChunk > 0 && s0 < W + kBand - 1; };
        // The tile of the chunk that starts at step s0: row j holds pixels s0 - j .. s0 - j + kChunk - 1 of row band + j.  An
        // instruction moves kRows rows of it, kBytes consecutive lanes the consecutive bytes of one row; from one instruction
        // to the next every lane advances by the same number of bytes.  A lane's kIters bytes wait four to a register.  An
        // offset outside the image (rows past H, pixels left or right of a row) is clamped into it, loaded and never used.
        const int lane_row = lane / kBytes, lane_byte = lane % kBytes;
        const bool lane_used = lane_row < kRows;
        const int image_bytes = H * (int)pitch;                               // (< 2^31: sides are at most 16 384)
        uint32_t staged[kIters / 4];
        auto fetch = [&](int s0) {
            const int first = (band + lane_row) * (int)pitch + 1 + (s0 - lane_row) * BPP + lane_byte;
            const int stride = kRows * ((int)pitch - BPP);
#pragma unroll
            for (int m = 0; m < kIters; ++m) {
                const uint32_t v = image[min(max(first + m * stride, 0), image_bytes - 1)];
                staged[m / 4] = (m % 4 ? staged[m / 4] : 0u) | v << (8 * (m % 4));
            }
        };
        uint32_t left = 0, corner = 0, last = 0;
        if (busy_at(-wave * kLag)) fetch(-wave * kLag);
        for (int g0 = 0; g0 < total; g0 += kChunk) {
            const int s0 = g0 - wave * kLag;                                  // this wave's first step of the chunk
            const bool busy = busy_at(s0);
            if (busy && lane_used) {
#pragma unroll
                for (int m = 0; m < kIters; ++m)
                    tile[(m * kRows + lane_row) * kPitch + lane_byte] = (uint8_t)(staged[m / 4] >> (8 * (m % 4)));
            }
            __syncthreads();
            if (busy_at(s0 + kChunk)) fetch(s0 + kChunk);                     // in flight while this chunk is computed
            if (busy) {
                // what the chain does not produce is read before it starts: this lane's row of the tile and, for lane 0, the
                // row above the band (written in earlier chunks, see kLag)
                uint32_t* mine = reinterpret_cast<uint32_t*>(tile + lane * kPitch);
                uint32_t raw[kBytes / 4], done[kBytes / 4], above[kChunk];
#pragma unroll
                for (int t = 0; t < kBytes / 4; ++t) { raw[t] = mine[t]; done[t] = 0; }
#pragma unroll
                // (x outside the row is clamped: such a read may meet a slot the wave above is writing in this very chunk -- its
                // value is never used, `corner` is reset at x <= 0 and the lane is inactive from x = W on; every value that IS
                // used was written at least one chunk earlier and is rewritten at least kRing - kLag + 63 steps later)
                for (int u = 0; u < kChunk; ++u) {
                    const int xc = min(max(s0 + u, 0), W - 1);
                    above[u] = wave > 0 ? ring[xc & (kRing - 1)] : r0 > 0 ? carry[xc] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    const int x = s0 + u - lane;
                    const bool active = valid && x >= 0 && x < W;
                    uint32_t up = __shfl_up(last, 1);                         // row above, pixel x: lane l - 1 one step ago
                    if (lane == 0) up = above[u];                             // ... or the band above, or nothing
                    if (x <= 0) { left = 0; corner = 0; }
                    uint32_t px = 0;
#pragma unroll
                    for (int k = 0; k < BPP; ++k) {
                        const int at = u * BPP + k;
                        const uint32_t v = unfilter_byte(ft, (raw[at / 4] >> (8 * (at % 4))) & 255, (left >> (8 * k)) & 255,
                                                         (up >> (8 * k)) & 255, (corner >> (8 * k)) & 255);
                        px |= v << (8 * k);
                        done[at / 4] |= v << (8 * (at % 4));                  // (a lane outside its row: never stored)
                    }
                    corner = up;
                    if (active) {
                        left = last = px;
                        if (lane == kBand - 1) {
                            if (wave + 1 < nw) ring[kRing + (x & (kRing - 1))] = px;      // the next wave's ring
                            else carry[x] = px;                                            // wave 0 of the next pass
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < kBytes / 4; ++t) mine[t] = done[t];
            }
            __syncthreads();
            if (busy && lane_used) {                                          // the finished pixels of the tile, row-contiguous
#pragma unroll 8
                for (int m = 0; m < kIters; ++m) {
                    const int j = m * kRows + lane_row, byte = (s0 - j) * BPP + lane_byte;
                    if (band + j < H && byte >= 0 && byte < line) image_out[(size_t)(band + j) * line + byte] = tile[j * kPitch + lane_byte];
                }
            }
            __syncthreads();                                                  // the tile is free, ring and carry are written
        }
    }
}

template <int BPP>
int launch(int n, int H, int W, const uint8_t* rows, uint8_t* out, hipStream_t stream) {
    const int nw = min(kMaxWaves, (H + kBand - 1) / kBand);
    const size_t lds = png_lds_bytes(W, BPP, nw);
    // The limit of dynamic LDS is raised ONCE per device, to what the largest image takes: a value per call would let two host
    // threads with different widths undo each other's, and would put a host call in front of every launch.
    static std::atomic<bool> raised[kMaxDevices];
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return -(int)e;
    if (device < 0 || device >= kMaxDevices) return STP3_EUNSUP;
    if (!raised[device].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&png_unfilter_kernel<BPP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)png_lds_bytes(kMaxSide, BPP, kMaxWaves));
        if (e != hipSuccess) return -(int)e;
        raised[device].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(png_unfilter_kernel<BPP>, dim3(n), dim3(nw * kBand), lds, stream, rows, H, W, out);
    e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // namespace

extern "C" {

int stp3_png_unfilter(const uint8_t* rows, int32_t n, int32_t height, int32_t width, int32_t bpp, uint8_t* out, void* stream) {
    if (!rows || !out || n < 1 || height < 1 || width < 1 || bpp < 1 || bpp > 4) return STP3_EINVAL;
    if (height > kMaxSide || width > kMaxSide) return STP3_EUNSUP;
    hipStream_t s = (hipStream_t)stream;
    switch (bpp) {
        case 1: return launch<1>(n, height, width, rows, out, s);
        case 2: return launch<2>(n, height, width, rows, out, s);
        case 3: return launch<3>(n, height, width, rows, out, s);
        default: return launch<4>(n, height, width, rows, out, s);
    }
}

}  // extern "C"
