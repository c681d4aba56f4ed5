// stp3_jpeg_huff.hip -- JPEG camera frames: the Huffman scan of a baseline stream decoded on gfx950 (include/stp3_hip.h, "the
// Huffman scan ON THE DEVICE"), into the coefficient buffers csrc/stp3_jpeg.hip reconstructs from.
//
// A Huffman stream is serial only until a decoder started at a wrong bit falls into step with the right one, which it does
// after a few codes (Klein & Wiseman 2003); Weissenberger & Schmidt (ICPP 2018) build a GPU decoder on that.  Here, adapted to
// JPEG's block structure: the scan (unstuffed and cut into segments at the restart markers by stp3_jpeg_scan_prepare) is cut
// into SUBSEQUENCES of kS bytes, one thread each, kG per workgroup.  The state of a decoder at a subsequence edge is
//     (bit position, block index within the MCU, zigzag index: 0 = the DC code is next)
// and fits one 32-bit word (the bit position relative to the edge: a symbol is at most 16 + 15 bits long).
//   sync    thread i decodes subsequence i from the assumed state "at the edge, first block of an MCU, DC next" (certain
//           for the first subsequence of a segment), records the state it leaves with as the ENTRY state of i + 1 and the
//           blocks it completed, then runs on: in round r it decodes subsequence i + r from its own state and overwrites
//           both records, until the entry state it would record is the one already there (from then on it would only
//           repeat its neighbour) or it reaches the end of the segment or of the workgroup.  Rounds are separated by a
//           barrier, so the later round -- the thread that started further left and knows more -- wins.  When no thread is
//           active the records inside the workgroup follow from its first entry state.  That state comes from the left
//           neighbour: launch L reads what the neighbour left in launch L - 1 (a ping-pong pair of edge arrays: no
//           workgroup waits for another), and only thread 0 has work, only if it changed.  A launch sets the image's
//           "changed" word when an edge state it writes differs from what the right neighbour consumed in the same launch;
//           a launch without such a change proves every record right, and the launches after it return at once.
//   scan    exclusive prefix sum of the blocks completed per subsequence: the first block number of each.
//   write   every thread decodes its subsequence again from its recorded entry state and stores AC values and the DC
//           DIFFERENCE of each block; here a code no table assigns, a run past 63 ... are errors (in `sync` a thread at a wrong
//           bit meets them all the time: it skips one bit and goes on).
//   dc      per component and segment: the running sum of the DC differences in decode order, bounded as the host bounds it.
//   status  one word per image.
// The bytes are UNTRUSTED and the machine is shared: every loop has a bound the host fixed, no loop waits for another
// workgroup, reads behind the image's subsequences give zeros, every store index is compared with coef_count.
// Plain C++ with LDS, barriers and atomicAdd: tests/hipcpu runs this source as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stp3_hip.h"
#include "stp3_jpeg_entropy.h"

namespace {

constexpr int kS = STP3_JPEG_SUB_BYTES;             // bytes per subsequence
constexpr int kSB = kS * 8;                         // bits per subsequence
constexpr int kG = STP3_JPEG_SUB_THREADS;           // subsequences per workgroup
constexpr int kMaxRounds = 64;
constexpr int kDcGrid = 2048;                       // workgroups along the segments in the DC pass
static_assert(sizeof(stp3_jpeg_huff_table) == 1420 && sizeof(stp3_jpeg_huff_table) % 4 == 0, "copied to LDS in dwords");

__device__ const uint8_t kZigzagToNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffDims {
    int N, nc, hs, vs, mcus_x, mcus_y, bpm, total_mcus, coef_count;
    int stride, max_subs, max_segs, nwg, rounds;
    int dc_seg_iters, dc_chunk_iters;               // loop bounds of the DC pass
};

// the workspace, carved by the host
struct Work {
    int32_t* flags;                                 // [N][rounds + 3]: changed per launch, error, slow subsequences
    uint32_t* entry;                                // [N][max_subs]: entry state per subsequence
    uint32_t* count;                                // [N][max_subs]: blocks completed per subsequence
    uint32_t* first;                                // [N][max_subs]: their exclusive prefix sum
    uint32_t* edge;                                 // [2][N][nwg + 1]: entry state of each workgroup's first subsequence
};

// what a decoding thread reads besides its own state
struct Ctx {
    const stp3_jpeg_huff_table* tabs;               // LDS: dc[0], dc[1], ac[0], ac[1]
    const uint16_t* q;                              // LDS: [3][64] zigzag
    const int* sel;                                 // LDS: [0..2] DC table per component, [3..5] AC table
    const uint8_t* natural;                         // LDS
    const uint32_t* words;                          // the image's subsequences as dwords
    uint32_t nwords;
    int hs, hsvs, bpm, mcus_x, coef_count, plane_y, plane_c;
};

struct Reader {
    uint64_t acc;                                   // bits at the top
    int have;
    uint32_t next, p;                               // the next dword to take; the bit position of the top bit
};

__device__ __forceinline__ uint32_t load_word(const Ctx& c, uint32_t i) { return i < c.nwords ? __builtin_bswap32(c.words[i]) : 0u; }

__device__ __forceinline__ void seek(const Ctx& c, Reader& r, uint32_t p) {
    r.p = p;
    r.next = (p >> 5) + 1;
    r.acc = (uint64_t)load_word(c, p >> 5) << (32 + (p & 31));
    r.have = 32 - (int)(p & 31);
}

// at least 32 bits behind it: a symbol with its magnitude bits has at most 31
__device__ __forceinline__ void refill(const Ctx& c, Reader& r) {
    if (r.have <= 32) {
        r.acc |= (uint64_t)load_word(c, r.next++) << (32 - r.have);
        r.have += 32;
    }
}

__device__ __forceinline__ void skip(Reader& r, int n) {
    r.acc <<= n;
    r.have -= n;
    r.p += (uint32_t)n;
}

// jdhuff.c as csrc/stp3_jpeg_entropy.h decode_symbol has it: (length << 8) | symbol, 0: a code the table does not assign
__device__ __forceinline__ uint32_t huff(const stp3_jpeg_huff_table& t, uint32_t top16) {
    const uint32_t e = t.look[top16 >> (16 - stp3_jpeg::kLookBits)];
    if (e) return e;
    for (int l = stp3_jpeg::kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(top16 >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int idx = t.valptr[l] + code;
            if (idx < 0 || idx > 255) return 0u;
            return (uint32_t)(l << 8) | t.vals[idx];
        }
    }
    return 0u;
}

// the s magnitude bits at the top of the reservoir, consumed (T.81 F.2.2.1 EXTEND); 1 <= s <= 15
__device__ __forceinline__ int receive_extend(Reader& r, int s) {
    const int v = (int)(r.acc >> (64 - s));
    skip(r, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

__device__ __forceinline__ bool dequantises(int v, int q) {
    return v >= -32767 && v <= 32767 && v * q >= -stp3_jpeg::kMaxDequantised && v * q <= stp3_jpeg::kMaxDequantised;
}

// where block number `blk` (decode order over the image; b = its index within the MCU) starts in the planar layout;
// coef_count (no valid index) for a block at or behind `blk_end`
__device__ __forceinline__ uint32_t block_base(const Ctx& c, uint32_t blk, uint32_t blk_end, int b) {
    if (blk >= blk_end) return (uint32_t)c.coef_count;
    const int mcu = (int)(blk / (uint32_t)c.bpm);
    const int my = mcu / c.mcus_x, mx = mcu - my * c.mcus_x;
    if (b < c.hsvs) {
        const int v = b / c.hs, u = b - v * c.hs, vs = c.hsvs / c.hs;
        return (uint32_t)(((my * vs + v) * (c.mcus_x * c.hs) + mx * c.hs + u) * 64);
    }
    return (uint32_t)(c.plane_y + (b - c.hsvs) * c.plane_c + (my * c.mcus_x + mx) * 64);
}

// Decodes the symbols that START in [r.p, end) from the state (b: block within the MCU, k: zigzag index) and returns the
// blocks completed.  At most kSB symbols: a symbol has at least one bit.  WRITE: coefficients are stored (the DC as its
// difference), block `blk` being the one the first symbol belongs to, and every irregularity sets `err`; without WRITE
// the caller ignores `err`: a thread at a wrong bit skips one bit and goes on.
template <bool WRITE>
__device__ __forceinline__ int decode_sub(const Ctx& c, Reader& r, int& b, int& k, uint32_t end, uint32_t seg_end, int16_t* coef,
                                          uint32_t blk, uint32_t blk_end, int& err) {
    int n = 0;
    uint32_t base = WRITE ? block_base(c, blk, blk_end, b) : 0u;
    for (int it = 0; it < kSB && r.p < end; ++it) {
        if (WRITE && blk + (uint32_t)n >= blk_end) break;      // the segment's MCUs are complete: what follows is padding
        refill(c, r);
        const int comp = b < c.hsvs ? 0 : b - c.hsvs + 1;
        const uint32_t e = huff(c.tabs[k == 0 ? c.sel[comp] : 2 + c.sel[3 + comp]], (uint32_t)(r.acc >> 48));
        const int len = (int)(e >> 8), sym = (int)(e & 255u);
        const int run = sym >> 4, s = sym & 15;
        bool done = false;
        int at = -1, v = 0;                                     // the zigzag index a value goes to
        if (e == 0u) {
            err = 1;
            skip(r, 1);
        } else if (k == 0) {                                    // (a DC symbol is a bit count <= 15: checked by the host)
            skip(r, len);
            if (s) v = receive_extend(r, s);
            at = 0;
            k = 1;
        } else if (s == 0) {
            if (run != 15) {                                    // end of block
                skip(r, len);
                done = true;
            } else if (k + 16 > 64) {
                err = 1;
                skip(r, 1);
            } else {
                skip(r, len);
                k += 16;
                done = k == 64;
            }
        } else if (k + run > 63) {                              // the run passes the last coefficient
            err = 1;
            skip(r, 1);
        } else {
            skip(r, len);
            k += run;
            v = receive_extend(r, s);
            at = k++;
            done = k == 64;
        }
        if (WRITE) {
            if (at > 0 && !dequantises(v, (int)c.q[comp * 64 + at])) err = 1;
            if (at >= 0) {
                const uint32_t idx = base + c.natural[at];
                if (idx < (uint32_t)c.coef_count) coef[idx] = (int16_t)v;
                else err = 1;
            }
            if (r.p > seg_end) err = 1;                         // a bit behind the segment's data was consumed
        }
        if (done) {
            k = 0;
            b = b + 1 == c.bpm ? 0 : b + 1;
            ++n;
            if (WRITE) base = block_base(c, blk + (uint32_t)n, blk_end, b);
        }
    }
    return n;
}

__device__ __forceinline__ uint32_t pack_state(uint32_t rel, int b, int k) { return rel | (uint32_t)b << 11 | (uint32_t)k << 14; }

// whether the descriptor fits the call: the same answer in every thread of the image
__device__ __forceinline__ bool desc_ok(const HuffDims& d, const stp3_jpeg_scan_desc& s) {
    if (s.nsub < 1 || s.nsub > d.max_subs || s.nseg < 1 || s.nseg > d.max_segs || s.restart_interval < 0) return false;
    if ((s.seg_offset | s.scan_offset | s.subseg_offset) & 3) return false;
    if (s.seg_offset < 0 || (int64_t)s.seg_offset + 12ll * s.nseg > d.stride) return false;
    if (s.scan_offset < 0 || (int64_t)s.scan_offset + (int64_t)kS * s.nsub > d.stride) return false;
    if (s.subseg_offset < 0 || (int64_t)s.subseg_offset + 4ll * s.nsub > d.stride) return false;
    for (int c = 0; c < d.nc; ++c)
        if (s.dc_table[c] < 0 || s.dc_table[c] > 1 || s.ac_table[c] < 0 || s.ac_table[c] > 1) return false;
    return true;
}

struct Lds {
    stp3_jpeg_huff_table tabs[4];
    uint16_t q[192];
    int sel[8];
    uint8_t natural[64];
};

// the tables of image n into LDS (every thread of the workgroup calls it; ends with a barrier) and the context around them
__device__ __forceinline__ Ctx load_ctx(const HuffDims& d, const uint8_t* scans, const stp3_jpeg_scan_desc& s, int n, Lds& l) {
    const int tid = threadIdx.x;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&s.dc[0]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&l.tabs[0]);
    for (int i = tid; i < (int)(4 * sizeof(stp3_jpeg_huff_table) / 4); i += kG) dst[i] = src[i];
    for (int i = tid; i < 192; i += kG) l.q[i] = s.quant[i >> 6][i & 63];
    if (tid < 3) {
        l.sel[tid] = tid < d.nc ? s.dc_table[tid] : 0;
        l.sel[3 + tid] = tid < d.nc ? s.ac_table[tid] : 0;
    }
    if (tid < 64) l.natural[tid] = kZigzagToNatural[tid];
    __syncthreads();
    Ctx c;
    c.tabs = l.tabs; c.q = l.q; c.sel = l.sel; c.natural = l.natural;
    c.words = reinterpret_cast<const uint32_t*>(scans + (size_t)n * d.stride + s.scan_offset);
    c.nwords = (uint32_t)s.nsub * (kS / 4);
    c.hs = d.hs; c.hsvs = d.hs * d.vs; c.bpm = d.bpm; c.mcus_x = d.mcus_x; c.coef_count = d.coef_count;
    c.plane_y = d.total_mcus * d.hs * d.vs * 64;
    c.plane_c = d.total_mcus * 64;
    return c;
}

// segment `seg` of the image: its first subsequence, the bit behind its data, its first MCU and the MCUs it holds
struct Segment { uint32_t first_sub, end_bit; int first_mcu, mcus; };

__device__ __forceinline__ Segment segment_of(const HuffDims& d, const uint8_t* scans, const stp3_jpeg_scan_desc& s, int n, int seg) {
    const int32_t* rec = reinterpret_cast<const int32_t*>(scans + (size_t)n * d.stride + s.seg_offset) + 3 * min(max(seg, 0), s.nseg - 1);
    Segment g;
    g.first_sub = (uint32_t)min(max(rec[0], 0), s.nsub - 1);
    const int64_t end = (int64_t)g.first_sub * kSB + max(rec[1], 0), all = (int64_t)s.nsub * kSB;
    g.end_bit = (uint32_t)(end < all ? end : all);
    g.first_mcu = min(max(rec[2], 0), d.total_mcus);
    g.mcus = s.restart_interval > 0 ? min(s.restart_interval, d.total_mcus - g.first_mcu) : d.total_mcus - g.first_mcu;
    return g;
}

// ---- sync: one bounded step -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kG) void jpeg_huff_sync_kernel(HuffDims d, const uint8_t* __restrict__ scans,
                                                            const stp3_jpeg_scan_desc* __restrict__ descs, Work w, int launch) {
    __shared__ Lds lds;
    __shared__ uint32_t entry_l[kG + 1];
    __shared__ uint32_t count_l[kG];
    __shared__ int seg_l[kG + 1];
    __shared__ int going[3];
    __shared__ int slow_l;
    const int tid = threadIdx.x, n = blockIdx.y, wg = blockIdx.x;
    int32_t* flags = w.flags + (size_t)n * (d.rounds + 3);
    if (launch > 0 && flags[launch - 1] == 0) return;           // (written by the launch before: the same in every thread)
    const stp3_jpeg_scan_desc& s = descs[n];
    if (!desc_ok(d, s)) {
        if (tid == 0 && wg == 0 && launch == 0) flags[d.rounds + 1] = 1;
        return;
    }
    const int base = wg * kG, cnt = min(kG, s.nsub - base);
    if (cnt <= 0) return;
    const Ctx c = load_ctx(d, scans, s, n, lds);
    const int32_t* subseg = reinterpret_cast<const int32_t*>(scans + (size_t)n * d.stride + s.subseg_offset);
    uint32_t* entry_g = w.entry + (size_t)n * d.max_subs + base;
    uint32_t* count_g = w.count + (size_t)n * d.max_subs + base;
    const uint32_t* edge_in = w.edge + ((size_t)((launch + 1) & 1) * d.N + n) * (d.nwg + 1);
    uint32_t* edge_out = w.edge + ((size_t)(launch & 1) * d.N + n) * (d.nwg + 1);
    const uint32_t assumed = pack_state(0u, 0, 0);

    for (int i = tid; i <= cnt; i += kG) seg_l[i] = base + i < s.nsub ? subseg[base + i] : -1;
    if (tid < 3) going[tid] = 0;
    if (tid == 0) slow_l = 0;
    if (tid < cnt) {
        entry_l[tid] = launch == 0 ? assumed : entry_g[tid];
        count_l[tid] = launch == 0 ? 0u : count_g[tid];
    }
    // what the right neighbour consumes in this launch: the assumed state, later what this workgroup left the launch before
    if (tid == 0) entry_l[cnt] = launch == 0 ? assumed : edge_in[wg + 1];
    __syncthreads();
    const uint32_t consumed = entry_l[cnt];
    bool active = tid < cnt;
    if (launch > 0) {                                           // only a new state at the left edge is work
        active = false;
        if (tid == 0) {
            const bool starts_segment = base == 0 || seg_l[0] != subseg[base - 1];
            const uint32_t in = starts_segment ? assumed : edge_in[wg];
            active = in != entry_l[0];
            entry_l[0] = in;
        }
    }
    int j = tid;                                                // the subsequence of the workgroup this thread decodes next
    const int seg = active ? seg_l[j] : 0;
    const Segment g = segment_of(d, scans, s, n, seg);
    int b = 0, k = 0, further = 0, unused = 0;
    Reader r = {0, 0, 0u, 0u};
    if (active) {
        const uint32_t e = entry_l[j];
        b = (int)(e >> 11 & 7u);
        if (b >= d.bpm) b = 0;
        k = (int)(e >> 14 & 63u);
        seek(c, r, (uint32_t)(base + j) * kSB + (e & 2047u));
    }
    __syncthreads();                                            // (entry_l[0] is read above, written below)
    for (int round = 0; round < kG; ++round) {
        if (active) {
            const uint32_t edge = (uint32_t)(base + j + 1) * kSB;
            count_l[j] = (uint32_t)decode_sub<false>(c, r, b, k, min(edge, g.end_bit), g.end_bit, nullptr, 0u, 0u, unused);
            active = false;
            if (seg_l[j + 1] == seg) {                          // (j + 1 <= cnt) the next subsequence continues the segment
                const uint32_t mine = pack_state(min(r.p - edge, 2047u), b, k);
                if (entry_l[j + 1] != mine) {
                    entry_l[j + 1] = mine;
                    active = ++j < cnt;                         // run on, up to the workgroup's edge
                    further += active;
                }
            }
            if (active) going[round % 3] = 1;
        }
        __syncthreads();
        const int more = going[round % 3];
        if (tid == 0) going[(round + 2) % 3] = 0;               // (last read before this barrier, next set behind the next one)
        if (!more) break;
    }
    if (launch == 0 && further > 1) atomicAdd(&slow_l, 1);
    __syncthreads();
    if (tid < cnt) {
        entry_g[tid] = entry_l[tid];
        count_g[tid] = count_l[tid];
    }
    if (tid == 0) {
        edge_out[wg + 1] = entry_l[cnt];
        if (entry_l[cnt] != consumed) atomicAdd(&flags[launch], 1);
        if (slow_l) atomicAdd(&flags[d.rounds + 2], slow_l);
    }
}

// inclusive sum over the kG threads of a workgroup; every thread calls it
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t (*buf)[kG], uint32_t* total) {
    const int tid = threadIdx.x;
    int src = 0;
    buf[0][tid] = v;
    __syncthreads();
    for (int dist = 1; dist < kG; dist <<= 1) {
        buf[src ^ 1][tid] = buf[src][tid] + (tid >= dist ? buf[src][tid - dist] : 0u);
        src ^= 1;
        __syncthreads();
    }
    const uint32_t mine = buf[src][tid];
    *total = buf[src][kG - 1];
    __syncthreads();
    return mine;
}

// ---- scan: the first block number of every subsequence (relative to the image's first) ------------------------------------
__global__ __launch_bounds__(kG) void jpeg_huff_scan_kernel(HuffDims d, const stp3_jpeg_scan_desc* __restrict__ descs, Work w) {
    __shared__ uint32_t buf[2][kG];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int32_t* flags = w.flags + (size_t)n * (d.rounds + 3);
    const stp3_jpeg_scan_desc& s = descs[n];
    if (flags[d.rounds] != 0 || flags[d.rounds + 1] != 0 || !desc_ok(d, s)) return;
    const uint32_t* count = w.count + (size_t)n * d.max_subs;
    uint32_t* first = w.first + (size_t)n * d.max_subs;
    uint32_t carry = 0u;
    for (int c0 = 0; c0 < d.max_subs; c0 += kG) {
        if (c0 >= s.nsub) break;
        const int i = c0 + tid;
        const uint32_t v = i < s.nsub ? count[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_scan(v, buf, &total);
        if (i < s.nsub) first[i] = carry + incl - v;
        carry += total;
    }
}

// ---- write -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kG) void jpeg_huff_write_kernel(HuffDims d, const uint8_t* __restrict__ scans,
                                                             const stp3_jpeg_scan_desc* __restrict__ descs, Work w,
                                                             int16_t* __restrict__ coef) {
    __shared__ Lds lds;
    const int tid = threadIdx.x, n = blockIdx.y, i = blockIdx.x * kG + tid;
    int32_t* flags = w.flags + (size_t)n * (d.rounds + 3);
    const stp3_jpeg_scan_desc& s = descs[n];
    if (flags[d.rounds] != 0 || flags[d.rounds + 1] != 0 || !desc_ok(d, s)) return;
    if ((int)blockIdx.x * kG >= s.nsub) return;
    const Ctx c = load_ctx(d, scans, s, n, lds);
    if (i >= s.nsub) return;
    const int32_t* subseg = reinterpret_cast<const int32_t*>(scans + (size_t)n * d.stride + s.subseg_offset);
    const int seg = subseg[i];
    const Segment g = segment_of(d, scans, s, n, seg);
    const uint32_t* first = w.first + (size_t)n * d.max_subs;
    const uint32_t e = w.entry[(size_t)n * d.max_subs + i];
    int b = (int)(e >> 11 & 7u), k = (int)(e >> 14 & 63u), err = 0;
    if (b >= d.bpm) { b = 0; err = 1; }
    Reader r;
    seek(c, r, (uint32_t)i * kSB + (e & 2047u));
    const uint32_t blk = (uint32_t)(g.first_mcu * d.bpm) + first[i] - first[g.first_sub];
    const uint32_t blk_end = (uint32_t)((g.first_mcu + g.mcus) * d.bpm);
    const int done = decode_sub<true>(c, r, b, k, min((uint32_t)(i + 1) * kSB, g.end_bit), g.end_bit, coef + (size_t)n * d.coef_count,
                                      blk, blk_end, err);
    if (i + 1 == s.nsub || subseg[i + 1] != seg) {              // the segment ends here: inside its last byte, with all its MCUs
        if (b != 0 || k != 0 || blk + (uint32_t)done != blk_end || r.p > g.end_bit || r.p + 8u <= g.end_bit) err = 1;
    } else if (r.p < (uint32_t)(i + 1) * kSB) {
        err = 1;                                                // ... and not before
    }
    if (err) flags[d.rounds + 1] = 1;
}

// ---- dc: the running sum of the differences, per component and segment -----------------------------------------------------
__global__ __launch_bounds__(kG) void jpeg_huff_dc_kernel(HuffDims d, const uint8_t* __restrict__ scans,
                                                          const stp3_jpeg_scan_desc* __restrict__ descs, Work w,
                                                          int16_t* __restrict__ coef) {
    __shared__ uint32_t buf[2][kG];
    const int tid = threadIdx.x, comp = blockIdx.y, n = blockIdx.z;
    int32_t* flags = w.flags + (size_t)n * (d.rounds + 3);
    const stp3_jpeg_scan_desc& s = descs[n];
    if (flags[d.rounds] != 0 || !desc_ok(d, s)) return;
    int16_t* image = coef + (size_t)n * d.coef_count;
    const int q0 = s.quant[comp][0];
    const int ch = comp == 0 ? d.hs : 1, bc = comp == 0 ? d.hs * d.vs : 1;
    const int plane = comp == 0 ? 0 : d.total_mcus * d.hs * d.vs * 64 + (comp - 1) * d.total_mcus * 64;
    int err = 0;
    for (int si = 0; si < d.dc_seg_iters; ++si) {
        const int seg = (int)blockIdx.x + si * kDcGrid;
        if (seg >= s.nseg) break;
        const Segment g = segment_of(d, scans, s, n, seg);
        const int items = g.mcus * bc;
        uint32_t carry = 0u;
        for (int ci = 0; ci < d.dc_chunk_iters; ++ci) {
            if (ci * kG >= items) break;
            const int idx = ci * kG + tid;
            const int mcu = g.first_mcu + idx / bc, bi = idx % bc;
            const int my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x, v = bi / ch, u = bi - v * ch;
            const int64_t at = (int64_t)plane + ((int64_t)(my * (bc / ch) + v) * (d.mcus_x * ch) + mx * ch + u) * 64;
            const bool valid = idx < items && at >= 0 && at < d.coef_count;
            uint32_t total;
            const uint32_t incl = block_scan(valid ? (uint32_t)(int32_t)image[at] : 0u, buf, &total);
            if (valid) {
                const int dc = (int)(carry + incl);             // exact up to the first value outside the bound
                if (!dequantises(dc, q0)) err = 1;
                image[at] = (int16_t)dc;
            }
            carry += total;
        }
    }
    if (err) flags[d.rounds + 1] = 1;
}

__global__ void jpeg_huff_status_kernel(HuffDims d, Work w, int32_t* __restrict__ status) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= d.N) return;
    const int32_t* flags = w.flags + (size_t)n * (d.rounds + 3);
    status[n] = flags[d.rounds] != 0 ? STP3_JPEG_NOT_CONVERGED : flags[d.rounds + 1] != 0 ? STP3_EINVAL : STP3_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int check_dims(const stp3_jpeg_huff_dims* p, int rounds, HuffDims* d) {
    if (!p || p->N <= 0 || p->width <= 0 || p->height <= 0) return STP3_EINVAL;
    if (p->components != 1 && p->components != 3) return STP3_EINVAL;
    const bool hv = (p->hs == 1 && p->vs == 1) || (p->components == 3 && p->hs == 2 && (p->vs == 1 || p->vs == 2));
    if (!hv || p->scan_stride < 1 || (p->scan_stride & 3) || p->max_subs < 1 || p->max_segs < 1) return STP3_EINVAL;
    if (rounds < 0 || rounds > kMaxRounds) return STP3_EINVAL;
    if (p->width > stp3_jpeg::kMaxSide || p->height > stp3_jpeg::kMaxSide || p->N > 65535) return STP3_EUNSUP;
    if (p->max_subs > (1 << 21) || p->max_segs > (int)stp3_jpeg::kMaxSegments) return STP3_EUNSUP;   // (bit positions: 31 bits)
    d->N = p->N; d->nc = p->components; d->hs = p->hs; d->vs = p->vs;
    d->mcus_x = (p->width + 8 * p->hs - 1) / (8 * p->hs);
    d->mcus_y = (p->height + 8 * p->vs - 1) / (8 * p->vs);
    d->bpm = p->hs * p->vs + (p->components == 3 ? 2 : 0);
    d->total_mcus = d->mcus_x * d->mcus_y;
    d->coef_count = d->total_mcus * d->bpm * 64;
    d->stride = p->scan_stride; d->max_subs = p->max_subs; d->max_segs = p->max_segs;
    d->nwg = (p->max_subs + kG - 1) / kG;
    d->rounds = rounds;
    d->dc_seg_iters = (p->max_segs + kDcGrid - 1) / kDcGrid;
    d->dc_chunk_iters = (d->total_mcus * p->hs * p->vs + kG - 1) / kG;
    return STP3_OK;
}

size_t carve(const HuffDims& d, void* base, Work* w) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? static_cast<char*>(base) + at : nullptr;
        at += align256(bytes);
        return p;
    };
    const size_t subs = (size_t)d.N * d.max_subs * 4;
    w->flags = static_cast<int32_t*>(take((size_t)d.N * (d.rounds + 3) * 4));
    w->entry = static_cast<uint32_t*>(take(subs));
    w->count = static_cast<uint32_t*>(take(subs));
    w->first = static_cast<uint32_t*>(take(subs));
    w->edge = static_cast<uint32_t*>(take((size_t)2 * d.N * (d.nwg + 1) * 4));
    return at;
}

}  // namespace

extern "C" {

size_t stp3_jpeg_scan_bytes(const stp3_jpeg_header* header, size_t len) { return header ? stp3_jpeg::scan_bytes(*header, len) : 0; }

int stp3_jpeg_scan_prepare(const uint8_t* data, size_t len, uint8_t* scan_out, size_t scan_capacity, stp3_jpeg_scan_desc* desc,
                           uint16_t* quant) {
    return stp3_jpeg::scan_prepare(data, len, scan_out, scan_capacity, desc, quant);
}

int stp3_jpeg_entropy_workspace_bytes(const stp3_jpeg_huff_dims* dims, int32_t sync_rounds, size_t* bytes) {
    HuffDims d;
    const int rc = check_dims(dims, sync_rounds, &d);
    if (rc != STP3_OK) return rc;
    if (!bytes) return STP3_EINVAL;
    Work w;
    *bytes = carve(d, nullptr, &w);
    return STP3_OK;
}

int stp3_jpeg_entropy_device(const stp3_jpeg_huff_dims* dims, const uint8_t* scans, const stp3_jpeg_scan_desc* descs, int16_t* coef,
                             int32_t* status, void* workspace, size_t workspace_bytes, int32_t sync_rounds, void* stream) {
    HuffDims d;
    const int rc = check_dims(dims, sync_rounds, &d);
    if (rc != STP3_OK) return rc;
    if (!scans || !descs || !coef || !status || !workspace) return STP3_EINVAL;
    if (((uintptr_t)scans & 3) || ((uintptr_t)descs & 3) || ((uintptr_t)workspace & 3)) return STP3_EINVAL;
    Work w;
    if (carve(d, workspace, &w) > workspace_bytes) return STP3_ENOSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w.flags, 0, (size_t)d.N * (d.rounds + 3) * 4, st);
    if (e != hipSuccess) return -(int)e;
    e = hipMemsetAsync(coef, 0, (size_t)d.N * d.coef_count * sizeof(int16_t), st);
    if (e != hipSuccess) return -(int)e;
    for (int launch = 0; launch <= d.rounds; ++launch)
        hipLaunchKernelGGL(jpeg_huff_sync_kernel, dim3(d.nwg, d.N), dim3(kG), 0, st, d, scans, descs, w, launch);
    hipLaunchKernelGGL(jpeg_huff_scan_kernel, dim3(d.N), dim3(kG), 0, st, d, descs, w);
    hipLaunchKernelGGL(jpeg_huff_write_kernel, dim3(d.nwg, d.N), dim3(kG), 0, st, d, scans, descs, w, coef);
    hipLaunchKernelGGL(jpeg_huff_dc_kernel, dim3(d.max_segs < kDcGrid ? d.max_segs : kDcGrid, d.nc, d.N), dim3(kG), 0, st, d, scans, descs,
                       w, coef);
    hipLaunchKernelGGL(jpeg_huff_status_kernel, dim3((d.N + 63) / 64), dim3(64), 0, st, d, w, status);
    e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
