// stp3_jpeg_entropy.h -- the serial half of a baseline JPEG decode, on the host: marker parsing and Huffman decoding of one
// stream into quantised coefficients (ITU-T T.81; the layouts are those of include/stp3_hip.h, "JPEG camera frames").
// Plain C++, no HIP: csrc/stp3_jpeg.hip wraps it in the C ABI (stp3_jpeg_info / stp3_jpeg_entropy) and
// tests/jpeg_host/main.cpp compiles it alone under the host sanitizers.
//
// Rules of the library, followed here: nothing persistent is allocated (the Huffman tables of a call live on its stack,
// about 14 KB), no global state, integer return codes, nothing throws.  The bytes are UNTRUSTED: every read is checked against
// the input length, every coefficient index against 64, every block index against the caller's buffer.
//
// Supported (anything else is STP3_EUNSUP, decided from the headers BEFORE the first coefficient is written): SOF0 / SOF1 with
// 8-bit samples, Huffman coding, one scan holding all components; one component (grey, decoded as 1x1 whatever factors it
// declares, as T.81 A.2.2 has it for a non-interleaved scan) or three components Y Cb Cr with luma sampling 1x1, 2x1 or 2x2
// and chroma 1x1.  The colour space of three components is decided as libjpeg's default_decompress_parms (jdapimin.c) does:
// JFIF seen: YCbCr; else an Adobe marker with transform 0: RGB; else component ids 'R','G','B': RGB; RGB is STP3_EUNSUP.
// A malformed or truncated stream is STP3_EINVAL: a code no table assigns, a run past coefficient 63, a missing table, a
// missing RSTn or EOI, entropy data that ends early (the zero bits appended behind the last byte were consumed), a
// coefficient whose dequantised value does not fit 16 bits (no 8-bit encoder writes one).  Bytes that are no marker in front
// of an RSTn or of EOI are skipped, as libjpeg skips them.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "stp3_hip.h"

namespace stp3_jpeg {

constexpr int kLookBits = 9;
constexpr int kMaxSide = 16384;                     // 1.5 * 2^28 coefficients at most: counts stay inside int32

// zigzag position -> natural (row-major) position
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    uint16_t look[1 << kLookBits];                  // (length << 8) | symbol for codes of at most kLookBits bits, 0: longer
    int32_t maxcode[18];                            // largest code of each length, -1: none (T.81 F.2.2.3)
    int32_t valptr[17];                             // index of the first symbol of each length, minus its first code
    uint8_t vals[256];
    int defined;
};

struct Frame {
    int width, height, ncomp, progressive, arithmetic, lossless_or_hier, precision, sof_seen;
    int id[4], h[4], v[4], tq[4];
    int restart_interval, jfif, adobe, adobe_transform;
    uint16_t quant[4][64];                          // zigzag order, as stored
    int quant_defined[4];
};

struct Reader {
    const uint8_t* p;
    size_t len, pos;
    uint64_t acc;                                   // bits at the top
    int nbits, fake;                                // valid bits; how many of them are zeros appended behind the data
};

inline int be16(const uint8_t* p, size_t len, size_t pos, int* v) {
    if (pos + 2 > len) return STP3_EINVAL;
    *v = (p[pos] << 8) | p[pos + 1];
    return STP3_OK;
}

// canonical code tables of one DHT entry: counts[1..16], the symbols behind them
inline int build_huff(Huff* t, const uint8_t* counts, const uint8_t* syms, int nsyms) {
    memset(t->look, 0, sizeof(t->look));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return STP3_EINVAL;            // more codes than the length has
        t->valptr[l] = k - code;
        if (l <= kLookBits)
            for (int i = 0; i < n; ++i) {
                const int first = (code + i) << (kLookBits - l);
                for (int j = 0; j < (1 << (kLookBits - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | syms[k + i]);
            }
        k += n;
        code += n;
        t->maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[17] = 0x7fffffff;
    if (k != nsyms) return STP3_EINVAL;
    memcpy(t->vals, syms, (size_t)nsyms);
    t->defined = 1;
    return STP3_OK;
}

// Walks the markers up to and including the SOS header.  *scan is the offset of the first entropy-coded byte.
inline int parse_headers(const uint8_t* p, size_t len, Frame* f, Huff* dc, Huff* ac, int* scan_tab, size_t* scan) {
    memset(f, 0, sizeof(*f));
    f->adobe_transform = -1;
    if (len < 4 || p[0] != 0xFF || p[1] != 0xD8) return STP3_EINVAL;
    size_t pos = 2;
    for (;;) {
        if (pos >= len || p[pos] != 0xFF) return STP3_EINVAL;
        while (pos < len && p[pos] == 0xFF) ++pos;              // fill bytes
        if (pos >= len) return STP3_EINVAL;
        const int m = p[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, a stray RSTn: no segment
        if (m == 0xD8 || m == 0xD9 || m == 0x00) return STP3_EINVAL;
        int seglen = 0;
        if (be16(p, len, pos, &seglen) != STP3_OK || seglen < 2 || pos + (size_t)seglen > len) return STP3_EINVAL;
        const uint8_t* s = p + pos + 2;
        const int n = seglen - 2;
        pos += (size_t)seglen;
        if (m == 0xDB) {                                        // DQT
            int i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3 || i + 1 + 64 * (pq + 1) > n) return STP3_EINVAL;
                for (int k = 0; k < 64; ++k) {
                    const int q = pq ? (s[i + 1 + 2 * k] << 8) | s[i + 2 + 2 * k] : s[i + 1 + k];
                    if (q == 0) return STP3_EINVAL;
                    f->quant[tq][k] = (uint16_t)q;
                }
                f->quant_defined[tq] = 1;
                i += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xC4) {                                 // DHT
            int i = 0;
            while (i < n) {
                if (i + 17 > n) return STP3_EINVAL;
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return STP3_EINVAL;
                int total = 0;
                for (int l = 0; l < 16; ++l) total += s[i + 1 + l];
                if (total > 256 || i + 17 + total > n) return STP3_EINVAL;
                if (tc == 0)
                    for (int k = 0; k < total; ++k)
                        if (s[i + 17 + k] > 15) return STP3_EINVAL;      // a DC category is a bit count
                if (build_huff(tc ? &ac[th] : &dc[th], s + i + 1, s + i + 17, total) != STP3_OK) return STP3_EINVAL;
                i += 17 + total;
            }
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {       // SOFn (0xC4 DHT taken above; 0xCC DAC below)
            if (m == 0xCC) continue;                            // arithmetic conditioning: only arithmetic frames read it
            if (f->sof_seen || n < 6) return STP3_EINVAL;
            f->sof_seen = 1;
            f->progressive = m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE;
            f->arithmetic = m >= 0xC9;
            f->lossless_or_hier = m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || m == 0xCB || m >= 0xCD;
            f->precision = s[0];
            f->height = (s[1] << 8) | s[2];
            f->width = (s[3] << 8) | s[4];
            f->ncomp = s[5];
            if (f->ncomp < 1 || f->ncomp > 4 || n != 6 + 3 * f->ncomp || f->width < 1 || f->height < 1) return STP3_EINVAL;
            for (int c = 0; c < f->ncomp; ++c) {
                f->id[c] = s[6 + 3 * c];
                f->h[c] = s[7 + 3 * c] >> 4;
                f->v[c] = s[7 + 3 * c] & 15;
                f->tq[c] = s[8 + 3 * c];
                if (f->h[c] < 1 || f->h[c] > 4 || f->v[c] < 1 || f->v[c] > 4 || f->tq[c] > 3) return STP3_EINVAL;
            }
        } else if (m == 0xDD) {                                 // DRI
            if (n != 2) return STP3_EINVAL;
            f->restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (n >= 5 && !memcmp(s, "JFIF", 5)) f->jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) {
                f->adobe = 1;
                f->adobe_transform = s[11];
            }
        } else if (m == 0xDA) {                                 // SOS
            if (!f->sof_seen || n < 1) return STP3_EINVAL;
            // what this decoder does not do is answered before the scan is looked at
            if (f->progressive || f->arithmetic || f->lossless_or_hier || f->precision != 8) return STP3_EUNSUP;
            if (f->ncomp != 1 && f->ncomp != 3) return STP3_EUNSUP;
            if (f->width > kMaxSide || f->height > kMaxSide) return STP3_EUNSUP;
            if (f->ncomp == 3) {
                const bool hv = (f->h[0] == 1 && f->v[0] == 1) || (f->h[0] == 2 && f->v[0] == 1) || (f->h[0] == 2 && f->v[0] == 2);
                if (!hv || f->h[1] != 1 || f->v[1] != 1 || f->h[2] != 1 || f->v[2] != 1) return STP3_EUNSUP;
                bool rgb = false;
                if (f->jfif) rgb = false;
                else if (f->adobe) rgb = f->adobe_transform == 0;
                else rgb = f->id[0] == 'R' && f->id[1] == 'G' && f->id[2] == 'B';
                if (rgb) return STP3_EUNSUP;
            }
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return STP3_EINVAL;
            if (ns != f->ncomp) return STP3_EUNSUP;             // one scan per component: a multi-scan file
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != f->id[c]) return STP3_EINVAL;
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3 || !dc[td].defined || !ac[ta].defined) return STP3_EINVAL;   // names a missing table
                if (!f->quant_defined[f->tq[c]]) return STP3_EINVAL;
                scan_tab[2 * c] = td;
                scan_tab[2 * c + 1] = ta;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return STP3_EINVAL;
            *scan = pos;
            return STP3_OK;
        }
        // APPn, COM and the rest: skipped
    }
}

inline void fill_header(const Frame& f, stp3_jpeg_header* h) {
    memset(h, 0, sizeof(*h));
    h->width = f.width;
    h->height = f.height;
    h->components = f.ncomp;
    h->hs = f.ncomp == 1 ? 1 : f.h[0];
    h->vs = f.ncomp == 1 ? 1 : f.v[0];
    h->mcus_x = (f.width + 8 * h->hs - 1) / (8 * h->hs);
    h->mcus_y = (f.height + 8 * h->vs - 1) / (8 * h->vs);
    h->restart_interval = f.restart_interval;
    int total = 0;
    for (int c = 0; c < f.ncomp; ++c) {
        h->blocks_x[c] = h->mcus_x * (c == 0 ? h->hs : 1);
        h->blocks_y[c] = h->mcus_y * (c == 0 ? h->vs : 1);
        total += h->blocks_x[c] * h->blocks_y[c] * 64;
    }
    h->coef_count = total;
}

inline void refill(Reader* r) {
    while (r->nbits <= 56) {
        if (r->pos < r->len) {
            const int b = r->p[r->pos];
            if (b != 0xFF) {
                r->acc |= (uint64_t)b << (56 - r->nbits);
                r->nbits += 8;
                ++r->pos;
                continue;
            }
            if (r->pos + 1 < r->len && r->p[r->pos + 1] == 0x00) {        // a stuffed 0xFF
                r->acc |= (uint64_t)0xFF << (56 - r->nbits);
                r->nbits += 8;
                r->pos += 2;
                continue;
            }
        }
        // a marker or the end of the input: zeros from here on; consuming one of them is an error (checked per block)
        r->fake += 64 - r->nbits;
        r->nbits = 64;
        return;
    }
}

inline int decode_symbol(Reader* r, const Huff& t, int* sym) {
    const uint32_t e = t.look[r->acc >> (64 - kLookBits)];
    if (e) {
        r->acc <<= e >> 8;
        r->nbits -= (int)(e >> 8);
        *sym = (int)(e & 255u);
        return STP3_OK;
    }
    const int32_t top = (int32_t)(r->acc >> 48);
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = top >> (16 - l);
        if (code <= t.maxcode[l]) {
            const int idx = t.valptr[l] + code;
            if (idx < 0 || idx > 255) return STP3_EINVAL;
            r->acc <<= l;
            r->nbits -= l;
            *sym = t.vals[idx];
            return STP3_OK;
        }
    }
    return STP3_EINVAL;                                         // a code no table assigns
}

// s magnitude bits -> the signed value (T.81 F.2.2.1 EXTEND)
inline int receive_extend(Reader* r, int s) {
    const int v = (int)(r->acc >> (64 - s));
    r->acc <<= s;
    r->nbits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// A coefficient is kept only if its dequantised value fits 16 bits (kMaxDequantised): every stream an 8-bit encoder writes
// stays far inside (|DCT| <= 1024 * 8 plus half a quantiser step), libjpeg-turbo's SIMD IDCT dequantises in 16 bits, and the
// bound keeps the DC predictor, which an adversarial stream would otherwise walk out of any integer type, inside +-32767.
constexpr int kMaxDequantised = 32767;

inline bool dequantises(int v, uint16_t q) { return v >= -32767 && v <= 32767 && v * (int)q >= -kMaxDequantised && v * (int)q <= kMaxDequantised; }

// q: the component's quantisation table in zigzag order, as stored
inline int decode_block(Reader* r, const Huff& dc, const Huff& ac, const uint16_t* q, int* pred, int16_t* blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    int sym = 0;
    if (r->nbits < 32) refill(r);
    if (decode_symbol(r, dc, &sym) != STP3_OK) return STP3_EINVAL;
    if (sym) *pred += receive_extend(r, sym);                   // (sym <= 15, |*pred| <= 32767 before: no overflow)
    if (!dequantises(*pred, q[0])) return STP3_EINVAL;
    blk[0] = (int16_t)*pred;
    for (int k = 1; k < 64;) {
        if (r->nbits < 32) refill(r);
        if (decode_symbol(r, ac, &sym) != STP3_OK) return STP3_EINVAL;
        const int run = sym >> 4, s = sym & 15;
        if (s == 0) {
            if (run != 15) break;                               // end of block
            k += 16;
            if (k > 64) return STP3_EINVAL;
            continue;
        }
        k += run;
        if (k > 63) return STP3_EINVAL;                         // the run passes the last coefficient
        const int v = receive_extend(r, s);
        if (!dequantises(v, q[k])) return STP3_EINVAL;
        blk[kNatural[k]] = (int16_t)v;
        ++k;
    }
    return r->nbits < r->fake ? STP3_EINVAL : STP3_OK;          // bits behind the end of the data were consumed
}

// The marker `want` behind the reader's byte position, consumed.  Bytes in front of it that are no marker (padding, junk)
// are skipped, as libjpeg's next_marker does with a warning; another marker in its place, or none, is an error.
inline int expect_marker(Reader* r, int want) {
    for (;;) {
        while (r->pos < r->len && r->p[r->pos] != 0xFF) ++r->pos;
        while (r->pos < r->len && r->p[r->pos] == 0xFF) ++r->pos;
        if (r->pos >= r->len) return STP3_EINVAL;
        if (r->p[r->pos] == 0x00) { ++r->pos; continue; }       // a stuffed 0xFF: data, not a marker
        if (r->p[r->pos] != want) return STP3_EINVAL;
        ++r->pos;
        return STP3_OK;
    }
}

inline int info(const uint8_t* data, size_t len, stp3_jpeg_header* hdr) {
    if (!data || !hdr) return STP3_EINVAL;
    Frame f;
    Huff dc[4], ac[4];
    for (int i = 0; i < 4; ++i) dc[i].defined = ac[i].defined = 0;
    int tab[8];
    size_t scan = 0;
    const int rc = parse_headers(data, len, &f, dc, ac, tab, &scan);
    if (rc != STP3_OK) return rc;
    fill_header(f, hdr);
    return STP3_OK;
}

// coef: hdr->coef_count int16 (capacity `coef_capacity` elements), component after component, each [blocks_y][blocks_x][64]
// in natural order; quant: [3][64] uint16 in natural order, one table per component (a grey stream fills all three alike).
inline int entropy(const uint8_t* data, size_t len, int16_t* coef, size_t coef_capacity, uint16_t* quant,
                   stp3_jpeg_header* hdr) {
    if (!data || !coef || !quant || !hdr) return STP3_EINVAL;
    Frame f;
    Huff dc[4], ac[4];
    for (int i = 0; i < 4; ++i) dc[i].defined = ac[i].defined = 0;
    int tab[8];
    size_t scan = 0;
    const int rc = parse_headers(data, len, &f, dc, ac, tab, &scan);
    if (rc != STP3_OK) return rc;
    stp3_jpeg_header h;
    fill_header(f, &h);
    if ((size_t)h.coef_count > coef_capacity) return STP3_EINVAL;
    for (int c = 0; c < 3; ++c) {
        const uint16_t* q = f.quant[f.tq[c < f.ncomp ? c : 0]];
        for (int k = 0; k < 64; ++k) quant[c * 64 + kNatural[k]] = q[k];
    }
    int16_t* plane[3] = {coef, coef, coef};
    for (int c = 1; c < f.ncomp; ++c) plane[c] = plane[c - 1] + (size_t)h.blocks_x[c - 1] * h.blocks_y[c - 1] * 64;
    Reader r = {data, len, scan, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    const int total = h.mcus_x * h.mcus_y;
    int until_restart = f.restart_interval ? f.restart_interval : total;
    int next_rst = 0;
    for (int mcu = 0; mcu < total; ++mcu) {
        if (until_restart == 0) {                               // RSTn: byte-align, reset the predictors
            r.acc = 0; r.nbits = 0; r.fake = 0;
            if (expect_marker(&r, 0xD0 + (next_rst & 7)) != STP3_OK) return STP3_EINVAL;
            ++next_rst;
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = f.restart_interval;
        }
        --until_restart;
        const int my = mcu / h.mcus_x, mx = mcu - my * h.mcus_x;
        for (int c = 0; c < f.ncomp; ++c) {
            const int ch = c == 0 ? h.hs : 1, cv = c == 0 ? h.vs : 1;
            for (int v = 0; v < cv; ++v)
                for (int u = 0; u < ch; ++u) {
                    const int by = my * cv + v, bx = mx * ch + u;
                    if (by >= h.blocks_y[c] || bx >= h.blocks_x[c]) return STP3_EINVAL;
                    const size_t at = ((size_t)by * h.blocks_x[c] + bx) * 64;
                    if ((size_t)(plane[c] - coef) + at + 64 > coef_capacity) return STP3_EINVAL;
                    if (decode_block(&r, dc[tab[2 * c]], ac[tab[2 * c + 1]], f.quant[f.tq[c]], &pred[c], plane[c] + at) != STP3_OK)
                        return STP3_EINVAL;
                }
        }
    }
    // every byte of the scan was taken into the reservoir when the data is whole: EOI follows
    r.acc = 0; r.nbits = 0; r.fake = 0;
    if (expect_marker(&r, 0xD9) != STP3_OK) return STP3_EINVAL;
    *hdr = h;
    return STP3_OK;
}

// ---- the scan prepared for the device decode (csrc/stp3_jpeg_huff.hip; include/stp3_hip.h, "the Huffman scan ON THE
// DEVICE") -----------------------------------------------------------------------------------------------------------
constexpr size_t kSubBytes = STP3_JPEG_SUB_BYTES;
constexpr size_t kMaxSegments = 65536, kMaxScanLen = (size_t)1 << 27;      // bit positions stay inside 31 bits

inline size_t segments_of(const stp3_jpeg_header& h) {
    const size_t total = (size_t)h.mcus_x * (size_t)h.mcus_y;
    return h.restart_interval > 0 ? (total + (size_t)h.restart_interval - 1) / (size_t)h.restart_interval : 1;
}

// an upper bound of what scan_prepare writes for a stream of `len` bytes with this header
inline size_t scan_bytes(const stp3_jpeg_header& h, size_t len) {
    const size_t nseg = segments_of(h), nsub = len / kSubBytes + nseg + 1;
    return (nseg * 12 + kSubBytes) + nsub * kSubBytes + nsub * 4;
}

inline void copy_table(stp3_jpeg_huff_table* d, const Huff& s) {
    memcpy(d->look, s.look, sizeof(d->look));
    memcpy(d->maxcode, s.maxcode, sizeof(d->maxcode));
    memset(d->valptr, 0, sizeof(d->valptr));
    memcpy(d->valptr + 1, s.valptr + 1, 16 * sizeof(int32_t));  // ([0] is never set nor read)
    memcpy(d->vals, s.vals, sizeof(d->vals));
}

// The entropy-coded bytes of the stream without byte stuffing, cut at the restart markers into segments padded to whole
// subsequences, and the descriptor the device decode reads.  Nothing is decoded here, so nothing is guessed: whatever is
// not "data, RSTn in sequence, data, ..., EOI" is STP3_JPEG_IRREGULAR and belongs to `entropy` above.
inline int scan_prepare(const uint8_t* data, size_t len, uint8_t* out, size_t capacity, stp3_jpeg_scan_desc* desc,
                        uint16_t* quant) {
    if (!data || !out || !desc || !quant) return STP3_EINVAL;
    Frame f;
    Huff dc[4], ac[4];
    for (int i = 0; i < 4; ++i) {
        memset(&dc[i], 0, sizeof(Huff));
        memset(&ac[i], 0, sizeof(Huff));
    }
    int tab[8];
    size_t pos = 0;
    const int rc = parse_headers(data, len, &f, dc, ac, tab, &pos);
    if (rc != STP3_OK) return rc;
    stp3_jpeg_header h;
    fill_header(f, &h);
    const size_t nseg = segments_of(h);
    if (nseg > kMaxSegments || len > kMaxScanLen) return STP3_JPEG_IRREGULAR;
    memset(desc, 0, sizeof(*desc));
    int dc_slot[4] = {-1, -1, -1, -1}, ac_slot[4] = {-1, -1, -1, -1}, ndc = 0, nac = 0;
    for (int c = 0; c < f.ncomp; ++c) {
        const int td = tab[2 * c], ta = tab[2 * c + 1];
        if (dc_slot[td] < 0) {
            if (ndc == 2) return STP3_JPEG_IRREGULAR;
            copy_table(&desc->dc[ndc], dc[td]);
            dc_slot[td] = ndc++;
        }
        if (ac_slot[ta] < 0) {
            if (nac == 2) return STP3_JPEG_IRREGULAR;
            copy_table(&desc->ac[nac], ac[ta]);
            ac_slot[ta] = nac++;
        }
        desc->dc_table[c] = dc_slot[td];
        desc->ac_table[c] = ac_slot[ta];
        memcpy(desc->quant[c], f.quant[f.tq[c]], 64 * sizeof(uint16_t));
    }
    for (int c = 0; c < 3; ++c) {
        const uint16_t* q = f.quant[f.tq[c < f.ncomp ? c : 0]];
        for (int k = 0; k < 64; ++k) quant[c * 64 + kNatural[k]] = q[k];
    }
    const size_t scan_off = (nseg * 12 + kSubBytes - 1) / kSubBytes * kSubBytes;
    if (scan_off > capacity) return STP3_EINVAL;
    const size_t room = capacity - scan_off;                    // for the subsequences and the table behind them
    size_t w = 0, seg = 0;
    for (;;) {
        const size_t seg_start = w;
        int marker = 0;
        for (;;) {                                              // data up to the next marker
            if (pos >= len) return STP3_JPEG_IRREGULAR;         // no EOI
            const uint8_t* ff = static_cast<const uint8_t*>(memchr(data + pos, 0xFF, len - pos));
            const size_t run = ff ? (size_t)(ff - (data + pos)) : len - pos;
            if (run + 1 > room - w) return STP3_EINVAL;         // (w <= room throughout; + 1: a stuffed 0xFF may follow)
            memcpy(out + scan_off + w, data + pos, run);
            w += run;
            pos += run;
            if (!ff || pos + 1 >= len) return STP3_JPEG_IRREGULAR;   // the data runs into the end: no EOI
            marker = data[pos + 1];
            pos += 2;
            if (marker != 0x00) break;
            out[scan_off + w++] = 0xFF;                         // a stuffed 0xFF: data
        }
        const size_t bytes = w - seg_start;
        const size_t padded = bytes ? (bytes + kSubBytes - 1) / kSubBytes * kSubBytes : kSubBytes;
        if (padded > room - seg_start) return STP3_EINVAL;
        memset(out + scan_off + w, 0, seg_start + padded - w);
        w = seg_start + padded;
        int32_t rec[3] = {(int32_t)(seg_start / kSubBytes), (int32_t)(bytes * 8),
                          (int32_t)(seg * (size_t)(f.restart_interval > 0 ? f.restart_interval : 0))};
        memcpy(out + seg * 12, rec, sizeof(rec));               // (seg < nseg: 12 * nseg <= scan_off <= capacity)
        if (marker == 0xD9) {
            if (seg + 1 != nseg) return STP3_JPEG_IRREGULAR;    // fewer restart intervals than the MCU count asks for
            break;
        }
        if (marker != 0xD0 + (int)(seg & 7) || seg + 1 >= nseg) return STP3_JPEG_IRREGULAR;
        ++seg;
    }
    const size_t nsub = w / kSubBytes;
    if (nsub * 4 > room - w) return STP3_EINVAL;
    for (size_t s = 0, i = 0; s < nseg; ++s) {
        int32_t next = (int32_t)nsub;
        if (s + 1 < nseg) memcpy(&next, out + (s + 1) * 12, 4);
        for (const int32_t v = (int32_t)s; i < (size_t)next; ++i) memcpy(out + scan_off + w + i * 4, &v, 4);
    }
    desc->nsub = (int32_t)nsub;
    desc->nseg = (int32_t)nseg;
    desc->seg_offset = 0;
    desc->scan_offset = (int32_t)scan_off;
    desc->subseg_offset = (int32_t)(scan_off + w);
    desc->used_bytes = (int32_t)(scan_off + w + nsub * 4);
    desc->components = f.ncomp;
    desc->hs = h.hs;
    desc->vs = h.vs;
    desc->mcus_x = h.mcus_x;
    desc->mcus_y = h.mcus_y;
    desc->restart_interval = f.restart_interval;
    desc->coef_count = h.coef_count;
    return STP3_OK;
}

}  // namespace stp3_jpeg
