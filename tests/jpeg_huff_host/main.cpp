// TEST INFRASTRUCTURE -- stp3_jpeg_scan_prepare (csrc/stp3_jpeg_entropy.h) alone in a stand-alone program, built with
// -fsanitize=address,undefined -fno-sanitize-recover by tests/test_jpeg_huff_host_cpu.py.  No HIP, no Python in the process.
//
//     jpeg_huff_host <streams.bin> <out.bin> <truncate_a> <truncate_b> <corruptions>
//
// streams.bin: repeated (uint32 little-endian length, bytes).  Runs stp3_jpeg_scan_prepare on every stream, on every
// truncation of streams number truncate_a and truncate_b and on `corruptions` seeded single-byte and single-bit corruptions
// spread over all streams.  Every buffer is a heap allocation of exactly the size the call is told (the scan buffer: what
// stp3_jpeg_scan_bytes announces, and once more what the first call reported as used), so that the sanitizer sees any access
// outside it.  out.bin, per whole stream: int32 return code and, when it is 0, nsub, nseg, the segment records, the
// subsequences, the segment of every subsequence -- the test compares them with its own statement of the walk.
// Exit status 0: every call returned 0, STP3_EINVAL, STP3_EUNSUP or STP3_JPEG_IRREGULAR, what stp3_jpeg_info refuses is
// refused with the same code, no truncation is accepted, and every accepted descriptor is consistent; 1 otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stp3_jpeg_entropy.h"

namespace {

int failures = 0;
constexpr int32_t kSub = STP3_JPEG_SUB_BYTES;

void fail(const char* what) {
    if (++failures < 10) std::fprintf(stderr, "failure: %s\n", what);
}

struct Prepared {
    int rc;
    stp3_jpeg_scan_desc desc;
    std::vector<uint8_t> scan;
};

// what an accepted call wrote must describe itself
void consistent(const stp3_jpeg_scan_desc& d, const uint8_t* scan, size_t capacity) {
    if (d.nsub < 1 || d.nseg < 1 || d.used_bytes < 0 || (size_t)d.used_bytes > capacity) return fail("counts");
    if (d.seg_offset != 0 || d.scan_offset % kSub || d.scan_offset < 12 * d.nseg) return fail("offsets");
    if (d.subseg_offset != d.scan_offset + d.nsub * kSub || d.used_bytes != d.subseg_offset + 4 * d.nsub) return fail("layout");
    int32_t next = 0;
    for (int32_t s = 0; s < d.nseg; ++s) {
        int32_t rec[3], sub = 0;
        std::memcpy(rec, scan + 12 * s, 12);
        if (rec[0] != next || rec[1] < 0 || rec[1] % 8 || rec[2] != s * d.restart_interval) return fail("segment record");
        const int32_t subs = rec[1] ? (rec[1] / 8 + kSub - 1) / kSub : 1;
        for (int32_t i = 0; i < subs; ++i) {
            if (rec[0] + i >= d.nsub) return fail("segment behind the subsequences");
            std::memcpy(&sub, scan + d.subseg_offset + 4 * (rec[0] + i), 4);
            if (sub != s) return fail("segment of a subsequence");
        }
        for (int32_t i = rec[1] / 8; i < subs * kSub; ++i)
            if (scan[d.scan_offset + rec[0] * kSub + i] != 0) return fail("padding");
        next = rec[0] + subs;
    }
    if (next != d.nsub) return fail("subsequences without a segment");
    for (int c = 0; c < d.components; ++c)
        if (d.dc_table[c] < 0 || d.dc_table[c] > 1 || d.ac_table[c] < 0 || d.ac_table[c] > 1) return fail("table index");
}

Prepared run(const uint8_t* bytes, size_t len) {
    Prepared p;
    uint8_t* data = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(data, bytes, len);
    stp3_jpeg_header h;
    const int info = stp3_jpeg::info(data, len, &h);
    const size_t capacity = info == STP3_OK ? stp3_jpeg::scan_bytes(h, len) : 64;
    uint8_t* scan = static_cast<uint8_t*>(std::malloc(capacity));
    stp3_jpeg_scan_desc* desc = static_cast<stp3_jpeg_scan_desc*>(std::malloc(sizeof(stp3_jpeg_scan_desc)));
    uint16_t* quant = static_cast<uint16_t*>(std::malloc(192 * sizeof(uint16_t)));
    p.rc = stp3_jpeg::scan_prepare(data, len, scan, capacity, desc, quant);
    if (p.rc != STP3_OK && p.rc != STP3_EINVAL && p.rc != STP3_EUNSUP && p.rc != STP3_JPEG_IRREGULAR) fail("return code");
    if (info != STP3_OK && p.rc != info) fail("differs from stp3_jpeg_info");
    if (p.rc == STP3_OK) {
        consistent(*desc, scan, capacity);
        p.desc = *desc;
        p.scan.assign(scan, scan + desc->used_bytes);
        // once more into a block of exactly the bytes used, and into one a byte short
        const size_t used = (size_t)desc->used_bytes;
        uint8_t* tight = static_cast<uint8_t*>(std::malloc(used));
        if (stp3_jpeg::scan_prepare(data, len, tight, used, desc, quant) != STP3_OK || std::memcmp(tight, scan, used)) fail("exact capacity");
        std::free(tight);
        tight = static_cast<uint8_t*>(std::malloc(used - 1));
        if (stp3_jpeg::scan_prepare(data, len, tight, used - 1, desc, quant) != STP3_EINVAL) fail("capacity a byte short");
        std::free(tight);
    }
    std::free(quant);
    std::free(desc);
    std::free(scan);
    std::free(data);
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<std::vector<uint8_t>> streams;
    for (;;) {
        uint8_t l[4];
        if (std::fread(l, 1, 4, f) != 4) break;
        std::vector<uint8_t> s((size_t)l[0] | (size_t)l[1] << 8 | (size_t)l[2] << 16 | (size_t)l[3] << 24);
        if (std::fread(s.data(), 1, s.size(), f) != s.size()) return 2;
        streams.push_back(s);
    }
    std::fclose(f);
    if (streams.empty()) return 2;
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    int prepared = 0, irregular = 0, accepted = 0;
    for (const auto& s : streams) {
        const Prepared p = run(s.data(), s.size());
        const int32_t rc = p.rc;
        std::fwrite(&rc, 4, 1, out);
        if (p.rc != STP3_OK) continue;
        ++prepared;
        std::fwrite(&p.desc.nsub, 4, 1, out);
        std::fwrite(&p.desc.nseg, 4, 1, out);
        std::fwrite(p.scan.data(), 1, 12 * (size_t)p.desc.nseg, out);
        std::fwrite(p.scan.data() + p.desc.scan_offset, 1, (size_t)p.desc.nsub * kSub, out);
        std::fwrite(p.scan.data() + p.desc.subseg_offset, 1, 4 * (size_t)p.desc.nsub, out);
    }
    std::fclose(out);
    for (int k = 3; k <= 4; ++k) {
        const auto& s = streams[(size_t)std::atoi(argv[k]) % streams.size()];
        for (size_t cut = 0; cut < s.size(); ++cut)
            if (run(s.data(), cut).rc == STP3_OK) fail("a truncated stream was accepted");
    }
    uint32_t rng = 2463534242u;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
    const int corruptions = std::atoi(argv[5]);
    for (int i = 0; i < corruptions; ++i) {
        std::vector<uint8_t> s = streams[next() % streams.size()];
        const size_t at = next() % s.size();
        if (i & 1) s[at] = (uint8_t)next();
        else s[at] ^= (uint8_t)(1u << (next() % 8));
        const int rc = run(s.data(), s.size()).rc;
        irregular += rc == STP3_JPEG_IRREGULAR;
        accepted += rc == STP3_OK;
    }
    std::printf("streams %zu prepared %d, corruptions %d accepted %d irregular %d, failures %d\n", streams.size(), prepared, corruptions,
                accepted, irregular, failures);
    return failures ? 1 : 0;
}
