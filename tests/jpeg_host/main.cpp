// TEST INFRASTRUCTURE -- the host entropy decoder (csrc/stp3_jpeg_entropy.h) alone in a stand-alone program, built with
// -fsanitize=address,undefined -fno-sanitize-recover by tests/test_jpeg_sanitize_cpu.py.  No HIP, no Python in the process.
//
//     jpeg_host <streams.bin> <truncate_a> <truncate_b> <corruptions>
//
// streams.bin: repeated (uint32 little-endian length, bytes).  Runs stp3_jpeg_info and stp3_jpeg_entropy on every stream, on
// every truncation of streams number truncate_a and truncate_b, and on `corruptions` seeded single-byte and single-bit
// corruptions spread over all streams, and on two crafted streams of 66 049 blocks that walk the DC predictor upwards and
// downwards by 32 767 per block.  Every buffer is a heap allocation of exactly the size the call is told, so that the
// sanitizer sees any access outside it.  Exit status 0: every call returned 0, STP3_EINVAL or STP3_EUNSUP (and every whole
// stream what `info` had announced); 1 otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stp3_jpeg_entropy.h"

namespace {

int failures = 0;

bool allowed(int rc) { return rc == STP3_OK || rc == STP3_EINVAL || rc == STP3_EUNSUP; }

// one pass over `len` bytes copied into a heap block of that size
int run(const uint8_t* bytes, size_t len) {
    uint8_t* data = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(data, bytes, len);
    stp3_jpeg_header h;
    const int rc = stp3_jpeg::info(data, len, &h);
    int rc2 = rc;
    if (!allowed(rc)) ++failures;
    const size_t n = rc == STP3_OK ? (size_t)h.coef_count : 64;
    int16_t* coef = static_cast<int16_t*>(std::malloc(n * sizeof(int16_t)));
    uint16_t* quant = static_cast<uint16_t*>(std::malloc(192 * sizeof(uint16_t)));
    stp3_jpeg_header h2;
    rc2 = stp3_jpeg::entropy(data, len, coef, n, quant, &h2);
    if (!allowed(rc2)) ++failures;
    if (rc != STP3_OK && rc2 == STP3_OK) ++failures;                  // decoded what the header parse refused
    if (rc2 == STP3_OK && (h2.coef_count != h.coef_count || h2.width != h.width || h2.height != h.height)) ++failures;
    std::free(quant);
    std::free(coef);
    std::free(data);
    return rc2;
}

// A syntactically valid grey stream of `height` x `width` whose DC table has the single code '0' for category 15 and whose
// AC table has the single code '0' for end of block: every block is '0', fifteen bits `bit`, '0' -- it adds +32767 (bit 1)
// or -32767 (bit 0) to the DC predictor, which 66 049 blocks would walk out of a 32-bit integer.
std::vector<uint8_t> dc_walk(int height, int width, int bit) {
    std::vector<uint8_t> s = {0xFF, 0xD8, 0xFF, 0xDB, 0x00, 0x43, 0x00};
    s.insert(s.end(), 64, 1);
    const uint8_t sof[] = {0xFF, 0xC0, 0x00, 0x0B, 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 1, 1, 0x11, 0};
    s.insert(s.end(), sof, sof + sizeof(sof));
    for (int tc = 0; tc < 2; ++tc) {
        const uint8_t dht[] = {0xFF, 0xC4, 0x00, 0x14, (uint8_t)(tc << 4), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (uint8_t)(tc ? 0x00 : 15)};
        s.insert(s.end(), dht, dht + sizeof(dht));
    }
    const uint8_t sos[] = {0xFF, 0xDA, 0x00, 0x08, 1, 1, 0x00, 0, 63, 0};
    s.insert(s.end(), sos, sos + sizeof(sos));
    const long blocks = (long)((height + 7) / 8) * ((width + 7) / 8);
    unsigned acc = 0;
    int n = 0;
    auto put = [&](int b) {
        acc = (acc << 1) | (unsigned)b;
        if (++n == 8) {
            s.push_back((uint8_t)acc);
            if ((uint8_t)acc == 0xFF) s.push_back(0x00);
            acc = 0;
            n = 0;
        }
    };
    for (long b = 0; b < blocks; ++b) {
        put(0);
        for (int i = 0; i < 15; ++i) put(bit);
        put(0);
    }
    while (n) put(1);
    s.push_back(0xFF);
    s.push_back(0xD9);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) return 2;
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
    int decoded = 0, refused = 0;
    for (const auto& s : streams) decoded += run(s.data(), s.size()) == STP3_OK;
    for (int k = 2; k <= 3; ++k) {
        const auto& s = streams[(size_t)std::atoi(argv[k]) % streams.size()];
        for (size_t cut = 0; cut < s.size(); ++cut)
            if (run(s.data(), cut) != STP3_EINVAL) ++failures;         // a truncated stream is never accepted
    }
    // values no encoder writes: refused, with every integer inside its type (the sanitizer watches)
    for (int bit = 0; bit < 2; ++bit) {
        const std::vector<uint8_t> s = dc_walk(2056, 2048, bit);
        if (run(s.data(), s.size()) != STP3_EINVAL) ++failures;
    }
    uint32_t rng = 2463534242u;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
    const int corruptions = std::atoi(argv[4]);
    for (int i = 0; i < corruptions; ++i) {
        std::vector<uint8_t> s = streams[next() % streams.size()];
        const size_t at = next() % s.size();
        if (i & 1) s[at] = (uint8_t)next();
        else s[at] ^= (uint8_t)(1u << (next() % 8));
        refused += run(s.data(), s.size()) != STP3_OK;
    }
    std::printf("streams %zu decoded %d, corruptions %d refused %d, failures %d\n", streams.size(), decoded, corruptions, refused,
                failures);
    return failures ? 1 : 0;
}
