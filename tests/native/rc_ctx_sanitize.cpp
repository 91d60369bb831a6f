// Stand-alone driver of the context-selecting range coder (pcgc_rc_encode_ctx / pcgc_rc_decode_ctx, pcgcv2_amd/csrc/hostcodec.cpp) for a
// run under AddressSanitizer and UndefinedBehaviorSanitizer — a CPU build of host code, no GPU and no Python involved:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       tests/native/rc_ctx_sanitize.cpp pcgcv2_amd/csrc/hostcodec.cpp -lz -lpthread -o /tmp/rc_ctx_sanitize && /tmp/rc_ctx_sanitize
//
// It codes random, extreme and cyclic inputs into exactly-sized heap buffers (so a write or read one byte past an end is caught), decodes
// them, and feeds the decoder every truncation of a short stream, trailing bytes and flipped bits.  Exit status 0 and "ok" = clean.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/pcgc_hip.h"
#include "../../pcgcv2_amd/csrc/occupancy_tables.h"

void pcgc_set_error(const char* fmt, ...) { (void)fmt; }        // (coords.hip in the library)

static const uint16_t P1[PCGC_OCC_CONTEXTS] = {PCGC_OCC_P1_VALUES};
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static std::vector<uint8_t> encode(const uint16_t* cdf, int R, const std::vector<uint16_t>& ctx, const std::vector<int16_t>& sym) {
    const int64_t n = (int64_t)sym.size();
    const int64_t need = -pcgc_rc_encode_ctx(cdf, R, 3, ctx.data(), sym.data(), n, nullptr, 0);      // too small on purpose: -needed
    REQUIRE(need > 0);
    uint8_t* exact = (uint8_t*)std::malloc((size_t)need);                                            // exactly sized: ASan guards both ends
    REQUIRE(pcgc_rc_encode_ctx(cdf, R, 3, ctx.data(), sym.data(), n, exact, need) == need);
    for (int64_t cap = 0; cap < need && cap < 40; ++cap) {                                            // every too-small capacity stays inside it
        uint8_t* small = (uint8_t*)std::malloc((size_t)cap + 1);
        REQUIRE(pcgc_rc_encode_ctx(cdf, R, 3, ctx.data(), sym.data(), n, small, cap) == -need);
        std::free(small);
    }
    std::vector<uint8_t> out(exact, exact + need);
    std::free(exact);
    return out;
}
static int decode(const uint16_t* cdf, int R, const std::vector<uint16_t>& ctx, const uint8_t* in, int64_t nbytes, std::vector<int16_t>& sym) {
    uint8_t* exact = (uint8_t*)std::malloc((size_t)nbytes + (nbytes == 0));                           // the decoder may not read past nbytes
    if (nbytes) std::memcpy(exact, in, (size_t)nbytes);
    sym.assign(ctx.size(), -1);
    const int rc = pcgc_rc_decode_ctx(cdf, R, 3, ctx.data(), exact, nbytes, sym.data(), (int64_t)ctx.size());
    std::free(exact);
    return rc;
}

int main() {
    const int R = PCGC_OCC_CONTEXTS;
    std::vector<uint16_t> cdf((size_t)R * 3, 0);
    for (int r = 0; r < R; ++r) cdf[(size_t)r * 3 + 1] = (uint16_t)(65536 - P1[r]);
    long streams = 0, refused = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (int64_t n : {0, 1, 2, 7, 100, 4097, 65537}) {
            std::vector<uint16_t> ctx((size_t)n); std::vector<int16_t> sym((size_t)n), got;
            for (int64_t i = 0; i < n; ++i) {
                if (kind == 0) { ctx[i] = (uint16_t)(i % R); sym[i] = (int16_t)(rnd() & 1); }
                else if (kind == 1) { ctx[i] = (uint16_t)(rnd() % R); sym[i] = (int16_t)((rnd() & 0xFFFF) < P1[ctx[i]]); }
                else if (kind == 2) { ctx[i] = (rnd() & 1) ? 0 : (uint16_t)(R - 1); sym[i] = (int16_t)(ctx[i] == 0); }       // the improbable bit every time
                else { ctx[i] = 176; sym[i] = (int16_t)(rnd() & 1); }
            }
            const std::vector<uint8_t> s = encode(cdf.data(), R, ctx, sym);
            REQUIRE(decode(cdf.data(), R, ctx, s.data(), (int64_t)s.size(), got) == 0 && got == sym);
            ++streams;
            if (kind == 0) {                                                                          // the channel coder's bytes on cyclic contexts
                std::vector<uint8_t> ref(s.size() + 8);
                REQUIRE(pcgc_rc_encode(cdf.data(), R, 3, sym.data(), n, ref.data(), (int64_t)ref.size()) == (int64_t)s.size());
                REQUIRE(std::memcmp(ref.data(), s.data(), s.size()) == 0);
            }
            if (n <= 4097) {
                const int64_t step = s.size() > 64 ? (int64_t)s.size() / 48 : 1;
                for (int64_t k = 0; k < (int64_t)s.size(); k += step) { REQUIRE(decode(cdf.data(), R, ctx, s.data(), k, got) == -3); ++refused; }
                std::vector<uint8_t> longer(s); longer.push_back(0);
                REQUIRE(decode(cdf.data(), R, ctx, longer.data(), (int64_t)longer.size(), got) == -3); ++refused;
                for (size_t at = 0; at < s.size(); at += (size_t)step) {                               // damage: refused, or other symbols; never a fault
                    std::vector<uint8_t> bad(s); bad[at] ^= (uint8_t)(1u << (rnd() & 7));
                    const int rc = decode(cdf.data(), R, ctx, bad.data(), (int64_t)bad.size(), got);
                    REQUIRE(rc == -3 || (rc == 0 && got != sym));
                    refused += rc == -3;
                }
                std::vector<uint8_t> noise(s.size() + 3);
                for (auto& b : noise) b = (uint8_t)rnd();
                (void)decode(cdf.data(), R, ctx, noise.data(), (int64_t)noise.size(), got);
            }
        }
    {   // arguments the functions must refuse without touching memory
        std::vector<uint16_t> ctx{(uint16_t)R}; std::vector<int16_t> sym{0}, got; uint8_t buf[8];
        REQUIRE(pcgc_rc_encode_ctx(cdf.data(), R, 3, ctx.data(), sym.data(), 1, buf, 8) == INT64_MIN);
        REQUIRE(decode(cdf.data(), R, ctx, buf, 1, got) == -2);
        ctx[0] = 0; sym[0] = 2;
        REQUIRE(pcgc_rc_encode_ctx(cdf.data(), R, 3, ctx.data(), sym.data(), 1, buf, 8) == INT64_MIN);
    }
    std::printf("ok: %ld streams round-tripped, %ld damaged streams refused\n", streams, refused);
    return 0;
}
