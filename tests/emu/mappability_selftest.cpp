// mappability_selftest.cpp — the host-compilable core of the mappability stage (mapad_amd/csrc/mappability_core.hpp) against a brute-force count over the text, in
// a stand-alone program meant for the address and undefined-behaviour sanitizers: the staging (pack16, staged_base, staged_valid at every offset of a block),
// count_start with the scalar rank queries for k around the word boundaries and e = 0 | 1, with and without the early stop, the palindrome rule, bits_in_range and
// possible_starts.  The text has only A, C, G, T, so the index's text is the sequence, '$', its reverse complement, '$'.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_index.hpp"
#include "../../mapad_amd/csrc/mappability_core.hpp"

using namespace mapad;
using namespace mapad::mappability;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (auto& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
static uint64_t occurrences(const std::string& text, const std::string& n) {
    uint64_t c = 0;
    for (size_t at = text.find(n); at != std::string::npos; at = text.find(n, at + 1)) ++c;
    return c;
}
static uint64_t loci(const std::string& text, const std::string& n) {
    const uint64_t s = occurrences(text, n);
    return n == revcomp(n) ? s / 2 : s;
}

int main() {
    std::mt19937 rng(7);
    std::string seq;
    for (int i = 0; i < 300; ++i) seq.push_back("ACGT"[rng() & 3]);
    seq.replace(120, 40, seq.substr(10, 40));             // an exact repeat
    seq.replace(170, 40, revcomp(seq.substr(60, 40)));    // a reverse-complement repeat
    seq.replace(250, 6, "GAATTC");                        // a palindrome
    seq.replace(270, 6, "GAATTG");                        // ... and a neighbour of it
    seq += std::string(140, 'A') + std::string(140, 'T'); // counts beyond a byte at small k
    const std::string text = seq + "$" + revcomp(seq) + "$";
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(seq.data());
    const uint64_t len = seq.size();
    const host::Index ix = host::build_index({"c"}, &sp, &len, 1234);
    const DevIndex v = ix.view();

    // staging: a lower-case and an invalid byte, every block offset
    std::string staged_src = seq;
    staged_src[33] = 'n'; staged_src[34] = (char)(staged_src[34] - 'A' + 'a');
    for (uint64_t blk0 = 0; blk0 < len; blk0 += kBlockStarts) {
        uint32_t base[kStageWords];
        uint16_t valid[kStageWords];
        for (int w = 0; w < kStageWords; ++w) {
            const uint64_t at = blk0 + 16ull * w;
            uint32_t b, vb;
            pack16(reinterpret_cast<const uint8_t*>(staged_src.data()) + at, at < len ? len - at : 0, b, vb);
            base[w] = b; valid[w] = (uint16_t)vb;
        }
        const Staged st{base, valid};
        for (int i = 0; i < kStageBases; ++i) {
            const uint64_t x = blk0 + i;
            const bool ok = x < len && x != 33;
            CHECK(staged_valid(st, i, 1) == ok, "valid bit at %llu", (unsigned long long)x);
            if (ok) CHECK(staged_base(st, i) == base_code((uint8_t)seq[x]), "base at %llu", (unsigned long long)x);
        }
        for (int k : {1, 15, 16, 17, 35, 255})
            for (int i = 0; i + k <= kStageBases; i += 7) {
                bool ok = blk0 + i + k <= len;
                for (int j = 0; ok && j < k; ++j) ok = blk0 + i + j != 33;
                CHECK(staged_valid(st, i, k) == ok, "staged_valid(%d, %d) of block %llu", i, k, (unsigned long long)blk0);
            }
    }

    // count_start against the brute force
    for (int k : {1, 2, 5, 6, 16, 31, 32, 33, 35, 64, 255})
        for (int e = 0; e <= (k <= 35 ? 1 : 0); ++e)
            for (uint64_t blk0 = 0; blk0 < len; blk0 += kBlockStarts) {
                uint32_t base[kStageWords];
                uint16_t valid[kStageWords];
                for (int w = 0; w < kStageWords; ++w) {
                    const uint64_t at = blk0 + 16ull * w;
                    uint32_t b, vb;
                    pack16(sp + at, at < len ? len - at : 0, b, vb);
                    base[w] = b; valid[w] = (uint16_t)vb;
                }
                const Staged st{base, valid};
                const int stride = e ? 3 : 1;  // (the brute force is slow)
                for (int p = 0; p < kBlockStarts && blk0 + p + k <= len; p += stride) {
                    const std::string kmer = seq.substr(blk0 + p, k);
                    uint64_t want = loci(text, kmer);
                    if (e)
                        for (int j = 0; j < k; ++j)
                            for (char b : std::string("ACGT"))
                                if (b != kmer[j]) { std::string n = kmer; n[j] = b; want += loci(text, n); }
                    if (want > 255) want = 255;
                    uint32_t s0 = 0, s1 = 0;
                    const uint32_t stop = count_start(v, st, p, k, e, false, ScalarQuery{}, s0), full = count_start(v, st, p, k, e, true, ScalarQuery{}, s1);
                    CHECK(stop == want && full == want, "k %d e %d start %llu: %u / %u, want %llu", k, e, (unsigned long long)(blk0 + p), stop, full, (unsigned long long)want);
                    CHECK(s0 <= s1 && s0 >= 1, "steps %u > %u", s0, s1);
                }
            }

    // bits_in_range and possible_starts against loops
    uint64_t words[8];
    for (auto& w : words) w = ((uint64_t)rng() << 32) | rng();
    for (int a = 0; a < 300; a += 5)
        for (int n : {1, 2, 35, 63, 64, 65, 128, 255}) {
            if (a + n > 512) continue;
            uint32_t want = 0;
            for (int i = a; i < a + n; ++i) want += (uint32_t)((words[i >> 6] >> (i & 63)) & 1u);
            CHECK(bits_in_range(words, a, n) == want, "bits_in_range(%d, %d)", a, n);
        }
    for (uint64_t L : {0ull, 1ull, 34ull, 35ull, 36ull, 100ull})
        for (uint32_t k : {1u, 2u, 35u, 255u})
            for (uint64_t x = 0; x < L; ++x) {
                uint32_t want = 0;
                for (uint64_t s = x + 1 >= k ? x + 1 - k : 0; s <= x; ++s) want += s + k <= L;
                CHECK(possible_starts(x, k, L) == want, "possible_starts(%llu, %u, %llu)", (unsigned long long)x, k, (unsigned long long)L);
            }
    for (uint32_t c = 1; c <= 255; ++c) {
        const int want = c == 1 ? 0 : c == 2 ? 1 : c <= 4 ? 2 : c <= 8 ? 3 : c <= 16 ? 4 : c <= 32 ? 5 : c <= 64 ? 6 : c <= 128 ? 7 : 8;
        CHECK(hist_bin(c) == want, "hist_bin(%u)", c);
    }
    if (fails) return 1;
    std::printf("mappability selftest ok\n");
    return 0;
}
