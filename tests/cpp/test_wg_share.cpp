// Host-only check of fdfk::wg_share (fdf_common.h), the split of a frame's index range
// [b, e) over the `chunks` workgroups of orient_kernel and describe_kernel, each share a whole
// number of passes of `per_pass` points.  No device, no libfdf.so.
#include <cstdint>
#include <cstdio>

#include "../../feature_detector_fast_amd/csrc/fdf_common.h"

int main() {
    const uint32_t passes[] = {4, 16, 32, 64, 128};
    const uint64_t bases[] = {0, 5, 1ull << 40};
    const uint32_t chunk_counts[] = {1, 2, 3, 7, 256, 1024};
    unsigned long cases = 0, failures = 0;
    auto fail = [&](const char* what, uint64_t b, uint64_t n, uint32_t chunks, uint32_t P,
                    uint32_t chunk) {
        if (++failures <= 20)
            std::fprintf(stderr, "%s: b=%llu n=%llu chunks=%u P=%u chunk=%u\n", what,
                         (unsigned long long)b, (unsigned long long)n, chunks, P, chunk);
    };
    for (const uint32_t P : passes) {
        const uint64_t lengths[] = {0, 1, P - 1ull, P, P + 1ull, 3ull * P + 2, 1000};
        for (const uint64_t n : lengths)
            for (const uint64_t b : bases)
                for (const uint32_t chunks : chunk_counts) {
                    const uint64_t e = b + n;
                    uint64_t next = b;              // where the shares so far end
                    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
                        const fdfk::IndexRange s = fdfk::wg_share(b, e, chunk, chunks, P);
                        // the kernels' arithmetic before the helper existed, written out
                        uint64_t per = ((e - b) + chunks - 1) / chunks;
                        per = (per + P - 1) / P * P;
                        const uint64_t lo = b + chunk * per < e ? b + chunk * per : e;
                        const uint64_t hi = lo + per < e ? lo + per : e;
                        if (s.lo != lo || s.hi != hi) fail("differs from the formula", b, n, chunks, P, chunk);
                        // contiguous and disjoint: every share starts where the one before ended
                        if (s.lo != next || s.hi < s.lo || s.hi > e) fail("not contiguous", b, n, chunks, P, chunk);
                        if (s.hi > s.lo && (s.lo - b) % P != 0) fail("not on a pass boundary", b, n, chunks, P, chunk);
                        next = s.hi;
                    }
                    if (next != e) fail("does not cover [b, e)", b, n, chunks, P, chunks);
                    ++cases;
                }
    }
    std::printf("wg_share: %lu cases, %lu failures\n", cases, failures);
    return failures ? 1 : 0;
}
