// resample_table_main.cpp - csrc/resample_table.h as a stand-alone program for the host sanitizers (tests/test_resample_abi.py compiles it
// host-only with the address and undefined-behaviour sanitizers: the header is plain C++, there is no device code and no HIP call).  It
// builds the table of every ratio and number of zero crossings the tests use, both filter shapes, into a heap block of exactly L T floats,
// so an index outside the table anywhere in the builder is a report, and prints one line per table:
//
//     L M zeros T checksum        checksum = sum_e (e + 1) bits(table[e]) mod 2^64
//
// which the test compares with the same figure of the library's table.  Refused arguments must write nothing: they are given a block of
// one float.  Exit status 0: no report, every entry finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "resample_table.h"

int main() {
    const int ratios[][2] = {{2, 1}, {1, 2}, {3, 2}, {2, 3}, {7, 3}, {3, 7}, {160, 147}, {147, 160}, {441, 1280}};
    const int zeros[] = {1, 2, 16, 64};
    const double shapes[][2] = {{0.9475937167399596, 14.769656459379492}, {0.85, 8.555504641634386}};
    int bad = 0;
    for (const auto& r : ratios)
        for (int z : zeros)
            for (const auto& s : shapes) {
                const int L = r[0], M = r[1], T = resample_table::taps(L, M, z);
                if (!T || (T & 1)) {
                    std::fprintf(stderr, "%d %d %d: no table\n", L, M, z);
                    bad = 1;
                    continue;
                }
                const size_t n = (size_t)L * T;
                float* table = new float[n];
                if (!resample_table::build(table, L, M, z, s[0], s[1])) bad = 1;
                uint64_t sum = 0;
                for (size_t e = 0; e < n; ++e) {
                    uint32_t bits;
                    std::memcpy(&bits, &table[e], 4);
                    sum += (uint64_t)(e + 1) * bits;
                    bad |= !std::isfinite(table[e]);
                }
                delete[] table;
                std::printf("%d %d %d %d %.17g %.17g %llu\n", L, M, z, T, s[0], s[1], (unsigned long long)sum);
            }
    // what the builder refuses, it refuses before it writes
    float* one = new float[1];
    one[0] = 7.0f;
    bad |= resample_table::build(one, 4, 2, 16, 0.85, 8.0) || resample_table::build(one, 2049, 1, 16, 0.85, 8.0) ||
           resample_table::build(one, 3, 2, 65, 0.85, 8.0) || resample_table::build(one, 3, 2, 0, 0.85, 8.0) ||
           resample_table::build(one, 1, 2048, 64, 0.85, 8.0) || resample_table::build(one, 3, 2, 16, 0.0, 8.0) ||
           resample_table::build(one, 3, 2, 16, 1.5, 8.0) || resample_table::build(one, 3, 2, 16, 0.85, -1.0) ||
           resample_table::build(one, 3, 2, 16, 0.85, 33.0) || resample_table::build(one, 3, 2, 16, NAN, 8.0) ||
           resample_table::build(nullptr, 3, 2, 16, 0.85, 8.0) || one[0] != 7.0f;
    delete[] one;
    bad |= resample_table::out_length(1000, 160, 147) != 1089 || resample_table::out_length(0, 1, 1) != 0 ||
           resample_table::out_length(INT64_MAX, 2048, 1) != 0 || resample_table::out_length(INT64_MAX, 1, 2048) != (INT64_MAX >> 11) + 1;
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
