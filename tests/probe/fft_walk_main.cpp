// fft_walk_main.cpp - the host walk of fft_walk.h as a stand-alone program for the host sanitizers (tests/test_fft_lds.py compiles it
// host-only with the address and undefined-behaviour sanitizers on the host code and none on a device: no device code, no HIP call).  For
// every M, mode and thread order it walks impulses and random images whose input, output and image buffers are heap blocks of exactly M
// elements, so an index outside [0, M) anywhere in fft_lds.h is a report.  Exit status 0: no report, every output finite, and the
// three thread orders agree byte for byte.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "fft_walk.h"

using fftwalk::cf;

static unsigned lcg_state = 12345u;
static float uniform() {                                // in (-1, 1)
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return ((int)(lcg_state >> 8) - (1 << 23) + 0.5f) * (1.0f / (1 << 23));
}

static int walk(int M, int mode, const cf* in, const char* what) {
    cf* out[fftwalk::N_ORDERS];
    int bad = 0;
    for (int o = 0; o < fftwalk::N_ORDERS; ++o) {
        out[o] = new cf[M];
        bad |= fftwalk::run(M, mode, o, -1, in, out[o], 1);
        for (int i = 0; i < M; ++i) bad |= !std::isfinite(out[o][i].x) || !std::isfinite(out[o][i].y);
        if (o) bad |= std::memcmp(out[0], out[o], sizeof(cf) * M) != 0;
    }
    for (int o = 0; o < fftwalk::N_ORDERS; ++o) delete[] out[o];
    if (bad) std::fprintf(stderr, "M=%d mode=%d %s: wrong\n", M, mode, what);
    return bad;
}

int main() {
    int bad = 0;
    cf* tab = new cf[4 * fftlds::FL_TAB];
    fftwalk::table(tab);
    delete[] tab;
    for (int M = 64; M <= 2048; M *= 2)
        for (int mode = 0; mode < fftwalk::N_MODES; ++mode) {
            cf* in = new cf[M];
            const int pos[] = {0, 1, 7, 8, 31, 32, M / 2 - 1, M / 2, M / 2 + 1, M - 1};
            for (int p : pos)
                for (int part = 0; part < 2; ++part) {
                    std::memset(in, 0, sizeof(cf) * M);
                    (part ? in[p].y : in[p].x) = 1.0f;
                    bad |= walk(M, mode, in, "impulse");
                }
            for (int rep = 0; rep < 3; ++rep) {
                for (int i = 0; i < M; ++i) in[i] = {uniform(), uniform()};
                bad |= walk(M, mode, in, "random");
            }
            for (int stop = 0; stop < 6; ++stop) {      // a walk ended early is still inside its buffers
                cf* out = new cf[M];
                bad |= fftwalk::run(M, mode, 2, stop, in, out, 1);
                delete[] out;
            }
            delete[] in;
        }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
