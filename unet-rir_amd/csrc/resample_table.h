// resample_table.h - the polyphase Kaiser-windowed sinc table of csrc/resample.hip, built on the host.  Plain C++: no HIP call, no
// device code, so that tests/probe/resample_table_main.cpp compiles it alone under the host sanitizers.
//
// Rates reduced to L / M (output / input, gcd 1), Z zero crossings to each side, rolloff r and Kaiser beta:
//
//     C = Z max(L, M)      s = r min(1, L / M)      W = C / L      D = ceil(C / L)      T = 2 D
//     h(tau) = s sinc(s tau) I0(beta sqrt(1 - (tau / W)^2)) / I0(beta)     for |tau| < W, else 0          sinc(u) = sin(pi u) / (pi u)
//     table[p][i] = h((p - (i - D + 1) L) / L)                              0 <= p < L, 0 <= i < T
//
// so that y[m] = sum_i table[p][i] x[q - D + 1 + i] with (q, p) = divmod(m M, L).  The support test is the integer one, |p - (i - D + 1) L|
// < C: an entry outside it is exactly 0.  Every entry is evaluated in fp64 at its own argument (no interpolated filter table) and rounded
// to fp32 once.  I0 is its power series sum_k ((x / 2)^2)^k / (k!)^2, run until a term no longer changes the sum (beta <= 32: 60 terms).
#pragma once
#include <math.h>

namespace resample_table {

constexpr int MAX_RATIO = 2048;             // L and M
constexpr int MAX_ZEROS = 64;
constexpr int MAX_TAPS = 8192;              // T
constexpr long long MAX_TABLE = 1 << 20;    // L T

inline int gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// T for a ratio and a number of zero crossings; 0: not supported
inline int taps(int L, int M, int zeros) {
    if (L < 1 || M < 1 || L > MAX_RATIO || M > MAX_RATIO || zeros < 1 || zeros > MAX_ZEROS || gcd(L, M) != 1) return 0;
    const long long C = (long long)zeros * (L > M ? L : M);
    const long long T = 2 * ((C + L - 1) / L);
    return T <= MAX_TAPS && T * L <= MAX_TABLE ? (int)T : 0;
}

// what the kernel takes: a ratio and an (even) T, whatever table they came from
inline bool geometry_ok(int L, int M, int T) {
    return L >= 1 && M >= 1 && L <= MAX_RATIO && M <= MAX_RATIO && gcd(L, M) == 1 && T >= 2 && T <= MAX_TAPS && !(T & 1) &&
           (long long)T * L <= MAX_TABLE;
}

// ceil(N L / M); 0 where N, L or M is not positive or the result leaves 62 bits
inline long long out_length(long long N, int L, int M) {
    if (N < 1 || L < 1 || M < 1) return 0;
    const unsigned __int128 v = ((unsigned __int128)N * (unsigned)L + (unsigned)(M - 1)) / (unsigned)M;
    return v < ((unsigned __int128)1 << 62) ? (long long)v : 0;
}

inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

inline double sinc(double u) {
    if (u == 0.0) return 1.0;
    const double a = M_PI * u;
    return sin(a) / a;
}

// table: L * T floats.  false: arguments outside what taps() and the parameter ranges allow (nothing is written)
inline bool build(float* table, int L, int M, int zeros, double rolloff, double beta) {
    const int T = taps(L, M, zeros);
    if (!table || !T || !(rolloff > 0.0 && rolloff <= 1.0) || !(beta >= 0.0 && beta <= 32.0)) return false;
    const long long C = (long long)zeros * (L > M ? L : M);
    const int D = T / 2;
    const double s = rolloff * (L < M ? (double)L / (double)M : 1.0);
    const double W = (double)C / (double)L;
    const double i0b = bessel_i0(beta);
    for (int p = 0; p < L; ++p) {
        for (int i = 0; i < T; ++i) {
            const long long k = p - (long long)(i - D + 1) * L;
            double v = 0.0;
            if (k > -C && k < C) {
                const double tau = (double)k / (double)L;
                const double u = tau / W;
                v = s * sinc(s * tau) * bessel_i0(beta * sqrt(1.0 - u * u)) / i0b;
            }
            table[(long long)p * T + i] = (float)v;
        }
    }
    return true;
}

}  // namespace resample_table
