// Host check of the private sin / cos / exp of slam-dynamic_amd/csrc/sd_sim3_math.h against the C library over the arguments an
// accepted OptimizeSim3 update can take: theta in [1e-5, 8] (below 1e-5 Sim3(update) takes its polynomial branch) and sigma in
// [-3, 3] (a scale change of e^3 in one step is already far outside what a loop closure sees).  Prints the largest difference in
// ulps of the library's value; exits 1 when it exceeds 1.  usage  sim3_math_check [samples per range]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sd_sim3_math.h"

static double ulps(double a, double ref)
{
    if (a == ref) return 0;
    int e;
    frexp(ref, &e);
    return fabs(a - ref) / ldexp(1.0, e - 53);
}

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 2000000;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double)(x >> 11) / 9007199254740992.0; };
    double ws = 0, wc = 0, we = 0;
    for (long i = 0; i < n; i++) {
        const double th = exp(log(1e-5) + next() * (log(8.0) - log(1e-5)));      // log-uniform: small angles matter as much as large ones
        double s, c;
        sd_s3_sincos(th, s, c);
        ws = fmax(ws, ulps(s, sin(th))); wc = fmax(wc, ulps(c, cos(th)));
        const double sg = (next() * 2 - 1) * 3.0;
        we = fmax(we, ulps(sd_s3_exp(sg), exp(sg)));
        const double tiny = (next() * 2 - 1) * 1e-4;                             // around the |sigma| < 1e-5 branch and the 1e-9 probes
        we = fmax(we, ulps(sd_s3_exp(tiny), exp(tiny)));
    }
    const double edge[] = {0.0, 1e-9, -1e-9, 1e-5, -1e-5, 709.0, -700.0, 1.0, -1.0};
    for (double v : edge) we = fmax(we, ulps(sd_s3_exp(v), exp(v)));
    printf("%ld samples: sin %.3f ulp, cos %.3f ulp, exp %.3f ulp\n", n, ws, wc, we);
    return (ws > 1.0 || wc > 1.0 || we > 1.0) ? 1 : 0;
}
