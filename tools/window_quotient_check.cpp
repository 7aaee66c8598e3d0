// window_quotient_check.cpp -- the quotient of csrc/window.hip (window_quotient: a float estimate of floor(S n / N), corrected with 32-bit
// integer arithmetic) on the host against 64-bit division.  The device's reciprocal is good to 1 ulp, so every case runs with the
// correctly rounded reciprocal and with its two neighbours.  Cases: the contract's range (n <= 257, N = n + up to 80 other counts,
// S <= N * the largest per-sample cost), at the edges and at random.
//   g++ -O2 -o window_quotient_check tools/window_quotient_check.cpp && ./window_quotient_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

static uint32_t quotient(uint32_t S, uint32_t n, uint32_t N, int ulp)
{
    float rn = 1.0f / (float)N;
    if (ulp) rn = std::nextafterf(rn, ulp > 0 ? 2.0f : 0.0f);
    const uint32_t lo = S * n;
    uint32_t q = (uint32_t)(((float)S * (float)n) * rn);
    int r = (int)(lo - q * N);
    q += (uint32_t)(int)std::floor((float)r * rn);
    r = (int)(lo - q * N);
    if (r < 0) {
        q -= 1u;
        r += (int)N;
    }
    if (r >= (int)N) q += 1u;
    return q;
}

static long check(uint32_t S, uint32_t n, uint32_t N)
{
    long bad = 0;
    const uint32_t want = (uint32_t)(((uint64_t)S * n) / N);
    for (int ulp = -1; ulp <= 1; ulp++)
        if (quotient(S, n, N, ulp) != want) {
            if (!bad) std::printf("S %u n %u N %u ulp %d: %u, want %u\n", S, n, N, ulp, quotient(S, n, N, ulp), want);
            bad++;
        }
    return bad;
}

int main()
{
    long bad = 0, cases = 0;
    std::mt19937_64 rng(12345);
    const uint32_t per[2] = {255u * 255u, 255u}, views[2] = {255u, 257u};
    for (int k = 0; k < 2; k++) {
        // edges: every count against window totals around its multiples, sums at 0, 1, the top and around multiples of N / n
        for (uint32_t n = 1; n <= views[k]; n++)
            for (uint32_t m = 1; m <= 81; m += (m < 4 || m > 78) ? 1 : 7)
                for (int dn = -1; dn <= 1; dn++) {
                    const uint32_t N = n * m + (uint32_t)dn;
                    if (N < n || N > 81u * views[k]) continue;
                    const uint64_t top = (uint64_t)N * per[k];
                    for (uint64_t S : {(uint64_t)0, (uint64_t)1, top, top - 1, top / 2, (uint64_t)N, (uint64_t)N - 1, (uint64_t)N * 1000 / n, (uint64_t)m * 77777}) {
                        if (S > top || S > 0xffffffffull) continue;
                        bad += check((uint32_t)S, n, N);
                        cases++;
                    }
                }
        for (long i = 0; i < 40000000; i++) {
            const uint32_t n = 1 + (uint32_t)(rng() % views[k]);
            const uint32_t N = n + (uint32_t)(rng() % (80u * views[k] + 1u));
            uint64_t top = (uint64_t)N * per[k];
            if (top > 0xffffffffull) top = 0xffffffffull;
            uint64_t S = rng() % (top + 1);
            if (i % 3 == 0) S = top - rng() % 1000 % (top + 1);
            if (((uint64_t)S * n) / N >= (1ull << 24) + (1ull << 20)) continue;   // outside the contract
            bad += check((uint32_t)S, n, N);
            cases++;
        }
    }
    std::printf("%ld cases, %ld wrong\n", cases, bad);
    return bad ? 1 : 0;
}
