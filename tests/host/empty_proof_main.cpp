// Stand-alone program (no device, no HIP): the arithmetic by which the threshold launch proves a live list empty
// (csrc/empty_proof.h, the one copy the kernels run).
//   1. the index for D: the smallest grid point d_j >= D for every D in [0, 0.5] -- grid points, one ulp to either side, the
//      edges, denormals -- and -1 (no proof) for D > 0.5, D < 0 and a NaN;
//   2. the bound: non-decreasing in d for M >= 0 (consecutive grid points, and a point against its neighbours one ulp away),
//      a NaN for M < 0 and for NaN pairs; the rounding to float never goes down;
//   3. the proof: for random sets of {A_t, M_t}, a group's d and tau_min, and ANY D >= d, T <= tau_min, "proved" (the envelope
//      entry for D below T) implies that the tail's own test -- !(U_t(d) < tau_min) for every item -- keeps nothing.  With negative
//      A, M = 0, +-inf, NaN anywhere, d on grid points and beside them, T = -inf.
// Exits 0 and prints "all checks passed".  Meant to be built with -fsanitize=address,undefined as well.
#include <math.h>
#include <stdio.h>

#include <random>
#include <string>
#include <vector>

#include "empty_proof.h"

namespace {

int g_failed = 0;

void fail(const std::string& what)
{
    if (++g_failed <= 20) printf("FAILED: %s\n", what.c_str());
}

// the tail's test, restated from csrc/decode_common.h dae_tile_is_live (a device function there)
bool tile_is_live(float A_t, float M_t, double d_max, float tau_min)
{
    const double d = d_max * (1.0 + 0x1p-40);
    const double A = (double)A_t, dm = d * (double)M_t;
    const double U = A + dm + (fabs(A) + fabs(dm)) * 0x1p-48;
    return !(U < (double)tau_min);
}

long long check_index()
{
    long long n = 0;
    for (int j = 0; j <= DAE_PROOF_GRID; ++j) {
        const float d = dae_proof_grid_d(j);
        if ((double)d != (double)j / 512.0) fail("grid point " + std::to_string(j) + " is not j / 512");
        if (dae_proof_index(d) != j) fail("index of grid point " + std::to_string(j));
        const float below = nextafterf(d, -INFINITY), above = nextafterf(d, INFINITY);
        if (j > 0 && dae_proof_index(below) != j) fail("index one ulp below grid point " + std::to_string(j));
        if (j < DAE_PROOF_GRID && dae_proof_index(above) != j + 1) fail("index one ulp above grid point " + std::to_string(j));
        n += 3;
    }
    if (dae_proof_index(nextafterf(0.5f, INFINITY)) != -1) fail("D one ulp above 0.5 has an index");
    if (dae_proof_index(0.75f) != -1 || dae_proof_index(INFINITY) != -1) fail("D > 0.5 has an index");
    if (dae_proof_index(-0.0f) != 0) fail("D = -0 is the first grid point");
    if (dae_proof_index(nextafterf(0.0f, -INFINITY)) != -1 || dae_proof_index(-1.0f) != -1 || dae_proof_index(-INFINITY) != -1)
        fail("D < 0 has an index");
    if (dae_proof_index(NAN) != -1) fail("a NaN D has an index");
    if (dae_proof_index(1.0e-45f) != 1 || dae_proof_index(1.0e-38f) != 1) fail("a tiny D > 0 takes grid point 1");
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(0.0f, 0.5f);
    for (int rep = 0; rep < 200000; ++rep) {
        const float D = u(rng);
        const int j = dae_proof_index(D);
        if (j < 0 || j > DAE_PROOF_GRID || dae_proof_grid_d(j) < D || (j > 0 && dae_proof_grid_d(j - 1) >= D)) {
            fail("index of a random D is not the smallest grid point at or above it");
            break;
        }
        ++n;
    }
    return n;
}

long long check_bound()
{
    long long n = 0;
    const float As[] = {-8.05f, -0.0f, 0.0f, 3.5f, -1.0e-30f, 1.0e30f, -1.0e30f, -3.4028235e38f};
    const float Ms[] = {0.0f, 0.78f, 1.0e-30f, 17.0f, 1.0e30f, 3.4028235e38f};
    for (float A : As)
        for (float M : Ms) {
            double prev = -INFINITY;
            for (int j = 0; j <= DAE_PROOF_GRID; ++j) {
                const double U = dae_proof_item(A, M, j);
                if (U != U) { fail("a finite pair with M >= 0 gives a NaN"); break; }
                if (U < prev) { fail("the bound goes down between grid points"); break; }
                const double d = (double)dae_proof_grid_d(j);
                if (dae_proof_bound(A, M, nextafter(d, -1.0)) > U || dae_proof_bound(A, M, nextafter(d, 1.0)) < U) {
                    fail("the bound is not monotone around a grid point");
                    break;
                }
                const float f = dae_proof_float_up(U);
                if ((double)f < U) { fail("the rounding to float went down"); break; }
                prev = U;
                ++n;
            }
        }
    if (dae_proof_item(1.0f, -0.5f, 3) == dae_proof_item(1.0f, -0.5f, 3)) fail("M < 0 gives no NaN");
    if (dae_proof_item(NAN, 0.5f, 3) == dae_proof_item(NAN, 0.5f, 3)) fail("a NaN A gives no NaN");
    if (dae_proof_item(1.0f, NAN, 3) == dae_proof_item(1.0f, NAN, 3)) fail("a NaN M gives no NaN");
    if (dae_proof_float_up(-INFINITY) != -INFINITY || dae_proof_float_up(INFINITY) != INFINITY) fail("the rounding moves an infinity");
    if (dae_proof_float_up(1.0e300) != INFINITY) fail("a double beyond float does not round up to +inf");
    if (dae_proof_holds(NAN, 0.0f) || dae_proof_holds(0.0f, NAN)) fail("the verdict holds on a NaN");
    if (dae_proof_holds(-INFINITY, -INFINITY) || dae_proof_holds(-1.0e30f, -INFINITY)) fail("the verdict holds for T = -inf");
    if (!dae_proof_holds(-INFINITY, 0.0f) || dae_proof_holds(1.0f, 1.0f)) fail("the verdict is not a strict <");
    return n;
}

// the envelope as filter_envelope_kernel builds it: the NaN-keeping maximum over the items, rounded up
float envelope_at(const std::vector<float>& A, const std::vector<float>& M, int j)
{
    double u = -INFINITY;
    for (size_t t = 0; t < A.size(); ++t) {
        const double v = dae_proof_item(A[t], M[t], j);
        u = (u != u) ? u : ((v > u || v != v) ? v : u);
    }
    return dae_proof_float_up(u);
}

long long check_proof()
{
    std::mt19937 rng(2024);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    long long n = 0, n_proved = 0;
    const float specials[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN};
    for (int rep = 0; rep < 20000; ++rep) {
        const int cnt = 1 + (int)(rng() % 40);
        std::vector<float> A(cnt), M(cnt);
        const int kind = rep % 8;                                    // 0-4: plain sets; 5: M = 0 mixed in; 6, 7: specials mixed in
        for (int t = 0; t < cnt; ++t) {
            A[t] = (float)(-12.0 + 6.0 * u01(rng));
            M[t] = (float)(2.0 * u01(rng));
            if (kind == 4) A[t] += 7.0f;                              // (around zero, both signs)
            if (kind == 5 && rng() % 3 == 0) M[t] = 0.0f;
            if (kind == 6 && rng() % 16 == 0) A[t] = specials[rng() % 5];
            if (kind == 7 && rng() % 16 == 0) M[t] = rng() % 2 ? specials[rng() % 5] : -(float)u01(rng);
        }
        // the group's d: on a grid point, one ulp to either side of one, or anywhere; now and then out of range or a NaN
        double d;
        const int dk = (int)(rng() % 6);
        const float gp = dae_proof_grid_d((int)(rng() % (DAE_PROOF_GRID + 1)));
        if (dk == 0) d = (double)gp;
        else if (dk == 1) d = (double)nextafterf(gp, -INFINITY) < 0.0 ? 0.0 : (double)nextafterf(gp, -INFINITY);
        else if (dk == 2) d = (double)nextafterf(gp, INFINITY);
        else d = 0.5 * u01(rng);
        if (rep % 97 == 0) d = 0.5 + u01(rng);
        if (rep % 101 == 0) d = (double)NAN;
        // D >= d as a float (the producer rounds up), sometimes larger
        float D = dae_proof_float_up(d);
        if (rng() % 4 == 0 && D == D) D += (float)(0.01 * u01(rng));
        float tau_min = (float)(-10.0 + 10.0 * u01(rng));
        if (rep % 53 == 0) tau_min = -INFINITY;
        if (rep % 59 == 0) tau_min = NAN;
        float T = tau_min;                                           // T <= tau_min
        if (rng() % 2 == 0 && T == T) T -= (float)u01(rng);
        if (rep % 61 == 0) T = -INFINITY;
        const int j = dae_proof_index(D);
        const bool proved = j >= 0 && dae_proof_holds(envelope_at(A, M, j), T);
        if (T == -INFINITY && proved) fail("proved with T = -inf");
        if (D != D && proved) fail("proved with a NaN D");
        if (proved) {
            ++n_proved;
            for (int t = 0; t < cnt; ++t)
                if (tile_is_live(A[t], M[t], d, tau_min)) { fail("proved, but the tail keeps an item (rep " + std::to_string(rep) + ")"); break; }
        }
        ++n;
    }
    if (n_proved < n / 20) fail("the fuzz proves almost nothing: " + std::to_string(n_proved) + " of " + std::to_string(n));
    printf("proof fuzz: %lld sets, %lld proved\n", n, n_proved);
    return n;
}

}  // namespace

int main()
{
    const long long a = check_index(), b = check_bound(), c = check_proof();
    printf("index %lld, bound %lld, proof %lld checks\n", a, b, c);
    if (g_failed) { printf("%d check(s) FAILED\n", g_failed); return 1; }
    printf("all checks passed\n");
    return 0;
}
