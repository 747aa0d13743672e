// fd_fit_host.h -- the dense host algebra of fd_fit_deltas and fd_fit_deltas_shot: the cotangent, the normal system in the
// deltas, its Cholesky factor, and a frame's right-hand side, energy and solve.  Plain C++ on host arrays: nothing here knows of
// a context or of the device, so a stand-alone program can include it (tests/tools/fit_host_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fd_fit {

// C (m x p) += A^T B for row-major A (k x m), B (k x p): rows of B and C are walked contiguously, k in blocks that stay in cache
inline void fit_atb(int m, int p, int k, const double *A, const double *B, double *Cm)
{
    constexpr int kb = 64;
    for (int k0 = 0; k0 < k; k0 += kb) {
        const int k1 = k0 + kb < k ? k0 + kb : k;
        for (int i = 0; i < m; ++i) {
            double *c = Cm + (size_t)i * p;
            for (int kk = k0; kk < k1; ++kk) {
                const double a = A[(size_t)kk * m + i];
                const double *b = B + (size_t)kk * p;
                for (int j = 0; j < p; ++j) c[j] += a * b[j];
            }
        }
    }
}

// a . b with four running sums (a dependent chain of n additions would set the pace of the factorisation)
inline double fit_dot(const double *a, const double *b, int n)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = 0;
    for (; k + 4 <= n; k += 4) { s0 += a[k] * b[k]; s1 += a[k + 1] * b[k + 1]; s2 += a[k + 2] * b[k + 2]; s3 += a[k + 3] * b[k + 3]; }
    for (; k < n; ++k) s0 += a[k] * b[k];
    return (s0 + s1) + (s2 + s3);
}

// A = L L^T in place on the lower triangle of the row-major A (order n); the pivots' extremes; false when a pivot is not
// above n 2^-52 times its diagonal entry, which is where a zero pivot lands in fp64
inline bool fit_cholesky(int n, double *A, double &pmin, double &pmax)
{
    pmin = INFINITY; pmax = 0.0;
    for (int j = 0; j < n; ++j) {
        double *rj = A + (size_t)j * n;
        const double ajj = rj[j];
        const double d = ajj - fit_dot(rj, rj, j);
        if (!(d > (double)n * 0x1p-52 * ajj) || !(d > 0.0) || !(d < INFINITY)) { pmin = d < pmin || d != d ? d : pmin; return false; }
        pmin = d < pmin ? d : pmin; pmax = d > pmax ? d : pmax;
        const double l = sqrt(d), inv = 1.0 / l;
        rj[j] = l;
        for (int i = j + 1; i < n; ++i) {
            double *ri = A + (size_t)i * n;
            ri[j] = (ri[j] - fit_dot(ri, rj, j)) * inv;
        }
    }
    return true;
}

// L L^T x = b for nrhs interleaved right-hand sides (b is n x nrhs row-major, overwritten with x)
inline void fit_cholesky_solve(int n, const double *L, int nrhs, double *b)
{
    for (int i = 0; i < n; ++i) {
        const double *ri = L + (size_t)i * n;
        for (int a = 0; a < nrhs; ++a) {
            double s = b[(size_t)i * nrhs + a];
            for (int k = 0; k < i; ++k) s -= ri[k] * b[(size_t)k * nrhs + a];
            b[(size_t)i * nrhs + a] = s / ri[i];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        for (int a = 0; a < nrhs; ++a) {
            double s = b[(size_t)i * nrhs + a];
            for (int k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * b[(size_t)k * nrhs + a];
            b[(size_t)i * nrhs + a] = s / L[(size_t)i * n + i];
        }
    }
}

// g = omega (T - P), the difference and the product in fp32; returns sum_v omega_v |T_v - P_v|^2
inline double fit_cotangent(int64_t N, const float *P_in, const float *T, const float *omega, float *g)
{
    double tt = 0.0;
    for (int64_t v = 0; v < N; ++v) {
        const float w = omega ? omega[v] : 1.f;
        double t2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const float d = T[3 * v + a] - P_in[3 * v + a];
            g[3 * v + a] = w * d;
            t2 += (double)d * (double)d;
        }
        if (w != 0.f) tt += (double)w * t2;
    }
    return tt;
}

// the normal system in the deltas: unknown 3 i + b with projection (order 3 M), else M with three right-hand sides.  Nothing
// in it depends on the target: one FitSystem serves every frame of a shot.
struct FitSystem {
    int M, n, nq, order;
    bool proj;
    double mu;
    const double *S;
    std::vector<double> G;              // S^T H_q S, nq x M x M
    std::vector<double> A;              // G in block form + mu I; its Cholesky factor after fit_factor
    double pmin = 0.0, pmax = 0.0;
    double at(int i, int bb, int k, int cc) const       // the (3 i + bb, 3 k + cc) entry of the block form, without mu
    {
        static const int qmap[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
        if (!proj) return bb == cc ? G[(size_t)i * M + k] : 0.0;
        return G[(size_t)qmap[bb][cc] * M * M + (size_t)i * M + k];
    }
};

inline void fit_compose_G(FitSystem &sys, const double *H)
{
    const int M = sys.M, n = sys.n;
    sys.G.assign((size_t)sys.nq * M * M, 0.0);
    std::vector<double> HS((size_t)n * M);
    for (int q = 0; q < sys.nq; ++q) {
        std::fill(HS.begin(), HS.end(), 0.0);
        fit_atb(n, M, n, H + (size_t)q * n * n, sys.S, HS.data());                 // H_q is symmetric: H_q^T S
        fit_atb(M, M, n, sys.S, HS.data(), sys.G.data() + (size_t)q * M * M);
    }
}

inline void fit_compose_A(FitSystem &sys)
{
    const int M = sys.M, order = sys.order;
    const double mu = sys.mu;
    sys.A.resize((size_t)order * order);
    if (sys.proj) {
        for (int i = 0; i < M; ++i)
            for (int bb = 0; bb < 3; ++bb)
                for (int k = 0; k < M; ++k)
                    for (int cc = 0; cc < 3; ++cc)
                        sys.A[(size_t)(3 * i + bb) * order + 3 * k + cc] = sys.at(i, bb, k, cc) + (i == k && bb == cc ? mu : 0.0);
    } else {
        for (int i = 0; i < M; ++i)
            for (int k = 0; k < M; ++k) sys.A[(size_t)i * M + k] = sys.G[(size_t)i * M + k] + (i == k ? mu : 0.0);
    }
}

inline bool fit_factor(FitSystem &sys) { return sys.order == 0 || fit_cholesky(sys.order, sys.A.data(), sys.pmin, sys.pmax); }

// one frame's right-hand side b = S^T c + mu delta0 (M x 3), with S^T c kept aside for the energy
inline void fit_rhs(const FitSystem &sys, const double *c, const float *delta0, std::vector<double> &b, std::vector<double> &Stc)
{
    const int M = sys.M;
    b.assign((size_t)M * 3, 0.0);
    fit_atb(M, 3, sys.n, sys.S, c, b.data());
    Stc = b;
    if (delta0) for (size_t i = 0; i < (size_t)M * 3; ++i) b[i] += sys.mu * (double)delta0[i];
}

// the energy of a delta (M x 3) by the quadratic form: d^T G d - 2 d^T S^T c + tt + mu |d - delta0|^2
inline double fit_energy(const FitSystem &sys, const std::vector<double> &Stc, double tt, const float *delta0, const double *d)
{
    const int M = sys.M;
    const bool proj = sys.proj;
    long double e = tt;
    for (int i = 0; i < M; ++i)
        for (int bb = 0; bb < 3; ++bb) {
            long double row = 0.0L;
            for (int k = 0; k < M; ++k)
                for (int cc = 0; cc < 3; ++cc) {
                    if (!proj && cc != bb) continue;
                    row += (long double)sys.at(i, bb, k, cc) * d[3 * k + cc];
                }
            const long double di = d[3 * i + bb], d0 = delta0 ? (long double)delta0[3 * i + bb] : 0.0L;
            e += di * row - 2.0L * di * Stc[3 * i + bb] + (long double)sys.mu * (di - d0) * (di - d0);
        }
    return (double)e;
}

inline double fit_energy_at_delta0(const FitSystem &sys, const std::vector<double> &Stc, double tt, const float *delta0)
{
    std::vector<double> d0v((size_t)sys.M * 3, 0.0);
    if (delta0) for (size_t i = 0; i < (size_t)sys.M * 3; ++i) d0v[i] = (double)delta0[i];
    return fit_energy(sys, Stc, tt, delta0, d0v.data());
}

// one frame's solve against the factor: without projection b is M x 3, three interleaved right-hand sides; with it b is one
// vector of 3 M in the same memory order
inline void fit_solve(const FitSystem &sys, double *b)
{
    if (sys.order > 0) fit_cholesky_solve(sys.order, sys.A.data(), sys.proj ? 1 : 3, b);
}
}  // namespace fd_fit
