// fit_host_check.cpp -- runs the dense host algebra of the delta fits (facedeform_amd/csrc/fd_fit_host.h) on arrays from a file,
// for tests/test_fit_host.py, which compiles it with the address and undefined-behaviour sanitizers.  Includes that header alone.
//
//   fit_host_check chol N NRHS IN OUT    IN: A (N x N), b (N x NRHS interleaved)       OUT: ok, pmin, pmax, x (N x NRHS)
//   fit_host_check sys M PROJ IN OUT     IN: mu, tt, S (n x M), H (nq x n x n), c (n x 3), delta0 (M x 3), d (M x 3); n = M + 4
//                                        OUT: G (nq x M x M), A (order x order), b (M x 3), S^T c (M x 3), E(d), E(delta0)
//   fit_host_check cot N OMEGA IN OUT    IN: P (N x 3), T (N x 3), omega (N)           OUT: tt, g (N x 3)
//
// Every array is raw float64; the float32 inputs (delta0, P, T, omega) hold float32 values and are narrowed here.  Order 0 of
// chol hands the functions null pointers: they must not touch memory.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fd_fit_host.h"

using namespace fd_fit;

static std::vector<double> read_all(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<double> v;
    double buf[512];
    size_t k;
    while ((k = fread(buf, sizeof(double), 512, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static void write_all(const char *path, const std::vector<double> &v)
{
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); exit(2); }
    if (!v.empty() && fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

// the next `count` values of `in` from *pos on
static const double *take(const std::vector<double> &in, size_t *pos, size_t count)
{
    if (*pos + count > in.size()) { fprintf(stderr, "input file too short\n"); exit(2); }
    const double *p = in.data() + *pos;
    *pos += count;
    return p;
}

static std::vector<float> narrowed(const double *p, size_t count) { return std::vector<float>(p, p + count); }

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: fit_host_check chol|sys|cot A B IN OUT\n"); return 2; }
    const std::string mode = argv[1];
    const int p1 = atoi(argv[2]), p2 = atoi(argv[3]);
    const std::vector<double> in = read_all(argv[4]);
    std::vector<double> out;
    size_t pos = 0;
    if (mode == "chol") {
        const int n = p1, nrhs = p2;
        const double *A_in = take(in, &pos, (size_t)n * n), *b_in = take(in, &pos, (size_t)n * nrhs);
        std::vector<double> A(A_in, A_in + (size_t)n * n), b(b_in, b_in + (size_t)n * nrhs);
        double pmin = -1.0, pmax = -1.0;
        const bool ok = fit_cholesky(n, n ? A.data() : nullptr, pmin, pmax);
        if (ok) fit_cholesky_solve(n, n ? A.data() : nullptr, nrhs, n ? b.data() : nullptr);
        out = {ok ? 1.0 : 0.0, pmin, pmax};
        out.insert(out.end(), b.begin(), b.end());
    } else if (mode == "sys") {
        FitSystem sys;
        sys.M = p1; sys.n = p1 + 4; sys.proj = p2 != 0;
        sys.nq = sys.proj ? 6 : 1; sys.order = sys.proj ? 3 * sys.M : sys.M;
        const size_t M = (size_t)sys.M, n = (size_t)sys.n;
        sys.mu = *take(in, &pos, 1);
        const double tt = *take(in, &pos, 1);
        sys.S = take(in, &pos, n * M);
        const double *H = take(in, &pos, (size_t)sys.nq * n * n);
        const double *c = take(in, &pos, n * 3);
        const std::vector<float> delta0 = narrowed(take(in, &pos, M * 3), M * 3);
        const double *d = take(in, &pos, M * 3);
        fit_compose_G(sys, H);
        std::vector<double> b, Stc;
        fit_rhs(sys, c, delta0.data(), b, Stc);
        const double E_d = fit_energy(sys, Stc, tt, delta0.data(), d);
        const double E_0 = fit_energy_at_delta0(sys, Stc, tt, delta0.data());
        fit_compose_A(sys);
        out = sys.G;
        out.insert(out.end(), sys.A.begin(), sys.A.end());
        out.insert(out.end(), b.begin(), b.end());
        out.insert(out.end(), Stc.begin(), Stc.end());
        out.push_back(E_d);
        out.push_back(E_0);
    } else if (mode == "cot") {
        const size_t N = (size_t)p1;
        const std::vector<float> P = narrowed(take(in, &pos, N * 3), N * 3), T = narrowed(take(in, &pos, N * 3), N * 3);
        const std::vector<float> omega = narrowed(take(in, &pos, N), N);
        std::vector<float> g(N * 3);
        const double tt = fit_cotangent((int64_t)N, P.data(), T.data(), p2 ? omega.data() : nullptr, g.data());
        out.push_back(tt);
        out.insert(out.end(), g.begin(), g.end());
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_all(argv[5], out);
    return 0;
}
