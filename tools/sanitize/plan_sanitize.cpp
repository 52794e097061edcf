// Host planners under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md §5's
// sanitizer row). Built by tools/sanitize/run.sh with the library's own
// sources (host code sanitized, device code compiled as usual and never launched): drives
// every host-only entry that plans or checks a schedule over the sizes the CPU tests cover:
//   gaplac_plan_check          - the single-GPU schedule's launch footprints (every mode),
//                                which also builds / checks every tail task list
//                                (build_tail_tasks, sim_order_tail_tasks, check_tail_tasks,
//                                interleave_tail_tasks) on its first call;
//   gaplac_plan_check_joint    - the joint posterior's three stages (the posterior evaluation,
//                                the covariance launches against both workspaces, the
//                                preloaded factorisation of order M, plain or with riding rows);
//   gaplac_plan_check_sparse   - the sparse entries' three stages (the posterior evaluation of
//                                order Mz with N + Ms riding rows, the launches that form S, the
//                                preloaded factorisation of order Mz) and gaplac_sparse_split;
//   gaplac_plan_check_sparse_grad - the same for gaplac_sparse_elbo_grad: the value's stages,
//                                the order-Mz launches against the gradient's scratch, alpha and
//                                the product kernel against the first workspace and the scratch;
//   gaplac_plan_check_sparse_grad_z - the same for gaplac_sparse_elbo_grad_z: the product's dZ
//                                variant and the dZ launches, the partials as a third region;
//   gaplac_plan_check_sparse_joint - the same for the sparse joint entries: the copy of the a rows,
//                                the covariance launches against the second and third workspace,
//                                the preloaded factorisation of order Ms, plain or with riding rows;
//   gaplac_plan_check_fit      - the fitted posterior: the tile copy and back-substitution of its
//                                creation and its two queries against the fit's own buffer;
//   gaplac_plan_check_laplace_fit - the fitted Laplace posterior: the create-time launches, the
//                                queries with the scaled build and the joint covariance against the
//                                fit's buffer and the second workspace;
//   gaplac_gauss_hermite / gaplac_laplace_predict - the observation-space predictions' host
//                                arithmetic over their edge cases;
//   gaplac_plan_check_schedule - the deferred-update accounting at every depth;
//   gaplac_dist_plan_check     - build_plan / check_plan of the distributed schedule;
//   gaplac_dist_plan           - the plan export;
//   gaplac_dist_plan_check_tail / gaplac_dist_plan_tail - the same with the tail gather.
// Exit 0 when every check passes and no sanitizer fired (halt_on_error=1).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/gaplac.h"

static int fails = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++fails;                      \
        }                                 \
    } while (0)

int main() {
    char msg[256];
    int64_t a = 0, b = 0;
    std::vector<int64_t> sizes;
    for (int64_t n = 1; n <= 300; ++n) sizes.push_back(n);
    for (int64_t n : {383, 384, 385, 511, 512, 513, 1000, 2047, 4095, 4096, 4097, 7000, 8192, 12000, 16384, 65536})
        sizes.push_back(n);
    long checks = 0;
    for (int spw : {1, 2, 4, 5, 8})
        for (int mode : {0, 1, 2, 3})  // 3: logpdf_multi, M responses as dense extra rows
            for (int64_t M : {1, 130, 1000, 6016, 6200}) {
                if (mode < 2 && M != 1) continue;
                for (int64_t N : sizes) {
                    if (mode == 1 && N > 16384) continue;
                    const int rc = gaplac_plan_check(N, mode, mode >= 2 ? M : 0, spw, &a, &b, msg, sizeof msg);
                    EXPECT(rc == 0 && b == 0, "plan_check N=%lld mode=%d M=%lld spw=%d: rc %d violations %lld %s",
                           (long long)N, mode, (long long)M, spw, rc, (long long)b, msg);
                    ++checks;
                }
            }
    // negative control: a workspace one element short must be reported
    for (int64_t N : {1, 127, 255, 300, 4096}) {
        const int rc = gaplac_plan_check(N, 8, 0, 4, &a, &b, msg, sizeof msg);
        EXPECT(rc == 0 && b >= 1, "negative control N=%lld not reported", (long long)N);
    }
    for (int64_t N : {1, 128, 300, 4096}) {  // mode 11: logpdf_multi against the short workspace
        const int rc = gaplac_plan_check(N, 11, 64, 4, &a, &b, msg, sizeof msg);
        EXPECT(rc == 0 && b >= 1, "negative control (mode 11) N=%lld not reported", (long long)N);
    }
    // gaplac_posterior_components: G * M packed rows through the posterior's launchers (mode 2 at
    // M = G * M), at the row counts of tests/test_gpu_components.py; mode 10: the
    // same walk against the short workspace
    for (int64_t rows : {231, 645, 510, 600, 258, 6144, 6147})
        for (int64_t N : {1, 50, 127, 128, 129, 300, 513, 700, 16384}) {
            int rc = gaplac_plan_check(N, 2, rows, 4, &a, &b, msg, sizeof msg);
            EXPECT(rc == 0 && a > 0 && b == 0, "plan_check (component rows) N=%lld rows=%lld: rc %d violations %lld %s",
                   (long long)N, (long long)rows, rc, (long long)b, msg);
            rc = gaplac_plan_check(N, 10, rows, 4, &a, &b, msg, sizeof msg);
            EXPECT(rc == 0 && b >= 1, "negative control (mode 10) N=%lld rows=%lld not reported", (long long)N,
                   (long long)rows);
            ++checks;
        }
    // the joint posterior: stages 1-3, then each workspace one element short
    for (int spw : {1, 4, 8})
        for (int64_t M : {1, 127, 128, 129, 1000, 10300})
            for (int64_t R : {0, 1, 130})
                for (int64_t N : sizes) {
                    const int rc = gaplac_plan_check_joint(N, M, R, spw, 0, &a, &b, msg, sizeof msg);
                    EXPECT(rc == 0 && a > 0 && b == 0, "plan_check_joint N=%lld M=%lld R=%lld spw=%d: rc %d violations %lld %s",
                           (long long)N, (long long)M, (long long)R, spw, rc, (long long)b, msg);
                    ++checks;
                }
    for (int short_ws : {1, 2})
        for (int64_t N : {1, 128, 300, 4096})
            for (int64_t R : {0, 5}) {
                const int rc = gaplac_plan_check_joint(N, 129, R, 4, short_ws, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && b >= 1, "negative control (joint, short_ws %d) N=%lld R=%lld not reported", short_ws,
                       (long long)N, (long long)R);
            }
    EXPECT(gaplac_plan_check_joint(10, 0, 0, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG, "joint: M = 0 accepted");
    // the sparse entries: stages 1-3 (Ms = 0: elbo; Ms > 0: the posterior), the split rule, then
    // each workspace one element short
    for (int spw : {1, 4, 8})
        for (int64_t Mz : {1, 5, 127, 128, 129, 257, 513, 1024, 4096})
            for (int64_t Ms : {0, 1, 129, 1000})
                for (int64_t N : {1, 5, 127, 128, 129, 300, 1023, 1024, 1025, 2051, 16384, 70000}) {
                    const int rc = gaplac_plan_check_sparse(N, Mz, Ms, spw, 0, &a, &b, msg, sizeof msg);
                    EXPECT(rc == 0 && a > 0 && b == 0, "plan_check_sparse N=%lld Mz=%lld Ms=%lld spw=%d: rc %d violations %lld %s",
                           (long long)N, (long long)Mz, (long long)Ms, spw, rc, (long long)b, msg);
                    int64_t chunks = 0, rows = 0;
                    EXPECT(gaplac_sparse_split(N, Mz, &chunks, &rows) == 0 && rows > 0 && chunks == (N + rows - 1) / rows,
                           "sparse_split N=%lld Mz=%lld", (long long)N, (long long)Mz);
                    ++checks;
                }
    for (int short_ws : {1, 2})
        for (int64_t N : {1, 128, 300, 4096})
            for (int64_t Ms : {0, 5}) {
                const int rc = gaplac_plan_check_sparse(N, 129, Ms, 4, short_ws, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && b >= 1, "negative control (sparse, short_ws %d) N=%lld Ms=%lld not reported", short_ws,
                       (long long)N, (long long)Ms);
            }
    EXPECT(gaplac_plan_check_sparse(10, 0, 0, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG, "sparse: Mz = 0 accepted");
    // the gradient of the bound: the value's stages, the order-Mz launches against the scratch, alpha
    // and the product kernel against the first workspace and the scratch; then each one element short
    for (int spw : {1, 4, 8})
        for (int64_t Mz : {1, 5, 127, 128, 129, 257, 513, 1024, 4096})
            for (int64_t N : {1, 5, 127, 128, 129, 300, 700, 1000, 2000, 2051, 16384, 262144}) {
                const int rc = gaplac_plan_check_sparse_grad(N, Mz, spw, 0, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && a > 0 && b == 0, "plan_check_sparse_grad N=%lld Mz=%lld spw=%d: rc %d violations %lld %s",
                       (long long)N, (long long)Mz, spw, rc, (long long)b, msg);
                ++checks;
            }
    for (int short_ws : {1, 2})
        for (int64_t N : {1, 128, 300, 4096})
            for (int64_t Mz : {1, 129, 1000}) {
                int64_t b0 = 0;
                int rc = gaplac_plan_check_sparse(N, Mz, 0, 4, short_ws, &a, &b0, msg, sizeof msg);
                rc = rc ? rc : gaplac_plan_check_sparse_grad(N, Mz, 4, short_ws, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && b >= b0 + 1, "negative control (sparse grad, short_ws %d) N=%lld Mz=%lld not reported",
                       short_ws, (long long)N, (long long)Mz);
            }
    EXPECT(gaplac_plan_check_sparse_grad(10, 0, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG, "sparse grad: Mz = 0 accepted");
    // the same with dZ: the product's dZ variant, the sums over the row tiles, the order-Mz part and
    // the finishing step, the buffer of the partials as a third region; then that one element short
    for (int spw : {1, 4, 8})
        for (int64_t Mz : {1, 5, 127, 128, 129, 257, 513, 1024, 4096})
            for (int64_t N : {1, 5, 127, 128, 129, 300, 700, 1000, 2000, 2051, 16384, 262144}) {
                const int T = 1 + (int)((N + Mz) % 16);
                int rc = gaplac_plan_check_sparse_grad_z(N, Mz, T, spw, 0, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && a > 0 && b == 0, "plan_check_sparse_grad_z N=%lld Mz=%lld T=%d spw=%d: rc %d violations %lld %s",
                       (long long)N, (long long)Mz, T, spw, rc, (long long)b, msg);
                rc = gaplac_plan_check_sparse_grad_z(N, Mz, T, spw, 3, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && b >= 1, "negative control (sparse grad z, short_ws 3) N=%lld Mz=%lld not reported",
                       (long long)N, (long long)Mz);
                ++checks;
            }
    // the sparse joint entries: the sparse posterior's stages, the copy of the a rows, the covariance
    // launches with the mirroring pass and the third factorisation (plain or with R riding rows);
    // then each of the three workspaces one element short
    for (int spw : {1, 4, 8})
        for (int64_t Mz : {1, 5, 127, 128, 129, 257, 1024, 4096})
            for (int64_t Ms : {1, 3, 127, 128, 129, 1000, 10300})
                for (int64_t R : {0, 1, 129})
                    for (int64_t N : {1, 5, 127, 128, 129, 300, 1025, 2051, 16384, 70000}) {
                        const int rc = gaplac_plan_check_sparse_joint(N, Mz, Ms, R, spw, 0, &a, &b, msg, sizeof msg);
                        EXPECT(rc == 0 && a > 0 && b == 0,
                               "plan_check_sparse_joint N=%lld Mz=%lld Ms=%lld R=%lld spw=%d: rc %d violations %lld %s",
                               (long long)N, (long long)Mz, (long long)Ms, (long long)R, spw, rc, (long long)b, msg);
                        ++checks;
                    }
    for (int short_ws : {1, 2, 3})
        for (int64_t N : {1, 127, 300, 4096})
            for (int64_t Ms : {1, 129, 1000})
                for (int64_t R : {0, 3}) {
                    const int rc = gaplac_plan_check_sparse_joint(N, 129, Ms, R, 4, short_ws, &a, &b, msg, sizeof msg);
                    EXPECT(rc == 0 && b >= 1, "negative control (sparse joint, short_ws %d) N=%lld Ms=%lld R=%lld not reported",
                           short_ws, (long long)N, (long long)Ms, (long long)R);
                }
    EXPECT(gaplac_plan_check_sparse_joint(10, 1, 0, 0, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG,
           "sparse joint: Ms = 0 accepted");
    // the fitted posterior: the create-time copy and back-substitution, one mean-and-variance query
    // in chunks of cap and one mean query against the fit's buffer; then the buffer one element short
    for (int spw : {1, 4, 8})
        for (int64_t N : {1, 5, 127, 128, 129, 300, 1000, 4096, 10239, 10240, 16384})
            for (int64_t cap : {1, 128, 129, 1024})
                for (int64_t M : {(int64_t)0, (int64_t)1, cap, cap + 1, 5 * cap + 3})
                    for (int short_ws : {0, 1}) {
                        const int rc = gaplac_plan_check_fit(N, cap, M, spw, short_ws, &a, &b, msg, sizeof msg);
                        EXPECT(rc == 0 && a > 0 && (short_ws ? b >= 1 : b == 0),
                               "plan_check_fit N=%lld cap=%lld M=%lld spw=%d short_ws=%d: rc %d violations %lld %s",
                               (long long)N, (long long)cap, (long long)M, spw, short_ws, rc, (long long)b, msg);
                        ++checks;
                    }
    EXPECT(gaplac_plan_check_fit(10, 0, 1, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG, "fit: cap = 0 accepted");
    // the Laplace entries: one Newton step with a trial point, the final factorisation and a
    // posterior query of M points in its chunks against the workspace and the vectors' buffer;
    // then both one element short
    for (int spw : {1, 4, 8})
        for (int64_t N : {1, 5, 127, 128, 129, 300, 1000, 4096, 10239, 10240, 16384})
            for (int64_t M : {0, 1, 128, 129, 4096, 4097, 9000})
                for (int short_ws : {0, 1}) {
                    const int rc = gaplac_plan_check_laplace(N, M, spw, short_ws, &a, &b, msg, sizeof msg);
                    EXPECT(rc == 0 && a > 0 && (short_ws ? b >= 1 : b == 0),
                           "plan_check_laplace N=%lld M=%lld spw=%d short_ws=%d: rc %d violations %lld %s", (long long)N,
                           (long long)M, spw, short_ws, rc, (long long)b, msg);
                    ++checks;
                }
    EXPECT(gaplac_plan_check_laplace(0, 1, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG, "laplace: N = 0 accepted");
    // the Laplace gradient: the Newton step, the final factorisation with identity rows, the
    // gradient's stages and ending; then the workspace (1) and the vectors' buffer (2) one element short
    for (int spw : {1, 4, 8})
        for (int64_t N : {1, 5, 127, 128, 129, 300, 1000, 2049, 3400, 4096, 10239, 10240, 16384})
            for (int short_ws : {0, 1, 2}) {
                const int rc = gaplac_plan_check_laplace_grad(N, spw, short_ws, &a, &b, msg, sizeof msg);
                EXPECT(rc == 0 && a > 0 && (short_ws ? b >= 1 : b == 0),
                       "plan_check_laplace_grad N=%lld spw=%d short_ws=%d: rc %d violations %lld %s", (long long)N, spw,
                       short_ws, rc, (long long)b, msg);
                ++checks;
            }
    EXPECT(gaplac_plan_check_laplace_grad(0, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG,
           "laplace gradient: N = 0 accepted");
    // the fitted Laplace posterior: create, a query of M points in chunks of cap, a matrix-free mean
    // and a joint covariance of min(M, cap) points; then the fit's buffer (1) and the covariance
    // workspace (2) one element short
    for (int spw : {1, 4, 8})
        for (int64_t N : {1, 5, 127, 128, 129, 300, 1000, 4096, 10239, 10240, 16384})
            for (int64_t cap : {1, 128, 129, 1024})
                for (int64_t M : {(int64_t)1, cap, cap + 1, 5 * cap + 3})
                    for (int short_ws : {0, 1, 2}) {
                        const int rc = gaplac_plan_check_laplace_fit(N, cap, M, spw, short_ws, &a, &b, msg, sizeof msg);
                        EXPECT(rc == 0 && a > 0 && (short_ws ? b >= 1 : b == 0),
                               "plan_check_laplace_fit N=%lld cap=%lld M=%lld spw=%d short_ws=%d: rc %d violations %lld %s",
                               (long long)N, (long long)cap, (long long)M, spw, short_ws, rc, (long long)b, msg);
                        ++checks;
                    }
    EXPECT(gaplac_plan_check_laplace_fit(10, 0, 1, 4, 0, &a, &b, msg, sizeof msg) == GAPLAC_E_ARG,
           "laplace fit: cap = 0 accepted");
    EXPECT(gaplac_fit_mode(nullptr, nullptr) == GAPLAC_E_ARG && gaplac_fit_mean_cov(nullptr, 0, nullptr, 0, 0.0, nullptr, nullptr, 0) == GAPLAC_E_ARG,
           "laplace fit: a NULL handle accepted");
    // the observation-space predictions: every order's rule, then the edge cases of every likelihood
    for (int Q = 1; Q <= 64; ++Q) {
        double x[64], w[64], sum = 0.0;
        EXPECT(gaplac_gauss_hermite(Q, x, w) == 0, "gauss_hermite Q=%d", Q);
        for (int q = 0; q < Q; ++q) sum += w[q];
        for (int q = 1; q < Q; ++q) EXPECT(x[q] > x[q - 1], "gauss_hermite Q=%d: nodes not ascending at %d", Q, q);
        EXPECT(std::fabs(sum - 1.7724538509055160) <= 1e-14, "gauss_hermite Q=%d: weights sum to %.17g", Q, sum);
        ++checks;
    }
    EXPECT(gaplac_gauss_hermite(0, nullptr, nullptr) == GAPLAC_E_ARG && gaplac_gauss_hermite(65, nullptr, nullptr) == GAPLAC_E_ARG,
           "gauss_hermite: a bad order accepted");
    {
        const double mean[] = {0.3, -40.0, 40.0, 9.0, NAN, 0.1, -2.0, 700.0};
        const double var[] = {0.2, 1.0, 1.0, 0.0, 0.5, INFINITY, -1e-14, 3.0};
        const double ysb[] = {1, 0, 1, 0, 1, 0, 1, 0}, ysp[] = {0, 3, 1e4, 7, 1, 2, 0, 5}, ysg[] = {0.1, -3, 2, 9, 0, 1, 2, 3};
        const double bad[] = {1, 0, 0.5, 0, 1, 0, 1, 0};
        double ym[8], yv[8], lp[8];
        for (int lik : {GAPLAC_LIK_GAUSSIAN, GAPLAC_LIK_BERNOULLI, GAPLAC_LIK_POISSON})
            for (int Q : {1, 2, 20, 32, 64})
                for (int64_t M : {0, 1, 8})
                    for (int outs = 0; outs < 8; ++outs)
                        for (int score : {0, 1}) {
                            const double* ys = !score ? nullptr : lik == GAPLAC_LIK_BERNOULLI ? ysb : lik == GAPLAC_LIK_POISSON ? ysp : ysg;
                            const int rc = gaplac_laplace_predict(lik, 0.1, M, mean, var, ys, Q, outs & 1 ? ym : nullptr,
                                                                  outs & 2 ? yv : nullptr, outs & 4 ? lp : nullptr);
                            EXPECT(rc == 0, "laplace_predict lik=%d Q=%d M=%lld outs=%d: rc %d", lik, Q, (long long)M, outs, rc);
                            if (rc == 0 && M == 8 && outs == 7 && score) {
                                EXPECT(std::isnan(ym[4]) && std::isnan(yv[5]) && std::isnan(lp[4]) && std::isnan(lp[5]),
                                       "laplace_predict lik=%d: a non-finite input did not give NaN", lik);
                                EXPECT(std::isfinite(lp[0]) && std::isfinite(lp[1]) && std::isfinite(lp[2]) && std::isfinite(lp[3]) &&
                                           std::isfinite(lp[6]),
                                       "laplace_predict lik=%d Q=%d: a finite input gave a non-finite score", lik, Q);
                            }
                            ++checks;
                        }
        EXPECT(gaplac_laplace_predict(GAPLAC_LIK_BERNOULLI, 0.0, 8, mean, var, bad, 32, ym, yv, lp) == GAPLAC_E_PARAM,
               "laplace_predict: ys outside the support accepted");
        EXPECT(gaplac_laplace_predict(9, 0.0, 8, mean, var, nullptr, 32, ym, yv, lp) == GAPLAC_E_KIND, "laplace_predict: lik 9 accepted");
        EXPECT(gaplac_laplace_predict(GAPLAC_LIK_POISSON, 0.0, 8, mean, var, nullptr, 65, ym, yv, lp) == GAPLAC_E_ARG,
               "laplace_predict: Q = 65 accepted");
    }
    for (int depth = 0; depth <= 8; ++depth) {
        if (depth == 1) continue;
        for (int ext : {0, 1})
            for (int64_t N : {1, 127, 1000, 4096, 10239, 10240, 12000, 16384, 20000, 33000, 40000, 50000, 65536})
                for (int sp : {0, 1, 2, 3}) {
                    const int spw[] = {4, 4, 2, 3}, pm[] = {40, 8, 24, 16};
                    const int rc = gaplac_plan_check_schedule(N, spw[sp], depth, ext, pm[sp], &a, msg, sizeof msg);
                    EXPECT(rc == 0 && a >= 1, "plan_check_schedule N=%lld spw=%d depth=%d ext=%d: %s", (long long)N,
                           spw[sp], depth, ext, msg);
                    ++checks;
                }
    }
    for (int depth : {1, 2, 3, 4, 5, 8})
        for (int spw : {1, 2, 4, 8})
            for (int pair_m : {0, 8, 40})
                for (int nt = 1; nt <= 600; ++nt) {
                    const int rc = gaplac_dist_plan_check(nt, spw, depth, pair_m, &a, msg, sizeof msg);
                    EXPECT(rc == 0, "dist_plan_check nt=%d spw=%d depth=%d pair_m=%d: %s", nt, spw, depth, pair_m, msg);
                    ++checks;
                    for (int tail : {1, 5, 48, 80, 128}) {
                        const int rt = gaplac_dist_plan_check_tail(nt, spw, depth, pair_m, tail, &a, msg, sizeof msg);
                        EXPECT(rt == 0, "dist_plan_check_tail nt=%d spw=%d depth=%d pair_m=%d tail=%d: %s", nt, spw,
                               depth, pair_m, tail, msg);
                        ++checks;
                        if (nt % 97 == 0) {
                            int64_t n = 0;
                            EXPECT(gaplac_dist_plan_tail(nt, spw, depth, pair_m, tail, nullptr, 0, &n) == 0 && n > 0,
                                   "dist_plan_tail size");
                            std::vector<int32_t> out((size_t)(5 * n));
                            EXPECT(gaplac_dist_plan_tail(nt, spw, depth, pair_m, tail, out.data(), 5 * n, &n) == 0,
                                   "dist_plan_tail export");
                        }
                    }
                    if (nt % 97 == 0) {  // the export, sized by a first call
                        int64_t n = 0;
                        EXPECT(gaplac_dist_plan(nt, spw, depth, pair_m, nullptr, 0, &n) == 0 && n > 0, "dist_plan size");
                        std::vector<int32_t> out((size_t)(5 * n));
                        EXPECT(gaplac_dist_plan(nt, spw, depth, pair_m, out.data(), 5 * n, &n) == 0, "dist_plan export");
                    }
                }
    std::printf("sanitized plan checks: %ld checks, %d failures\n", checks, fails);
    return fails ? 1 : 0;
}
