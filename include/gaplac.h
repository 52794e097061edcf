/*
 * gaplac.h — C-ABI of libgaplac_hip.so, the MI355X (gfx950) backend for GaPLAC's
 * per-MCMC-step Gaussian-process log-marginal-likelihood.
 *
 * The reference computes, for every evaluation (AbstractGPs 0.5.12 `logpdf(::FiniteGP, v)`,
 * reached from /root/reference/CLI/src/mcmc.jl:35 and /root/reference/CLI/src/select.jl:49-50):
 *
 *     C    = sum_t K_t(X) + noise * I          (kernelmatrix of the tree built by
 *                                               GaPLAC.kernel, src/abstractgp_translations.jl:45-71)
 *     U    = chol_upper(C)                     (LAPACK dpotrf('U'))
 *     logp = -( N*log(2*pi) + 2*sum(log U_ii) + ||U^-T v||^2 ) / 2
 *
 * Each entry point below replaces one piece of that chain; all are plain C, plain
 * pointers and sizes, no device types in the signatures. Host buffers passed in are
 * copied during the call and never retained.
 *
 * Return convention (mirrors LinearAlgebra.cholesky(check=true) and the argument checks
 * of KernelFunctions constructors):
 *     0   success
 *    >0   potrf `info`: 1-based order of the first leading minor that is not positive
 *         definite (the Julia glue rethrows LinearAlgebra.PosDefException(info));
 *         *out_logpdf is NaN
 *    <0   an argument error (GAPLAC_E_*) or a HIP/RCCL runtime error; *out_logpdf is NaN
 *         and gaplac_last_error() holds the text.
 */
#ifndef GAPLAC_H
#define GAPLAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAPLAC_ABI_VERSION 1

/* Kernel-term kinds. Each is the KernelFunctions 0.10.38 kernel that
 * src/abstractgp_translations.jl:8-15 builds for one GaPLAC formula term. */
enum gaplac_kind {
    GAPLAC_SQEXP  = 1, /* SqExp(:x; l)  -> SqExponentialKernel ∘ ScaleTransform(1/l):
                          k = exp(-((x_i - x_j)/l)^2 / 2)       src/gp_parts.jl:21-27 */
    GAPLAC_OU     = 2, /* OU(:x; l)     -> ExponentialKernel ∘ ScaleTransform(1/l):
                          k = exp(-|x_i - x_j|/l)                src/gp_parts.jl:37-43 */
    GAPLAC_LINEAR = 3, /* Linear(:x; c) -> LinearKernel(c): k = x_i*x_j + c, c >= 0
                                                                 src/gp_parts.jl:29-35 */
    GAPLAC_CAT    = 4, /* Cat(:x)       -> CategoricalKernel: k = |x_i - x_j| > 0 ? 0 : 1
                          (the reference's kappa(d2) = d2 > 0 ? 0.0 : 1.0: equal categories 1,
                          and a NaN category 1 with every point, itself included; a non-finite
                          x under SQEXP / OU gives NaN where the difference is NaN, the prior
                          variance k(x, x) included)     src/gp_parts.jl:11-13,45-47 */
    GAPLAC_NOISE  = 5  /* extension (absent in the reference):
                          k = param * delta_ij by index; col ignored */
};

/* One formula term after lowering. `param` is the lengthscale l (SQEXP, OU), the
 * intercept c (LINEAR) or the variance (NOISE); ignored for CAT.
 * `group`: terms with equal group multiply, groups add. The reference lowering
 * (kernel(), abstractgp_translations.jl:45-69) only ever produces sums, so each term has
 * its own group; shared groups are the true-product extension.
 * Terms of one group must be contiguous in the array. */
typedef struct gaplac_term {
    int32_t kind;
    int32_t col;     /* 0-based column of X */
    double  param;
    int32_t group;
    int32_t reserved; /* must be 0 */
} gaplac_term;

#define GAPLAC_MAX_TERMS 16

/* error codes (<0) */
#define GAPLAC_E_ARG      (-1)  /* N < 0, D < 1 with terms reading X, ldx < N, null pointer */
#define GAPLAC_E_KIND     (-2)  /* unknown term kind / too many terms / bad group order */
#define GAPLAC_E_PARAM    (-3)  /* l <= 0 or non-finite, c < 0, noise < 0 */
#define GAPLAC_E_COL      (-4)  /* column index outside [0, D) */
#define GAPLAC_E_NODEVICE (-5)  /* no HIP device / device index out of range */
#define GAPLAC_E_HIP      (-6)  /* HIP runtime failure (text in gaplac_last_error) */
#define GAPLAC_E_OOM      (-7)  /* device allocation failed */
#define GAPLAC_E_COMM     (-8)  /* RCCL failure / communicator missing */

typedef struct gaplac_ctx gaplac_ctx;

/* Context: one device, one persistent workspace (the (N+1)-augmented covariance,
 * grown on demand and reused across MCMC steps), two HIP streams. Not re-entrant;
 * distinct contexts may be used from distinct threads.
 * Replaces: nothing in the reference (AbstractGPs allocates ~2T+3 N×N temporaries per
 * logpdf); needed so repeated MCMC evaluations do not re-allocate. */
int  gaplac_ctx_create(int device, gaplac_ctx** out);
int  gaplac_ctx_destroy(gaplac_ctx* ctx);
/* Free the context's large device workspaces (the evaluation matrix, the batched-select
 * workspace sets, the batch lanes) after waiting for its work; the next call allocates
 * again. For callers that share a device between several contexts or processes.
 * Replaces: nothing (the reference frees its temporaries per call). */
int  gaplac_ctx_release(gaplac_ctx* ctx);
const char* gaplac_last_error(const gaplac_ctx* ctx);
int  gaplac_abi_version(void);

/* The hot path. Host pointers. X is N×D column-major with leading dimension ldx (Julia
 * `Matrix(df[!, vars])` wrapped as RowVecs: observations are rows), v has N entries
 * (`y` in select.jl:49-50, the latent `fx` in mcmc.jl:35). noise is the FiniteGP
 * observation variance (0.1 at every reference call site).
 * Replaces: AbstractGPs.logpdf(FiniteGP(GP(kernel(formula)), RowVecs(X), noise), v)
 *           = kernelmatrix (KernelFunctions) + cholesky(Symmetric) (dpotrf 'U')
 *             + logdet + sum(abs2, U' \ v).
 * out_logdet / out_quad may be NULL. */
int gaplac_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                  int32_t T, const gaplac_term* terms, double noise, const double* v,
                  double* out_logpdf, double* out_logdet, double* out_quad);

/* Same, with X and v already resident in device memory (HBM) on the ctx's device.
 * This is the entry the throughput benchmark times. */
int gaplac_logpdf_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx,
                         int32_t T, const gaplac_term* terms, double noise, const double* dv,
                         double* out_logpdf, double* out_logdet, double* out_quad);

/* Batched select (BASELINE config 5): nmodels independent formulas over the same X and
 * v; model m uses terms[term_offset[m] .. term_offset[m+1]). Replaces the two (or more)
 * `logpdf(pr_k, y_k)` calls of CLI/src/select.jl:49-50. out_logpdf / out_info have
 * nmodels entries; the return value is 0 when the batch ran (per-model PD failures are
 * reported in out_info[m] > 0 with out_logpdf[m] = NaN) and <0 on argument/runtime
 * errors. Each result is bitwise that model's gaplac_logpdf. Device memory: up to two
 * workspace sets of GAPLAC_BATCH_W (32) matrices of (N+1 rounded up to 128)^2 doubles,
 * fewer models per set when the free device memory (hipMemGetInfo, 2 GiB kept free) does
 * not hold them, and the two-lane path below two; gaplac_ctx_release frees them. */
int gaplac_logpdf_batch(gaplac_ctx* ctx, int32_t nmodels, int64_t N, int32_t D,
                        const double* X, int64_t ldx, const int32_t* term_offset,
                        const gaplac_term* terms, double noise, const double* v,
                        double* out_logpdf, int64_t* out_info);

/* Gradient of the same log-marginal-likelihood. NUTS in
 * CLI/src/mcmc.jl:31-41 differentiates logpdf(FiniteGP(GP(kernel(formula; ℓ)), RowVecs(X),
 * 0.1), fx) with ForwardDiff Duals, which cannot cross a ccall; the GaPLAC-owned method
 * returns the analytic gradient instead (a ChainRules rrule / Dual overload):
 *     out_dv[i]     = d logp / d v_i          = -(C^{-1} v)_i                  (N entries)
 *     out_dparam[t] = d logp / d param_t      = 1/2 (a' dC a - tr(C^{-1} dC)),  a = C^{-1} v,
 *                     dC = dK_t/dparam_t (times the other terms of t's product group):
 *                     l of SQEXP / OU (k u^2/l, k |u|/l with u = x_i/l - x_j/l), c of LINEAR (1),
 *                     the variance of a NOISE term (delta_ij); 0 for CAT (no parameter)
 *     out_dnoise    = d logp / d noise        (dC = I)
 * The mcmc glue sums out_dparam over the terms whose variable is in `--infer` (they share ℓ).
 * Any output pointer may be NULL. Same return convention as gaplac_logpdf (outputs NaN on
 * error / PosDefException). Replaces: ForwardDiff.gradient through AbstractGPs.logpdf. */
int gaplac_logpdf_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                       int32_t T, const gaplac_term* terms, double noise, const double* v,
                       double* out_logpdf, double* out_dv, double* out_dparam, double* out_dnoise);
/* Same with X and v resident on the device (outputs are host pointers). */
int gaplac_logpdf_grad_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx,
                              int32_t T, const gaplac_term* terms, double noise, const double* dv,
                              double* out_logpdf, double* out_dv, double* out_dparam, double* out_dnoise);

/* Posterior mean and variance at M test points:
 *     mean_j = k(xs_j, X) C^{-1} y,   var_j = k(xs_j, xs_j) - k(xs_j, X) C^{-1} k(X, xs_j)
 * with C = K(X) + noise I (the FiniteGP's covariance) and the latent kernel k (no noise) for
 * the test points. Xs is M x D column-major (leading dimension ldxs) with the same columns as
 * X. Replaces: mean_and_var(posterior(FiniteGP(GP(k), X, noise), y), xs) of AbstractGPs
 * 0.5.12, reached from src/plotting.jl:8-12 (and posterior(pr, y) in CLI/src/select.jl:51-52).
 * Same return convention as gaplac_logpdf (PosDefException info > 0; outputs NaN). */
int gaplac_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                              int32_t T, const gaplac_term* terms, double noise, const double* y,
                              int64_t M, const double* Xs, int64_t ldxs,
                              double* out_mean, double* out_var);

/* Per-component posteriors at M test points (the arithmetic of the reference's `fitplot`
 * command, "the posteriors of different components of the GP"): for a formula k = sum_g k_g,
 *     mean_g(xs_j) = K_g(xs_j, X) C^{-1} y
 *     var_g(xs_j)  = k_g(xs_j, xs_j) - K_g(xs_j, X) C^{-1} K_g(X, xs_j)
 * with C = K(X) + noise I built from every term and K_g from component g's terms only. All G
 * components ride one factorisation as G*M extra rows. comp has T entries: comp[t] in [0, G) is
 * the component of term t, -1 puts the term in none; all terms of one product group must carry
 * the same value (GAPLAC_E_KIND otherwise). out_mean / out_var are M x G column-major (leading
 * dimensions ldm / ldv; rows M .. ld-1 are never written); either may be NULL. A component
 * without terms is the zero process (mean and variance exactly +0.0); a component made of a
 * NOISE term has mean exactly 0 and the term's variance; the observation noise belongs to no
 * component. The component means sum to gaplac_posterior_mean_var's mean when every non-NOISE
 * term is in a component.
 * Same return convention as gaplac_posterior_mean_var: every output entry is NaN-filled first
 * and stays NaN on a PosDefException (info > 0); the context stays usable after every failure.
 * GAPLAC_E_ARG also for G < 0, comp NULL with G > 0 and T > 0, an entry outside [-1, G),
 * ldm < M or ldv < M for a non-NULL output. G = 0 or M = 0: 0 after the argument and term
 * checks, nothing written. N = 0: the prior (mean 0, variance kdiag_g). GAPLAC_E_OOM when
 * ceil(G*M/128) > 65535 or the rows do not fit in device memory beside the matrix (no chunking).
 * Replaces: mean_and_var(posterior(FiniteGP(GP(k), X, noise), y) with the kernel k_g, xs) per
 *           component, as the reference's unimplemented `fitplot` (README) would need; nothing
 *           in AbstractGPs 0.5.12 does it in one call. */
int gaplac_posterior_components(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                                int32_t T, const gaplac_term* terms, double noise, const double* y,
                                int64_t M, const double* Xs, int64_t ldxs,
                                int32_t G, const int32_t* comp,
                                double* out_mean, int64_t ldm, double* out_var, int64_t ldv);

/* Fitted posterior: the factorisation done once and kept, then queried at any number of test
 * sets (what AbstractGPs' PosteriorGP holds: the Cholesky factor and alpha = C^{-1} y).
 * The create entry runs the evaluation of the plain logpdf entry (its logpdf, logdet and quad
 * are bitwise that entry's for the same arguments) and moves the factor's lower tiles, the
 * diagonal blocks' inverses, z = L^{-1} y, X, the terms and noise into device memory the fit
 * owns, with room for cap test rows below the factor; it then computes alpha = L^{-T} z by
 * back-substitution. The context's workspace is free again afterwards: any entry may run on the
 * context between queries, and several fits may live on one context. cap >= 1 is the largest
 * number of test points solved at once; a mean-and-variance query of more points runs in chunks
 * of cap rows (rows are independent, so M has no upper limit).
 * Returns 0, info > 0 on a PosDefException (*out is NULL, the text of the last error names the
 * matrix), GAPLAC_E_ARG also for cap < 1 or out NULL, GAPLAC_E_OOM when the fit's buffer
 * ((Np + 128 ceil(cap/128)) Np doubles and a few vectors, Np = roundup(N+1, 128)) does not fit
 * or ceil(cap/128) > 65535. The context stays usable after every failure. N = 0: a fit of the
 * empty FiniteGP (logpdf -0, every query returns the prior).
 * Replaces: posterior(FiniteGP(GP(k), X, noise), y) of AbstractGPs 0.5.12 (src/plotting.jl:8-12,
 *           CLI/src/select.jl:51-52), the object; the queries below are its mean_and_var. */
typedef struct gaplac_fit gaplac_fit;
int gaplac_fit_create(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                      int32_t T, const gaplac_term* terms, double noise, const double* y,
                      int64_t cap, gaplac_fit** out);
/* Frees the fit (NULL: 0). Valid before or after its context's destruction, which frees the
 * fit's device memory and leaves the handle good for this call only. */
int gaplac_fit_destroy(gaplac_fit* fit);
/* N, cap and the evaluation's results; any pointer may be NULL. GAPLAC_E_ARG for a NULL fit. */
int gaplac_fit_info(const gaplac_fit* fit, int64_t* out_N, int64_t* out_cap, double* out_logpdf,
                    double* out_logdet, double* out_quad);
/* alpha = C^{-1} y (N values), as computed at creation. */
int gaplac_fit_alpha(gaplac_fit* fit, double* out_alpha);
/* Posterior mean at M test points, matrix-free: mean_j = sum_n k(xs_j, x_n) alpha_n with the
 * latent kernel (no noise; a NOISE term is 0 across point sets). Nothing of size M x N is
 * stored and the factor is not read. Any M. */
int gaplac_fit_mean(gaplac_fit* fit, int64_t M, const double* Xs, int64_t ldxs, double* out_mean);
/* Posterior mean and variance at M test points, the arithmetic of the one-shot posterior entry
 * without its factorisation: K(xs, X) is written below the kept factor, solved against it
 * (V^T = K(xs, X) L^{-T}), and mean_j = V^T[j,:] z, var_j = k(xs_j, xs_j) - |V^T[j,:]|^2.
 * out_mean may be NULL; out_var NULL gives the matrix-free mean entry above.
 * All three queries: outputs are NaN-filled first; GAPLAC_E_ARG for a NULL fit, a fit whose
 * context has been destroyed, M < 0, Xs NULL or ldxs < M with M > 0 and D > 0, a NULL output of
 * positive size; M = 0 writes nothing; a fit of N = 0 gives the prior (mean 0, variance kdiag).
 * Two identical calls give bitwise identical results. */
int gaplac_fit_mean_var(gaplac_fit* fit, int64_t M, const double* Xs, int64_t ldxs,
                        double* out_mean, double* out_var);

/* Laplace approximation of a latent GP under a non-Gaussian observation model (Rasmussen &
 * Williams, Algorithms 3.1 and 5.1; ApproximateGPs.jl's LaplaceApproximation). The latent
 * covariance is K = sum_t K_t(X) + jitter I (the terms' own NOISE stays in K; jitter >= 0 stands
 * where noise does in the other entries); the likelihood factorises over the observations:
 *   GAPLAC_LIK_GAUSSIAN   y_i ~ N(f_i, lik_param), lik_param = variance > 0 (the approximation is
 *                         exact: log q = gaplac_logpdf at noise = jitter + lik_param)
 *   GAPLAC_LIK_BERNOULLI  logistic link, y_i in {0, 1}: log p = y f - log(1 + e^f)
 *   GAPLAC_LIK_POISSON    exp link, y_i a non-negative integer value: log p = y f - e^f - lgamma(y+1)
 * Newton's iteration on psi(a) = -a^T f / 2 + sum_i log p(y_i | f_i), f = K a, from a = a0 (NULL:
 * 0): per step one factorisation of B = I + sqrt(W) K sqrt(W) (W = -d^2 log p / df^2 >= 0), then the
 * step (a, f) + s ((a+, f+) - (a, f)) with the first s = 1, 1/2, ... (at most 20 halvings) whose psi
 * is finite and >= psi_old - tol (1 + |psi_old|). It stops when |psi_new - psi_old| <= tol (1 +
 * |psi_new|) (*out_converged = 1) or after max_iter steps (*out_converged = 0: not an error; the
 * results are those of the last iterate). Then W at the last iterate, one more factorisation, and
 *   log q(y | X) = -a^T f / 2 + sum_i log p(y_i | f_i) - sum_i log L_ii.
 * out_f / out_a (N values, either may be NULL): the mode f and a = K^{-1} f = grad log p(y | f);
 * a is a warm start (a0) for a call with nearby parameters. *out_iters: Newton steps taken.
 * Outputs are NaN-filled first. Returns 0; info > 0 (also in *out_info) when a factorisation of B
 * failed, which an indefinite matrix cannot cause (B >= I): W was not finite (an overflowing
 * e^f), the last error's text names B; GAPLAC_E_KIND for an unknown lik; GAPLAC_E_PARAM for
 * jitter < 0, tol <= 0 or non-finite, max_iter < 1, a Gaussian variance <= 0, or a y outside the
 * likelihood's support (checked on the host before anything is launched); GAPLAC_E_ARG as the
 * other entries. N = 0: log q = 0, no steps, converged. The context stays usable after every
 * failure; two identical calls give bitwise identical results. Not in the reference (its formula's
 * likelihood slot is parsed and ignored). */
#define GAPLAC_LIK_GAUSSIAN 0   /* lik_param = variance > 0 */
#define GAPLAC_LIK_BERNOULLI 1  /* logistic link, y in {0, 1} */
#define GAPLAC_LIK_POISSON 2    /* exp link, y a non-negative integer value */
int gaplac_laplace_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                          int32_t T, const gaplac_term* terms, double jitter, int32_t lik,
                          double lik_param, const double* y, int32_t max_iter, double tol,
                          const double* a0 /* NULL: 0 */, double* out_logq,
                          double* out_f /* N, may be NULL */, double* out_a /* N, may be NULL */,
                          int32_t* out_iters, int32_t* out_converged, int64_t* out_info);
/* The same iteration, then the latent posterior at M test points (ld ldxs):
 *   mean_j = sum_n k(xs_j, x_n) a_n,   var_j = k(xs_j, xs_j) - |L^{-1} (sqrt(W) k(X, xs_j))|^2,
 * the rows sqrt(W_n) k(x_n, xs_j) riding below B in the final factorisation (test points beyond
 * 4096 in further chunks, each with a factorisation of its own). out_mean / out_var: M values,
 * either may be NULL. GAPLAC_E_ARG also for M < 0, Xs NULL or ldxs < M. N = 0: the prior (mean 0,
 * variance kdiag). */
int gaplac_laplace_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X,
                                      int64_t ldx, int32_t T, const gaplac_term* terms, double jitter,
                                      int32_t lik, double lik_param, const double* y, int32_t max_iter,
                                      double tol, const double* a0, int64_t M, const double* Xs,
                                      int64_t ldxs, double* out_logq, double* out_mean, double* out_var,
                                      int32_t* out_iters, int32_t* out_converged, int64_t* out_info);
/* The same iteration (f, a, iters and converged come out bitwise equal to gaplac_laplace_logpdf's),
 * then the gradient of log q in every term's parameter and in the jitter (Rasmussen & Williams,
 * Algorithm 5.1). With K~ = K + jitter I, R = sqrt(W) B^{-1} sqrt(W), rho_i = (d^3 log p / df_i^3) /
 * W_i (Bernoulli: tanh(f_i / 2); Poisson: -1; Gaussian: 0; nothing is divided by W):
 *   s2 = (1 - diag B^{-1}) rho / 2,   u = s2 - R (K~ s2),
 *   d log q / d theta_t = 1/2 sum_ij (a_i a_j - R_ij) dK~_ij/dtheta_t + sum_ij u_i dK~_ij/dtheta_t a_j,
 *   d log q / d jitter  = 1/2 (a^T a - tr R) + u^T a.
 * The first sums are the explicit part (the mode held fixed), the second the implicit part (the
 * mode moves with the parameter). The final factorisation of B carries identity rows, which leave
 * L^{-T}; its rows scaled by sqrt(W) give R as a product, and gaplac_logpdf_grad's contraction runs
 * on it with alpha = a. out_dparam[t]: explicit + implicit, in the term's own parameter (l, c or a
 * Noise term's variance; 0 for Cat), inside a product group times the group's other terms.
 * *out_djitter likewise; for the Gaussian likelihood d log q / d lik_param equals *out_djitter
 * (log q depends on jitter + lik_param alone). out_implicit (T + 1 values): the implicit parts of
 * dparam and djitter alone (exactly 0 for the Gaussian likelihood). Every output pointer may be
 * NULL; all are NaN-filled first. Return codes, *out_info and the context's state after a failure as
 * gaplac_laplace_logpdf; N = 0: log q = 0 and every gradient 0. Not converged (*out_converged = 0)
 * is not an error: the gradient is then the same expression at the last iterate, which is not the
 * exact derivative of the reported log q (the expression assumes a stationary point). Two
 * identical calls give bitwise identical results. Not in the reference. */
int gaplac_laplace_logpdf_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                               int32_t T, const gaplac_term* terms, double jitter, int32_t lik,
                               double lik_param, const double* y, int32_t max_iter, double tol,
                               const double* a0 /* NULL: 0 */, double* out_logq,
                               double* out_f /* N */, double* out_a /* N */, int32_t* out_iters,
                               int32_t* out_converged, int64_t* out_info, double* out_dparam /* T */,
                               double* out_djitter,
                               double* out_implicit /* T + 1: the implicit parts of dparam and djitter, may be NULL */);

/* Fitted Laplace posterior: gaplac_laplace_logpdf's iteration (same arguments, checks, return
 * codes; f, a, log q, iters and converged bitwise that entry's), after whose final factorisation
 * the factor of B = I + sqrt(W) K~ sqrt(W), the diagonal blocks' inverses, X, the terms (noise =
 * jitter), sqrt(W), the mode f and a = grad log p(y | f) move into a gaplac_fit with room for cap
 * test rows, as gaplac_fit_create does for the exact posterior. The handle is the same type with a
 * kind inside: gaplac_fit_destroy, the context's bookkeeping and every query take both kinds.
 *   gaplac_fit_info      logpdf := log q, logdet := log|B|, quad := a^T f
 *   gaplac_fit_alpha     a (no back-substitution: a is the iteration's)
 *   gaplac_fit_mean      sum_n k(xs_j, x_n) a_n, matrix-free
 *   gaplac_fit_mean_var  per chunk of cap points the rows sqrt(W_n) k(xs_j, x_n) are written below
 *                        the kept factor and solved against it; var_j = k(xs_j, xs_j) - |V_j|^2, the
 *                        mean the matrix-free one
 * Not converged is not an error (the handle holds the last iterate, *out_converged = 0). A failed
 * factorisation of B gives info > 0 and no handle (*out = NULL). GAPLAC_E_ARG also for cap < 1 or
 * out NULL. N = 0: a fit that returns the prior. The context's workspace is free afterwards. */
int gaplac_laplace_fit_create(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                              int32_t T, const gaplac_term* terms, double jitter, int32_t lik,
                              double lik_param, const double* y, int32_t max_iter, double tol,
                              const double* a0 /* NULL: 0 */, int64_t cap, gaplac_fit** out,
                              int32_t* out_iters, int32_t* out_converged, int64_t* out_info);
/* The mode f (N values) of a Laplace fit. GAPLAC_E_ARG for a NULL or an exact fit. */
int gaplac_fit_mode(gaplac_fit* fit, double* out_f);
/* What a Laplace fit was created with and how its iteration ended; any pointer may be NULL.
 * GAPLAC_E_ARG for a NULL or an exact fit. */
int gaplac_fit_laplace_info(const gaplac_fit* fit, int32_t* out_lik, double* out_lik_param,
                            double* out_jitter, int32_t* out_iters, int32_t* out_converged);
/* Mean and joint covariance at M <= cap test points from a fit of either kind: the query's rows,
 * then Sigma* = K(xs) + noise_s I - V^T V, full and exactly symmetric (M x M column-major, leading
 * dimension ldc), in the format of gaplac_posterior_mean_cov, formed in the context's second
 * workspace. out_mean may be NULL; out_cov NULL gives the matrix-free mean. Outputs are NaN-filled
 * first. GAPLAC_E_ARG for M > cap (the message says so), noise_s < 0 or non-finite, ldc < M, a
 * NULL fit or one whose context is gone, and as the other queries. N = 0: the prior's Gram. */
int gaplac_fit_mean_cov(gaplac_fit* fit, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                        double* out_mean, double* out_cov, int64_t ldc);

/* Observation-space predictions from a latent (mean, var): host arithmetic, no context, no device.
 * gaplac_gauss_hermite: the physicists' Gauss-Hermite rule of order 1 <= Q <= 64 (weight e^{-x^2},
 * ascending nodes; either output may be NULL), computed once per Q in long double by Newton on the
 * orthonormal Hermite recurrence. GAPLAC_E_ARG for Q outside [1, 64].
 * gaplac_laplace_predict: per point, v = max(var, 0), sigma = sqrt(v) and
 *   int h(f) N(f | mean, v) df ~ pi^{-1/2} sum_q w_q h(mean + sqrt(2) sigma x_q):
 *   GAUSSIAN   ymean = mean, yvar = v + lik_param, logp = log N(ys; mean, v + lik_param) (Q unused)
 *   POISSON    ymean = exp(mean + v/2), yvar = ymean + expm1(v) ymean^2 (closed forms),
 *              logp = logsumexp_q[log w_q + ys f_q - e^{f_q} - lgamma(ys + 1)] - log(pi)/2
 *   BERNOULLI  ymean = p = pi^{-1/2} sum_q w_q sigma(f_q), yvar = p (1 - p),
 *              logp = logsumexp_q[log w_q + ys f_q - log(1 + e^{f_q})] - log(pi)/2
 * v = 0 gives log p(ys | mean) itself. ys NULL: no score. Every output may be NULL; outputs are
 * NaN-filled first and stay NaN at a point whose mean or variance is not finite. GAPLAC_E_KIND for
 * an unknown lik; GAPLAC_E_PARAM for a ys outside the likelihood's support or a Gaussian variance
 * < 0; GAPLAC_E_ARG for M < 0, mean or var NULL with M > 0, or Q outside [1, 64] (non-Gaussian). */
int gaplac_gauss_hermite(int32_t Q, double* nodes, double* weights);
int gaplac_laplace_predict(int32_t lik, double lik_param, int64_t M, const double* mean,
                           const double* var, const double* ys /* NULL: no score */, int32_t Q,
                           double* out_ymean, double* out_yvar, double* out_logp);

/* One draw of the FiniteGP: out = L z with C = K(X) + noise I = L L^T
 * and z the N standard-normal values the caller drew (the host keeps the RNG stream, so a
 * given z gives the same sample as the reference). Replaces: rand(rng, FiniteGP(GP(k), X,
 * noise)) = mean + cholesky(C).U' * randn(rng, N) (zero mean), reached from
 * CLI/src/sample.jl:25. */
int gaplac_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                int32_t T, const gaplac_term* terms, double noise, const double* z, double* out);

/* Matrix form of logpdf: R response vectors (the columns of Y, N x R column-major, leading
 * dimension ldy) scored against one FiniteGP with ONE factorisation: the responses ride along
 * as R extra rows of the factored matrix (as the posterior's test points do), so about a
 * thousand of them cost a few ms beyond a single gaplac_logpdf at N = 16384.
 *     out_logpdf[r] = -( N*log(2*pi) + logdet + ||U^-T Y[:,r]||^2 ) / 2,  out_quad[r] the last term
 * out_logdet (one value) and out_quad (R values) may be NULL. Same return convention as
 * gaplac_logpdf; on a PosDefException (info > 0) every output entry is NaN. GAPLAC_E_ARG also
 * for R < 0, Y NULL with R > 0 and N > 0, ldy < N, out_logpdf NULL. R = 0: returns 0 after the
 * argument and term checks and writes nothing; N = 0: -0.0 per column. All R rows must fit in
 * device memory beside the matrix (GAPLAC_E_OOM otherwise, as for the posterior's M; no chunking).
 * Replaces: AbstractGPs.logpdf(f::FiniteGP, Y::AbstractMatrix) (AbstractGPs 0.5.12: one
 *           mean_and_cov + cholesky, then diag_Xt_invA_X(C, Y)), one log-density per column. */
int gaplac_logpdf_multi(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                        int32_t T, const gaplac_term* terms, double noise,
                        int64_t R, const double* Y, int64_t ldy,
                        double* out_logpdf, double* out_logdet, double* out_quad);
/* Same, with X and Y already resident in device memory (HBM) on the ctx's device; Y is read
 * in place (not copied). Outputs are host pointers.
 * Replaces: the same logpdf(f::FiniteGP, Y::AbstractMatrix) for device-resident inputs. */
int gaplac_logpdf_multi_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx,
                               int32_t T, const gaplac_term* terms, double noise,
                               int64_t R, const double* dY, int64_t ldy,
                               double* out_logpdf, double* out_logdet, double* out_quad);

/* Matrix form of rand: R draws with one factorisation, out = L Z with Z the N x R matrix of
 * standard-normal values the caller drew (leading dimension ldz) and out N x R (leading
 * dimension ldo; rows N .. ldo-1 are never written). A column's sample does not depend on
 * R or on the column's position. Same return convention as gaplac_rand (out NaN on failure).
 * GAPLAC_E_ARG also for R < 0, Z NULL with R > 0 and N > 0, ldz < N, ldo < N, out NULL;
 * R = 0 or N = 0: returns 0 after the checks, out untouched.
 * Replaces: rand(rng, f::FiniteGP, n::Int) = cholesky(C).U' * randn(rng, N, n) (zero mean) of
 *           AbstractGPs 0.5.12; CLI/src/sample.jl:25's one draw is vec(rand(rng, f, 1)). */
int gaplac_rand_multi(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                      int32_t T, const gaplac_term* terms, double noise,
                      int64_t R, const double* Z, int64_t ldz, double* out, int64_t ldo);

/* Joint posterior at M test points: with C = K(X) + noise I = L L^T, V = L^{-1} K(X, xs) and
 * z = L^{-1} y,
 *     m = V^T z,   Sigma* = gram(Xs, terms, noise_s) - V^T V = L* L*^T
 * where gram(Xs, terms, noise_s) is the test points' own Gram matrix as gaplac_gram builds it
 * (noise_s on the diagonal; a NOISE term adds its variance on the diagonal only and is 0 across
 * the two point sets). m is the mean gaplac_posterior_mean_var returns. One factorisation of
 * order N (the posterior evaluation), one fp64-MFMA kernel for Sigma* and, for rand / logpdf, a
 * second factorisation of order M of the matrix that kernel left in device memory.
 * Common convention: every output is NaN-filled first; info > 0 when either Cholesky fails
 * (all outputs stay NaN; gaplac_last_error names the matrix: the training covariance, or the
 * test-point covariance with info = the 1-based leading minor of Sigma*). GAPLAC_E_ARG for
 * noise_s < 0 or non-finite, M < 0, R < 0, a leading dimension below M, a NULL matrix of
 * positive size, out / out_logpdf NULL. M = 0 or R = 0: 0 after the argument and term checks,
 * nothing written. N = 0: the posterior is the prior at the test points (mean 0, gaplac_gram,
 * gaplac_rand_multi, gaplac_logpdf_multi on (Xs, noise_s)). GAPLAC_E_OOM when the two
 * workspaces do not fit (no chunking). The context stays usable after every failure.
 *
 * mean_cov: m (M values) and the full symmetric Sigma* (M x M column-major, leading dimension
 * ldc; both triangles written, exact mirror images; rows M .. ldc-1 untouched). Either output
 * may be NULL. No second factorisation: an indefinite Sigma* is returned as it is.
 * Replaces: mean_and_cov(posterior(fx, y)(xs, noise_s)) of AbstractGPs 0.5.12. */
int gaplac_posterior_mean_cov(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                              int32_t T, const gaplac_term* terms, double noise, const double* y,
                              int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                              double* out_mean, double* out_cov, int64_t ldc);
/* rand: out = m 1^T + L* Z for the M x R standard-normal matrix Z the caller drew (leading
 * dimension ldz); out is M x R (ldo; rows M .. ldo-1 untouched). A column's sample depends
 * neither on R nor on the column's position.
 * Replaces: rand(rng, posterior(fx, y)(xs, noise_s), R). */
int gaplac_posterior_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                          int32_t T, const gaplac_term* terms, double noise, const double* y,
                          int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                          int64_t R, const double* Z, int64_t ldz, double* out, int64_t ldo);
/* logpdf: out_logpdf[r] = -(M log 2pi + logdet Sigma* + |L*^{-1} (Ys[:, r] - m)|^2) / 2 for the
 * M x R matrix Ys of held-out responses (ldys); out_logdet (one value) and out_quad (R values)
 * may be NULL. Replaces: logpdf(posterior(fx, y)(xs, noise_s), Ys). */
int gaplac_posterior_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                            int32_t T, const gaplac_term* terms, double noise, const double* y,
                            int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                            int64_t R, const double* Ys, int64_t ldys,
                            double* out_logpdf, double* out_logdet, double* out_quad);

/* Inducing-point (VFE, Titsias) approximation: Mz inducing inputs Z (Mz x D column-major, leading
 * dimension ldz, the same columns as X) stand in for the N training points, so nothing of order
 * N x N is formed. jitter >= 0 is the variance of f(z, jitter). Terms, groups and NOISE terms mean
 * what they mean for gaplac_posterior_mean_var with (Z, jitter) as the training set and the rows
 * of X, then Xs, as its test points (cross-covariances use the latent kernel; a NOISE term is 0
 * across point sets and counts in the kernel diagonal). With Kuu + jitter I = L L^T,
 * V^T = K(X, Z) L^{-T} (N x Mz), a_j = L^{-1} K(Z, xs_j), S = noise I + (V^T)^T V^T = L_S L_S^T,
 * w = (V^T)^T y and u = L_S^{-1} w:
 *     trace  = sum_n ( k(x_n, x_n) - |V^T[n, :]|^2 )
 *     logdet = (N - Mz) log noise + 2 sum_i log (L_S)_ii
 *     quad   = ( y^T y - |u|^2 ) / noise
 *     dtc    = -( N log 2pi + logdet + quad ) / 2      = log N(y | 0, Q + noise I),
 *                                                         Q = K(X, Z) (Kuu + jitter I)^{-1} K(Z, X)
 *     elbo   = dtc - trace / (2 noise)
 *     mean_j = (L_S^{-1} a_j) . u
 *     var_j  = k(xs_j, xs_j) - |a_j|^2 + noise |L_S^{-1} a_j|^2
 * One factorisation of order Mz with the N (+ Ms) points riding as extra rows, one fp64-MFMA
 * product for S split over N into chunks summed in a fixed order (the split depends on (N, Mz)
 * alone: a call is bitwise repeatable), and a second factorisation of order Mz.
 * Common convention: every output is NaN-filled first; info > 0 when either Cholesky fails (all
 * outputs stay NaN; gaplac_last_error names the matrix: the inducing covariance, or S).
 * GAPLAC_E_PARAM for noise <= 0 or non-finite, jitter < 0 or non-finite; GAPLAC_E_ARG for
 * Mz < 0, Ms < 0, a leading dimension below its row count, a NULL matrix of positive size,
 * out_elbo NULL; GAPLAC_E_OOM when the workspaces do not fit or ceil((N + Ms)/128) > 65535 (no
 * chunking). N = 0: elbo = dtc = 0 (trace, logdet, quad 0) and the posterior is the prior (mean 0,
 * variance k(xs_j, xs_j)). Mz = 0: Q = 0 (dtc = log N(y | 0, noise I), trace = sum_n k(x_n, x_n),
 * the posterior is the prior). Ms = 0: 0 after the argument and term checks, nothing written.
 * The context stays usable after every failure.
 *
 * elbo: every output except out_elbo may be NULL.
 * Replaces: elbo(VFE(f(z, jitter)), f(x, noise), y) and dtc(...) of AbstractGPs 0.5.12 (out_dtc). */
int gaplac_sparse_elbo(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                       int32_t T, const gaplac_term* terms, double noise, const double* y,
                       int64_t Mz, const double* Z, int64_t ldz, double jitter,
                       double* out_elbo, double* out_dtc, double* out_trace, double* out_logdet,
                       double* out_quad);
/* The approximate posterior at Ms test points Xs (Ms x D column-major, leading dimension ldxs);
 * out_mean / out_var have Ms entries; either may be NULL.
 * Replaces: mean_and_var(posterior(VFE(f(z, jitter)), f(x, noise), y), xs) of AbstractGPs 0.5.12. */
int gaplac_sparse_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                                     int32_t T, const gaplac_term* terms, double noise, const double* y,
                                     int64_t Mz, const double* Z, int64_t ldz, double jitter,
                                     int64_t Ms, const double* Xs, int64_t ldxs,
                                     double* out_mean, double* out_var);
/* The bound and its gradient with respect to y, the term parameters, the observation variance
 * and jitter (the inducing inputs Z stay fixed: a CAT column has no derivative). With c = S^{-1} w
 * = L_S^{-T} u, alpha = (y - V^T c) / noise, ctil = L^{-T} c, Phi = I / noise - S^{-1},
 * W' = L^{-T} Phi, G_uf = ctil alpha^T + W' V (Mz x N, never stored) and
 * G_uu = -( ctil ctil^T + L^{-T} (S / noise - 2 I + noise S^{-1}) L^{-1} ) / 2:
 *     out_dy[n]     = -alpha_n
 *     out_dparam[t] = -sum_n dk(x_n, x_n)/dtheta_t / (2 noise) + sum G_uf o dK(Z, X)/dtheta_t
 *                     + sum G_uu o dK(Z)/dtheta_t
 *     out_dnoise    = ( alpha^T alpha - (N - Mz + noise tr S^{-1}) / noise ) / 2 + trace / (2 noise^2)
 *     out_djitter   = tr G_uu
 * dk/dtheta_t is gaplac_logpdf_grad's (l of SQEXP / OU, c of LINEAR, the variance of a NOISE term;
 * 0 for CAT; times the other terms of t's product group); a NOISE term is 0 across point sets.
 * out_elbo is bitwise gaplac_sparse_elbo's for the same arguments (the value runs by the same
 * schedule first). The N-long work is one GEMV for alpha and one fp64-MFMA product with the
 * contraction in its epilogue, reduced in a fixed order: a call is bitwise repeatable. out_dy has
 * N entries, out_dparam T; every output except out_elbo may be NULL. Conventions, errors and the
 * closed forms for N = 0 (everything 0) and Mz = 0 (dy = -y / noise, djitter = 0) as above.
 * Replaces: the gradient of elbo(VFE(f(z, jitter)), f(x, noise), y) (no analytic form in the
 * reference: AbstractGPs differentiates it by AD). */
int gaplac_sparse_elbo_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                            int32_t T, const gaplac_term* terms, double noise, const double* y,
                            int64_t Mz, const double* Z, int64_t ldz, double jitter,
                            double* out_elbo, double* out_dy, double* out_dparam, double* out_dnoise,
                            double* out_djitter);
/* gaplac_sparse_elbo_grad, and the gradient with respect to the inducing inputs. For inducing
 * point m and column d of Z, with G_uf and G_uu as above:
 *     out_dZ[d lddz + m] = sum over the terms t with col_t = d of
 *           sum_n  G_uf[m, n]  d1 k_t(z_m, x_n)  prod_{s != t in t's group} k_s(z_m, x_n)
 *       + 2 sum_m' G_uu[m, m'] d1 k_t(z_m, z_m') prod_{s != t in t's group} k_s(z_m, z_m')
 * d1 k(a, b) is the derivative in the first argument's coordinate: -k (a - b) / l^2 for SQEXP,
 * -k sign(a - b) / l for OU, b for LINEAR, 0 for CAT and NOISE. For OU sign(0) = 0: at coinciding
 * coordinates the kernel has a kink and the entry returns the symmetric subgradient. The m' = m
 * term is kept (2 G_uu[m, m] z_m for LINEAR); a NOISE factor inside a product group is the delta
 * of m and m' in K(Z) and 0 across point sets, as in the value. out_dZ is Mz x D column-major with
 * leading dimension lddz >= Mz; rows Mz .. lddz - 1 are never written; a column that no SQEXP / OU /
 * LINEAR term reads is exactly +0.0. With out_dZ == NULL the call is gaplac_sparse_elbo_grad
 * (nothing more is launched or allocated). Every other output is bitwise gaplac_sparse_elbo_grad's
 * for the same arguments, whether or not out_dZ is NULL. The sums over the rows n run in the
 * product kernel's epilogue, per 128 rows, and those partials and the column tiles of G_uu are
 * added in ascending order, the terms that share a column in term order: a call is bitwise
 * repeatable. Conventions and errors as gaplac_sparse_elbo_grad; GAPLAC_E_ARG also for lddz < Mz
 * with a non-NULL out_dZ (out_dZ is then left as it was; the other outputs are NaN). N = 0: dZ is
 * all 0; Mz = 0: nothing is written; after a PosDefException every entry is NaN.
 * Replaces: the gradient of the same bound with respect to z (AD in the reference's stack). */
int gaplac_sparse_elbo_grad_z(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                              int32_t T, const gaplac_term* terms, double noise, const double* y,
                              int64_t Mz, const double* Z, int64_t ldz, double jitter,
                              double* out_elbo, double* out_dy, double* out_dparam, double* out_dnoise,
                              double* out_djitter, double* out_dZ, int64_t lddz);
/* The joint forms of the approximate posterior at the Ms test points, observed with variance
 * noise_s >= 0. With L, a_j, S, L_S, u as above and b_j = L_S^{-1} a_j:
 *     m_j    = b_j . u                       (the mean gaplac_sparse_posterior_mean_var returns)
 *     Sigma* = gram(Xs, terms, noise_s) - A^T A + noise B^T B = L* L*^T,
 *                                            A = [a_j], B = [b_j]  (Mz x Ms)
 * where gram(Xs, terms, noise_s) is the test points' own Gram matrix as gaplac_gram builds it
 * (noise_s on the diagonal; a NOISE term counts on its diagonal and is 0 across point sets). The
 * three stages of gaplac_sparse_posterior_mean_var (the mean by the same launches), one fp64-MFMA
 * kernel for Sigma* (per element one accumulator chain: the b products in ascending k from zero,
 * folded into the Gram entry as gram - noise * acc, then the a products in ascending k; nothing
 * split, so a call is bitwise repeatable and an entry does not depend on Ms or on where its
 * points stand) into a third workspace and, for rand / logpdf, a third factorisation, of order
 * Ms, of the matrix that kernel left in device memory.
 * Conventions are those of the joint entries and of the sparse entries combined: every output is
 * NaN-filled first; info > 0 when any of the three Choleskys fails (all outputs stay NaN;
 * gaplac_last_error names the matrix: the inducing covariance, S, or the test-point covariance
 * with info = the 1-based leading minor of Sigma*). GAPLAC_E_PARAM for noise <= 0 or jitter < 0
 * (or non-finite); GAPLAC_E_ARG for noise_s < 0 or non-finite, negative sizes, a leading dimension
 * below its row count, a NULL matrix of positive size, out / out_logpdf NULL; GAPLAC_E_OOM when
 * ceil((N + Ms)/128) > 65535, ceil(R/128) > 65535 or the three workspaces do not fit (no
 * chunking). Ms = 0 or R = 0: 0 after the argument and term checks, nothing written. N = 0 or
 * Mz = 0: the prior at the test points (mean 0, gaplac_gram, gaplac_rand_multi,
 * gaplac_logpdf_multi on (Xs, noise_s)). The context stays usable after every failure.
 *
 * mean_cov: m (Ms values) and the full symmetric Sigma* (Ms x Ms column-major, leading dimension
 * ldc; both triangles written, exact mirror images; rows Ms .. ldc-1 untouched). Either output
 * may be NULL. No third factorisation: an indefinite Sigma* is returned as it is.
 * Replaces: mean_and_cov(posterior(VFE(f(z, jitter)), f(x, noise), y)(xs, noise_s)) of
 * AbstractGPs 0.5.12. */
int gaplac_sparse_posterior_mean_cov(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                                     int32_t T, const gaplac_term* terms, double noise, const double* y,
                                     int64_t Mz, const double* Z, int64_t ldz, double jitter,
                                     int64_t Ms, const double* Xs, int64_t ldxs, double noise_s,
                                     double* out_mean, double* out_cov, int64_t ldc);
/* rand: out = m 1^T + L* E for the Ms x R standard-normal matrix E the caller drew (leading
 * dimension lde); out is Ms x R (ldo; rows Ms .. ldo-1 untouched). A column's sample depends
 * neither on R nor on the column's position.
 * Replaces: rand(rng, posterior(VFE(f(z, jitter)), f(x, noise), y)(xs, noise_s), R). */
int gaplac_sparse_posterior_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                                 int32_t T, const gaplac_term* terms, double noise, const double* y,
                                 int64_t Mz, const double* Z, int64_t ldz, double jitter,
                                 int64_t Ms, const double* Xs, int64_t ldxs, double noise_s,
                                 int64_t R, const double* E, int64_t lde, double* out, int64_t ldo);
/* logpdf: out_logpdf[r] = -(Ms log 2pi + logdet Sigma* + |L*^{-1} (Ys[:, r] - m)|^2) / 2 for the
 * Ms x R matrix Ys of held-out responses (ldys); out_logdet (one value) and out_quad (R values)
 * may be NULL.
 * Replaces: logpdf(posterior(VFE(f(z, jitter)), f(x, noise), y)(xs, noise_s), Ys). */
int gaplac_sparse_posterior_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                                   int32_t T, const gaplac_term* terms, double noise, const double* y,
                                   int64_t Mz, const double* Z, int64_t ldz, double jitter,
                                   int64_t Ms, const double* Xs, int64_t ldxs, double noise_s,
                                   int64_t R, const double* Ys, int64_t ldys,
                                   double* out_logpdf, double* out_logdet, double* out_quad);
/* Host-only: the split of the product for S over the N rows, *out_chunks chunks of
 * *out_chunk_rows rows (the last one ragged), summed in ascending order. A function of (N, Mz)
 * alone. GAPLAC_E_ARG for N < 0, Mz < 0 or a NULL output. Not in the reference. */
int gaplac_sparse_split(int64_t N, int64_t Mz, int64_t* out_chunks, int64_t* out_chunk_rows);

/* Debug / parity entries (tests only; not on the timed path). */
/* Gram matrix sum_t K_t(X) + noise*I as a dense N×N column-major host matrix
 * (replaces KernelFunctions.kernelmatrix + Diagonal(Fill(noise, N))). */
int gaplac_gram(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                int32_t T, const gaplac_term* terms, double noise, double* out_C, int64_t ldc);
/* Measurement (bench.py extra.gram): the same Gram built from host inputs into the
 * context's workspace by one plain-grid launch, reps times, each bracketed by hipEvents on
 * the launching stream; best_ms = the fastest launch, bytes = its algorithmic HBM bytes
 * (8 Np(Np+1)/2 written + 8 N (D+1) read, Np = N+1 rounded up to 128). */
int gaplac_gram_time(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                     int32_t T, const gaplac_term* terms, double noise, const double* v,
                     int32_t reps, double* best_ms, double* bytes);
/* Lower Cholesky factor L = U^T of the same C (dense N×N column-major, upper part
 * zeroed) and z = L^{-1} v (replaces cholesky(Symmetric(C)).U' and U' \ v). */
int gaplac_factor(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx,
                  int32_t T, const gaplac_term* terms, double noise, const double* v,
                  double* out_L, int64_t ldl, double* out_z);

/* Per-kernel timing of the evaluations run while profiling is on (off by default),
 * accumulated until gaplac_reset_stats. gaplac_set_profiling mode:
 *   0 off;
 *   1 per-launch device timestamps of every kernel (first workgroup start, last wave
 *     end; 100 MHz s_memrealtime);
 *   2 hipEvents recorded on the launching stream around every bulk trailing-update
 *     (tile_syrk_kernel) launch and every -C^{-1} tile launch of a gradient evaluation,
 *     the production schedule otherwise unchanged: fills syrk_* and cinv_* only, read
 *     back at gaplac_get_stats. */
typedef struct gaplac_stats {
    int64_t evals;
    int64_t syrk_launches;      /* bulk trailing-update launches (tile_gemm_kernel<0>) */
    double  syrk_ms;            /* summed event time of those launches */
    double  syrk_flops;         /* algorithmic flops of those launches */
    double  gram_ms;
    double  gram_bytes;         /* algorithmic bytes of the Gram launches */
    int64_t gram_launches;
    double  panel_ms;           /* diagonal-block potrf launches, summed */
    double  trsm_ms;            /* panel TRSM launches, summed */
    double  colupd_ms;          /* lookahead column-update launches, summed */
    double  total_ms;           /* whole evaluation, first kernel to result */
    double  syrk_bytes;         /* algorithmic HBM bytes of the bulk launches: C tiles read +
                                   written once, panel rows read once */
    int64_t small_launches;     /* small trailing updates (quad_bulk_kernel), not in syrk_* */
    double  small_ms;
    /* gradient evaluations (gaplac_logpdf_grad), profiling mode 1 */
    double  grad_rows_ms;       /* identity-row substitution + updates (L^{-T} rows) */
    int64_t cinv_launches;      /* -C^{-1} = -L^{-T} L^{-1} tile launches (cinv_tile_kernel) */
    double  cinv_ms;
    double  contract_ms;        /* dC/dtheta contraction (grad_contract_kernel) */
    /* persistent tail (tail_kernel: the last tile columns as one dataflow launch) */
    int64_t tail_launches;
    double  tail_ms;
    /* profiling mode 2: every bulk-type launch of the super-panel phase (triangle updates,
       bands, split heads, whole-tile lookaheads; they overlap since round 6): summed
       algorithmic flops, launches, and the union of their event intervals */
    double  bulk_flops;
    int64_t bulk_launches;
    double  bulk_union_ms;
} gaplac_stats;
int gaplac_set_profiling(gaplac_ctx* ctx, int mode);
int gaplac_get_stats(gaplac_ctx* ctx, gaplac_stats* out);
int gaplac_reset_stats(gaplac_ctx* ctx);

/* Launch-footprint check of one evaluation's schedule, on the host only (no device, no
 * context): walks every launch gaplac_logpdf (mode 0), gaplac_logpdf_grad (mode 1) or
 * gaplac_posterior_mean_var at M test points (mode 2; also gaplac_posterior_components, whose
 * G components at M' points are M = G*M' rows behind the same launchers) or gaplac_logpdf_multi
 * of M responses (mode 3) would enqueue for order N with
 * super-panel width spw, and checks the element range each launch's grid touches against
 * the workspace the context allocates for N. Every launcher applies the same check before
 * a real launch (a violating launch is not enqueued; the entry returns GAPLAC_E_ARG).
 * Returns 0 (the counts are valid) or GAPLAC_E_ARG for bad arguments; *out_violations is
 * the number of launches outside the workspace and msg (msglen bytes) the first one.
 * mode + 8: the same walk against a workspace one element short (the guard's negative
 * control: the last Gram tile must be reported).
 * Not in the reference (an internal guard). */
int gaplac_plan_check(int64_t N, int32_t mode, int64_t M, int32_t spw, int64_t* out_launches,
                      int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for the joint posterior entries: the posterior evaluation of order N with M
 * test points, the covariance launches against both workspaces, and the second factorisation
 * of order M (R > 0: with R riding rows, as gaplac_posterior_logpdf; R = 0: plain, as
 * gaplac_posterior_rand). short_ws 1 / 2: the order-N / order-M workspace one element short
 * (the negative controls); 0: as allocated. Not in the reference. */
int gaplac_plan_check_joint(int64_t N, int64_t M, int64_t R, int32_t spw, int32_t short_ws,
                            int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for the sparse entries: the posterior evaluation of order Mz with N + Ms riding
 * rows, the launches that form S (and, with Ms > 0, the transposing copy of the test points'
 * rows) against both workspaces, and the second factorisation of order Mz (Ms > 0: with Ms riding
 * rows and their reduction, as gaplac_sparse_posterior_mean_var; Ms = 0: plain, as
 * gaplac_sparse_elbo). short_ws 1 / 2: the first / second workspace one element short (the
 * negative controls); 0: as allocated. Not in the reference. */
int gaplac_plan_check_sparse(int64_t N, int64_t Mz, int64_t Ms, int32_t spw, int32_t short_ws,
                             int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for a fitted posterior with room for cap test rows: the create-time launches
 * after the evaluation (the tile copy out of the workspace, z, the back-substitution), one
 * mean-and-variance query of M points in chunks of cap, and one matrix-free mean query of M
 * points, all against the fit's buffer. short_ws 1: the buffer one element short (the negative
 * control: the back-substitution's first launch leaves it); 0: as allocated. Not in the
 * reference. */
int gaplac_plan_check_fit(int64_t N, int64_t cap, int64_t M, int32_t spw, int32_t short_ws,
                          int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for the Laplace entries: one Newton step (the likelihood, the matrix-free
 * products, the Gram, the B build, the factorisation of the prebuilt matrix, z, the
 * back-substitution, the step and one trial point), the final factorisation, and with M > 0 one
 * posterior query of M points in its chunks (the response matrix, the factorisation with its
 * riding rows, the matrix-free mean), all against the workspace and the vectors' buffer.
 * short_ws 1: both one element short (the negative control); 0: as allocated. Not in the
 * reference. */
int gaplac_plan_check_laplace(int64_t N, int64_t M, int32_t spw, int32_t short_ws,
                              int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for gaplac_laplace_logpdf_grad: one Newton step as above, the final factorisation
 * of B with identity rows, and the gradient's launches (the row scaling with diag B^{-1}, s2, the
 * matrix-free product, the two products by Y, gaplac_logpdf_grad's ending with alpha = a, the
 * bilinear form), against the workspace and the vectors' buffer. short_ws 1: the workspace one
 * element short; 2: the vectors' buffer (the negative controls); 0: as allocated. Not in the
 * reference. */
int gaplac_plan_check_laplace_grad(int64_t N, int32_t spw, int32_t short_ws, int64_t* out_launches,
                                   int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for a Laplace fit (the iteration and its final factorisation are
 * gaplac_plan_check_laplace's): the create-time launches after the final factorisation, one
 * mean-and-variance query of M points in chunks of cap with the scaled build of the rows, one
 * matrix-free mean and one gaplac_fit_mean_cov of min(M, cap) points. short_ws 1: the fit's buffer
 * one element short; 2: the covariance workspace. GAPLAC_E_ARG for N < 1, cap < 1, M < 0, spw
 * outside [1, 8], short_ws outside [0, 2]. */
int gaplac_plan_check_laplace_fit(int64_t N, int64_t cap, int64_t M, int32_t spw, int32_t short_ws,
                                  int64_t* out_launches, int64_t* out_violations, char* msg,
                                  int64_t msglen);
/* The same check for gaplac_sparse_elbo_grad: gaplac_plan_check_sparse at Ms = 0, then the
 * gradient's launches: the order-Mz ones against its scratch, alpha and the product kernel against
 * the first workspace and the scratch. short_ws 1: the first workspace one element short; 2: the
 * second workspace and the gradient's scratch one element short (the negative controls); 0: as
 * allocated. Not in the reference. */
int gaplac_plan_check_sparse_grad(int64_t N, int64_t Mz, int32_t spw, int32_t short_ws,
                                  int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for gaplac_sparse_elbo_grad_z with T terms and a non-NULL out_dZ: the walk of
 * gaplac_plan_check_sparse_grad with the product kernel's dZ variant in the product's place,
 * followed by the dZ launches (the sum over the row tiles, the order-Mz part, the finishing
 * step), against the first workspace, the scratch and the buffer of dZ's partials. short_ws 1 / 2
 * as there; 3: the buffer of the partials one element short (the finishing step's store leaves
 * it); 0: as allocated. Not in the reference. */
int gaplac_plan_check_sparse_grad_z(int64_t N, int64_t Mz, int32_t T, int32_t spw, int32_t short_ws,
                                    int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* The same check for the sparse joint entries: gaplac_plan_check_sparse with Ms >= 1 test points,
 * then the tile-aligned copy of the test points' rows against the first workspace, the covariance
 * launches (with the mirroring pass) against the second and third, and the third factorisation, of
 * order Ms (R > 0: with R riding rows, as gaplac_sparse_posterior_logpdf; R = 0: plain, as
 * gaplac_sparse_posterior_rand). short_ws 1 / 2 / 3: the first / second / third workspace one
 * element short (the negative controls); 0: as allocated. Not in the reference. */
int gaplac_plan_check_sparse_joint(int64_t N, int64_t Mz, int64_t Ms, int64_t R, int32_t spw, int32_t short_ws,
                                   int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen);
/* Host-only accounting of the single-GPU schedule for order N (GAPLAC_SPW = spw,
 * GAPLAC_PAIR_DEPTH = depth (0: auto), band extension pair_ext (0/1), GAPLAC_PAIR_M =
 * pair_m): every tile column gets every earlier panel column exactly once, in order, before
 * its factorisation, and every update reads factored panel columns. 0, or GAPLAC_E_ARG with
 * the first violation in msg; *out_records: launches and factorisations recorded. Not in the
 * reference (an internal guard). */
int gaplac_plan_check_schedule(int64_t N, int32_t spw, int32_t depth, int32_t pair_ext, int32_t pair_m,
                               int64_t* out_records, char* msg, int64_t msglen);

/* ------------------------------------------------------------------------------------
 * Distributed evaluation (BASELINE configs[3]: N = 65536 over the GPUs of one node; one
 * process per GPU). 1-D block-column cyclic Cholesky: super-panels of spw 128-wide
 * tile columns are dealt round-robin over the ranks; each rank builds and stores only its
 * own columns of the lower triangle (the Gram shards with no redistribution) and the only
 * data-path exchange is one broadcast per super-panel of the factored panel, which the
 * HOST enqueues with its collective library (ncclBroadcast = RCCL over xGMI) on the
 * stream gaplac_dist_comm_begin returns. Same result as gaplac_logpdf (<= 1e-9 rel).
 * Replaces, like gaplac_logpdf: AbstractGPs.logpdf(FiniteGP, v) — the GaPLAC-owned method
 * would dispatch here when the job runs on several GPUs.
 *
 * Per rank, per evaluation (every call only enqueues, except finish):
 *   gaplac_dist_begin(...)                         -> nsteps (nsp without the tail gather)
 *   if (owner(0) == rank) gaplac_dist_factor(d, 0)         (owner: gaplac_dist_owner)
 *   bcast(0)
 *   for s in 0..nsteps-1:
 *       if (s+1 < nsteps && owner(s+1) == rank) gaplac_dist_factor(d, s+1)
 *       gaplac_dist_update(d, s)
 *       if (s+1 < nsteps) bcast(s+1)
 *   [the tail gather, when set: see gaplac_dist_set_tail]
 *   gaplac_dist_finish(d, &logdet_part, &quad_part, &info_part)
 *   allreduce: logdet = sum, quad = sum, info = min over nonzero; then
 *   logpdf = -(N*log(2*pi) + logdet + quad) / 2   (NaN / PosDefException if info > 0)
 * where bcast(s) = gaplac_dist_chunks(d, s, &nc);
 *                  for c in 0..nc-1:
 *                      gaplac_dist_panel_chunk(d, s, c, &buf, &count, &root);
 *                      gaplac_dist_comm_begin_chunk(d, s, c, &stream);
 *                      ncclBroadcast(buf, buf, count, ncclDouble, root, comm, stream);
 *                      gaplac_dist_comm_end_chunk(d, s, c);
 * A chunk is a run of the panel's tile columns (gaplac_dist_configure): its owner packs it
 * as soon as its last column is final and the next owner's lookahead consumes it as it
 * arrives, so broadcasts overlap both chains. The whole panel as one
 * broadcast (gaplac_dist_panel / _comm_begin / _comm_end) is the one-chunk case.
 * ---------------------------------------------------------------------------------- */
typedef struct gaplac_dist gaplac_dist;
int gaplac_dist_create(int device, int nranks, int rank, int spw, gaplac_dist** out);
int gaplac_dist_destroy(gaplac_dist* d);
const char* gaplac_dist_last_error(const gaplac_dist* d);
/* Padded order Np = roundup(N+1, 128), tile columns nt, super-panels nsp, this rank's
 * local tile columns nloc, and the doubles one panel buffer must hold. */
int gaplac_dist_geometry(gaplac_dist* d, int64_t N, int64_t* Np, int32_t* nt, int32_t* nsp,
                         int32_t* nloc, int64_t* panel_elems);
/* Optional: two caller-owned device panel buffers (e.g. allocated by the collective
 * library's host binding), each of >= panel_elems doubles; NULLs = library-owned. */
int gaplac_dist_set_panel_buffers(gaplac_dist* d, void* buf0, void* buf1, int64_t capacity);
/* Inputs as for gaplac_logpdf (inputs_on_device: X and v are device pointers). Builds
 * this rank's Gram tiles; returns the number of super-panels in *out_nsp. */
int gaplac_dist_begin(gaplac_dist* d, int64_t N, int32_t D, const double* X, int64_t ldx,
                      int32_t T, const gaplac_term* terms, double noise, const double* v,
                      int inputs_on_device, int32_t* out_nsp);
/* Schedule options, before gaplac_dist_set_panel_buffers / begin (< 0 keeps the current
 * value; defaults from GAPLAC_DIST_DEPTH / _CHUNK / _BIG / _BIG_MIN / _ALONE): depth =
 * super-panels per deferred bulk update (1..8), chunk = tile columns per broadcast chunk
 * (1..spw), big = bulk kernel choice (0: never the large-launch kernel; 1: per rank,
 * launches of >= big_min tiles while this rank runs no chain; 2: by launch size, as on one
 * GPU — for ranks that share one device), alone = 1: a rank's bulk update waits while it
 * factors the next super-panel (the chain gets the whole GPU). Defaults with several ranks
 * (the one-GPU replay's best at N = 65536 over 8): depth 2, chunk 2, big 1,
 * alone 1; with one rank: chunk = spw, big 2, alone 0. */
int gaplac_dist_configure(gaplac_dist* d, int32_t depth, int32_t chunk, int32_t big, int32_t big_min,
                          int32_t alone);
/* Super-panel layout, before begin: snake = 1 deals the super-panels boustrophedon (rank r
 * owns super-panel u*nranks + r in even rounds u, u*nranks + nranks-1-r in odd ones), which
 * evens out the ranks' trailing-update work; 0 = round-robin. Default: 1
 * with several ranks. owner: the rank that owns super-panel s (factors it and roots its
 * broadcast). */
int gaplac_dist_set_layout(gaplac_dist* d, int32_t snake);
int gaplac_dist_owner(gaplac_dist* d, int32_t s, int32_t* out_rank);
int gaplac_dist_factor(gaplac_dist* d, int32_t s);   /* owner of super-panel s only */
int gaplac_dist_chunks(gaplac_dist* d, int32_t s, int32_t* out_chunks);
int gaplac_dist_panel_chunk(gaplac_dist* d, int32_t s, int32_t c, void** buf, int64_t* count,
                            int32_t* root);
int gaplac_dist_comm_begin_chunk(gaplac_dist* d, int32_t s, int32_t c, void** hip_stream);
int gaplac_dist_comm_end_chunk(gaplac_dist* d, int32_t s, int32_t c);
int gaplac_dist_panel(gaplac_dist* d, int32_t s, void** buf, int64_t* count, int32_t* root);
int gaplac_dist_comm_begin(gaplac_dist* d, int32_t s, void** hip_stream);
int gaplac_dist_comm_end(gaplac_dist* d, int32_t s);
int gaplac_dist_update(gaplac_dist* d, int32_t s);
/* This rank's partial logdet / quad and first failing pivot (0 = none); synchronises. */
int gaplac_dist_finish(gaplac_dist* d, double* logdet_part, double* quad_part, int64_t* info_part);
/* Debug / parity: this rank's column storage (Np x nloc*128, column-major) to host. */
int gaplac_dist_local(gaplac_dist* d, double* out, int64_t ld);
/* Host-only (no HIP calls): checks the step plan for nt tile columns — every super-panel
 * gets every earlier panel once, in order, before its chain. 0 or GAPLAC_E_ARG (msg). */
int gaplac_dist_plan_check(int32_t nt, int32_t spw, int32_t depth, int32_t pair_m, int64_t* out_ops,
                           char* msg, int64_t msglen);
/* Host-only: the plan's ops as (step, kind, sp, first panel, last panel) int32 quintuples
 * (kind 0: that super-panel, 1: every super-panel from it on, 2: the step's event after
 * super-panel step+2 is up to date); *out_n = op count, out may be NULL. */
int gaplac_dist_plan(int32_t nt, int32_t spw, int32_t depth, int32_t pair_m, int32_t* out, int64_t cap,
                     int64_t* out_n);
/* Tail gather (off by default). tail_cols > 0: the super-panels whose columns all lie in
 * the last tail_cols (<= 128) tile columns are not factored by the distributed steps. After
 * the last step's update every rank sends its columns of that trailing matrix (from each
 * super-panel's first row down) to rank `root`, which factors it with the single-GPU
 * persistent tail; begin then returns the number of distributed steps (fewer than nsp).
 * Per rank, after the step loop:
 *   gaplac_dist_tail_begin(d, &stream);      packs this rank's segments on stream
 *   for i in 0..nseg-1: gaplac_dist_tail_segment(d, i, &buf, &count, &src);
 *       src == rank != root: ncclSend(buf, count, ncclDouble, root, comm, stream)
 *       rank == root != src: ncclRecv(buf, count, ncclDouble, src, comm, stream)
 *   (all inside one ncclGroupStart / ncclGroupEnd)
 *   gaplac_dist_tail_end(d);                  the root factors the gathered matrix
 * then finish as before (the root's partial sums include the tail's). The reference's
 * logpdf is the same single evaluation (CLI/src/mcmc.jl:35); nothing in it is split. 0 = off
 * (the default with one rank). Not in the reference. */
int gaplac_dist_set_tail(gaplac_dist* d, int32_t tail_cols, int32_t root);
/* For order N, before begin: segments of the gather (0: none), the doubles this rank's
 * segment buffer needs, and the steps begin will return. */
int gaplac_dist_tail_geometry(gaplac_dist* d, int64_t N, int32_t* nseg, int64_t* buf_elems,
                              int32_t* nsteps);
/* Optional caller-owned device segment buffer of >= buf_elems doubles (NULL: library-owned). */
int gaplac_dist_set_tail_buffer(gaplac_dist* d, void* buf, int64_t capacity);
int gaplac_dist_tail_segment(gaplac_dist* d, int32_t i, void** buf, int64_t* count, int32_t* src);
int gaplac_dist_tail_begin(gaplac_dist* d, void** hip_stream);
int gaplac_dist_tail_end(gaplac_dist* d);
/* Host-only: the plan and its check with the tail gather of tail_cols tile columns. */
int gaplac_dist_plan_check_tail(int32_t nt, int32_t spw, int32_t depth, int32_t pair_m, int32_t tail_cols,
                                int64_t* out_ops, char* msg, int64_t msglen);
int gaplac_dist_plan_tail(int32_t nt, int32_t spw, int32_t depth, int32_t pair_m, int32_t tail_cols,
                          int32_t* out, int64_t cap, int64_t* out_n);
/* Replay of one rank's schedule on one GPU (diagnostics): the other ranks'
 * panels arrive as copies from their (already factored) contexts on a modelled timeline.
 * replay_enable(N) before begin turns device timestamps on (0: off); replay_chunk replaces bcast's
 * broadcast of one chunk (times in 10 ns ticks); replay_stamps copies the timestamps out;
 * replay_info: a chunk's bytes and the stamp layout. Not in the reference. */
int gaplac_dist_replay_enable(gaplac_dist* d, int64_t N);
int gaplac_dist_replay_chunk(gaplac_dist* d, const gaplac_dist* owner, int32_t s, int32_t c,
                             int64_t f_ticks, int64_t band_ticks, int64_t lat_ticks,
                             int64_t xfer_ticks, int64_t copy_ticks);
int gaplac_dist_replay_stamps(gaplac_dist* d, uint64_t* out, int64_t n);
/* The tail gather on the replayed rank (in place of tail_begin / the transfers / tail_end):
 * the root's segments from the owners' contexts of a loopback run with the same gather,
 * released at max(END(last step), Gram end + senders_end) + lat + the largest sender's
 * bytes x ticks_per_byte (senders_end: the latest sender's last update end in its own
 * replay, relative to its Gram end; 0 = this rank's own END). */
int gaplac_dist_replay_tail(gaplac_dist* d, const gaplac_dist* const* owners, int32_t nowners,
                            int64_t lat_ticks, double ticks_per_byte, int64_t copy_ticks,
                            int64_t senders_end);
int gaplac_dist_replay_info(gaplac_dist* d, int32_t s, int32_t c, int64_t* bytes, int32_t* per_step,
                            int32_t* maxc);

#ifdef __cplusplus
}
#endif
#endif /* GAPLAC_H */
