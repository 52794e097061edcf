// Host side of libgaplac_hip.so: the C-ABI declared in include/gaplac.h.
//
// One evaluation = Gram build + blocked right-looking Cholesky of the (N+1)-augmented
// matrix with one-panel lookahead + logdet/quad reduction:
//
//   s_main : gram | wait(P0) syrk_tri(2..) rec(R0) | wait(P1) syrk_tri(3..) rec(R1) | ...
//   s_panel:        potrf(0) trsm(0) rec(P0) | syrk_col(1) potrf(1) trsm(1) rec(P1) |
//                   wait(R0) syrk_col(2) potrf(2) trsm(2) rec(P2) | ...
// (details at factor_and_reduce)
#include "gaplac_internal.h"

#include <cstddef>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace gaplac;

namespace gaplac {
// What one evaluation carries besides its matrix: the rows that ride below it, factored along
// (lda = Np + 128 tiles), and the two flags that describe the same evaluation. A value: an entry
// builds one with a named constructor and passes it to eval_device, whose EvalScope installs it
// in the context for that call and puts "none" back on every way out. Nothing else writes it.
//   mode 1 = identity rows E = [I 0] -> L^{-T} (gradient, gaplac_logpdf_grad)
//   mode 2 = K(xs, X) -> (L^{-1} K(X, xs))^T (posterior, gaplac_posterior_mean_var, §10)
//   mode 3 = Y^T -> (L^{-1} Y)^T (the responses of gaplac_logpdf_multi, §10.5)
// Modes 2 and 3 are dense rows (dense_rows): one schedule for both.
struct ExtraRows {
    int mode = 0;   // 0: none
    int tiles = 0;  // tile rows
    int64_t M = 0;  // mode 2: test points; mode 3: responses R
    // mode 2, gaplac_posterior_components (§10.7): the M = G * Mc rows are packed components,
    // built and finished per row by the selector; everything between sees M ordinary rows
    bool comp = false;
    CompSel sel{};
    // mode 3: the responses on the device, ld ldy, and N values subtracted from every response
    // (or nullptr)
    const double* Y = nullptr;
    int64_t ldy = 0;
    const double* sub = nullptr;
    bool prebuilt = false;    // the matrix is already in the workspace: no Gram launch (§10.6)
    bool singletons = true;   // mode 1: single-term product groups only (the fused path's case)
    // mode 1: the evaluation stops after the factorisation; the caller runs the gradient's ending
    // (enqueue_grad_ending) itself, with its own alpha (the Laplace gradient, §10.14)
    bool defer_ending = false;

    static ExtraRows dense(int mode, int64_t n) {  // n rows in ceil(n / 128) tile rows
        ExtraRows x;
        x.mode = mode;
        x.tiles = (int)((n + NB - 1) / NB);
        x.M = n;
        return x;
    }
    // identity rows for order N: one tile row per tile column of the augmented matrix
    static ExtraRows identity(int64_t N, bool singletons = true) {
        ExtraRows x;
        x.mode = 1;
        x.tiles = (int)((N + NB) / NB);
        x.singletons = singletons;
        return x;
    }
    static ExtraRows test_points(int64_t M) { return dense(2, M); }
    static ExtraRows components(const CompSel& sel) {  // G * Mc packed rows
        ExtraRows x = dense(2, (int64_t)sel.G * sel.Mc);
        x.comp = true;
        x.sel = sel;
        return x;
    }
    static ExtraRows responses(int64_t R, const double* Y, int64_t ldy, const double* sub = nullptr) {
        ExtraRows x = dense(3, R);
        x.Y = Y;
        x.ldy = ldy;
        x.sub = sub;
        return x;
    }
    ExtraRows deferred() const {
        ExtraRows x = *this;
        x.defer_ending = true;
        return x;
    }
    // the same rows on a matrix the caller has already put in the workspace
    ExtraRows on_prebuilt() const {
        ExtraRows x = *this;
        x.prebuilt = true;
        return x;
    }
};
}  // namespace gaplac

struct gaplac_ctx {
    int device = 0;
    hipStream_t s_main = nullptr, s_panel = nullptr;
    hipStream_t s_extra = nullptr;  // extra rows (gradient / posterior), beside the bulk updates
    hipStream_t s_xrest = nullptr;  // extra rows: their updates beyond the next SP
    hipEvent_t ev_xinit = nullptr, ev_xdone = nullptr;
    hipEvent_t ev_xc[2] = {}, ev_xr[2] = {};  // extra rows: SP chain done (s_extra), SP rest done (s_xrest)
    hipEvent_t ev_P[2] = {}, ev_R[2] = {}, ev_gram = nullptr, ev_gram2 = nullptr;
    hipEvent_t ev_split[2] = {}, ev_rest[2] = {};  // split bulk updates (factor_and_reduce), ping-pong
    double* A = nullptr;
    size_t A_elems = 0;
    double* Dinv = nullptr;  // per diagonal block: 8 inverses of its 16x16 sub-blocks
    size_t Dinv_elems = 0;
    // Tile lists for the bulk trailing updates: the list for an m x m triangle is a
    // prefix-independent array, so one list per m, all packed: offset[m] into tiles.
    uint32_t* tiles = nullptr;
    size_t tiles_elems = 0;
    int tiles_nt = 0;
    std::vector<size_t> tile_off;
    // band lists (paired updates): tile columns 0 .. spw-1 of an m-row trailing matrix, rows
    // r >= c, rows outer; packed after the triangle lists, band_off[m] into tiles
    std::vector<size_t> band_off;
    double* dX = nullptr;
    size_t dX_elems = 0;
    double* dv = nullptr;
    size_t dv_elems = 0;
    EvalResult* dres = nullptr;
    EvalResult* hres = nullptr;  // pinned
    TermPack* dtp = nullptr;     // device copy of the term descriptor (read by gram_kernel)
    TermPack* htp = nullptr;     // pinned staging for it
    std::string err;
    // profiling: 1 = per-launch device timestamps (KTime slots, see kt_begin/kt_end);
    // 2 = hipEvents recorded on s_main around every bulk tile_syrk launch (eager launches),
    //     read back by gaplac_get_stats
    int prof_mode = 0;
    std::vector<hipEvent_t> evpool;
    struct EvPair {
        size_t i0;
        double flops, bytes;
        int kind;  // 0 bulk tile_syrk launch, 8 cinv_tile launch
    };
    std::vector<EvPair> evpairs;
    // Schedule switches, read once in gaplac_ctx_create; the defaults are
    // the measured best at N = 16384.
    bool serial = false;  // GAPLAC_SERIAL=1: one stream, no overlap (per-kernel timing)
    bool dry = false;     // host-only walk of the schedule (gaplac_plan_check): no HIP calls
    int spw = 4;          // GAPLAC_SPW: super-panel width in 128-column tiles (bulk K = 128 spw)
    int tail_s = 32;      // GAPLAC_TAIL_S: the last ~tail_s tile columns run serially on one stream
                          //   (default 48 with the persistent tail, 32 without)
    int pair_ext = 1;     // 1 = a deferring step also updates the band after next (§3.2)
    int band_tiles_m = 64;  // GAPLAC_BAND_TILES_M: bands of >= this many tile rows as whole tiles
    int grad_fused = 1;     // GAPLAC_GRAD_FUSED: -C^{-1} contracted inside cinv_contract_kernel (0: stored, then contracted)
    int la_tiles_m = 120;   // the lookahead of >= this many tile rows as whole tiles (0: never)
    // GAPLAC_TAIL_SIM: the single-evaluation tail list ordered by a simulated schedule
    // (sim_order_tail_tasks); -1 = for tails of fewer than 80 tile columns (measured: T = 33
    // -4.4%, T = 65 -1.3%, T = 80 +0.3%), 0 never, 1 always
    int tail_sim = -1;
    int pair_m = 40;      // GAPLAC_PAIR_M: paired bulk updates while >= this many tile rows follow the band
    int pair_depth = 0;   // (plan checks only) super-panels per deferred bulk update (0: 4 from 256 tile
                          //   columns on, else 2; N = 65536 1439 -> 1427 ms, 16k 26.97 -> 27.14 ms at 3-4)
    int ncu = 256;        // compute units of the device
    bool tailk = true;    // GAPLAC_TAILK: the serial tail as one persistent dataflow launch (tail_kernel)
    TailCtl* tctl = nullptr;     // its completion counters (zeroed per launch)
    uint32_t* ttasks = nullptr;  // its task list for ttasks_T tile columns
    size_t ttasks_elems = 0;
    int ttasks_T = -1, ttasks_X = 0, ttasks_n = 0;
    bool ttasks_G = false;  // the list holds the Gram's tile tasks (gram_in_tail)
    std::string ttrace_path;     // GAPLAC_TAIL_TRACE: append per-task times of every tail launch here
    int tail_fault = -1;         // GAPLAC_TAIL_FAULT (tests only): skip this tail column's diagonal block
    unsigned long long* ttrace = nullptr;
    size_t ttrace_elems = 0;
    gaplac_stats stats{};
    struct Slot {
        int kind;  // 0 bulk syrk, 1 gram, 2 diag, 4 trsm, 5 column update, 6 small bulk
        double work;
        double bytes;  // kind 0: algorithmic HBM bytes
    };
    std::vector<Slot> slots;     // slots of the launches being enqueued
    KTime* dkt = nullptr;        // device slot array
    KTime* hkt = nullptr;        // pinned copy
    size_t kt_cap = 0;
    bool recording = false;      // assign slots while enqueuing
    // Batched select: models in flight on independent lanes (child contexts with their
    // own workspace and streams; they read the parent's uploaded X and v).
    std::vector<gaplac_ctx*> lanes;
    // Fitted posteriors created on this context (gaplac_fit_create): each owns
    // its device buffer; gaplac_ctx_destroy frees the buffers and orphans the handles
    std::vector<struct gaplac_fit*> fits;
    int batch_lanes = 2;           // GAPLAC_BATCH_LANES (measured at N=8192: 1 lane 138, 2 lanes 191, 3-6 lanes 161-187 evals/s)
    int tail_share = 1;            // lanes sharing the GPU (gaplac_logpdf_batch): tail grid = CUs / share
    int batch_w = 32;              // GAPLAC_BATCH_W: models per tail launch when the whole matrix is in the tail
    int batch_lag = -1;            // GAPLAC_BATCH_LAG: tile columns between consecutive models of a tail launch
                                   // (-1: 3/8 of the matrix's tile columns)
#ifndef GAPLAC_SINGLE_GROUP
#define GAPLAC_SINGLE_GROUP 2
#endif
#ifndef GAPLAC_BATCH_GROUP
#define GAPLAC_BATCH_GROUP 2
#endif
#ifndef GAPLAC_QUAD_LAST
#define GAPLAC_QUAD_LAST 24
#endif
    int batch_gw = 8, batch_near = 2;  // the batched tail's deep-task width and near distance (A/B: §3.4)
    // single evaluations: quadrant next-column updates in the last 24 tail columns (the
    // latency-bound end) and pipelined half-tile TRSMs; batched lists: whole tiles and
    // whole-tile TRSMs throughout (select: 258 -> 267 evals/s)
    // the batched-tail workspace (gaplac_logpdf_batch): batch_w matrices
    struct BatchWs {
        double* A = nullptr;
        size_t A_elems = 0;
        double* Dinv = nullptr;
        size_t Dinv_elems = 0;
        EvalResult* dres = nullptr;
        size_t dres_elems = 0;
        EvalResult* hres = nullptr;  // pinned
        TermPack* dtp = nullptr;
        size_t dtp_elems = 0;
        TermPack* htp = nullptr;  // pinned
        int host_cap = 0;
        TailCtl* ctl = nullptr;
        size_t ctl_elems = 0;
        uint32_t* tasks = nullptr;
        size_t tasks_elems = 0;
        int tasks_T = -1, tasks_B = 0, tasks_n = 0, tasks_lag = -1;
        hipEvent_t ev_gram = nullptr, ev_done = nullptr;  // Grams written (s_panel); launch retired (s_main)
        bool busy = false;                                // a launch on this set is in flight
        int m0 = 0, B = 0;                                // its models
    } bw[2];  // two sets: one launch's Grams overlap the previous launch's tail
    bool borrowed_inputs = false;  // dX / dv belong to the parent
    // The evaluation in flight (none between evaluations): written by EvalScope alone, read by
    // the engine (factor_and_reduce, tail_allowed, ensure_workspace, enqueue_eval_body, ...)
    ExtraRows xr;
    double* dXs = nullptr;  // mode 2: test inputs (ld xr.M; per-component rows: ld xr.sel.Mc)
    size_t dXs_elems = 0;
    double* dY = nullptr;  // gaplac_logpdf_multi: the host matrix's copy (ld N)
    size_t dY_elems = 0;
    double* mres = nullptr;  // mode 3 results: quad[R], then logpdf[R]
    size_t mres_elems = 0;
    // gaplac_rand_multi: Z (ld Np, so the kernel's 16-byte loads are aligned) and OUT (ld N)
    double* dZ = nullptr;
    size_t dZ_elems = 0;
    double* dO = nullptr;
    size_t dO_elems = 0;
    double* pmean = nullptr;
    double* pvar = nullptr;
    size_t pmv_elems = 0;
    // Joint posterior: the order-M workspace that post_cov_kernel fills and the
    // second factorisation runs in. For that factorisation A and B change places (WsSwap) and
    // the evaluation is described as on_prebuilt(): it finds its matrix already built.
    double* B = nullptr;
    size_t B_elems = 0;
    // Joint covariance of the inducing-point posterior: the order-Ms workspace that
    // sparse_post_cov_kernel fills and the third factorisation runs in (both others are live by
    // then), and the tile-aligned copy of the a rows
    double* C = nullptr;
    size_t C_elems = 0;
    double* sj_rows = nullptr;
    size_t sj_rows_elems = 0;
    // Inducing-point approximation: y on the device and the chunk partials of S
    double* sp_y = nullptr;
    size_t sp_y_elems = 0;
    double* sp_part = nullptr;
    size_t sp_part_elems = 0;
    // Its gradient: the order-Mz scratch (three column storages of leading
    // dimension 2 Np), the first factorisation's Dinv kept across the second, and the vectors
    bool sg_keep = false;  // gaplac_sparse_elbo_grad is running: the stages keep S and Dinv
    double* sg = nullptr;
    size_t sg_elems = 0;
    double* sg_dinv = nullptr;
    size_t sg_dinv_elems = 0;
    double* sg_v = nullptr;
    size_t sg_v_elems = 0;
    // The gradient with respect to the inducing inputs: partials and the result
    double* sgz = nullptr;
    size_t sgz_elems = 0;
    // gradient: alpha, partial sums, the XCD-balanced C^{-1} tile list
    double* galpha = nullptr;
    size_t galpha_elems = 0;
    double* gdv = nullptr;
    size_t gdv_elems = 0;
    double* gz = nullptr;  // z (row N of the factor), contiguous: alpha's input beside cinv
    size_t gz_elems = 0;
    double* gpart = nullptr;
    size_t gpart_elems = 0;
    double* gout = nullptr;   // device: T+1 results
    double* hgout = nullptr;  // pinned copy
    GradTermPack* dgp = nullptr;
    GradTermPack* hgp = nullptr;  // pinned staging
    uint32_t* glist = nullptr;
    size_t glist_elems = 0;
    int glist_m = -1, glist_blocks = 0;
    // Laplace approximation: every vector of the Newton iteration, the partial
    // sums and the matrix-free products' scratch in one buffer (LapDims)
    double* lap = nullptr;
    size_t lap_elems = 0;
};

namespace {

int set_err(gaplac_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int set_err(gaplac_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return code;
}

#define HIPCK(ctx, call)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return set_err(ctx, GAPLAC_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// HIP runtime calls of the schedule itself (events, waits, copies): skipped in a dry run.
#define HIPQ(ctx, call)                    \
    do {                                   \
        if (!(ctx)->dry) HIPCK(ctx, call); \
    } while (0)

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// What a context owns, written once: gaplac_ctx_create, gaplac_ctx_destroy and
// gaplac_ctx_release walk these lists (evpool's events and the lanes are the only other
// resources). The struct itself stays plain: the dry runs keep one on the stack.
std::array<hipEvent_t*, 20> ctx_events(gaplac_ctx* c) {
    return {&c->ev_P[0],       &c->ev_P[1],       &c->ev_R[0],       &c->ev_R[1],
            &c->ev_xc[0],      &c->ev_xc[1],      &c->ev_xr[0],      &c->ev_xr[1],
            &c->ev_split[0],   &c->ev_split[1],   &c->ev_rest[0],    &c->ev_rest[1],
            &c->ev_gram,       &c->ev_gram2,      &c->ev_xinit,      &c->ev_xdone,
            &c->bw[0].ev_gram, &c->bw[0].ev_done, &c->bw[1].ev_gram, &c->bw[1].ev_done};
}

struct Buf {
    void** p;
    size_t* cap;   // the capacity kept beside a buffer that gaplac_ctx_release drops (else nullptr)
    size_t fixed;  // > 0: this many bytes from gaplac_ctx_create on; 0: grown on demand
    bool pinned;   // host memory (hipHostMalloc)
};
template <typename T>
Buf buf(T** p, size_t fixed = 0, bool pinned = false, size_t* cap = nullptr) {
    return {reinterpret_cast<void**>(p), cap, fixed, pinned};
}
template <typename T>
Buf large(T** p, size_t* cap) { return buf(p, 0, false, cap); }

std::vector<Buf> ctx_buffers(gaplac_ctx* c) {
    constexpr size_t gout_bytes = sizeof(double) * (GAPLAC_MAX_TERMS + 1);
    std::vector<Buf> b{large(&c->A, &c->A_elems), large(&c->Dinv, &c->Dinv_elems), buf(&c->tiles), buf(&c->dX),
                       buf(&c->dv), buf(&c->dres, sizeof(EvalResult)), buf(&c->hres, sizeof(EvalResult), true),
                       buf(&c->dtp, sizeof(TermPack)), buf(&c->htp, sizeof(TermPack), true), buf(&c->tctl),
                       buf(&c->ttasks), buf(&c->ttrace), buf(&c->dkt), buf(&c->hkt, 0, true), buf(&c->dXs),
                       buf(&c->pmean), buf(&c->pvar), buf(&c->galpha), buf(&c->gdv), buf(&c->gz), buf(&c->gpart),
                       buf(&c->gout, gout_bytes), buf(&c->hgout, gout_bytes, true), buf(&c->dgp, sizeof(GradTermPack)),
                       buf(&c->hgp, sizeof(GradTermPack), true), buf(&c->glist), large(&c->dY, &c->dY_elems),
                       buf(&c->mres), large(&c->dZ, &c->dZ_elems), large(&c->dO, &c->dO_elems),
                       large(&c->B, &c->B_elems), large(&c->sp_y, &c->sp_y_elems),
                       large(&c->sp_part, &c->sp_part_elems), large(&c->sg, &c->sg_elems),
                       large(&c->sg_dinv, &c->sg_dinv_elems), large(&c->sg_v, &c->sg_v_elems),
                       large(&c->sgz, &c->sgz_elems), large(&c->C, &c->C_elems),
                       large(&c->sj_rows, &c->sj_rows_elems), large(&c->lap, &c->lap_elems)};
    for (auto& w : c->bw)
        b.insert(b.end(), {large(&w.A, &w.A_elems), large(&w.Dinv, &w.Dinv_elems), buf(&w.dres), buf(&w.dtp),
                           buf(&w.hres, 0, true), buf(&w.htp, 0, true), buf(&w.ctl), buf(&w.tasks)});
    return b;
}

void free_buf(const Buf& b) {
    if (*b.p) (void)(b.pinned ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
    if (b.cap) *b.cap = 0;
}

// Wait for everything the context has enqueued (every stream it holds); the first error.
hipError_t sync_streams(gaplac_ctx* c) {
    hipError_t first = hipSuccess;
    for (hipStream_t s : {c->s_main, c->s_panel, c->s_extra, c->s_xrest}) {
        const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

}  // namespace

// Validate terms and build the kernel-argument pack. Mirrors the argument checks of the
// KernelFunctions constructors GaPLAC calls (src/abstractgp_translations.jl:8-15):
// LinearKernel requires c >= 0; ScaleTransform(1/l) requires a positive finite scale.
static int pfail(std::string* err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static int pfail(std::string* err, int code, const char* fmt, ...) {
    if (err) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        *err = buf;
    }
    return code;
}

int gaplac::pack_terms(int32_t D, int32_t T, const gaplac_term* terms, TermPack* tp, std::string* err) {
#define fail(...) pfail(err, __VA_ARGS__)
    if (T < 0 || T > GAPLAC_MAX_TERMS) return fail(GAPLAC_E_KIND, "term count %d outside [0, %d]", T, GAPLAC_MAX_TERMS);
    if (T > 0 && !terms) return fail(GAPLAC_E_ARG, "terms is NULL");
    std::memset(tp, 0, sizeof *tp);
    tp->T = T;
    for (int t = 0; t < T; ++t) {
        const gaplac_term& x = terms[t];
        if (x.reserved != 0) return fail(GAPLAC_E_ARG, "term %d: reserved field not 0", t);
        // groups must be contiguous: a group id seen before must be the previous term's
        for (int u = 0; u + 1 < t; ++u)
            if (terms[u].group == x.group && terms[t - 1].group != x.group)
                return fail(GAPLAC_E_KIND, "term %d: product group %d not contiguous", t, x.group);
        tp->kind[t] = x.kind;
        tp->col[t] = x.col;
        switch (x.kind) {
            case GAPLAC_SQEXP:
            case GAPLAC_OU:
                if (!(x.param > 0.0) || !std::isfinite(x.param))
                    return fail(GAPLAC_E_PARAM, "term %d: lengthscale %g must be > 0", t, x.param);
                tp->p[t] = 1.0 / x.param;  // ScaleTransform(inv(l))
                if (!(tp->p[t] > 0.0)) return fail(GAPLAC_E_PARAM, "term %d: scale 1/l underflows", t);
                break;
            case GAPLAC_LINEAR:
                if (!(x.param >= 0.0) || !std::isfinite(x.param))
                    return fail(GAPLAC_E_PARAM, "term %d: c = %g must be >= 0", t, x.param);
                tp->p[t] = x.param;
                break;
            case GAPLAC_CAT:
                tp->p[t] = 0.0;
                break;
            case GAPLAC_NOISE:
                if (!(x.param >= 0.0) || !std::isfinite(x.param))
                    return fail(GAPLAC_E_PARAM, "term %d: noise variance %g must be >= 0", t, x.param);
                tp->p[t] = x.param;
                tp->col[t] = 0;
                break;
            default:
                return fail(GAPLAC_E_KIND, "term %d: unknown kind %d", t, x.kind);
        }
        if (x.kind != GAPLAC_NOISE && (x.col < 0 || x.col >= D))
            return fail(GAPLAC_E_COL, "term %d: column %d outside [0, %d)", t, x.col, D);
        tp->last_in_group[t] = (t == T - 1 || terms[t + 1].group != x.group) ? 1 : 0;
    }
#undef fail
    return 0;
}

namespace {

int pack_terms(gaplac_ctx* ctx, int32_t D, int32_t T, const gaplac_term* terms, TermPack* tp) {
    return gaplac::pack_terms(D, T, terms, tp, ctx ? &ctx->err : nullptr);
}

int check_common(gaplac_ctx* ctx, int64_t N, int32_t D, const void* X, int64_t ldx, double noise,
                 const void* v) {
    if (!ctx) return GAPLAC_E_ARG;
    if (N < 0) return set_err(ctx, GAPLAC_E_ARG, "N = %lld < 0", (long long)N);
    if (N > 0 && D > 0 && (!X || ldx < N))
        return set_err(ctx, GAPLAC_E_ARG, "X NULL or ldx %lld < N %lld", (long long)ldx,
                       (long long)N);
    if (N > 0 && !v) return set_err(ctx, GAPLAC_E_ARG, "v is NULL");
    if (D < 0) return set_err(ctx, GAPLAC_E_ARG, "D = %d < 0", D);
    if (!(noise >= 0.0) || !std::isfinite(noise))
        return set_err(ctx, GAPLAC_E_PARAM, "noise %g must be finite and >= 0", noise);
    return 0;
}

template <typename T>
int ensure(gaplac_ctx* ctx, T** p, size_t* cap, size_t n) {
    if (*cap >= n) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)) != hipSuccess)
        return set_err(ctx, GAPLAC_E_OOM, "hipMalloc of %zu bytes failed", n * sizeof(T));
    *cap = n;
    return 0;
}

// Profiling slot for the next launch (nullptr when profiling is off).
KTime* slot(gaplac_ctx* ctx, int kind, double work, double bytes = 0.0) {
    if (!ctx->recording) return nullptr;
    const size_t i = ctx->slots.size();
    if (i >= ctx->kt_cap) return nullptr;
    ctx->slots.push_back({kind, work, bytes});
    return ctx->dkt + i;
}

// Algorithmic flops of one bulk trailing-update launch per 128 of K: lower triangle
// (incl. diagonal) of the m x m tile triangle, 2 flops per multiply-add.
double syrk_flops(int m) {
    const double nbd = NB;
    const double rows = (double)m * nbd;
    return 2.0 * nbd * rows * (rows + 1) / 2.0;
}

// Algorithmic HBM bytes of one bulk trailing-update launch over the m x m tile triangle
// with K = kd: every C tile read and written once, the m*NB panel rows read once.
double syrk_bytes(int m, int kd) {
    const double tiles = (double)m * (m + 1) / 2.0;
    return tiles * NB * NB * 8.0 * 2.0 + (double)m * NB * kd * 8.0;
}

// Algorithmic flops of a band launch: the W tile columns of an mbd-row trailing matrix
// (rows r >= c), K = kd: W diagonal tiles (lower triangle incl. diagonal), the rest whole.
double band_flops(int mbd, int W, int kd) {
    const int w = std::min(W, mbd);
    const double tiles = (double)w * mbd - (double)w * (w - 1) / 2.0;
    return (tiles - w) * 2.0 * NB * NB * kd + (double)w * NB * (NB + 1) * kd;
}

// Fold the device timestamps of the given slots into ctx->stats (ticks: 100 MHz).
int accumulate_slots(gaplac_ctx* ctx, const std::vector<gaplac_ctx::Slot>& slots) {
    if (slots.empty()) return 0;
    HIPCK(ctx, hipMemcpy(ctx->hkt, ctx->dkt, slots.size() * sizeof(KTime), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, t1 = 0;
    for (size_t i = 0; i < slots.size(); ++i) {
        const KTime& t = ctx->hkt[i];
        if (t.end < t.start || t.start == ~0ull) continue;
        const double ms = (double)(t.end - t.start) * 1e-5;
#if defined(GAPLAC_CLOCK) && GAPLAC_CLOCK
        if (t.clk_rt > 0)  // diagnostic build: the clock each bulk launch held
            std::fprintf(stderr, "clk slot %zu kind %d %.3f ms %.3f GHz, %llu workgroups, %.0f cycles each\n", i,
                         slots[i].kind, ms, (double)t.clk_mt / (double)t.clk_rt * 0.1, t.clk_n,
                         (double)t.clk_mt / (double)std::max(1ull, t.clk_n));
#endif
        t0 = std::min(t0, t.start);
        t1 = std::max(t1, t.end);
        switch (slots[i].kind) {
            case 0:
                ctx->stats.syrk_ms += ms;
                ctx->stats.syrk_flops += slots[i].work;
                ctx->stats.syrk_launches += 1;
                ctx->stats.syrk_bytes += slots[i].bytes;
                break;
            case 6:
                ctx->stats.small_ms += ms;
                ctx->stats.small_launches += 1;
                break;
            case 7:
                ctx->stats.grad_rows_ms += ms;
                break;
            case 8:
                ctx->stats.cinv_ms += ms;
                ctx->stats.cinv_launches += 1;
                break;
            case 9:
                ctx->stats.contract_ms += ms;
                break;
            case 10:
                ctx->stats.tail_ms += ms;
                ctx->stats.tail_launches += 1;
                break;
            case 1:
                ctx->stats.gram_ms += ms;
                ctx->stats.gram_bytes += slots[i].work;
                ctx->stats.gram_launches += 1;
                break;
            case 2:
                ctx->stats.panel_ms += ms;
                break;
            case 4:
                ctx->stats.trsm_ms += ms;
                break;
            default:
                ctx->stats.colupd_ms += ms;
                break;
        }
    }
    if (t1 > t0) ctx->stats.total_ms += (double)(t1 - t0) * 1e-5;
    ctx->stats.evals += 1;
    return 0;
}

// Factor the augmented matrix already built in ctx->A (Gram launched on s_main).
//
// Super-panels of W 128-wide tile columns (SP p covers tile columns pW .. pW+W-1,
// GAPLAC_SPW, default 4): the panel chain factors 128-wide blocks, the bulk trailing
// update applies a whole super-panel at once (K = 128 W). Measured per 128x128 tile:
// ~10 us fixed (C load, first staging, epilogue) + K at the MFMA ceiling, so larger K
// amortises the fixed part (and cuts C-tile HBM traffic per flop by W).
//
// Two streams, eager launches. s_panel (highest priority, all CUs) runs the critical path
// in order; s_main (lowest priority) runs the Gram and the bulk updates. Super-panel
// boundaries come from superpanel_starts() (width spw; the last ~tail_s tile columns are
// factored by serial_tail() on s_main alone).
//   s_panel: wait R(p-1) | col_update(columns of SP p+1, with SP p, K=128W)
//            | for each column c of SP p+1: [col_update(c with c-1..first, K=128)] potrf(c) trsm(c)
//            | rec P(p+1)
//   s_main : wait P(p)   | syrk_tri(tile columns >= (p+2)W, with SP p, K=128W) | rec R(p)
// Within SP p+1 the chain is right-looking with K=128 column updates (each column gets
// the previous columns of its own super-panel). Columns of SP p+1 receive SP p-1 in
// R(p-1) and SP p in the lookahead col_update; within a step the streams touch disjoint
// tile columns. Events ping-pong (p & 1).
// GAPLAC_CHAIN_SKIP (-D, timing diagnostics only: the result is void): 1 = the super-panel
// chain's column updates, diagonal blocks and TRSMs are not launched, 2 = nor the
// lookahead; what the evaluation costs without the chain's CU share and latency.
#ifndef GAPLAC_CHAIN_SKIP
#define GAPLAC_CHAIN_SKIP 0
#endif
int factor_superpanel(gaplac_ctx* ctx, hipStream_t sp, int64_t N, int64_t lda, int nt, int c0, int c1) {
    if (GAPLAC_CHAIN_SKIP >= 1 && !ctx->dry) return 0;
    for (int c = c0; c < c1; ++c) {
        double* Acol = ctx->A + (int64_t)c * NB * lda;
        if (c > c0)
            launch_col_update(sp, ctx->A, lda, Panel{Acol - NB * lda, lda, 0}, nt, c, c, c1 - c, NB,
                              slot(ctx, 5, 0));
        double* Dk = ctx->Dinv + (size_t)c * DINV_PER_BLOCK;
        if ((int64_t)c * NB < N)
            launch_potrf_diag(sp, Acol + (int64_t)c * NB, lda, N, (int64_t)c * NB, Dk, ctx->dres, slot(ctx, 2, 0));
        launch_trsm(sp, Acol, lda, nt, c, Dk, slot(ctx, 4, 0));
    }
    return 0;
}

// Extra rows, tile rows nt .. nt + xr.tiles - 1 of the column storage,
// factored along on s_main, off the critical path: once SP p's columns are final (P(p)),
// its extra-row tiles get the column-by-column substitution (the earlier columns of the SP
// applied first, K = 128), then SP p is applied to every later column (K = 128 W).
// Identity rows (gradient): only rows E <= c of column c are nonzero (Y = L^{-T} is upper
// triangular), so each step touches rows [0, c] / [0, end of SP); tiles below Y's diagonal
// stay exactly zero and are never written. Cross-covariance rows (posterior): all rows.
// extra-row updates of at least this many tiles run as whole 128x128 tiles (tile_syrk_kernel),
// not quadrants: gradient 79.4 -> 78.0 ms with the split below (profiles/r04r_xr_ab.txt)
constexpr int XR_TILE_MIN = 128;

static void extra_rows_chain(gaplac_ctx* ctx, hipStream_t sm, int64_t lda, int nt, int c0, int c1) {
    const int W = ctx->spw;
    const bool tri = ctx->xr.mode == 1;
    const int mt = ctx->xr.tiles;
    for (int c = c0; c < c1; ++c) {
        double* Acol = ctx->A + (int64_t)c * NB * lda;
        if (c > c0) {
            const int rows = tri ? c : mt;
            BulkArgs ba{ctx->A, lda, Panel{Acol - NB * lda, lda, 0}, nullptr, rows * (c1 - c), NB, nt, c,
                        ColMap{1, 0, W}};
            ba.rect_rows = rows;
            ba.tile_min = XR_TILE_MIN;
            launch_bulk(sm, ba, slot(ctx, 7, 0));
        }
        launch_trsm_rows(sm, Acol, lda, c, nt, tri ? c + 1 : mt, ctx->Dinv + (size_t)c * DINV_PER_BLOCK,
                         slot(ctx, 7, 0));
    }
}

// SP [c0, c1)'s extra-row tiles applied to tile columns [jb, je) of the extra rows (K = 128 W)
static void extra_rows_update(gaplac_ctx* ctx, hipStream_t sm, int64_t lda, int nt, int c0, int c1, int jb,
                              int je) {
    if (je <= jb) return;
    const int rows = ctx->xr.mode == 1 ? c1 : ctx->xr.tiles;
    BulkArgs ba{ctx->A, lda, Panel{ctx->A + (int64_t)c0 * NB * lda, lda, 0}, nullptr, rows * (je - jb),
                (c1 - c0) * NB, nt, jb, ColMap{1, 0, ctx->spw}};
    ba.rect_rows = rows;
    ba.tile_min = XR_TILE_MIN;
    launch_bulk(sm, ba, slot(ctx, 7, 0));
}

// Super-panel boundaries: tile columns sp[p] .. sp[p+1]-1 form SP p, width spw. With a
// serial tail (tail_s > 0, plain logpdf) the list stops at the first boundary with at
// most tail_s tile columns after it; those columns are factored by serial_tail().
// The whole matrix in the persistent tail (no super-panels): plain logpdf with at most
// tail_s (and TAIL_TMAX) tile columns.
// Which evaluations take a tail: plain logpdf, and dense extra rows (posterior, logpdf_multi)
// when they fit beside the tail's columns (the persistent tail factors them along, §10); the
// gradient's identity rows (one per column) never do.
// Dense extra rows (the posterior's cross-covariance rows, the responses of logpdf_multi):
// every row of every column is nonzero, so both take the same schedule.
static bool dense_rows(const gaplac_ctx* ctx) { return ctx->xr.mode == 2 || ctx->xr.mode == 3; }

static bool tail_allowed(const gaplac_ctx* ctx) {
    return ctx->xr.mode == 0 || (dense_rows(ctx) && ctx->tailk && ctx->tail_s > 0 &&
                                 ctx->xr.tiles + std::min(ctx->tail_s, TAIL_TMAX) <= TAIL_TMAX);
}

static bool whole_in_tail(const gaplac_ctx* ctx, int nt) {
    return tail_allowed(ctx) && ctx->tailk && ctx->tail_s > 0 && nt <= TAIL_TMAX && nt <= ctx->tail_s;
}

// The Gram inside the tail (TAIL_G tasks, -D GAPLAC_TAIL_GRAM=0 turns it off): a plain
// single evaluation whose matrix lies whole in the tail builds its Gram tiles as the tail's
// first tasks instead of in two launches before it (N = 4096: the Gram launches, their gaps
// and the tail's start behind them were ~50 us of the 1.15 ms evaluation).
// Needs the tile stores' buffer offsets (< 2^31 bytes per tile column span).
#ifndef GAPLAC_TAIL_GRAM
#define GAPLAC_TAIL_GRAM 1
#endif
static bool gram_in_tail(const gaplac_ctx* ctx, int nt, int64_t lda) {
    return GAPLAC_TAIL_GRAM && ctx->xr.mode == 0 && !ctx->xr.prebuilt && whole_in_tail(ctx, nt) &&
           ((int64_t)(NB - 1) * lda + NB) * 8 < ((int64_t)1 << 31);
}

// The term descriptor reaches ctx->dtp through the evaluation's first launch
// (init_result_ctl_kernel, when the Gram is inside the tail) instead of a copy.
static bool tp_by_init(const gaplac_ctx* ctx, int64_t N) {
    const int64_t Np = round_up(N + 1, NB);
    return gram_in_tail(ctx, (int)(Np / NB), Np + (int64_t)NB * ctx->xr.tiles);
}

static std::vector<int> superpanel_starts(const gaplac_ctx* ctx, int nt) {
    std::vector<int> sp{0};
    // a matrix the persistent tail covers whole (plain logpdf, at most TAIL_TMAX tile
    // columns, within tail_s): no super-panel at all, every column in the tail kernel
    if (whole_in_tail(ctx, nt)) return sp;
    int c = 0;
    while (c < nt) {
        if (tail_allowed(ctx) && ctx->tail_s > 0 && c > 0 && nt - c <= ctx->tail_s) break;
        c = std::min(c + ctx->spw, nt);
        sp.push_back(c);
    }
    return sp;
}

// Serial tail: tile columns ts .. nt-1 factored right-looking on one stream,
// after the bulk update that applied the last super-panel to them: per column the whole
// remaining triangle gets the previous column (K = 128), then the diagonal block and the
// TRSM. No events: in the chain-bound tail every event record or cross-stream wait costs
// ~6-12 us of dispatch latency on the critical path, more than the small updates save by
// overlapping.
static void serial_tail(gaplac_ctx* ctx, hipStream_t sm, int64_t N, int64_t lda, int nt, int ts) {
    for (int c = ts; c < nt; ++c) {
        double* Acol = ctx->A + (int64_t)c * NB * lda;
        if (c > ts) {
            const int m = nt - c;
            BulkArgs ba{ctx->A, lda, Panel{Acol - NB * lda, lda, 0}, ctx->tiles + ctx->tile_off[(size_t)m],
                        m * (m + 1) / 2, NB, c, c, ColMap{1, 0, ctx->spw}};
            launch_bulk(sm, ba, slot(ctx, 6, 0));
        }
        double* Dk = ctx->Dinv + (size_t)c * DINV_PER_BLOCK;
        if ((int64_t)c * NB < N)
            launch_potrf_diag(sm, Acol + (int64_t)c * NB, lda, N, (int64_t)c * NB, Dk, ctx->dres, slot(ctx, 2, 0));
        launch_trsm(sm, Acol, lda, nt, c, Dk, slot(ctx, 4, 0));
    }
}

// Super-panels per deferred bulk update (pair_depth, or by size: see gaplac_ctx::pair_depth)
static int deferral_depth(const gaplac_ctx* ctx, int nt) {
    return ctx->pair_depth > 0 ? ctx->pair_depth : nt >= 256 ? 4 : 2;
}

// Paired bulk updates (GAPLAC_PAIR_M): does step p defer its bulk update
// (only the next-needed bands get SP p; the columns after them get SPs p and p+1 together
// at step p+1)? pend: the super-panel still pending (-1: none).
static bool pair_defer(const gaplac_ctx* ctx, const std::vector<int>& spc, int nt, int p, int pend) {
    const int nsp = (int)spc.size() - 1;
    const int jb = p + 2 <= nsp ? spc[(size_t)p + 2] : spc[(size_t)nsp];
    const int je = p + 3 <= nsp ? spc[(size_t)p + 3] : spc[(size_t)nsp];
    return ctx->pair_m > 0 && (pend < 0 || p - pend + 1 < deferral_depth(ctx, nt)) && !ctx->serial &&
           !ctx->xr.mode && je > jb && p + 1 + ctx->pair_ext < nsp && p + 3 + ctx->pair_ext <= nsp &&
           nt - spc[(size_t)p + 3 + ctx->pair_ext] >= ctx->pair_m;
}

// Latency-shaped (quadrant) columns of a single evaluation's tail: with the simulated
// order a tail of at most 40 tile columns takes them in every column (N = 4096: -2%; at T =
// 65 all columns cost +4%, 40 of them +1.5%), else the last GAPLAC_QUAD_LAST.
static int tail_quad_last(bool sim, int T) { return sim && T <= 40 ? TAIL_TMAX : GAPLAC_QUAD_LAST; }

// Deep-task width of a single evaluation's tail: 4 columns (K = 512), or 8 (K = 1024) for
// tails of at least GAPLAC_GW8_T tile columns (-D; A/B switch).
#ifndef GAPLAC_GW8_T
#define GAPLAC_GW8_T 1000
#endif
static int tail_gw(int T) { return T >= GAPLAC_GW8_T ? 8 : 4; }

}  // namespace
namespace gaplac {
// The single-evaluation tail list of T tile columns (X extra tile rows), as eval_device
// launches it; also the distributed root's gathered tail (gaplac_dist.hip). tail_sim as
// gaplac_ctx::tail_sim; workers: the persistent grid the simulated order plans for.
void build_single_tail_list(int T, int X, int tail_sim, int workers, std::vector<uint32_t>& out, bool gram) {
    const bool sim = (tail_sim > 0 || (tail_sim < 0 && T < 80)) && X == 0;
    out.clear();
    build_tail_tasks(T, out, nullptr, tail_gw(T), 4, tail_quad_last(sim, T), false, GAPLAC_SINGLE_GROUP, X, sim ? 1 : 0);
    if (sim && workers > 0) sim_order_tail_tasks(T, out, workers);
    if (gram && X == 0) add_gram_tasks(T, out);
}
}  // namespace gaplac
namespace {

// Split bulk updates (GAPLAC_SPLIT, -D): plain evaluations whose
// super-panel phase defers in pairs (depth 2); a triangle launch is split only when its
// rest keeps at least SPLIT_REST_MIN tile columns.
#ifndef GAPLAC_SPLIT
#define GAPLAC_SPLIT 1
#endif
constexpr int SPLIT_REST_MIN = 16;
#ifndef GAPLAC_SPLIT_MINCOLS
#define GAPLAC_SPLIT_MINCOLS 32
#endif
#ifndef GAPLAC_SPLIT_DEPTH
#define GAPLAC_SPLIT_DEPTH 2  // deferral depths the split applies to (the head is depth x W columns)
#endif
static bool split_wanted(const gaplac_ctx* ctx, int nt) {
    const std::vector<int> spc = superpanel_starts(ctx, nt);  // (a short super-panel phase: not worth it)
    return GAPLAC_SPLIT && ctx->xr.mode == 0 && !ctx->serial && deferral_depth(ctx, nt) <= GAPLAC_SPLIT_DEPTH &&
           !whole_in_tail(ctx, nt) && spc.back() >= GAPLAC_SPLIT_MINCOLS;
}
static bool split_bulk(const gaplac_ctx* ctx, int nt) {
    return split_wanted(ctx, nt) && (ctx->s_xrest != nullptr || ctx->dry);
}

// Profiling mode 2: `launch` between two hipEvents on its stream st when `timed` (a pair of
// evpool, grown on first use; gaplac_get_stats reads the pairs back as pr describes them).
template <typename Launch>
int timed_launch(gaplac_ctx* ctx, bool timed, hipStream_t st, gaplac_ctx::EvPair pr, Launch&& launch) {
    if (timed) {
        pr.i0 = 2 * ctx->evpairs.size();
        while (ctx->evpool.size() < pr.i0 + 2) {
            hipEvent_t e;
            HIPQ(ctx, hipEventCreate(&e));
            ctx->evpool.push_back(e);
        }
        HIPQ(ctx, hipEventRecord(ctx->evpool[pr.i0], st));
    }
    launch();
    if (timed) {
        HIPQ(ctx, hipEventRecord(ctx->evpool[pr.i0 + 1], st));
        ctx->evpairs.push_back(pr);
    }
    return 0;
}

// The band list's launch: the W tile columns from b0 of the trailing matrix (rows from their
// diagonal down, nt - b0 tile rows) get the panel pn, K = kdep; whole: as 128x128 tiles only.
BulkArgs band_args(const gaplac_ctx* ctx, int64_t lda, int nt, int b0, const Panel& pn, int kdep, bool whole) {
    const int W = ctx->spw, mbd = nt - b0;
    BulkArgs bb{ctx->A, lda, pn, ctx->tiles + ctx->band_off[(size_t)mbd], W * mbd - W * (W - 1) / 2, kdep, b0, b0,
                ColMap{1, 0, W}};
    bb.max_r = mbd - 1;
    bb.max_c = W - 1;
    bb.whole = whole ? 1 : 0;
    return bb;
}

// ... launched on st; in profiling mode 2 whole-tile bands (heads, lookaheads, large bands:
// kind 5) are event-timed, for the bulk phase's union of launch intervals
int band_launch(gaplac_ctx* ctx, hipStream_t st, int64_t lda, int nt, int b0, const Panel& pn, int kdep, bool whole) {
    const BulkArgs bb = band_args(ctx, lda, nt, b0, pn, kdep, whole);
    return timed_launch(ctx, ctx->prof_mode == 2 && whole && !ctx->xr.mode, st,
                        {0, band_flops(nt - b0, ctx->spw, kdep), 0.0, 5},
                        [&] { launch_bulk(st, bb, slot(ctx, 5, 0)); });
}

// s_main waits for what the extra rows' streams hold (gradient / posterior, not serial)
int join_extra_streams(gaplac_ctx* ctx, hipStream_t sm) {
    if (!ctx->xr.mode || ctx->serial) return 0;
    for (hipStream_t sx : {ctx->s_extra, ctx->s_xrest}) {
        HIPQ(ctx, hipEventRecord(ctx->ev_xdone, sx));
        HIPQ(ctx, hipStreamWaitEvent(sm, ctx->ev_xdone, 0));
    }
    return 0;
}

int factor_and_reduce(gaplac_ctx* ctx, int64_t N, int64_t lda, int nt) {
    hipStream_t sm = ctx->s_main;
    hipStream_t sp = ctx->serial ? sm : ctx->s_panel;
    const int W = ctx->spw;
    const std::vector<int> spc = superpanel_starts(ctx, nt);
    const int nsp = (int)spc.size() - 1;
    int frc;
    // Split bulk updates (split_bulk): a bulk update's first 2W tile columns
    // (what the next steps' bands read) stay on s_main, the rest goes to s_xrest, so the
    // next steps' small band launches run beside it instead of after it. rest_from: first
    // tile column of the rest still in flight there; every later launch that reaches it
    // waits for ev_rest first (on its own stream).
    const bool split = split_bulk(ctx, nt);
    hipStream_t sr = ctx->s_xrest;
    int rest_from = nt + 1, nsplit = 0;
    auto wait_rest = [&](hipStream_t st, int col_end) {
        if (col_end <= rest_from) return 0;
        HIPQ(ctx, hipStreamWaitEvent(st, ctx->ev_rest[(nsplit - 1) & 1], 0));
        if (st == sm) rest_from = nt + 1;  // s_main is past it for good (s_panel waits behind s_main's marks)
        return 0;
    };
    if (nsp > 0) {
        HIPQ(ctx, hipStreamWaitEvent(sp, ctx->ev_gram, 0));  // first W tile columns built
        if ((frc = factor_superpanel(ctx, sp, N, lda, nt, spc[0], spc[1]))) return frc;
        HIPQ(ctx, hipEventRecord(ctx->ev_P[0], sp));
    }
    // bulk trailing update of the triangle of tile columns >= j0 with the panel pn (K = kd)
    auto bulk_tri = [&](int j0, const Panel& pn, int kdep) -> int {
        if (j0 >= nt) return 0;
        if ((frc = wait_rest(sm, nt))) return frc;
        int jr = j0;  // first tile column of the triangle launch (after the head)
        hipStream_t st = sm;
        const int hw = deferral_depth(ctx, nt) * W;  // head width
        if (split && nt - j0 >= hw + SPLIT_REST_MIN && ctx->band_off.size() > (size_t)(nt - j0)) {
            // what s_main holds so far (this step's panel wait, earlier updates) before the rest
            HIPQ(ctx, hipEventRecord(ctx->ev_split[nsplit & 1], sm));
            // head: tile columns [j0, j0 + hw) as band launches (whole tiles) on s_main
            for (int b0 = j0; b0 < j0 + hw; b0 += W)
                if ((frc = band_launch(ctx, sm, lda, nt, b0, pn, kdep, true))) return frc;
            jr = j0 + hw;
            st = sr;
            HIPQ(ctx, hipStreamWaitEvent(sr, ctx->ev_split[nsplit & 1], 0));
        }
        const int m = nt - jr;
        BulkArgs ba{ctx->A, lda, pn, ctx->tiles + ctx->tile_off[(size_t)m], m * (m + 1) / 2, kdep, jr, jr,
                    ColMap{1, 0, W}};
        const bool small = syrk_is_small(ba.ntiles);
        const double fl = syrk_flops(m) * (kdep / NB), by = syrk_bytes(m, kdep);
        KTime* kt = small ? slot(ctx, 6, 0) : slot(ctx, 0, fl, by);
        if ((frc = timed_launch(ctx, ctx->prof_mode == 2 && !small, st, {0, fl, by, 0},
                                [&] { launch_bulk(st, ba, kt); })))
            return frc;
        if (st == sr) {
            HIPQ(ctx, hipEventRecord(ctx->ev_rest[nsplit & 1], sr));
            ++nsplit;
            rest_from = jr;
        }
        return 0;
    };
    int pend = -1;  // the super-panel not yet applied to the columns >= dcol (paired updates)
    int dcol = nt;
    for (int p = 0; p < nsp; ++p) {
        const int c0 = spc[(size_t)p], c1 = spc[(size_t)p + 1];
        const int kd = (c1 - c0) * NB;  // depth of super-panel p
        if (p + 1 < nsp) {
            if (p >= 1)
                HIPQ(ctx, hipStreamWaitEvent(sp, ctx->ev_R[(p - 1) & 1], 0));
            else
                HIPQ(ctx, hipStreamWaitEvent(sp, ctx->ev_gram2, 0));  // rest of the Gram built
            const int c2 = spc[(size_t)p + 2];
            // (SP p+1's columns in a split update's rest still in flight)
            if ((frc = wait_rest(sp, c2))) return frc;
            const int mla = nt - c1;
            const Panel pn{ctx->A + (int64_t)c0 * NB * lda, lda, 0};
            if (GAPLAC_CHAIN_SKIP >= 2 && !ctx->dry) {
            } else if (ctx->la_tiles_m > 0 && mla >= ctx->la_tiles_m && c2 - c1 == W && ctx->band_off.size() > (size_t)mla &&
                       !ctx->xr.mode) {
                // the lookahead as whole 128x128 tiles (the band list of SP p+1's columns):
                // less CU time than the quadrant kernel while the trailing matrix is large
                if ((frc = band_launch(ctx, sp, lda, nt, c1, pn, kd, true))) return frc;
            } else {
                launch_col_update(sp, ctx->A, lda, pn, nt, c1, c1, c2 - c1, kd, slot(ctx, 5, 0));
            }
            if ((frc = factor_superpanel(ctx, sp, N, lda, nt, c1, c2))) return frc;
            HIPQ(ctx, hipEventRecord(ctx->ev_P[(p + 1) & 1], sp));
        }
        HIPQ(ctx, hipStreamWaitEvent(sm, ctx->ev_P[p & 1], 0));
        // tile columns after SP p+1; the last super-panel also updates a serial tail
        const int jb = p + 2 <= nsp ? spc[(size_t)p + 2] : spc[(size_t)nsp];
        // Paired bulk updates (GAPLAC_PAIR_M): at a deferring step only the next-needed band
        // (SP p+2's columns; with GAPLAC_PAIR_EXT also SP p+3's) gets SP p, and the tile
        // columns after it get SPs p and p+1 in one K = 2 x 128W update at step p+1 (band
        // first, then R(p), then the rest). Columns >= dcol lack SP pend.
        const int je = p + 3 <= nsp ? spc[(size_t)p + 3] : spc[(size_t)nsp];
        const bool defer = pair_defer(ctx, spc, nt, p, pend);
        // a band [b0, b1) with the panel columns pc .. c1-1
        auto band = [&](int b0, int b1, int pc) -> int {
            if (b1 <= b0) return 0;
            if (int rc = wait_rest(sm, b1)) return rc;
            const Panel pn{ctx->A + (int64_t)pc * NB * lda, lda, 0};
            const int kb = (c1 - pc) * NB, mbd = nt - b0;
            // through the tile kernel (a list of the band's tiles; quadrants if small)
            if (b1 - b0 == W && ctx->band_off.size() > (size_t)mbd)
                return band_launch(ctx, sm, lda, nt, b0, pn, kb, mbd >= ctx->band_tiles_m);
            launch_col_update(sm, ctx->A, lda, pn, nt, b0, b0, b1 - b0, kb, slot(ctx, 5, 0));
            return 0;
        };
        // first panel column a band starting at tile column b0 still lacks: columns >= dcol
        // lack every super-panel from pend on, the others only this step's
        auto first_panel = [&](int b0) { return pend >= 0 && b0 >= dcol ? spc[(size_t)pend] : c0; };
        if (defer && pend >= 0) {
            // a deeper deferral (GAPLAC_PAIR_DEPTH > 2): the next-needed band gets this
            // step's panel, the band after it every panel from pend on
            if ((frc = band(jb, je, first_panel(jb)))) return frc;
            HIPQ(ctx, hipEventRecord(ctx->ev_R[p & 1], sm));
            const int e1 = ctx->pair_ext > 0 ? spc[(size_t)p + 4] : je;
            if ((frc = band(je, e1, first_panel(je)))) return frc;
            dcol = std::max(dcol, e1);
        } else if (defer) {
            if ((frc = band(jb, je, c0))) return frc;
            HIPQ(ctx, hipEventRecord(ctx->ev_R[p & 1], sm));
            dcol = ctx->pair_ext > 0 ? spc[(size_t)p + 4] : je;
            if ((frc = band(je, dcol, c0))) return frc;
            pend = p;
        } else if (pend >= 0) {
            if ((frc = band(jb, je, je <= dcol ? c0 : spc[(size_t)pend]))) return frc;
            HIPQ(ctx, hipEventRecord(ctx->ev_R[p & 1], sm));
            if ((frc = band(je, dcol, c0))) return frc;  // (not produced by the schedule above)
            const Panel pnl{ctx->A + (int64_t)spc[(size_t)pend] * NB * lda, lda, 0};
            if ((frc = bulk_tri(std::max(je, dcol), pnl, (c1 - spc[(size_t)pend]) * NB))) return frc;
            pend = -1;
        } else {
            if ((frc = bulk_tri(jb, Panel{ctx->A + (int64_t)c0 * NB * lda, lda, 0}, kd))) return frc;
            HIPQ(ctx, hipEventRecord(ctx->ev_R[p & 1], sm));
        }
        if (ctx->xr.mode) {
            // extra rows: they only need SP p final (P(p)) and touch rows no other stream
            // writes. s_extra takes SP p's column chain and then its update of SP p+1's
            // columns; the update of the columns after those (the bulk of the K = 128 W work)
            // goes on s_xrest, so the chain of SP p+1 runs beside it instead of after it
            // (DESIGN.md §9). Every tile still gets the SPs in order: the update of SP p+1's
            // columns waits for SP p-1's update of the columns after SP p, SP p's chain for
            // SP p-2's.
            hipStream_t sx = ctx->serial ? sm : ctx->s_extra;
            if (sx == sm) {
                extra_rows_chain(ctx, sx, lda, nt, c0, c1);
                extra_rows_update(ctx, sx, lda, nt, c0, c1, c1, nt);
            } else {
                hipStream_t sr = ctx->s_xrest;
                if (p >= 1) {  // SP p-1 on the columns after SP p
                    HIPQ(ctx, hipStreamWaitEvent(sr, ctx->ev_xc[(p - 1) & 1], 0));
                    extra_rows_update(ctx, sr, lda, nt, spc[(size_t)p - 1], c0, c1, nt);
                    HIPQ(ctx, hipEventRecord(ctx->ev_xr[(p - 1) & 1], sr));
                }
                HIPQ(ctx, hipStreamWaitEvent(sx, ctx->ev_P[p & 1], 0));
                if (p >= 2) HIPQ(ctx, hipStreamWaitEvent(sx, ctx->ev_xr[(p - 2) & 1], 0));
                extra_rows_chain(ctx, sx, lda, nt, c0, c1);
                HIPQ(ctx, hipEventRecord(ctx->ev_xc[p & 1], sx));
                if (p >= 1) HIPQ(ctx, hipStreamWaitEvent(sx, ctx->ev_xr[(p - 1) & 1], 0));
                extra_rows_update(ctx, sx, lda, nt, c0, c1, c1, p + 2 <= nsp ? spc[(size_t)p + 2] : nt);
            }
        }
    }
    if ((frc = wait_rest(sm, nt))) return frc;  // every split update's rest before the tail
    if (spc[(size_t)nsp] < nt) {
        const int ts = spc[(size_t)nsp], T = nt - ts;
        // dense extra rows: factored along inside the tail
        const int X = dense_rows(ctx) ? ctx->xr.tiles : 0;
        if (ctx->tailk && T + X <= TAIL_TMAX && (ctx->xr.mode == 0 || X > 0)) {
            // the tail as one persistent dataflow launch
            // the extra rows' super-panel updates of the tail's columns land first
            if ((frc = join_extra_streams(ctx, sm))) return frc;
            const bool gram = ts == 0 && gram_in_tail(ctx, nt, lda);
            if (ctx->dry) {  // gaplac_plan_check: the task list's dependency order
                std::vector<uint32_t> host;
                build_single_tail_list(T, X, ctx->tail_sim, 0, host, gram);
                std::string why;
                if (!check_tail_tasks(T, host, &why, X, gram)) return set_err(ctx, GAPLAC_E_ARG, "%s", why.c_str());
            }
            if ((ctx->ttasks_T != T || ctx->ttasks_X != X || ctx->ttasks_G != gram) && !ctx->dry) {
                std::vector<uint32_t> host;
                build_single_tail_list(T, X, ctx->tail_sim, std::max(1, ctx->ncu / std::max(1, ctx->tail_share)), host,
                                       gram);
                int rc;
                if ((rc = ensure(ctx, &ctx->ttasks, &ctx->ttasks_elems, host.size()))) return rc;
                HIPCK(ctx, hipMemcpy(ctx->ttasks, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
                ctx->ttasks_T = T;
                ctx->ttasks_X = X;
                ctx->ttasks_G = gram;
                ctx->ttasks_n = (int)host.size();
            }
            if (!ctx->tctl && !ctx->dry)
                HIPCK(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->tctl), sizeof(TailCtl)));
            if (!gram) HIPQ(ctx, hipMemsetAsync(ctx->tctl, 0, sizeof(TailCtl), sm));  // (gram: zeroed at the start)
            const int nts = ctx->dry ? (int)(T * (T + 1) * (T + 2) / 6 + 3 * T * T + X * T * (T + 3) / 2 +
                                             (gram ? T * (T + 1) / 2 : 0))
                                     : ctx->ttasks_n;
            if (!ctx->ttrace_path.empty() && !ctx->dry) {
                int rc;
                if ((rc = ensure(ctx, &ctx->ttrace, &ctx->ttrace_elems, 3 * (size_t)nts + (size_t)TAIL_DSTAMPS * T)))
                    return rc;
            }
            TailArgs ta{ctx->A, lda, N, ts, T, ctx->Dinv, ctx->dres, ctx->tctl, ctx->ttasks, nts,
                        ctx->ttrace_path.empty() ? nullptr : ctx->ttrace};
            ta.fault = ctx->tail_fault;
            ta.xrows = X;
            if (gram) {  // the inputs the Gram launches would have read (enqueue_eval_body)
                ta.gX = ctx->dX;
                ta.gldx = N;
                ta.gv = ctx->dv;
                ta.gtp = ctx->dtp;
            }
            // batch lanes run their tails side by side: each persistent grid takes its share
            // of the CUs (one tail workgroup fills a CU's LDS), so no tail waits for another
            launch_tail(sm, ta, std::min(std::max(1, ctx->ncu / std::max(1, ctx->tail_share)), nts), slot(ctx, 10, 0));
        } else {
            serial_tail(ctx, sm, N, lda, nt, ts);
        }
    }
    if ((frc = join_extra_streams(ctx, sm))) return frc;
    launch_reduce(sm, ctx->A, lda, N, (int64_t)nt * NB, ColMap{1, 0, 1}, ctx->dres);
    HIPQ(ctx, hipGetLastError());
    return 0;
}

// Where the packed lists of ctx->tiles lie for nt tile columns (set in ctx; returns their
// total length): tile_off[m] the m x m triangle's list, m = 1..nt, then band_off[m] the band
// list of an m-row trailing matrix (its first spw tile columns, rows r >= c, rows outer).
size_t set_tile_layout(gaplac_ctx* ctx, int nt) {
    size_t k = 0;
    ctx->tile_off.assign((size_t)nt + 1, 0);
    for (int m = 1; m <= nt; ++m) {
        ctx->tile_off[(size_t)m] = k;
        k += (size_t)m * (m + 1) / 2;
    }
    ctx->band_off.assign((size_t)nt + 1, k);
    for (int m = 1; m <= nt; ++m) {
        const size_t w = (size_t)std::min(ctx->spw, m);
        ctx->band_off[(size_t)m] = k;
        k += w * m - w * (w - 1) / 2;
    }
    return k;
}

// Upload the super-tile ordered lists for every triangle size m = 1..nt (once per nt).
int ensure_tile_lists(gaplac_ctx* ctx, int nt) {
    if (ctx->tiles_nt >= nt) return 0;
    ctx->tiles_nt = 0;  // (until the upload below has succeeded)
    const size_t total = set_tile_layout(ctx, nt);
    std::vector<uint32_t> host(total);
    for (int m = 1; m <= nt; ++m) {
        build_tile_list(m, host.data() + ctx->tile_off[(size_t)m]);
        size_t k = ctx->band_off[(size_t)m];
        for (int r = 0; r < m; ++r)
            for (int c = 0; c < ctx->spw && c <= r; ++c) host[k++] = (uint32_t)r | ((uint32_t)c << 16);
    }
    int rc;
    if ((rc = ensure(ctx, &ctx->tiles, &ctx->tiles_elems, total))) return rc;
    HIPCK(ctx, hipMemcpy(ctx->tiles, host.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->tiles_nt = nt;
    return 0;
}

// The gradient's ending after a factorisation with identity rows (Y = L^{-T} below the factor,
// lda = 2 Np): the contraction of alpha alpha^T - Y Y^T with every dC/dtheta into ctx->gout and
// its pinned copy. alpha == nullptr (gaplac_logpdf_grad): alpha = Y z from the factor's row N,
// into ctx->galpha. Else (the Laplace gradient, whose Y is scaled to Y Y^T = R, DESIGN.md
// §10.14): the caller's vector, final on s_main.
int enqueue_grad_ending(gaplac_ctx* ctx, int64_t N, int64_t Np, int64_t lda, const double* alpha) {
    int rc;
    // Fused (single-term groups): alpha = Y z first (HBM-bound, ~0.2 ms alone), then M =
    // -C^{-1} tile by tile contracted in place with every dC/dtheta (cinv_contract_kernel:
    // the tile is never stored nor read back), all on s_main.
    // Else (or GAPLAC_GRAD_FUSED=0): alpha on s_extra beside M over the factor storage on
    // s_main (both only read Y; z is copied out first, cinv may overwrite row N), then the
    // contraction on s_main once alpha is in. Both end in the fixed-order reduction.
    const bool fused = ctx->grad_fused && ctx->xr.singletons;
    hipStream_t sm = ctx->s_main;
    hipStream_t sx = fused || ctx->serial || alpha ? sm : ctx->s_extra;  // alpha's stream
    const int m = (int)((N + NB - 1) / NB);
    launch_zero_tail_cols(sm, ctx->A, lda, Np, N);
    if (!alpha) {
        launch_copy_z(sm, ctx->A, lda, N, ctx->gz);
        if (sx != sm) {
            HIPQ(ctx, hipEventRecord(ctx->ev_xinit, sm));
            HIPQ(ctx, hipStreamWaitEvent(sx, ctx->ev_xinit, 0));
        }
        launch_alpha(sx, ctx->A, lda, Np, N, ctx->gz, ctx->gpart, ctx->galpha, ctx->gdv);
        if (sx != sm) HIPQ(ctx, hipEventRecord(ctx->ev_xdone, sx));
        alpha = ctx->galpha;
    }
    if ((rc = timed_launch(ctx, ctx->prof_mode == 2, sm, {0, 0.0, 0.0, 8}, [&] {
             if (fused)
                 launch_cinv_contract(sm, ctx->A, lda, Np, N, ctx->dX, N, alpha, ctx->dtp, ctx->glist,
                                      ctx->glist_blocks, ctx->gpart, slot(ctx, 8, 0));
             else
                 launch_cinv_tiles(sm, ctx->A, lda, Np, ctx->glist, ctx->glist_blocks, m, slot(ctx, 8, 0));
         })))
        return rc;
    if (!fused) {
        if (sx != sm) HIPQ(ctx, hipStreamWaitEvent(sm, ctx->ev_xdone, 0));
        launch_grad_contract(sm, ctx->A, lda, N, ctx->dX, N, alpha, ctx->dtp, ctx->dgp, ctx->gpart,
                             slot(ctx, 9, 0));
    }
    launch_grad_reduce(sm, ctx->gpart, m * (m + 1) / 2, ctx->htp->T, ctx->gout);
    HIPQ(ctx, hipMemcpyAsync(ctx->hgout, ctx->gout, sizeof(double) * (GAPLAC_MAX_TERMS + 1),
                              hipMemcpyDeviceToHost, sm));
    return 0;
}

// Everything one evaluation puts on the streams (eager launch or graph capture): reset
// the result record (and the profiling slots), Gram build, factorisation schedule,
// reduction, result copy to the pinned host record. Inputs: ctx->dX (ld N), ctx->dv,
// ctx->dtp.
int enqueue_eval_body(gaplac_ctx* ctx, int64_t N, int32_t D, int64_t Np, int nt) {
    const int64_t lda = Np + (int64_t)NB * ctx->xr.tiles;
    const bool gram_tail = gram_in_tail(ctx, nt, lda);
    if (gram_tail && !ctx->tctl && !ctx->dry) HIPCK(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->tctl), sizeof(TailCtl)));
    if (gram_tail)  // the tail's counters zeroed here (factor_and_reduce then skips its memset)
        launch_init_result_ctl(ctx->s_main, ctx->dres, ctx->tctl, *ctx->htp, ctx->dtp);
    else
        launch_init_result(ctx->s_main, ctx->dres);
    if (ctx->recording) launch_kt_reset(ctx->s_main, ctx->dkt, (int)ctx->kt_cap);
    // Gram in two launches: the first super-panel's tile columns, then the rest (the panel
    // chain starts on the first part while the second is still being written; the second as
    // a work queue of two workgroups per CU, so the chain's kernels fit beside it, §4).
    auto tri = [](double m) { return m * (m + 1) / 2; };
    const double bpt = 8.0 * NB * NB;  // bytes per tile
    const double b1 = bpt * (tri(nt) - tri(std::max(0, nt - ctx->spw))) + 8.0 * (double)N * (D + 1);
    const double b2 = bpt * tri(std::max(0, nt - ctx->spw));
    if (ctx->xr.prebuilt) {
        // the matrix is already in the workspace (post_cov_kernel, earlier on s_main): the panel
        // stream's two waits for the Gram hold behind it
        HIPQ(ctx, hipEventRecord(ctx->ev_gram, ctx->s_main));
        HIPQ(ctx, hipEventRecord(ctx->ev_gram2, ctx->s_main));
    } else if (!gram_tail) {  // (else the tail's first tasks build it)
        launch_gram(ctx->s_main, ctx->A, lda, N, nt, ctx->dX, N, ctx->dv, ctx->dtp, 1, ctx->spw, slot(ctx, 1, b1));
        HIPQ(ctx, hipEventRecord(ctx->ev_gram, ctx->s_main));
        launch_gram_queue(ctx->s_main, ctx->A, lda, N, nt, ctx->dX, N, ctx->dv, ctx->dtp, ctx->spw, nt, 2, ctx->dres,
                          slot(ctx, 1, b2));
        HIPQ(ctx, hipEventRecord(ctx->ev_gram2, ctx->s_main));
    }
    if (ctx->xr.mode == 1) launch_init_identity_rows(ctx->s_main, ctx->A, lda, Np, nt, ctx->spw);
    if (ctx->xr.mode == 2)
        launch_cross_gram(ctx->s_main, ctx->A, lda, Np, nt, N, ctx->xr.M, ctx->xr.tiles, ctx->dX, N, ctx->dXs,
                          ctx->xr.comp ? ctx->xr.sel.Mc : ctx->xr.M, ctx->dtp, ctx->xr.comp ? &ctx->xr.sel : nullptr);
    if (ctx->xr.mode == 3)
        launch_rows_from_matrix(ctx->s_main, ctx->A, lda, Np, nt, N, ctx->xr.M, ctx->xr.tiles, ctx->xr.Y,
                                ctx->xr.ldy, ctx->xr.sub);
    if (ctx->xr.mode && !ctx->serial) {  // the extra-row stream starts after their init
        HIPQ(ctx, hipEventRecord(ctx->ev_xinit, ctx->s_main));
        HIPQ(ctx, hipStreamWaitEvent(ctx->s_extra, ctx->ev_xinit, 0));
    }
    int rc;
    if ((rc = factor_and_reduce(ctx, N, lda, nt))) return rc;
    if (ctx->xr.mode == 2)
        launch_posterior(ctx->s_main, ctx->A, lda, Np, N, ctx->xr.M, ctx->dXs,
                         ctx->xr.comp ? ctx->xr.sel.Mc : ctx->xr.M, ctx->dtp, ctx->gpart, ctx->pmean, ctx->pvar,
                         ctx->xr.comp ? &ctx->xr.sel : nullptr);
    if (ctx->xr.mode == 3)
        launch_quad_rows(ctx->s_main, ctx->A, lda, Np, N, ctx->xr.M, ctx->dres, ctx->gpart, ctx->mres,
                         ctx->mres ? ctx->mres + ctx->xr.M : nullptr /* (a dry walk has no buffers) */);
    if (ctx->xr.mode == 1 && !ctx->xr.defer_ending && (rc = enqueue_grad_ending(ctx, N, Np, lda, nullptr))) return rc;
    HIPQ(ctx, hipMemcpyAsync(ctx->hres, ctx->dres, offsetof(EvalResult, part), hipMemcpyDeviceToHost,
                              ctx->s_main));
    return 0;
}

// The schedule under a footprint guard over ctx->A (unless the caller installed one, as
// gaplac_plan_check's dry run does): a launch whose grid would touch elements outside
// the workspace is not enqueued and the evaluation fails with GAPLAC_E_ARG.
int enqueue_eval(gaplac_ctx* ctx, int64_t N, int32_t D, int64_t Np, int nt) {
    LaunchGuard local;
    LaunchGuard* g = current_guard();
    const bool own = g == nullptr;
    if (own) {
        local.base = ctx->A;
        local.elems = (int64_t)ctx->A_elems;
        g = &local;
    }
    GuardScope scope(g);
    const int64_t v0 = g->violations;
    const int rc = enqueue_eval_body(ctx, N, D, Np, nt);
    if (rc) return rc;
    if (g->violations > v0)
        return set_err(ctx, GAPLAC_E_ARG, "launch footprint outside the workspace (N=%lld): %s", (long long)N,
                       g->first.c_str());
    return 0;
}

// The optional streams (lowest priority, like s_main), created when first wanted and kept:
// the only creation site besides gaplac_ctx_create's two base streams. Stream budget (a
// process gets 4 hardware queues by default; streams beyond them share a queue and may
// serialise behind one another):
//   plain logpdf context, no split (split_wanted)    2  s_main, s_panel
//   plain logpdf context at a split size             3  + s_xrest
//   gradient / posterior context                     4  + s_extra, s_xrest (the measured 79.4 ->
//                                                       78.0 ms of DESIGN.md §9 had no other stream busy)
//   two batch lanes (contexts), no split / split     4 / 6
// The batch lanes were measured at N = 8192 only (no split, 4 streams); no
// batch-lane measurement at a split size exists.
int ensure_streams(gaplac_ctx* ctx, bool want_extra, bool want_xrest) {
    int least = 0, greatest = 0;
    for (hipStream_t* s : {want_extra ? &ctx->s_extra : nullptr, want_xrest ? &ctx->s_xrest : nullptr}) {
        if (!s || *s) continue;
        HIPCK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCK(ctx, hipStreamCreateWithPriority(s, hipStreamNonBlocking, least));
    }
    return 0;
}

// Workspace for order N (grown on demand).
int ensure_workspace(gaplac_ctx* ctx, int64_t N) {
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    int rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, &ctx->A, &ctx->A_elems, (size_t)(Np + (int64_t)NB * ctx->xr.tiles) * Np))) return rc;
    // the extra rows take both optional streams; the split bulk updates of a plain evaluation
    // (factor_and_reduce) take s_xrest, which would idle there
    if ((rc = ensure_streams(ctx, ctx->xr.mode != 0, ctx->xr.mode != 0 || split_wanted(ctx, nt)))) return rc;
    if (ctx->xr.mode == 2) {
        const size_t M = (size_t)ctx->xr.M;
        if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, 2 * M * (size_t)((N + 511) / 512)))) return rc;
        if (ctx->pmv_elems < M) {
            if (ctx->pmean) (void)hipFree(ctx->pmean);
            if (ctx->pvar) (void)hipFree(ctx->pvar);
            ctx->pmean = ctx->pvar = nullptr;
            ctx->pmv_elems = 0;
            if (hipMalloc(reinterpret_cast<void**>(&ctx->pmean), M * 8) != hipSuccess ||
                hipMalloc(reinterpret_cast<void**>(&ctx->pvar), M * 8) != hipSuccess)
                return set_err(ctx, GAPLAC_E_OOM, "hipMalloc of posterior outputs failed");
            ctx->pmv_elems = M;
        }
    }
    if (ctx->xr.mode == 3) {
        const size_t R = (size_t)ctx->xr.M;
        if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, R * (size_t)((N + 511) / 512)))) return rc;
        if ((rc = ensure(ctx, &ctx->mres, &ctx->mres_elems, 2 * R))) return rc;
    }
    if (ctx->xr.mode == 1) {
        const int m = (int)((N + NB - 1) / NB);
        const size_t nk = (size_t)((N + 511) / 512);
        const size_t part = std::max(nk * (size_t)N, (size_t)m * (m + 1) / 2 * (GAPLAC_MAX_TERMS + 1));
        if ((rc = ensure(ctx, &ctx->galpha, &ctx->galpha_elems, (size_t)N))) return rc;
        if ((rc = ensure(ctx, &ctx->gdv, &ctx->gdv_elems, (size_t)N))) return rc;
        if ((rc = ensure(ctx, &ctx->gz, &ctx->gz_elems, (size_t)N))) return rc;
        if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, part))) return rc;
        if (ctx->glist_m != m) {
            std::vector<uint32_t> host;
            build_grad_list(m, host);
            if ((rc = ensure(ctx, &ctx->glist, &ctx->glist_elems, host.size()))) return rc;
            HIPCK(ctx, hipMemcpy(ctx->glist, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            ctx->glist_m = m;
            ctx->glist_blocks = (int)host.size();
        }
    }
    if ((rc = ensure(ctx, &ctx->Dinv, &ctx->Dinv_elems, (size_t)nt * DINV_PER_BLOCK))) return rc;
    return ensure_tile_lists(ctx, nt);
}

// The one writer of ctx->xr: the description holds for as long as this lives (one evaluation's
// enqueue, or one dry walk) and "none" is back on every way out.
struct EvalScope {
    gaplac_ctx* c;
    EvalScope(gaplac_ctx* ctx, const ExtraRows& xr) : c(ctx) { c->xr = xr; }
    ~EvalScope() { c->xr = ExtraRows{}; }
};

// Eager enqueue of one evaluation (no profiling, no wait): the batch lanes.
int eval_enqueue(gaplac_ctx* ctx, int64_t N, int32_t D, const TermPack& tp) {
    EvalScope scope(ctx, ExtraRows{});
    int rc;
    if ((rc = ensure_workspace(ctx, N))) return rc;
    const int64_t Np = round_up(N + 1, NB);
    *ctx->htp = tp;
    if (!tp_by_init(ctx, N))
        HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    ctx->slots.clear();
    ctx->recording = false;
    return enqueue_eval(ctx, N, D, Np, (int)(Np / NB));
}

int eval_wait(gaplac_ctx* ctx, EvalResult* out) {
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    *out = *ctx->hres;
    if (out->err) return set_err(ctx, GAPLAC_E_HIP, "in-kernel wait expired (code %u)", out->err);
    return 0;
}

// Full evaluation; inputs already in ctx->dX (ld N) / ctx->dv, term pack in tp (host), the
// riding rows (and whether the matrix is prebuilt) in xr. Leaves the factor in ctx->A.
int eval_device(gaplac_ctx* ctx, int64_t N, int32_t D, const TermPack& tp, const ExtraRows& xr, EvalResult* out) {
    EvalScope scope(ctx, xr);
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    int rc;
    if ((rc = ensure_workspace(ctx, N))) return rc;
    const bool prof = ctx->prof_mode == 1;
    if (prof) {
        const size_t need = (size_t)nt * 9 + 32;  // launches per evaluation, with margin
        if (ctx->kt_cap < need) {
            if ((rc = ensure(ctx, &ctx->dkt, &ctx->kt_cap, need))) return rc;
            if (ctx->hkt) (void)hipHostFree(ctx->hkt);
            ctx->hkt = nullptr;
            HIPCK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->hkt), ctx->kt_cap * sizeof(KTime), 0));
        }
    }
    *ctx->htp = tp;
    if (!tp_by_init(ctx, N))
        HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    ctx->slots.clear();
    ctx->recording = prof;
    rc = enqueue_eval(ctx, N, D, Np, nt);
    ctx->recording = false;
    if (rc) return rc;
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    *out = *ctx->hres;
    if (out->err) return set_err(ctx, GAPLAC_E_HIP, "in-kernel wait expired (code %u)", out->err);
    if (!ctx->ttrace_path.empty() && ctx->ttrace && ctx->ttasks_n > 0) {  // diagnostics: task timeline
        std::vector<unsigned long long> tr(3 * (size_t)ctx->ttasks_n);
        std::vector<uint32_t> tk((size_t)ctx->ttasks_n);
        HIPCK(ctx, hipMemcpy(tr.data(), ctx->ttrace, tr.size() * 8, hipMemcpyDeviceToHost));
        HIPCK(ctx, hipMemcpy(tk.data(), ctx->ttasks, tk.size() * 4, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(ctx->ttrace_path.c_str(), "a")) {
            std::fprintf(f, "# N=%lld T=%d tasks=%d\n", (long long)N, ctx->ttasks_T, ctx->ttasks_n);
            for (size_t i = 0; i < tk.size(); ++i)
                std::fprintf(f, "%zu %u %llu %llu %llu\n", i, tk[i], tr[3 * i], tr[3 * i + 1], tr[3 * i + 2]);
            std::fclose(f);
        }
        // the diagonal blocks' phase times (potrf_diag2_body), one line per tile column
        std::vector<unsigned long long> ds((size_t)TAIL_DSTAMPS * ctx->ttasks_T);
        HIPCK(ctx, hipMemcpy(ds.data(), ctx->ttrace + 3 * (size_t)ctx->ttasks_n, ds.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen((ctx->ttrace_path + ".d").c_str(), "a")) {
            std::fprintf(f, "# N=%lld T=%d\n", (long long)N, ctx->ttasks_T);
            for (int k = 0; k < ctx->ttasks_T; ++k) {
                std::fprintf(f, "%d", k);
                for (int i = 0; i < TAIL_DSTAMPS; ++i) std::fprintf(f, " %llu", ds[(size_t)TAIL_DSTAMPS * k + i]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
    }
    if (prof) {
        rc = accumulate_slots(ctx, ctx->slots);
        ctx->slots.clear();
    }
    return rc;
}

int finish(const EvalResult& r, double* out_logpdf, double* out_logdet, double* out_quad) {
    if (out_logdet) *out_logdet = r.logdet;
    if (out_quad) *out_quad = r.quad;
    if (r.info != ~0ull) {
        if (out_logpdf) *out_logpdf = NAN;
        return (int)(r.info > 0x7fffffffull ? 0x7fffffff : r.info);
    }
    if (out_logpdf) *out_logpdf = r.logpdf;
    return 0;
}

// The inputs into the context's buffers (ld N), from the host or, for the _device entries,
// from device memory: a ~N*(D+1)*8-byte D2D copy that keeps the captured graph's pointers fixed.
int upload(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, const double* v,
           hipMemcpyKind kind = hipMemcpyHostToDevice) {
    int rc;
    const size_t nx = (size_t)N * (size_t)(D > 0 ? D : 1);
    if ((rc = ensure(ctx, &ctx->dX, &ctx->dX_elems, nx))) return rc;
    if ((rc = ensure(ctx, &ctx->dv, &ctx->dv_elems, (size_t)N))) return rc;
    if (D > 0)
        HIPCK(ctx, hipMemcpy2DAsync(ctx->dX, (size_t)N * 8, X, (size_t)ldx * 8, (size_t)N * 8, (size_t)D, kind,
                                    ctx->s_main));
    HIPCK(ctx, hipMemcpyAsync(ctx->dv, v, (size_t)N * 8, kind, ctx->s_main));
    return 0;
}

void nan_out(double* a, double* b, double* c) {
    if (a) *a = NAN;
    if (b) *b = NAN;
    if (c) *c = NAN;
}

// Test inputs into ctx->dXs (ld rows): rows [r0, r0 + m) from the host block Xs (ld ldxs).
int upload_test_inputs(gaplac_ctx* ctx, int32_t D, int64_t rows, int64_t r0, int64_t m, const double* Xs,
                       int64_t ldxs) {
    int rc;
    if ((rc = ensure(ctx, &ctx->dXs, &ctx->dXs_elems, (size_t)rows * (size_t)(D > 0 ? D : 1)))) return rc;
    if (D > 0 && m > 0)
        HIPCK(ctx, hipMemcpy2DAsync(ctx->dXs + r0, (size_t)rows * 8, Xs, (size_t)ldxs * 8, (size_t)m * 8, (size_t)D,
                                    hipMemcpyHostToDevice, ctx->s_main));
    return 0;
}

// Launches outside an evaluation, under a footprint guard over ctx->A (with_B: and ctx->B as its
// second region): a launch whose grid would leave them is not enqueued and the entry fails.
template <typename Launches>
int guarded_on(gaplac_ctx* ctx, const double* base, size_t elems, const double* base2, size_t elems2,
               Launches&& launches, const double* base3 = nullptr, size_t elems3 = 0);
template <typename Launches>
int guarded(gaplac_ctx* ctx, bool with_B, Launches&& launches) {
    return guarded_on(ctx, ctx->A, ctx->A_elems, with_B ? ctx->B : nullptr, with_B ? ctx->B_elems : 0, launches);
}
// The same over any two (or three) allocations (the second and third may be null).
template <typename Launches>
int guarded_on(gaplac_ctx* ctx, const double* base, size_t elems, const double* base2, size_t elems2,
               Launches&& launches, const double* base3, size_t elems3) {
    LaunchGuard g{base, (int64_t)elems, base2, (int64_t)elems2, base3, (int64_t)elems3};
    {
        GuardScope scope(&g);
        launches();
    }
    if (g.violations)
        return set_err(ctx, GAPLAC_E_ARG, "launch footprint outside the workspace: %s", g.first.c_str());
    HIPCK(ctx, hipGetLastError());
    return 0;
}

// Diagnostics (GAPLAC_TAIL_TRACE): `stage` on s_main between two hipEvents, "a b ms" of it alone
// appended to <trace path><ext>; without a trace path, `stage` and nothing else.
template <typename Stage>
int trace_timed(gaplac_ctx* ctx, const char* ext, int64_t a, int64_t b, Stage&& stage) {
    if (ctx->ttrace_path.empty()) return stage();
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Owner {  // the events end with this call, whichever way it returns
        hipEvent_t* e;
        ~Owner() {
            for (int i = 0; i < 2; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } owner{ev};
    HIPCK(ctx, hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) return set_err(ctx, GAPLAC_E_HIP, "hipEventCreate failed");
    (void)hipEventRecord(ev[0], ctx->s_main);
    if (int rc = stage()) return rc;
    float ms = 0.f;
    const bool ok = hipEventRecord(ev[1], ctx->s_main) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
                    hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess;
    if (FILE* f = ok ? std::fopen((ctx->ttrace_path + ext).c_str(), "a") : nullptr) {
        std::fprintf(f, "%lld %lld %.6f\n", (long long)a, (long long)b, (double)ms);
        std::fclose(f);
    }
    return 0;
}

// k(x_j, x_j) of row j of a host matrix (the prior variance; a NOISE term counts). With a
// selector: of component g alone (a term outside it contributes the factor 0.0). noise_groups:
// the product groups that hold a NOISE term alone (0 across point sets: the diagonal part of K
// that a matrix-free product leaves out).
constexpr bool NOISE_GROUPS_ONLY = true;  // host_kdiag's last argument
double host_kdiag(const TermPack& tp, const double* X, int64_t ldx, int64_t j, const CompSel* sel = nullptr,
                  int32_t g = 0, bool noise_groups = false) {
    double kd = 0.0, pr = 1.0;
    bool has_noise = false;
    for (int t = 0; t < tp.T; ++t) {
        const double x = tp.kind[t] == GAPLAC_NOISE ? 0.0 : X[(int64_t)tp.col[t] * ldx + j];
        double k = 1.0;  // CAT: kappa(d) = d > 0 ? 0 : 1 is 1 at any x, NaN included
        // SQEXP / OU: exp(0) with u - u = 0, or NaN where the scaled coordinate u = x / l is not finite
        // (u - u is NaN: the Gram's diagonal there)
        if ((tp.kind[t] == GAPLAC_SQEXP || tp.kind[t] == GAPLAC_OU) && !std::isfinite(tp.p[t] * x)) k = NAN;
        if (tp.kind[t] == GAPLAC_LINEAR) k = x * x + tp.p[t];
        if (tp.kind[t] == GAPLAC_NOISE) {
            k = tp.p[t];
            has_noise = true;
        }
        pr *= !sel || sel->comp[t] == g ? k : 0.0;
        if (tp.last_in_group[t]) {
            if (has_noise || !noise_groups) kd += pr;
            pr = 1.0;
            has_noise = false;
        }
    }
    return kd;
}

// Shared body of gaplac_logpdf / _device.
int logpdf_impl(gaplac_ctx* ctx, bool on_device, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                const gaplac_term* terms, double noise, const double* v, double* out_logpdf, double* out_logdet,
                double* out_quad) {
    nan_out(out_logpdf, out_logdet, out_quad);
    int rc = check_common(ctx, N, D, X, ldx, noise, v);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (N == 0) {  // logpdf of an empty FiniteGP: -(0 + 0 + 0)/2
        if (out_logpdf) *out_logpdf = -0.0;
        if (out_logdet) *out_logdet = 0.0;
        if (out_quad) *out_quad = 0.0;
        return 0;
    }
    tp.noise = noise;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, v, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice))) return rc;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows{}, &r))) return rc;
    return finish(r, out_logpdf, out_logdet, out_quad);
}

// The product groups' bounds per term (terms validated by pack_terms: groups are contiguous);
// true when every group is a single term.
bool pack_groups(int32_t T, const gaplac_term* terms, GradTermPack* gp) {
    bool singletons = true;
    for (int t = 0; t < T; ++t) {
        int a = t, b = t + 1;
        while (a > 0 && terms[a - 1].group == terms[t].group) --a;
        while (b < T && terms[b].group == terms[t].group) ++b;
        gp->gstart[t] = a;
        gp->gend[t] = b;
        singletons = singletons && b - a == 1;
    }
    return singletons;
}

// Shared body of gaplac_logpdf_grad / _device.
int logpdf_grad_impl(gaplac_ctx* ctx, bool on_device, int64_t N, int32_t D, const double* X, int64_t ldx,
                     int32_t T, const gaplac_term* terms, double noise, const double* v, double* out_logpdf,
                     double* out_dv, double* out_dparam, double* out_dnoise) {
    if (out_logpdf) *out_logpdf = NAN;
    if (out_dnoise) *out_dnoise = NAN;
    if (out_dparam && T > 0)
        for (int t = 0; t < T && t < GAPLAC_MAX_TERMS; ++t) out_dparam[t] = NAN;
    if (out_dv)
        for (int64_t i = 0; i < N; ++i) out_dv[i] = NAN;
    int rc = check_common(ctx, N, D, X, ldx, noise, v);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (N == 0) {
        if (out_logpdf) *out_logpdf = -0.0;
        if (out_dnoise) *out_dnoise = 0.0;
        if (out_dparam)
            for (int t = 0; t < T; ++t) out_dparam[t] = 0.0;
        return 0;
    }
    GradTermPack gp{};
    const bool singletons = pack_groups(T, terms, &gp);
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, v, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice))) return rc;
    tp.noise = noise;
    *ctx->hgp = gp;
    HIPCK(ctx, hipMemcpyAsync(ctx->dgp, ctx->hgp, sizeof(GradTermPack), hipMemcpyHostToDevice, ctx->s_main));
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows::identity(N, singletons), &r))) return rc;
    rc = finish(r, out_logpdf, nullptr, nullptr);
    if (rc) return rc;  // PosDefException: gradients stay NaN
    if (out_dv) HIPCK(ctx, hipMemcpy(out_dv, ctx->gdv, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    if (out_dparam)
        for (int t = 0; t < T; ++t) out_dparam[t] = ctx->hgout[t];
    if (out_dnoise) *out_dnoise = ctx->hgout[T];
    return 0;
}

// Shared body of gaplac_posterior_mean_var.
int posterior_impl(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                   const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                   int64_t ldxs, double* out_mean, double* out_var) {
    for (int64_t j = 0; j < M; ++j) {
        if (out_mean) out_mean[j] = NAN;
        if (out_var) out_var[j] = NAN;
    }
    int rc = check_common(ctx, N, D, X, ldx, noise, y);
    if (rc) return rc;
    if (M < 0 || (M > 0 && D > 0 && (!Xs || ldxs < M)))
        return set_err(ctx, GAPLAC_E_ARG, "M < 0, or Xs NULL / ldxs < M");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (M == 0) return 0;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if (N == 0) {  // posterior of an empty FiniteGP = the prior: mean 0, var kdiag
        for (int64_t j = 0; j < M; ++j) {
            if (out_mean) out_mean[j] = 0.0;
            if (out_var) out_var[j] = host_kdiag(tp, Xs, ldxs, j);
        }
        return 0;
    }
    if ((rc = upload(ctx, N, D, X, ldx, y))) return rc;
    if ((rc = upload_test_inputs(ctx, D, M, 0, M, Xs, ldxs))) return rc;
    tp.noise = noise;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows::test_points(M), &r))) return rc;
    rc = finish(r, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (out_mean) HIPCK(ctx, hipMemcpy(out_mean, ctx->pmean, (size_t)M * 8, hipMemcpyDeviceToHost));
    if (out_var) HIPCK(ctx, hipMemcpy(out_var, ctx->pvar, (size_t)M * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Body of gaplac_posterior_components: the posterior evaluation with the
// G components' cross-covariances as G * M packed riding rows (ExtraRows::components).
int posterior_components_impl(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                              int64_t ldxs, int32_t G, const int32_t* comp, double* out_mean, int64_t ldm,
                              double* out_var, int64_t ldv) {
    if (!ctx) return GAPLAC_E_ARG;
    if (G < 0 || M < 0 || (out_mean && ldm < M) || (out_var && ldv < M))
        return set_err(ctx, GAPLAC_E_ARG, "G < 0, M < 0, or ldm / ldv < M");
    for (int32_t g = 0; g < G; ++g)
        for (int64_t j = 0; j < M; ++j) {
            if (out_mean) out_mean[g * ldm + j] = NAN;
            if (out_var) out_var[g * ldv + j] = NAN;
        }
    int rc = check_common(ctx, N, D, X, ldx, noise, y);
    if (rc) return rc;
    if (M > 0 && D > 0 && (!Xs || ldxs < M)) return set_err(ctx, GAPLAC_E_ARG, "Xs NULL / ldxs < M");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (G > 0 && T > 0 && !comp) return set_err(ctx, GAPLAC_E_ARG, "comp is NULL");
    CompSel sel{};
    sel.Mc = M;
    sel.G = G;
    for (int t = 0; t < GAPLAC_MAX_TERMS; ++t) sel.comp[t] = -1;
    for (int t = 0; comp && t < T; ++t) {
        if (comp[t] < -1 || comp[t] >= G)
            return set_err(ctx, GAPLAC_E_ARG, "comp[%d] = %d outside [-1, %d)", t, comp[t], G);
        sel.comp[t] = comp[t];
    }
    for (int t = 0; comp && t + 1 < T; ++t)
        if (!tp.last_in_group[t] && comp[t] != comp[t + 1])
            return set_err(ctx, GAPLAC_E_KIND, "terms %d and %d: one product group in two components", t, t + 1);
    if (G == 0 || M == 0) return 0;
    if (M > ((int64_t)65535 * NB) / G)  // the cross-covariance grid's tile rows
        return set_err(ctx, GAPLAC_E_OOM, "G * M = %d * %lld rows exceed 65535 tile rows", G, (long long)M);
    HIPCK(ctx, hipSetDevice(ctx->device));
    if (N == 0) {  // the prior per component: mean 0, var kdiag_g
        for (int32_t g = 0; g < G; ++g)
            for (int64_t j = 0; j < M; ++j) {
                if (out_mean) out_mean[g * ldm + j] = 0.0;
                if (out_var) out_var[g * ldv + j] = host_kdiag(tp, Xs, ldxs, j, &sel, g);
            }
        return 0;
    }
    if ((rc = upload(ctx, N, D, X, ldx, y))) return rc;
    if ((rc = upload_test_inputs(ctx, D, M, 0, M, Xs, ldxs))) return rc;
    tp.noise = noise;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows::components(sel), &r))) return rc;
    rc = finish(r, nullptr, nullptr, nullptr);
    if (rc) return rc;
    // (pmean / pvar hold the G columns packed, leading dimension M)
    if (out_mean)
        HIPCK(ctx, hipMemcpy2D(out_mean, (size_t)ldm * 8, ctx->pmean, (size_t)M * 8, (size_t)M * 8, (size_t)G,
                               hipMemcpyDeviceToHost));
    if (out_var)
        HIPCK(ctx, hipMemcpy2D(out_var, (size_t)ldv * 8, ctx->pvar, (size_t)M * 8, (size_t)M * 8, (size_t)G,
                               hipMemcpyDeviceToHost));
    return 0;
}

// Shared body of gaplac_logpdf_multi / _device: one factorisation, the R responses as
// dense extra rows (ExtraRows::responses). Column 0 also rides in row N as v (the evaluation's own
// quad is not used: all R results come from the extra rows, one code path per column).
int logpdf_multi_impl(gaplac_ctx* ctx, bool on_device, int64_t N, int32_t D, const double* X, int64_t ldx,
                      int32_t T, const gaplac_term* terms, double noise, int64_t R, const double* Y, int64_t ldy,
                      double* out_logpdf, double* out_logdet, double* out_quad) {
    if (!ctx) return GAPLAC_E_ARG;
    if (R < 0 || !out_logpdf) return set_err(ctx, GAPLAC_E_ARG, "R = %lld < 0 or out_logpdf NULL", (long long)R);
    auto fill = [&](double lp, double ld, double q) {
        for (int64_t r = 0; r < R; ++r) {
            out_logpdf[r] = lp;
            if (out_quad) out_quad[r] = q;
        }
        if (out_logdet && R > 0) *out_logdet = ld;
    };
    fill(NAN, NAN, NAN);
    int rc = check_common(ctx, N, D, X, ldx, noise, ctx /* v: the matrix is checked below */);
    if (rc) return rc;
    if (ldy < N || (R > 0 && N > 0 && !Y))
        return set_err(ctx, GAPLAC_E_ARG, "Y NULL or ldy %lld < N %lld", (long long)ldy, (long long)N);
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (R == 0) return 0;
    if (N == 0) {  // one empty FiniteGP per column
        fill(-0.0, 0.0, 0.0);
        return 0;
    }
    if ((R + NB - 1) / NB > 65535)  // (one grid row of the transposing launch per tile row)
        return set_err(ctx, GAPLAC_E_OOM, "R = %lld: more than 65535 tile rows in one call", (long long)R);
    tp.noise = noise;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, Y, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice))) return rc;
    if (!on_device) {
        if ((rc = ensure(ctx, &ctx->dY, &ctx->dY_elems, (size_t)N * (size_t)R))) return rc;
        HIPCK(ctx, hipMemcpy2DAsync(ctx->dY, (size_t)N * 8, Y, (size_t)ldy * 8, (size_t)N * 8, (size_t)R,
                                    hipMemcpyHostToDevice, ctx->s_main));
    }
    EvalResult r;
    const ExtraRows xr = on_device ? ExtraRows::responses(R, Y, ldy) : ExtraRows::responses(R, ctx->dY, N);
    if ((rc = eval_device(ctx, N, D, tp, xr, &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr))) return rc;  // PosDefException: every output stays NaN
    if (out_logdet) *out_logdet = r.logdet;
    if (out_quad) HIPCK(ctx, hipMemcpy(out_quad, ctx->mres, (size_t)R * 8, hipMemcpyDeviceToHost));
    HIPCK(ctx, hipMemcpy(out_logpdf, ctx->mres + R, (size_t)R * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- joint posterior at test points ----

// The second factorisation runs in B: A and B change places for as long as this lives.
// (Given another workspace, A changes places with that one: the sparse joint entries' third, §10.11.)
struct WsSwap {
    gaplac_ctx* c;
    double** w;
    size_t* w_elems;
    explicit WsSwap(gaplac_ctx* ctx) : WsSwap(ctx, &ctx->B, &ctx->B_elems) {}
    WsSwap(gaplac_ctx* ctx, double** other, size_t* other_elems) : c(ctx), w(other), w_elems(other_elems) { flip(); }
    ~WsSwap() { flip(); }
    void flip() {
        std::swap(c->A, *w);
        std::swap(c->A_elems, *w_elems);
    }
};

// Paddings and leading dimensions of the two workspaces, for the entries and for
// gaplac_plan_check_joint alike: A of order N with the M test points in mt riding tile rows, B of
// order M with R responses in rt riding tile rows (R = 0: none).
struct JointDims {
    int mt, rt;
    int64_t Np, Mp, lda, ldb;
};
JointDims joint_dims(int64_t N, int64_t M, int64_t R) {
    JointDims d;
    d.mt = (int)((M + NB - 1) / NB);
    d.rt = (int)((R + NB - 1) / NB);
    d.Np = round_up(N + 1, NB);
    d.Mp = round_up(M + 1, NB);
    d.lda = d.Np + (int64_t)NB * d.mt;
    d.ldb = d.Mp + (int64_t)NB * d.rt;
    return d;
}

// Stage 2's launches, run by joint_stages and walked dry by gaplac_plan_check_joint (Xs, mean and
// dtp may be null there): the augmented matrix of Sigma* into B (row M, the v row, carries the
// mean: its results are not used), and with `mirror` its upper triangle from the lower.
void joint_cov_launches(hipStream_t s, const JointDims& d, int64_t N, int64_t M, double* A, double* B,
                        const double* Xs, const double* mean, const TermPack* dtp, bool mirror) {
    launch_post_cov(s, A, d.lda, d.Np, N, M, B, d.ldb, Xs, M, mean, dtp);
    if (mirror) launch_mirror_lower(s, B, d.ldb, M);
}

// The draws O (N x R, ld N) = L Z (Z with the factor's leading dimension), plus `mean` per
// column when given: gaplac_rand_multi and gaplac_posterior_rand.
void draws_launches(hipStream_t s, const double* A, int64_t lda, int64_t N, const double* Z, int64_t R, double* O,
                    const double* mean) {
    launch_lower_mm(s, A, lda, N, Z, lda, R, O, N);
    if (mean) launch_add_mean(s, O, N, N, R, mean);
}

// Stages 1 and 2: the posterior evaluation (M test points: V^T below the factor, the mean in
// ctx->pmean), then, unless cov is Cov::none, the augmented matrix of Sigma* into ctx->B, laid
// out for a factorisation of order M with R riding responses (Cov::full: mirrored into a full
// matrix). tp comes in with the training noise and leaves with noise_s (the pack of stages 2 and
// 3, also in ctx->dtp).
enum class Cov { none, lower, full };
int joint_stages(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, TermPack& tp, const double* y,
                 int64_t M, const double* Xs, int64_t ldxs, double noise_s, int64_t R, Cov cov) {
    int rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, y))) return rc;
    if ((rc = upload_test_inputs(ctx, D, M, 0, M, Xs, ldxs))) return rc;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows::test_points(M), &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr)))
        return set_err(ctx, rc, "the training covariance K(X) + noise I is not positive definite (leading minor %d)", rc);
    if (cov == Cov::none) return 0;
    const JointDims d = joint_dims(N, M, R);
    if ((rc = ensure(ctx, &ctx->B, &ctx->B_elems, (size_t)d.ldb * (size_t)d.Mp))) return rc;
    tp.noise = noise_s;
    *ctx->htp = tp;  // (stage 1 has retired: eval_device waited for it)
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    // <trace path>.pc: "N M ms" of the covariance launches alone
    return trace_timed(ctx, ".pc", N, M, [&] {
        return guarded(ctx, true, [&] {
            joint_cov_launches(ctx->s_main, d, N, M, ctx->A, ctx->B, ctx->dXs, ctx->pmean, ctx->dtp, cov == Cov::full);
        });
    });
}

// Stage 3: the factorisation of order M of the matrix in ctx->B (A and B already swapped by the
// caller's WsSwap), which xr describes as prebuilt, with or without riding rows. info > 0: the
// leading minor of Sigma* (or of the matrix `what` names: the sparse entries factor their S the
// same way, §10.8).
int joint_factor(gaplac_ctx* ctx, int64_t M, int32_t D, const TermPack& tp, const ExtraRows& xr, EvalResult* r,
                 const char* what = "the test-point covariance Sigma*") {
    int rc = eval_device(ctx, M, D, tp, xr, r);
    if (rc) return rc;
    if ((rc = finish(*r, nullptr, nullptr, nullptr)))
        return set_err(ctx, rc, "%s is not positive definite (leading minor %d)", what, rc);
    return 0;
}

// ---- inducing-point (VFE) approximation ----
// The K-split of the stage-2 product: chunks of chunk_rows rows, a function of (N, Mz) alone
// (never of the device, its free CUs or timing), so a call's summation order is fixed. Chunks
// are SPARSE_CHUNK rows unless that would make more than SPARSE_PART_TILES partial tiles
// (1 GiB of partials); then whole multiples of SPARSE_CHUNK. At N = 16384 .. 262144 and Mz =
// 256 .. 4096 that is 96 .. 7854 workgroups of at least 1024 rows each.
constexpr int64_t SPARSE_CHUNK = 1024;
constexpr int64_t SPARSE_PART_TILES = 8192;
void sparse_split(int64_t N, int64_t Mz, int64_t* chunks, int64_t* chunk_rows) {
    const int64_t ntb = round_up(Mz + 1, NB) / NB, ntl = ntb * (ntb + 1) / 2;
    const int64_t max_chunks = std::max<int64_t>(1, SPARSE_PART_TILES / ntl);
    const int64_t blocks = (N + SPARSE_CHUNK - 1) / SPARSE_CHUNK;
    const int64_t rows = SPARSE_CHUNK * std::max<int64_t>(1, (blocks + max_chunks - 1) / max_chunks);
    *chunk_rows = rows;
    *chunks = (N + rows - 1) / rows;
}

// Argument checks the two entries share, after their own (output pointers).
int sparse_check(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, double noise, const double* y,
                 int64_t Mz, const double* Z, int64_t ldz, double jitter, int64_t Ms, const double* Xs, int64_t ldxs) {
    int rc = check_common(ctx, N, D, X, ldx, noise, y);
    if (rc) return rc;
    if (!(noise > 0.0)) return set_err(ctx, GAPLAC_E_PARAM, "noise %g must be > 0", noise);
    if (!(jitter >= 0.0) || !std::isfinite(jitter))
        return set_err(ctx, GAPLAC_E_PARAM, "jitter %g must be finite and >= 0", jitter);
    if (Mz < 0 || (Mz > 0 && D > 0 && (!Z || ldz < Mz)))
        return set_err(ctx, GAPLAC_E_ARG, "Mz = %lld < 0, or Z NULL / ldz %lld < Mz", (long long)Mz, (long long)ldz);
    if (Ms < 0 || (Ms > 0 && D > 0 && (!Xs || ldxs < Ms)))
        return set_err(ctx, GAPLAC_E_ARG, "Ms = %lld < 0, or Xs NULL / ldxs %lld < Ms", (long long)Ms, (long long)ldxs);
    if (N > 0 && Mz > 0 && (N + Ms + NB - 1) / NB > 65535)  // (one grid row of the cross-covariance launch per tile row)
        return set_err(ctx, GAPLAC_E_OOM, "N + Ms = %lld: more than 65535 tile rows in one call", (long long)(N + Ms));
    return 0;
}

// Paddings, leading dimensions and the stage-2 split, for the entries and for
// gaplac_plan_check_sparse alike: A of order Mz with the N + Ms rows of X and Xs in mt riding tile
// rows, B of order Mz (ntb tile columns) with the Ms rows a_j in rt riding tile rows (Ms = 0: none).
struct SparseDims {
    int mt, rt;
    int64_t Np, lda, ldb, ntb, chunks, chunk_rows;
};
SparseDims sparse_dims(int64_t N, int64_t Mz, int64_t Ms) {
    SparseDims d;
    d.mt = (int)((N + Ms + NB - 1) / NB);
    d.rt = (int)((Ms + NB - 1) / NB);
    d.Np = round_up(Mz + 1, NB);
    d.lda = d.Np + (int64_t)NB * d.mt;
    d.ldb = d.Np + (int64_t)NB * d.rt;
    d.ntb = d.Np / NB;
    sparse_split(N, Mz, &d.chunks, &d.chunk_rows);
    return d;
}

// The gradient's order-Mz scratch (§10.9): three column storages of Np columns, leading dimension
// ld = 2 Np (a factor's copy above its identity rows), and the offsets of its vectors.
struct SparseGradDims {
    int nt;
    int64_t Np, ld;
    // vectors (doubles): u, c, -c, ctil, -ctil, zeros (Np each), the results, alpha (N)
    int64_t u, c, nc, ct, nct, zero, out, alpha;
};
constexpr int64_t SG_OUT_UU = 0, SG_OUT_UF = GAPLAC_MAX_TERMS + 1, SG_OUT_TR = 2 * (GAPLAC_MAX_TERMS + 1);
constexpr int64_t SG_OUT = 2 * (GAPLAC_MAX_TERMS + 1) + 2;
SparseGradDims sparse_grad_dims(int64_t Mz) {
    SparseGradDims g;
    g.Np = round_up(Mz + 1, NB);
    g.nt = (int)(g.Np / NB);
    g.ld = 2 * g.Np;
    g.u = 0;
    g.c = g.Np;
    g.nc = 2 * g.Np;
    g.ct = 3 * g.Np;
    g.nct = 4 * g.Np;
    g.zero = 5 * g.Np;
    g.out = 6 * g.Np;
    g.alpha = 6 * g.Np + SG_OUT;
    return g;
}

// The launches after an evaluation, run by the entries and walked dry by gaplac_plan_check_sparse
// (the buffers besides A and B may be null there). Stage 2: the augmented matrix of S into B.
void sparse_s_launches(hipStream_t s, const SparseDims& d, int64_t N, int64_t Mz, double* A, const double* y,
                       double* part, double* B, double noise) {
    launch_rows_syrk(s, A, d.lda, d.Np, Mz, N, (int64_t)NB * d.mt, y, d.chunks, d.chunk_rows, part, B, d.ldb, noise);
}
// Y (Mz x Ms, ld Mz) = the a_j rows of stage 1 (riding rows N .. N + Ms - 1), transposed
void sparse_rows_launches(hipStream_t s, const SparseDims& d, int64_t N, int64_t Mz, int64_t Ms, const double* A,
                          double* Y) {
    launch_rows_to_matrix(s, A, d.lda, d.Np, N, Mz, Ms, Y, Mz);
}
// mode 2's reduction over the rows of stage 3 (A: the workspace of S): the dot with the v row (u)
// and the row norm
void sparse_post_launches(hipStream_t s, const SparseDims& d, int64_t Mz, int64_t Ms, double noise, const double* A,
                          double* partial, double* mean, double* var) {
    launch_sparse_post(s, A, d.ldb, d.Np, Mz, Ms, noise, partial, mean, var);
}

// Stages 1 and 2. Stage 1 is the posterior evaluation of the training set (Z, jitter) with v = 0
// and the N rows of X, then the Ms rows of Xs, as its test points: V^T (and a_j^T) below the
// factor, k(x, x) - |row|^2 in ctx->pvar; *trace = the sum of the first N of those, in order.
// Stage 2 writes the augmented matrix of S into ctx->B, laid out for a factorisation of order Mz
// with the Ms rows riding. tp carries noise = sigma^2 (the pack of stage 3).
int sparse_stages(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, const TermPack& tp,
                  const double* y, int64_t Mz, const double* Z, int64_t ldz, double jitter, int64_t Ms,
                  const double* Xs, int64_t ldxs, double* trace) {
    int rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    const std::vector<double> zeros((size_t)Mz, 0.0);
    if ((rc = upload(ctx, Mz, D, Z, ldz, zeros.data()))) return rc;
    const int64_t R = N + Ms;
    if ((rc = upload_test_inputs(ctx, D, R, 0, N, X, ldx))) return rc;
    if ((rc = upload_test_inputs(ctx, D, R, N, Ms, Xs, ldxs))) return rc;
    if ((rc = ensure(ctx, &ctx->sp_y, &ctx->sp_y_elems, (size_t)N))) return rc;
    HIPCK(ctx, hipMemcpyAsync(ctx->sp_y, y, (size_t)N * 8, hipMemcpyHostToDevice, ctx->s_main));
    TermPack tp1 = tp;
    tp1.noise = jitter;
    EvalResult r;
    if ((rc = eval_device(ctx, Mz, D, tp1, ExtraRows::test_points(R), &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr)))
        return set_err(ctx, rc, "the inducing covariance K(Z) + jitter I is not positive definite (leading minor %d)", rc);
    const SparseDims d = sparse_dims(N, Mz, Ms);
    if ((rc = ensure(ctx, &ctx->B, &ctx->B_elems, (size_t)d.ldb * (size_t)d.Np))) return rc;
    if ((rc = ensure(ctx, &ctx->sp_part, &ctx->sp_part_elems,
                     (size_t)d.chunks * (size_t)(d.ntb * (d.ntb + 1) / 2) * (size_t)(NB * NB))))
        return rc;
    // <trace path>.ss: "N Mz ms" of the stage-2 launches alone
    rc = trace_timed(ctx, ".ss", N, Mz, [&] {
        return guarded(ctx, true, [&] {
            sparse_s_launches(ctx->s_main, d, N, Mz, ctx->A, ctx->sp_y, ctx->sp_part, ctx->B, tp.noise);
        });
    });
    if (rc) return rc;
    if (ctx->sg_keep) {  // the gradient (§10.9): S before stage 3 factors it, Dinv before stage 3 reuses it
        const SparseGradDims gd = sparse_grad_dims(Mz);
        if ((rc = ensure(ctx, &ctx->sg, &ctx->sg_elems, (size_t)(3 * gd.ld * gd.Np)))) return rc;
        if ((rc = ensure(ctx, &ctx->sg_dinv, &ctx->sg_dinv_elems, (size_t)gd.nt * DINV_PER_BLOCK))) return rc;
        HIPCK(ctx, hipMemcpy2DAsync(ctx->sg + 2 * gd.ld * gd.Np, (size_t)gd.ld * 8, ctx->B, (size_t)d.ldb * 8,
                                    (size_t)gd.Np * 8, (size_t)gd.Np, hipMemcpyDeviceToDevice, ctx->s_main));
        HIPCK(ctx, hipMemcpyAsync(ctx->sg_dinv, ctx->Dinv, (size_t)gd.nt * DINV_PER_BLOCK * 8,
                                  hipMemcpyDeviceToDevice, ctx->s_main));
    }
    if (trace) {  // (stage 1 has retired: eval_device waited for it)
        std::vector<double> pv((size_t)N);
        HIPCK(ctx, hipMemcpy(pv.data(), ctx->pvar, (size_t)N * 8, hipMemcpyDeviceToHost));
        double t = 0.0;
        for (int64_t n = 0; n < N; ++n) t += pv[(size_t)n];
        *trace = t;
    }
    return 0;
}

// Stage 3 is joint_factor on ctx->B (info > 0: the leading minor of S).
constexpr const char* SPARSE_S = "S = noise I + V V^T";

int sparse_elbo_impl(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                     const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z, int64_t ldz,
                     double jitter, double* out_elbo, double* out_dtc, double* out_trace, double* out_logdet,
                     double* out_quad) {
    if (!ctx) return GAPLAC_E_ARG;
    for (double* o : {out_elbo, out_dtc, out_trace, out_logdet, out_quad})
        if (o) *o = NAN;
    if (!out_elbo) return set_err(ctx, GAPLAC_E_ARG, "out_elbo is NULL");
    int rc = sparse_check(ctx, N, D, X, ldx, noise, y, Mz, Z, ldz, jitter, 0, nullptr, 0);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    tp.noise = noise;
    const double log2pi = 1.8378770664093453;  // Julia's log2π
    double trace = 0.0, logdet = 0.0, quad = 0.0, yty = 0.0;
    for (int64_t n = 0; n < N; ++n) yty += y[n] * y[n];
    if (N > 0 && Mz == 0) {  // Q = 0: the model is N(0, noise I), the trace the prior variances
        for (int64_t n = 0; n < N; ++n) trace += host_kdiag(tp, X, ldx, n);
        logdet = (double)N * std::log(noise);
        quad = yty / noise;
    } else if (N > 0) {
        if ((rc = sparse_stages(ctx, N, D, X, ldx, tp, y, Mz, Z, ldz, jitter, 0, nullptr, 0, &trace))) return rc;
        WsSwap swap(ctx);  // from here on ctx->A is the workspace of S
        EvalResult r2;
        if ((rc = joint_factor(ctx, Mz, D, tp, ExtraRows{}.on_prebuilt(), &r2, SPARSE_S))) return rc;
        logdet = (double)(N - Mz) * std::log(noise) + r2.logdet;
        quad = (yty - r2.quad) / noise;
    }
    const double dtc = N > 0 ? -(((double)N * log2pi + logdet) + quad) / 2.0 : 0.0;
    *out_elbo = N > 0 ? dtc - trace / (2.0 * noise) : 0.0;
    if (out_dtc) *out_dtc = dtc;
    if (out_trace) *out_trace = trace;
    if (out_logdet) *out_logdet = logdet;
    if (out_quad) *out_quad = quad;
    return 0;
}

// ---- gradient of the bound ----
// The order-Mz launches, run by the entry under a guard over the scratch G and walked dry by
// gaplac_plan_check_sparse_grad (the buffers besides G may be fake there). G1 = [L; I], G2 =
// [L_S; I] and G3's top = S come in; G3's bottom = W', vec's c / ctil and the results leave.
void sparse_grad_mz_launches(hipStream_t s, const SparseGradDims& g, int64_t Mz, double* G, const double* dinv1,
                             const double* dinv2, double* vec, double* part, double noise, const double* Z,
                             const TermPack* dtp, const GradTermPack* dgp, int T) {
    const int64_t Np = g.Np, ld = g.ld;
    double *G1 = G, *G2 = G + ld * Np, *G3 = G + 2 * ld * Np;
    launch_init_identity_rows(s, G1, ld, Np, g.nt, g.nt);
    launch_init_identity_rows(s, G2, ld, Np, g.nt, g.nt);
    launch_rows_solve(s, G1, ld, g.nt, dinv1);  // Y1 = L^{-T}
    launch_rows_solve(s, G2, ld, g.nt, dinv2);  // Y2 = L_S^{-T}
    launch_zero_tail_cols(s, G1, ld, Np, Mz);
    launch_zero_tail_cols(s, G2, ld, Np, Mz);
    launch_copy_z(s, G2, ld, Mz, vec + g.u);                                              // u: L_S's v row
    launch_alpha(s, G2, ld, Np, Mz, vec + g.u, part, vec + g.c, vec + g.nc);              // c = Y2 u
    launch_alpha(s, G1, ld, Np, Mz, vec + g.c, part, vec + g.ct, vec + g.nct);            // ctil = Y1 c
    launch_sg_nt(s, G2 + Np, ld, G2 + Np, ld, Np, true, true, G2, ld, Mz, 1.0, 1.0 / noise, 0.0, nullptr);  // Phi
    launch_sg_nt(s, G1 + Np, ld, G2, ld, Np, true, false, G3 + Np, ld, Mz, -1.0, 0.0, 0.0, nullptr);       // W' = Y1 Phi
    launch_sg_h(s, G3, G2, G2 + Np, ld, Np, Mz, noise, vec + g.out + SG_OUT_TR);                            // H, tr Phi
    launch_sg_nt(s, G1 + Np, ld, G2 + Np, ld, Np, true, false, G1, ld, Mz, -1.0, 0.0, 0.0, nullptr);       // Y1 H
    launch_sg_nt(s, G1, ld, G1 + Np, ld, Np, false, true, G3, ld, Mz, 0.5, 0.0, -0.5, vec + g.ct);         // G_uu
    // sum G_uu o dKuu/dtheta (alpha = 0: the weights are G_uu alone); slot T: tr G_uu
    launch_grad_contract(s, G3, ld, Mz, Z, Mz, vec + g.zero, dtp, dgp, part, nullptr);
    const int m = (int)((Mz + NB - 1) / NB);
    launch_grad_reduce(s, part, m * (m + 1) / 2, T, vec + g.out + SG_OUT_UU);
}
// The N-long launches, under a guard over the first workspace A and G: alpha, then the product.
void sparse_grad_alpha_launches(hipStream_t s, const SparseDims& d, const SparseGradDims& g, int64_t N, int64_t Mz,
                                const double* A, double* vec, double* part, double noise, const double* y) {
    launch_sparse_alpha(s, A, d.lda, d.Np, Mz, N, vec + g.c, y, noise, part, vec + g.alpha);
}
void sparse_grad_uf_launches(hipStream_t s, const SparseDims& d, const SparseGradDims& g, int64_t N, int64_t Mz,
                             const double* A, const double* G, double* vec, double* part, const double* X,
                             const double* Z, const TermPack* dtp, const GradTermPack* dgp, bool groups, int T,
                             double* dz = nullptr, int D = 0) {
    launch_sparse_guf(s, A, d.lda, d.Np, N, Mz, G + 2 * g.ld * g.Np + g.Np, g.ld, X, N, Z, Mz, vec + g.alpha,
                      vec + g.ct, dtp, dgp, groups, part, dz, T);
    launch_grad_reduce(s, part, (int)(((N + NB - 1) / NB) * ((Mz + NB - 1) / NB)), T, vec + g.out + SG_OUT_UF);
    // dz (§10.10): the product above was its dZ variant; the reductions, the order-Mz part from G_uu
    // (G3's upper slot) and the finishing step follow
    if (dz) launch_sparse_dz(s, sparse_dz_dims(N, Mz, T, D), G + 2 * g.ld * g.Np, g.ld, Mz, T, D, Z, Mz, dtp, dgp, dz);
}
size_t sparse_grad_part_elems(int64_t N, int64_t Mz) {
    const size_t nk = (size_t)((Mz + 511) / 512), m = (size_t)((Mz + NB - 1) / NB), mt = (size_t)((N + NB - 1) / NB);
    const size_t S = GAPLAC_MAX_TERMS + 1;
    return std::max(std::max(nk * (size_t)Mz, nk * (size_t)N), std::max(m * (m + 1) / 2 * S, mt * m * S));
}

// sum_n dk(x_n, x_n)/dtheta_t on the host (host_kdiag's loop): 1 for LINEAR's c and a NOISE
// term's variance, 0 for a lengthscale (u = 0) and CAT, times the other terms of t's group.
void host_dkdiag(const TermPack& tp, const GradTermPack& gp, const double* X, int64_t ldx, int64_t N, double* out) {
    for (int t = 0; t < tp.T; ++t) {
        out[t] = 0.0;
        if (tp.kind[t] != GAPLAC_LINEAR && tp.kind[t] != GAPLAC_NOISE) continue;
        for (int64_t n = 0; n < N; ++n) {
            double d = 1.0;
            for (int s = gp.gstart[t]; s < gp.gend[t]; ++s) {
                if (s == t) continue;
                const double x = tp.kind[s] == GAPLAC_NOISE ? 0.0 : X[(int64_t)tp.col[s] * ldx + n];
                if (tp.kind[s] == GAPLAC_LINEAR) d *= x * x + tp.p[s];
                if (tp.kind[s] == GAPLAC_NOISE) d *= tp.p[s];
            }
            out[t] += d;
        }
    }
}

int sparse_elbo_grad_impl(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                          const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                          int64_t ldz, double jitter, double* out_elbo, double* out_dy, double* out_dparam,
                          double* out_dnoise, double* out_djitter, double* out_dZ = nullptr, int64_t lddz = 0) {
    if (!ctx) return GAPLAC_E_ARG;
    for (double* o : {out_elbo, out_dnoise, out_djitter})
        if (o) *o = NAN;
    for (int t = 0; out_dparam && t < T && t < GAPLAC_MAX_TERMS; ++t) out_dparam[t] = NAN;
    for (int64_t n = 0; out_dy && n < N; ++n) out_dy[n] = NAN;
    if (out_dZ && lddz < Mz) return set_err(ctx, GAPLAC_E_ARG, "lddz (%lld) < Mz (%lld)", (long long)lddz, (long long)Mz);
    for (int32_t c = 0; out_dZ && c < D; ++c)
        for (int64_t m = 0; m < Mz; ++m) out_dZ[(int64_t)c * lddz + m] = NAN;
    // the value, by its own schedule; with sg_keep its stages leave S and the first Dinv behind
    struct Keep {
        gaplac_ctx* c;
        explicit Keep(gaplac_ctx* ctx) : c(ctx) { c->sg_keep = true; }
        ~Keep() { c->sg_keep = false; }
    } keep(ctx);
    if (!out_elbo) return set_err(ctx, GAPLAC_E_ARG, "out_elbo is NULL");
    double elbo = NAN, trace = NAN;
    int rc = sparse_elbo_impl(ctx, N, D, X, ldx, T, terms, noise, y, Mz, Z, ldz, jitter, &elbo, nullptr, &trace, nullptr,
                              nullptr);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    GradTermPack gp{};
    const bool groups = !pack_groups(T, terms, &gp);
    double dsum[GAPLAC_MAX_TERMS + 1] = {};
    host_dkdiag(tp, gp, X, ldx, N, dsum);
    std::vector<double> alpha((size_t)std::max<int64_t>(N, 0));
    double outs[SG_OUT] = {};
    if (N > 0 && Mz == 0) {  // Q = 0: alpha = y / noise, no inducing pieces
        for (int64_t n = 0; n < N; ++n) alpha[(size_t)n] = y[n] / noise;
    } else if (N > 0) {
        const SparseDims d = sparse_dims(N, Mz, 0);
        const SparseGradDims g = sparse_grad_dims(Mz);
        HIPCK(ctx, hipSetDevice(ctx->device));
        if ((rc = ensure(ctx, &ctx->sg_v, &ctx->sg_v_elems, (size_t)(g.alpha + N)))) return rc;
        if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, sparse_grad_part_elems(N, Mz)))) return rc;
        const SparseDzDims zd = sparse_dz_dims(N, Mz, T, D);
        if (out_dZ && (rc = ensure(ctx, &ctx->sgz, &ctx->sgz_elems, (size_t)zd.elems))) return rc;
        double* const dz = out_dZ ? ctx->sgz : nullptr;
        // (the value has retired: ctx->A is the first workspace again, L above V^T; ctx->B holds L_S,
        // ctx->Dinv its inverses, ctx->dX = Z, ctx->dXs = X, ctx->dtp the pack)
        double* const G = ctx->sg;
        HIPCK(ctx, hipMemcpy2DAsync(G, (size_t)g.ld * 8, ctx->A, (size_t)d.lda * 8, (size_t)g.Np * 8, (size_t)g.Np,
                                    hipMemcpyDeviceToDevice, ctx->s_main));
        HIPCK(ctx, hipMemcpy2DAsync(G + g.ld * g.Np, (size_t)g.ld * 8, ctx->B, (size_t)d.ldb * 8, (size_t)g.Np * 8,
                                    (size_t)g.Np, hipMemcpyDeviceToDevice, ctx->s_main));
        HIPCK(ctx, hipMemsetAsync(ctx->sg_v + g.zero, 0, (size_t)g.Np * 8, ctx->s_main));
        *ctx->hgp = gp;
        HIPCK(ctx, hipMemcpyAsync(ctx->dgp, ctx->hgp, sizeof(GradTermPack), hipMemcpyHostToDevice, ctx->s_main));
        if ((rc = guarded_on(ctx, G, ctx->sg_elems, nullptr, 0, [&] {
                 sparse_grad_mz_launches(ctx->s_main, g, Mz, G, ctx->sg_dinv, ctx->Dinv, ctx->sg_v, ctx->gpart, noise,
                                         ctx->dX, ctx->dtp, ctx->dgp, T);
             })))
            return rc;
        if ((rc = guarded_on(ctx, ctx->A, ctx->A_elems, G, ctx->sg_elems, [&] {
                 sparse_grad_alpha_launches(ctx->s_main, d, g, N, Mz, ctx->A, ctx->sg_v, ctx->gpart, noise, ctx->sp_y);
             })))
            return rc;
        // <trace path>.sg: "N Mz ms" of the product kernel (and its reductions, dZ's included) alone
        rc = trace_timed(ctx, ".sg", N, Mz, [&] {
            return guarded_on(
                ctx, ctx->A, ctx->A_elems, G, ctx->sg_elems,
                [&] {
                    sparse_grad_uf_launches(ctx->s_main, d, g, N, Mz, ctx->A, G, ctx->sg_v, ctx->gpart, ctx->dXs,
                                            ctx->dX, ctx->dtp, ctx->dgp, groups, T, dz, D);
                },
                dz, dz ? ctx->sgz_elems : 0);
        });
        if (rc) return rc;
        if (dz)
            HIPCK(ctx, hipMemcpy2DAsync(out_dZ, (size_t)lddz * 8, dz + zd.out, (size_t)Mz * 8, (size_t)Mz * 8, (size_t)D,
                                        hipMemcpyDeviceToHost, ctx->s_main));
        HIPCK(ctx, hipMemcpyAsync(alpha.data(), ctx->sg_v + g.alpha, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->s_main));
        HIPCK(ctx, hipMemcpyAsync(outs, ctx->sg_v + g.out, sizeof outs, hipMemcpyDeviceToHost, ctx->s_main));
        HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    }
    double ata = 0.0;
    for (int64_t n = 0; n < N; ++n) ata += alpha[(size_t)n] * alpha[(size_t)n];
    if (out_elbo) *out_elbo = elbo;
    for (int64_t n = 0; out_dy && n < N; ++n) out_dy[n] = -alpha[(size_t)n];
    for (int t = 0; out_dparam && t < T; ++t)
        out_dparam[t] = N > 0 ? -dsum[t] / (2.0 * noise) + 2.0 * outs[SG_OUT_UF + t] + 2.0 * outs[SG_OUT_UU + t] : 0.0;
    // (N - Mz + noise tr S^{-1}) / noise = N / noise - tr Phi
    if (out_dnoise)
        *out_dnoise = N > 0 ? 0.5 * (ata - ((double)N / noise - outs[SG_OUT_TR])) + trace / (2.0 * noise * noise) : 0.0;
    if (out_djitter) *out_djitter = N > 0 ? 2.0 * outs[SG_OUT_UU + T] : 0.0;
    if (N == 0)  // no data: the bound is 0 whatever Z is
        for (int32_t c = 0; out_dZ && c < D; ++c)
            for (int64_t m = 0; m < Mz; ++m) out_dZ[(int64_t)c * lddz + m] = 0.0;
    return 0;
}

int sparse_posterior_impl(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                          const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                          int64_t ldz, double jitter, int64_t Ms, const double* Xs, int64_t ldxs, double* out_mean,
                          double* out_var) {
    if (!ctx) return GAPLAC_E_ARG;
    for (int64_t j = 0; j < Ms; ++j) {
        if (out_mean) out_mean[j] = NAN;
        if (out_var) out_var[j] = NAN;
    }
    int rc = sparse_check(ctx, N, D, X, ldx, noise, y, Mz, Z, ldz, jitter, Ms, Xs, ldxs);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (Ms == 0) return 0;
    if (N == 0 || Mz == 0) {  // no data, or Q = 0: the prior
        for (int64_t j = 0; j < Ms; ++j) {
            if (out_mean) out_mean[j] = 0.0;
            if (out_var) out_var[j] = host_kdiag(tp, Xs, ldxs, j);
        }
        return 0;
    }
    tp.noise = noise;
    if ((rc = sparse_stages(ctx, N, D, X, ldx, tp, y, Mz, Z, ldz, jitter, Ms, Xs, ldxs, nullptr))) return rc;
    const SparseDims d = sparse_dims(N, Mz, Ms);
    // the a_j rows of stage 1, transposed, are the matrix whose columns ride stage 3 (mode 3's row source)
    if ((rc = ensure(ctx, &ctx->dY, &ctx->dY_elems, (size_t)Mz * (size_t)Ms))) return rc;
    if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, 2 * (size_t)Ms * (size_t)((Mz + 511) / 512)))) return rc;
    if ((rc = guarded(ctx, false, [&] { sparse_rows_launches(ctx->s_main, d, N, Mz, Ms, ctx->A, ctx->dY); })))
        return rc;
    WsSwap swap(ctx);
    EvalResult r2;
    if ((rc = joint_factor(ctx, Mz, D, tp, ExtraRows::responses(Ms, ctx->dY, Mz).on_prebuilt(), &r2, SPARSE_S)))
        return rc;
    if ((rc = guarded(ctx, false, [&] {
             sparse_post_launches(ctx->s_main, d, Mz, Ms, noise, ctx->A, ctx->gpart, ctx->pmean, ctx->pvar + N);
         })))
        return rc;
    if (out_mean) HIPCK(ctx, hipMemcpyAsync(out_mean, ctx->pmean, (size_t)Ms * 8, hipMemcpyDeviceToHost, ctx->s_main));
    if (out_var)
        HIPCK(ctx, hipMemcpyAsync(out_var, ctx->pvar + N, (size_t)Ms * 8, hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

// ---- joint covariance, draws and logpdf of the inducing-point posterior ----
// The third workspace C of order Ms with R responses in rt riding tile rows (R = 0: none), and the
// tile-aligned copy of the a rows (Np columns, leading dimension ldr), for the entries and for
// gaplac_plan_check_sparse_joint alike.
struct SparseJointDims {
    int rt;
    int64_t Msp, ldc, ldr;
};
SparseJointDims sparse_joint_dims(int64_t Ms, int64_t R) {
    SparseJointDims j;
    j.rt = (int)((R + NB - 1) / NB);
    j.Msp = round_up(Ms + 1, NB);
    j.ldc = j.Msp + (int64_t)NB * j.rt;
    j.ldr = round_up(Ms, NB);
    return j;
}

// The a rows of stage 1 (A: the first workspace) into their tile-aligned copy.
void sparse_joint_copy_launches(hipStream_t s, const SparseDims& d, const SparseJointDims& j, int64_t N, int64_t Mz,
                                int64_t Ms, const double* A, double* rows) {
    launch_sparse_rows_copy(s, A, d.lda, d.Np, N, Mz, Ms, rows, j.ldr);
}
// After stage 3 and the mean's reduction (Bw: the second workspace): the augmented matrix of Sigma*
// into C (row Ms, the v row, carries the mean: its results are not used), and with `mirror` its
// upper triangle from the lower. Run by the entries and walked dry by the plan check (Xs, mean and
// dtp may be null there).
void sparse_joint_cov_launches(hipStream_t s, const SparseDims& d, const SparseJointDims& j, int64_t Mz, int64_t Ms,
                               double* Bw, const double* rows, double* C, const double* Xs, int64_t ldxs,
                               const double* mean, const TermPack* dtp, double noise, bool mirror) {
    launch_sparse_post_cov(s, Bw, d.ldb, d.Np, Mz, Ms, rows, j.ldr, C, j.ldc, Xs, ldxs, mean, dtp, noise);
    if (mirror) launch_mirror_lower(s, C, j.ldc, Ms);
}

// The three stages of gaplac_sparse_posterior_mean_var (the mean in ctx->pmean, by the same
// launches), then the augmented matrix of Sigma* into ctx->C, laid out for a factorisation of
// order Ms with R riding responses (mirror: mirrored into a full matrix). tp comes in with the
// training noise and leaves with noise_s (the pack of the third factorisation, also in ctx->dtp).
// On return the workspaces are back in their places: the caller rotates C in for its factorisation.
int sparse_joint_stages(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, TermPack& tp,
                        const double* y, int64_t Mz, const double* Z, int64_t ldz, double jitter, int64_t Ms,
                        const double* Xs, int64_t ldxs, double noise_s, int64_t R, bool mirror) {
    int rc;
    const double noise = tp.noise;
    if ((rc = sparse_stages(ctx, N, D, X, ldx, tp, y, Mz, Z, ldz, jitter, Ms, Xs, ldxs, nullptr))) return rc;
    const SparseDims d = sparse_dims(N, Mz, Ms);
    const SparseJointDims j = sparse_joint_dims(Ms, R);
    if ((rc = ensure(ctx, &ctx->dY, &ctx->dY_elems, (size_t)Mz * (size_t)Ms))) return rc;
    if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, 2 * (size_t)Ms * (size_t)((Mz + 511) / 512)))) return rc;
    if ((rc = ensure(ctx, &ctx->sj_rows, &ctx->sj_rows_elems, (size_t)d.Np * (size_t)j.ldr))) return rc;
    if ((rc = ensure(ctx, &ctx->C, &ctx->C_elems, (size_t)j.ldc * (size_t)j.Msp))) return rc;
    if ((rc = guarded_on(ctx, ctx->A, ctx->A_elems, ctx->sj_rows, ctx->sj_rows_elems, [&] {
             sparse_rows_launches(ctx->s_main, d, N, Mz, Ms, ctx->A, ctx->dY);
             sparse_joint_copy_launches(ctx->s_main, d, j, N, Mz, Ms, ctx->A, ctx->sj_rows);
         })))
        return rc;
    WsSwap swap(ctx);  // ctx->A is the workspace of S until this returns
    EvalResult r2;
    if ((rc = joint_factor(ctx, Mz, D, tp, ExtraRows::responses(Ms, ctx->dY, Mz).on_prebuilt(), &r2, SPARSE_S)))
        return rc;
    if ((rc = guarded(ctx, false, [&] {
             sparse_post_launches(ctx->s_main, d, Mz, Ms, noise, ctx->A, ctx->gpart, ctx->pmean, ctx->pvar + N);
         })))
        return rc;
    tp.noise = noise_s;
    *ctx->htp = tp;  // (stage 3 has retired: eval_device waited for it)
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    // <trace path>.sj: "Mz Ms ms" of the covariance launches alone
    return trace_timed(ctx, ".sj", Mz, Ms, [&] {
        return guarded_on(
            ctx, ctx->A, ctx->A_elems, ctx->C, ctx->C_elems,
            [&] {
                sparse_joint_cov_launches(ctx->s_main, d, j, Mz, Ms, ctx->A, ctx->sj_rows, ctx->C, ctx->dXs + N, N + Ms,
                                          ctx->pmean, ctx->dtp, noise, mirror);
            },
            ctx->sj_rows, ctx->sj_rows_elems);
    });
}

// ---- the joint entries of both models (§10.6, §10.11), written once ----
// The model of a joint call, in the entries' argument order: exact, or `sparse` (inducing points).
struct JointModel {
    int64_t N;
    int32_t D;
    const double* X;
    int64_t ldx;
    int32_t T;
    const gaplac_term* terms;
    double noise;
    const double* y;
    bool sparse = false;
    int64_t Mz = 0;
    const double* Z = nullptr;
    int64_t ldz = 0;
    double jitter = 0.0;
    bool no_data() const { return N == 0 || (sparse && Mz == 0); }  // (or Q = 0): the posterior is the prior
    const char* m_name() const { return sparse ? "Ms" : "M"; }       // in the error texts
};

// The checks the three entries share, after their own (sizes and output pointers), and the pack.
int joint_check(gaplac_ctx* ctx, const JointModel& m, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                TermPack* tp) {
    int rc = m.sparse ? sparse_check(ctx, m.N, m.D, m.X, m.ldx, m.noise, m.y, m.Mz, m.Z, m.ldz, m.jitter, M, Xs, ldxs)
                      : check_common(ctx, m.N, m.D, m.X, m.ldx, m.noise, m.y);
    if (rc) return rc;
    if (!m.sparse && M > 0 && m.D > 0 && (!Xs || ldxs < M)) return set_err(ctx, GAPLAC_E_ARG, "Xs NULL or ldxs < M");
    if (!(noise_s >= 0.0) || !std::isfinite(noise_s))
        return set_err(ctx, GAPLAC_E_ARG, "noise_s %g must be finite and >= 0", noise_s);
    return pack_terms(ctx, m.D, m.T, m.terms, tp);
}

// The model's stages up to Sigma*, laid out for a factorisation of order M with R riding responses, in
// ctx->B (the sparse entries: their third workspace, ctx->C). tp leaves with noise_s.
int joint_model_stages(gaplac_ctx* ctx, const JointModel& m, TermPack& tp, int64_t M, const double* Xs, int64_t ldxs,
                       double noise_s, int64_t R, Cov cov) {
    tp.noise = m.noise;
    if (!m.sparse) return joint_stages(ctx, m.N, m.D, m.X, m.ldx, tp, m.y, M, Xs, ldxs, noise_s, R, cov);
    return sparse_joint_stages(ctx, m.N, m.D, m.X, m.ldx, tp, m.y, m.Mz, m.Z, m.ldz, m.jitter, M, Xs, ldxs, noise_s, R,
                               cov == Cov::full);
}

// NaN into out_mean and the M x M block of out_cov (rows M .. ldc-1 are the caller's), where given.
void nan_mean_cov(int64_t M, double* out_mean, double* out_cov, int64_t ldc) {
    for (int64_t j = 0; j < M; ++j) {
        if (out_mean) out_mean[j] = NAN;
        if (out_cov)
            for (int64_t i = 0; i < M; ++i) out_cov[j * ldc + i] = NAN;
    }
}
// The prior at the test points: its covariance by gaplac_gram and a zero mean.
int prior_mean_cov(gaplac_ctx* ctx, int32_t D, int32_t T, const gaplac_term* terms, int64_t M, const double* Xs,
                   int64_t ldxs, double noise_s, double* out_mean, double* out_cov, int64_t ldc) {
    int rc;
    if (out_cov && (rc = gaplac_gram(ctx, M, D, Xs, ldxs, T, terms, noise_s, out_cov, ldc))) return rc;
    for (int64_t j = 0; j < M && out_mean; ++j) out_mean[j] = 0.0;
    return 0;
}
// The covariance (the M x M block of dcov, ld ldd) and the mean read back; s_main has retired on return.
int read_mean_cov(gaplac_ctx* ctx, int64_t M, const double* dcov, int64_t ldd, const double* dmean, double* out_mean,
                  double* out_cov, int64_t ldc) {
    if (out_cov)
        HIPCK(ctx, hipMemcpy2DAsync(out_cov, (size_t)ldc * 8, dcov, (size_t)ldd * 8, (size_t)M * 8, (size_t)M,
                                    hipMemcpyDeviceToHost, ctx->s_main));
    if (out_mean) HIPCK(ctx, hipMemcpyAsync(out_mean, dmean, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

// gaplac_posterior_mean_cov and gaplac_sparse_posterior_mean_cov.
int joint_mean_cov(gaplac_ctx* ctx, const JointModel& m, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                   double* out_mean, double* out_cov, int64_t ldc) {
    if (!ctx) return GAPLAC_E_ARG;
    if (M < 0 || (out_cov && ldc < M))
        return set_err(ctx, GAPLAC_E_ARG, "%s = %lld < 0 or ldc < %s", m.m_name(), (long long)M, m.m_name());
    nan_mean_cov(M, out_mean, out_cov, ldc);
    TermPack tp;
    int rc = joint_check(ctx, m, M, Xs, ldxs, noise_s, &tp);
    if (rc || M == 0) return rc;
    if (m.no_data()) return prior_mean_cov(ctx, m.D, m.T, m.terms, M, Xs, ldxs, noise_s, out_mean, out_cov, ldc);
    if (m.sparse && !out_cov)  // the mean alone: the three stages of gaplac_sparse_posterior_mean_var
        return sparse_posterior_impl(ctx, m.N, m.D, m.X, m.ldx, m.T, m.terms, m.noise, m.y, m.Mz, m.Z, m.ldz, m.jitter,
                                     M, Xs, ldxs, out_mean, nullptr);
    if ((rc = joint_model_stages(ctx, m, tp, M, Xs, ldxs, noise_s, 0, out_cov ? Cov::full : Cov::none))) return rc;
    return read_mean_cov(ctx, M, m.sparse ? ctx->C : ctx->B, round_up(M + 1, NB), ctx->pmean, out_mean, out_cov, ldc);
}

// gaplac_posterior_rand and gaplac_sparse_posterior_rand (which calls its Z "E"): out = m 1^T + L* Z.
int joint_rand(gaplac_ctx* ctx, const JointModel& m, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
               int64_t R, const double* Z, int64_t ldz, double* out, int64_t ldo) {
    if (!ctx) return GAPLAC_E_ARG;
    if (M < 0 || R < 0 || !out || ldz < M || ldo < M || (R > 0 && M > 0 && !Z))
        return set_err(ctx, GAPLAC_E_ARG, "%s < 0, R < 0, %s / out NULL, or %s / ldo < %s", m.m_name(),
                       m.sparse ? "E" : "Z", m.sparse ? "lde" : "ldz", m.m_name());
    for (int64_t r = 0; r < R; ++r)  // (rows M .. ldo-1 of out are the caller's)
        for (int64_t i = 0; i < M; ++i) out[r * ldo + i] = NAN;
    TermPack tp;
    int rc = joint_check(ctx, m, M, Xs, ldxs, noise_s, &tp);
    if (rc || M == 0 || R == 0) return rc;
    if (m.no_data())  // the prior at the test points
        return gaplac_rand_multi(ctx, M, m.D, Xs, ldxs, m.T, m.terms, noise_s, R, Z, ldz, out, ldo);
    if (m.sparse && (R + NB - 1) / NB > 65535)  // (the sparse entry alone: the exact one takes any R)
        return set_err(ctx, GAPLAC_E_OOM, "R = %lld: more than 65535 tile rows in one call", (long long)R);
    if ((rc = joint_model_stages(ctx, m, tp, M, Xs, ldxs, noise_s, 0, Cov::lower))) return rc;
    const int64_t Mp = round_up(M + 1, NB);
    if ((rc = ensure(ctx, &ctx->dZ, &ctx->dZ_elems, (size_t)Mp * (size_t)R))) return rc;
    if ((rc = ensure(ctx, &ctx->dO, &ctx->dO_elems, (size_t)M * (size_t)R))) return rc;
    HIPCK(ctx, hipMemcpy2DAsync(ctx->dZ, (size_t)Mp * 8, Z, (size_t)ldz * 8, (size_t)M * 8, (size_t)R,
                                hipMemcpyHostToDevice, ctx->s_main));
    WsSwap swap(ctx, m.sparse ? &ctx->C : &ctx->B, m.sparse ? &ctx->C_elems : &ctx->B_elems);  // ctx->A: order M
    EvalResult r;
    if ((rc = joint_factor(ctx, M, m.D, tp, ExtraRows{}.on_prebuilt(), &r))) return rc;
    if ((rc = guarded(ctx, false, [&] { draws_launches(ctx->s_main, ctx->A, Mp, M, ctx->dZ, R, ctx->dO, ctx->pmean); })))
        return rc;
    HIPCK(ctx, hipMemcpy2DAsync(out, (size_t)ldo * 8, ctx->dO, (size_t)M * 8, (size_t)M * 8, (size_t)R,
                                hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

// gaplac_posterior_logpdf and gaplac_sparse_posterior_logpdf: every column of Ys under the joint posterior.
int joint_logpdf(gaplac_ctx* ctx, const JointModel& m, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                 int64_t R, const double* Ys, int64_t ldys, double* out_logpdf, double* out_logdet, double* out_quad) {
    if (!ctx) return GAPLAC_E_ARG;
    if (M < 0 || R < 0 || !out_logpdf || ldys < M || (R > 0 && M > 0 && !Ys))
        return set_err(ctx, GAPLAC_E_ARG, "%s < 0, R < 0, Ys / out_logpdf NULL, or ldys < %s", m.m_name(), m.m_name());
    if (M > 0 && R > 0) {  // (an empty call writes nothing)
        for (int64_t r = 0; r < R; ++r) {
            out_logpdf[r] = NAN;
            if (out_quad) out_quad[r] = NAN;
        }
        if (out_logdet) *out_logdet = NAN;
    }
    TermPack tp;
    int rc = joint_check(ctx, m, M, Xs, ldxs, noise_s, &tp);
    if (rc || M == 0 || R == 0) return rc;
    if (m.no_data())  // the prior at the test points
        return gaplac_logpdf_multi(ctx, M, m.D, Xs, ldxs, m.T, m.terms, noise_s, R, Ys, ldys, out_logpdf, out_logdet,
                                   out_quad);
    if ((R + NB - 1) / NB > 65535)  // (one grid row of the transposing launch per tile row)
        return set_err(ctx, GAPLAC_E_OOM, "R = %lld: more than 65535 tile rows in one call", (long long)R);
    if ((rc = joint_model_stages(ctx, m, tp, M, Xs, ldxs, noise_s, R, Cov::lower))) return rc;
    // (sparse: ctx->dY held the transposed a rows for stage 3, which has retired: the responses take it over)
    if ((rc = ensure(ctx, &ctx->dY, &ctx->dY_elems, (size_t)M * (size_t)R))) return rc;
    HIPCK(ctx, hipMemcpy2DAsync(ctx->dY, (size_t)M * 8, Ys, (size_t)ldys * 8, (size_t)M * 8, (size_t)R,
                                hipMemcpyHostToDevice, ctx->s_main));
    WsSwap swap(ctx, m.sparse ? &ctx->C : &ctx->B, m.sparse ? &ctx->C_elems : &ctx->B_elems);
    // the rows hold (Ys - m 1^T)^T and ride along as the responses of gaplac_logpdf_multi do
    EvalResult r;
    if ((rc = joint_factor(ctx, M, m.D, tp, ExtraRows::responses(R, ctx->dY, M, ctx->pmean).on_prebuilt(), &r)))
        return rc;
    if (out_logdet) *out_logdet = r.logdet;
    if (out_quad) HIPCK(ctx, hipMemcpy(out_quad, ctx->mres, (size_t)R * 8, hipMemcpyDeviceToHost));
    HIPCK(ctx, hipMemcpy(out_logpdf, ctx->mres + R, (size_t)R * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

// Batched tail: models m0 .. m0+B-1 of a select batch whose matrix lies
// whole in the persistent tail, evaluated together on workspace set p: the Grams and
// result records on s_panel (so they run beside the previous launch's tail on s_main),
// then on s_main ONE tail launch whose task list interleaves the B models' lists as a
// software pipeline (interleave_tail_tasks), and one reduction per model. Each model's
// tasks, and so its arithmetic, are those of its single evaluation: the results are
// bitwise the same. Nothing here waits for the launch; batch_tail_finish collects it.
static int batch_tail_finish(gaplac_ctx* ctx, int p, double* out_logpdf, int64_t* out_info);

static int batch_tail_enqueue(gaplac_ctx* ctx, int64_t N, const std::vector<TermPack>& packs, int m0, int B, int p,
                              double* out_logpdf, int64_t* out_info) {
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    const int64_t lda = Np;
    const size_t astride = (size_t)Np * (size_t)Np, dstride = (size_t)nt * DINV_PER_BLOCK;
    gaplac_ctx::BatchWs& w = ctx->bw[p];
    int rc;
    if (w.busy && (rc = batch_tail_finish(ctx, p, out_logpdf, out_info))) return rc;  // the set's last launch
    if ((rc = ensure(ctx, &w.A, &w.A_elems, astride * (size_t)B))) return rc;
    if ((rc = ensure(ctx, &w.Dinv, &w.Dinv_elems, dstride * (size_t)B))) return rc;
    if ((rc = ensure(ctx, &w.dres, &w.dres_elems, (size_t)B))) return rc;
    if ((rc = ensure(ctx, &w.dtp, &w.dtp_elems, (size_t)B))) return rc;
    if ((rc = ensure(ctx, &w.ctl, &w.ctl_elems, (size_t)B))) return rc;
    if (w.host_cap < B) {
        if (w.hres) (void)hipHostFree(w.hres);
        if (w.htp) (void)hipHostFree(w.htp);
        w.hres = nullptr;
        w.htp = nullptr;
        w.host_cap = 0;
        HIPCK(ctx, hipHostMalloc(reinterpret_cast<void**>(&w.hres), sizeof(EvalResult) * (size_t)B, 0));
        HIPCK(ctx, hipHostMalloc(reinterpret_cast<void**>(&w.htp), sizeof(TermPack) * (size_t)B, 0));
        w.host_cap = B;
    }
    const int lag = ctx->batch_lag >= 0 ? ctx->batch_lag : (3 * nt + 4) / 8;
    const int lkey = lag * 100 + ctx->batch_gw * 10 + ctx->batch_near;
    if (w.tasks_T != nt || w.tasks_B != B || w.tasks_lag != lkey) {
        std::vector<uint32_t> one, all;
        std::vector<size_t> cs;
        build_tail_tasks(nt, one, &cs, ctx->batch_gw, ctx->batch_near, 0, true, GAPLAC_BATCH_GROUP);
        interleave_tail_tasks(one, cs, B, lag, all);
        if ((rc = ensure(ctx, &w.tasks, &w.tasks_elems, all.size()))) return rc;
        HIPCK(ctx, hipMemcpy(w.tasks, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        w.tasks_T = nt;
        w.tasks_B = B;
        w.tasks_lag = lkey;
        w.tasks_n = (int)all.size();
    }
    const bool trace = !ctx->ttrace_path.empty();  // diagnostics: launches one at a time
    // (+ the diagonal blocks' phase times, which a one-model launch records)
    if (trace && (rc = ensure(ctx, &ctx->ttrace, &ctx->ttrace_elems, 3 * (size_t)w.tasks_n + (size_t)TAIL_DSTAMPS * nt)))
        return rc;
    hipStream_t g = ctx->s_panel, s = ctx->s_main;
    for (int b = 0; b < B; ++b) w.htp[b] = packs[(size_t)(m0 + b)];
    // From the first enqueue on, a failure must not leave this call's work in flight (the
    // Grams read dX / dv, which the next call's upload overwrites): drain both streams first.
    auto bail = [&](int code) {
        (void)hipStreamSynchronize(g);
        (void)hipStreamSynchronize(s);
        return code;
    };
#define BATCHCK(call)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return bail(set_err(ctx, GAPLAC_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)));      \
    } while (0)
    LaunchGuard guard;
    guard.base = w.A;
    guard.elems = (int64_t)(astride * (size_t)B);
    {
        GuardScope scope(&guard);
        BATCHCK(hipMemcpyAsync(w.dtp, w.htp, sizeof(TermPack) * (size_t)B, hipMemcpyHostToDevice, g));
        for (int b = 0; b < B; ++b) {
            launch_init_result(g, w.dres + b);
            launch_gram(g, w.A + astride * (size_t)b, lda, N, nt, ctx->dX, N, ctx->dv, w.dtp + b, 0, 0, nullptr);
        }
        BATCHCK(hipEventRecord(w.ev_gram, g));
        BATCHCK(hipStreamWaitEvent(s, w.ev_gram, 0));
        BATCHCK(hipMemsetAsync(w.ctl, 0, sizeof(TailCtl) * (size_t)B, s));
        TailArgs ta{w.A, lda, N, 0, nt, w.Dinv, w.dres, w.ctl, w.tasks, w.tasks_n, trace ? ctx->ttrace : nullptr};
        ta.a_stride = (int64_t)astride;
        ta.dinv_stride = (int64_t)dstride;
        ta.nmodels = B;
        ta.fault = ctx->tail_fault;
        if (!guard.violations) launch_tail(s, ta, std::min(ctx->ncu, w.tasks_n), nullptr);
        for (int b = 0; b < B; ++b)
            launch_reduce(s, w.A + astride * (size_t)b, lda, N, (int64_t)nt * NB, ColMap{1, 0, 1}, w.dres + b);
    }
    if (guard.violations)
        return bail(set_err(ctx, GAPLAC_E_ARG, "batched tail: launch footprint outside the workspace: %s",
                            guard.first.c_str()));
    BATCHCK(hipGetLastError());
    BATCHCK(hipMemcpyAsync(w.hres, w.dres, sizeof(EvalResult) * (size_t)B, hipMemcpyDeviceToHost, s));
    BATCHCK(hipEventRecord(w.ev_done, s));
#undef BATCHCK
    w.busy = true;
    w.m0 = m0;
    w.B = B;
    if (!ctx->ttrace_path.empty()) {  // diagnostics: the launch's task timeline
        if ((rc = batch_tail_finish(ctx, p, out_logpdf, out_info))) return rc;
        std::vector<unsigned long long> tr(3 * (size_t)w.tasks_n);
        std::vector<uint32_t> tk((size_t)w.tasks_n);
        HIPCK(ctx, hipMemcpy(tr.data(), ctx->ttrace, tr.size() * 8, hipMemcpyDeviceToHost));
        HIPCK(ctx, hipMemcpy(tk.data(), w.tasks, tk.size() * 4, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(ctx->ttrace_path.c_str(), "a")) {
            std::fprintf(f, "# N=%lld T=%d tasks=%d models=%d (batched)\n", (long long)N, nt, w.tasks_n, B);
            for (size_t i = 0; i < tk.size(); ++i)
                std::fprintf(f, "%zu %u %llu %llu %llu\n", i, tk[i], tr[3 * i], tr[3 * i + 1], tr[3 * i + 2]);
            std::fclose(f);
        }
    }
    return 0;
}

static int batch_tail_finish(gaplac_ctx* ctx, int p, double* out_logpdf, int64_t* out_info) {
    gaplac_ctx::BatchWs& w = ctx->bw[p];
    if (!w.busy) return 0;
    w.busy = false;
    HIPCK(ctx, hipEventSynchronize(w.ev_done));
    for (int b = 0; b < w.B; ++b) {
        if (w.hres[b].err) return set_err(ctx, GAPLAC_E_HIP, "batched tail: in-kernel wait expired (code %u)", w.hres[b].err);
        out_info[w.m0 + b] = finish(w.hres[b], &out_logpdf[w.m0 + b], nullptr, nullptr);
    }
    return 0;
}

// A host-only walk of one evaluation's schedule (every plan check): c, a context on the
// stack with its switches set, carries the description xr as an evaluation would (EvalScope)
// and gets the workspace size and tile layout ensure_workspace would give it for order N
// behind a fake pointer (never dereferenced: the walk only does pointer arithmetic against
// the guard's base); the schedule is enqueued dry under g, whose workspace is short_by
// elements short (the negative control).
// after (optional): further launches in the walk's context and under its guard, after the evaluation's.
static int dry_walk(gaplac_ctx& c, int64_t N, const ExtraRows& xr, LaunchGuard& g, int64_t short_by = 0,
                    const std::function<int(gaplac_ctx&)>& after = nullptr) {
    EvalScope scope(&c, xr);
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    double* const fake = reinterpret_cast<double*>((uintptr_t)1 << 44);
    TermPack tp{};
    tp.T = 1;
    c.dry = true;
    c.tail_s = 80;  // as gaplac_ctx_create sets it with the persistent tail
    c.A = c.Dinv = fake;
    c.A_elems = (size_t)(Np + (int64_t)NB * c.xr.tiles) * (size_t)Np;
    c.tiles = reinterpret_cast<uint32_t*>(fake);
    c.htp = &tp;
    set_tile_layout(&c, nt);
    c.tiles_nt = nt;
    if (c.xr.mode == 1) {
        std::vector<uint32_t> gl;
        build_grad_list((int)((N + NB - 1) / NB), gl);
        c.glist_blocks = (int)gl.size();
    }
    g.base = fake;
    g.elems = (int64_t)c.A_elems - short_by;
    g.dry = true;
    int rc;
    {
        GuardScope gscope(&g);
        rc = enqueue_eval(&c, N, 1, Np, nt);
        if (rc == 0 && after) rc = after(c);
    }
    c.htp = nullptr;  // nothing of the walk's stays behind in c
    c.A = c.Dinv = nullptr;
    c.tiles = nullptr;
    return rc;
}

// What every gaplac_plan_check_* entry is written on: the fake regions, the entries'
// own *_launches functions run under a dry guard, the dry evaluations between them, and the report.
// Launches and violations add up; `first` is the first violation in walk order. After an evaluation
// fails for another reason than a violation the walk does nothing more and report() returns that code.
namespace {
struct PlanWalk {
    int spw;
    int rc = 0;
    int64_t launches = 0, violations = 0;
    std::string first;
    const LaunchGuard* open = nullptr;  // the evaluation whose `after` is running

    // The never-dereferenced base of fake region k. An evaluation's workspace is region 0 (dry_walk).
    static double* region(int k) { return reinterpret_cast<double*>((uintptr_t)1 << (44 + k)); }

    void note(const LaunchGuard& g) { if (first.empty() && g.violations) first = g.first; }
    void add(const LaunchGuard& g) {
        launches += g.launches;
        violations += g.violations;
        note(g);
    }
    // `run` under a fresh dry guard over up to three regions, in guarded_on's shape.
    template <typename Launches>
    void on(const double* base, int64_t elems, const double* base2, int64_t elems2, Launches&& run,
            const double* base3 = nullptr, int64_t elems3 = 0) {
        if (rc) return;
        if (open) note(*open);  // (inside an evaluation: what that has found so far came first)
        LaunchGuard g{base, elems, base2, elems2, base3, elems3, /*dry*/ true};
        {
            GuardScope scope(&g);
            run();
        }
        add(g);
    }
    // One evaluation of order N with the rows xr, walked dry in a context of its own whose
    // workspace is short_by elements short; base2: a second region for the launches of `after`.
    // GAPLAC_E_ARG with violations is the walk's finding, reported in the counts, not a failure.
    void eval(int64_t N, const ExtraRows& xr, int64_t short_by = 0,
              const std::function<int(gaplac_ctx&)>& after = nullptr, const double* base2 = nullptr,
              int64_t elems2 = 0) {
        if (rc) return;
        gaplac_ctx c;
        c.spw = spw;
        LaunchGuard g;
        g.base2 = base2;
        g.elems2 = elems2;
        open = &g;
        rc = dry_walk(c, N, xr, g, short_by, after);
        open = nullptr;
        if (rc == GAPLAC_E_ARG && g.violations) rc = 0;
        add(g);
    }
    int report(int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen) const {
        if (out_launches) *out_launches = launches;
        if (out_violations) *out_violations = violations;
        if (msg && msglen > 0) std::snprintf(msg, (size_t)msglen, "%s", first.c_str());
        return rc;
    }
};
}  // namespace

// ---------------------------------------------------------------------------------
// Fitted posterior: one factorisation kept, queried many times.
// ---------------------------------------------------------------------------------

// Where everything a fit keeps lies in its one device buffer (offsets in doubles). L comes first
// (the launchers' footprints are relative to it) and alpha last: the back-substitution's first
// launch writes the buffer's last element, so a buffer one element short is always reported.
struct FitDims {
    int64_t Np, ldl, nk, nkm, qc, Dm;
    int nt;
    int64_t L, dinv, X, Xs, part, mean, var, tp, alpha, elems;
    int64_t sw, fhat;  // a Laplace fit (§10.15): sqrt(W) and the mode, before alpha (which stays last)
};
// test points per launch of the matrix-free mean (it needs no riding rows, so cap does not bind it)
constexpr int64_t FIT_MEAN_CHUNK = 8192;

static FitDims fit_dims(int64_t N, int32_t D, int64_t cap, bool laplace = false) {
    FitDims d{};
    d.Np = round_up(N + 1, NB);
    d.nt = (int)(d.Np / NB);
    const int64_t ct = (cap + NB - 1) / NB;
    d.ldl = d.Np + NB * ct;
    d.nk = (N + 511) / 512;
    d.nkm = (N + 255) / 256;
    d.qc = std::max(cap, FIT_MEAN_CHUNK);
    d.Dm = D > 0 ? D : 1;
    d.L = 0;
    d.dinv = d.L + d.ldl * d.Np;
    d.X = d.dinv + (int64_t)d.nt * DINV_PER_BLOCK;
    d.Xs = d.X + N * d.Dm;
    d.part = d.Xs + d.qc * d.Dm;
    d.mean = d.part + std::max(2 * d.nk * cap, d.nkm * d.qc);
    d.var = d.mean + d.qc;
    d.tp = d.var + d.qc;
    d.sw = d.tp + (int64_t)((sizeof(TermPack) + 7) / 8);
    d.fhat = d.sw + (laplace ? N : 0);
    d.alpha = d.fhat + (laplace ? N : 0);
    d.elems = d.alpha + N;
    return d;
}

struct gaplac_fit {
    gaplac_ctx* ctx = nullptr;  // nullptr once the context has been destroyed
    int device = 0;
    int64_t N = 0, cap = 0;
    int32_t D = 0;
    TermPack tp{};  // host copy (noise inside)
    double logpdf = NAN, logdet = NAN, quad = NAN;
    FitDims d{};
    double* buf = nullptr;
    // kind 1: the latent posterior of the Laplace approximation (§10.15): the factor is B's, alpha
    // is a = grad log p(y | f) at the mode, logpdf = log q, logdet = log|B|, quad = a^T f
    int kind = 0;
    int32_t lik = 0, iters = 0, converged = 0;
    double lik_param = 0.0, jitter = 0.0;
    std::vector<gaplac_term> terms;  // the caller's terms (the prior's Gram of an empty fit)
};

// The create-time launches after the evaluation: the factor's lower tiles out of the context's
// workspace A (ld lda), z out of the factor's row N into alpha, and the back-substitution.
static void fit_create_launches(hipStream_t s, const FitDims& d, int64_t N, const double* A, int64_t lda,
                                double* buf) {
    launch_fit_copy(s, A, lda, d.nt, buf + d.L, d.ldl);
    launch_copy_z(s, buf + d.L, d.ldl, N, buf + d.alpha);
    launch_fit_backsub(s, buf + d.L, d.ldl, N, buf + d.alpha);
}

static void fit_mean_launches(hipStream_t s, const FitDims& d, int64_t N, int64_t m, double* buf) {
    launch_fit_mean(s, N, m, buf + d.X, N, buf + d.alpha, buf + d.Xs, m,
                    reinterpret_cast<const TermPack*>(buf + d.tp), buf + d.part, buf + d.mean);
}

// One chunk of m <= cap test points (their inputs at d.Xs, ld m): K(xs, X) into the reserved
// rows, the rows' solve against the factor, mean and variance into d.mean / d.var.
// laplace: the rows are sw_n k(xs_j, x_n) below the factor of B; launch_posterior's variance is the
// latent one, its V^T z mean is not the posterior's (row N of B's factor is no L^{-1} y) and is
// overwritten by the matrix-free mean with a.
static void fit_query_launches(hipStream_t s, const FitDims& d, int64_t N, int64_t m, int W, double* buf,
                               bool laplace = false) {
    const int mt = (int)((m + NB - 1) / NB);
    const TermPack* dtp = reinterpret_cast<const TermPack*>(buf + d.tp);
    if (laplace)
        launch_cross_gram_scaled(s, buf + d.L, d.ldl, d.Np, d.nt, N, m, mt, buf + d.X, N, buf + d.Xs, m, dtp,
                                 buf + d.sw);
    else
        launch_cross_gram(s, buf + d.L, d.ldl, d.Np, d.nt, N, m, mt, buf + d.X, N, buf + d.Xs, m, dtp);
    launch_fit_rows_solve(s, buf + d.L, d.ldl, d.nt, mt, W, buf + d.dinv);
    launch_posterior(s, buf + d.L, d.ldl, d.Np, N, m, buf + d.Xs, m, dtp, buf + d.part, buf + d.mean, buf + d.var);
    if (laplace) fit_mean_launches(s, d, N, m, buf);
}

// After a query's launches for m <= cap points (their rows solved below the factor, the mean in
// d.mean): Sigma* = K(xs) + noise_s I - V^T V into the context's second workspace B (ld ldb), full
// and symmetric. dtp: the pack with noise = noise_s.
static void fit_cov_launches(hipStream_t s, const FitDims& d, int64_t N, int64_t m, double* buf, double* B,
                             int64_t ldb, const TermPack* dtp) {
    launch_post_cov(s, buf + d.L, d.ldl, d.Np, N, m, B, ldb, buf + d.Xs, m, buf + d.mean, dtp);
    launch_mirror_lower(s, B, ldb, m);
}

static void fit_unregister(gaplac_fit* f) {
    if (!f->ctx) return;
    auto& v = f->ctx->fits;
    v.erase(std::remove(v.begin(), v.end(), f), v.end());
    f->ctx = nullptr;
}

extern "C" int gaplac_fit_create(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                 const gaplac_term* terms, double noise, const double* y, int64_t cap,
                                 gaplac_fit** out) {
    if (!out) return ctx ? set_err(ctx, GAPLAC_E_ARG, "out is NULL") : GAPLAC_E_ARG;
    *out = nullptr;
    int rc = check_common(ctx, N, D, X, ldx, noise, y);
    if (rc) return rc;
    if (cap < 1) return set_err(ctx, GAPLAC_E_ARG, "cap = %lld < 1", (long long)cap);
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    tp.noise = noise;
    std::unique_ptr<gaplac_fit> f(new gaplac_fit());
    f->device = ctx->device;
    f->N = N;
    f->cap = cap;
    f->D = D;
    f->tp = tp;
    f->terms.assign(terms, terms + T);
    if (N == 0) {  // the empty FiniteGP: its logpdf, and the prior at every query
        f->logpdf = -0.0;
        f->logdet = f->quad = 0.0;
    } else {
        if ((cap + NB - 1) / NB > 65535)
            return set_err(ctx, GAPLAC_E_OOM, "cap = %lld: more than 65535 tile rows", (long long)cap);
        HIPCK(ctx, hipSetDevice(ctx->device));
        if ((rc = upload(ctx, N, D, X, ldx, y))) return rc;
        EvalResult r;
        if ((rc = eval_device(ctx, N, D, tp, ExtraRows{}, &r))) return rc;
        if ((rc = finish(r, &f->logpdf, &f->logdet, &f->quad)))
            return set_err(ctx, rc, "K(X) + noise I (order %lld) is not positive definite: its Cholesky factorisation "
                                    "failed at leading minor %d; no fit",
                           (long long)N, rc);
        f->d = fit_dims(N, D, cap);
        const FitDims& d = f->d;
        if (hipMalloc(reinterpret_cast<void**>(&f->buf), (size_t)d.elems * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            f->buf = nullptr;
            return set_err(ctx, GAPLAC_E_OOM, "hipMalloc of the fit's %lld bytes failed", (long long)d.elems * 8);
        }
        struct Drop {  // the buffer goes with a failed create
            gaplac_fit* f;
            bool keep = false;
            ~Drop() {
                if (!keep && f->buf) (void)hipFree(f->buf);
            }
        } drop{f.get()};
        hipStream_t s = ctx->s_main;
        rc = guarded_on(ctx, f->buf, (size_t)d.elems, ctx->A, ctx->A_elems,
                        [&] { fit_create_launches(s, d, N, ctx->A, d.Np, f->buf); });
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        HIPCK(ctx, hipMemcpyAsync(f->buf + d.dinv, ctx->Dinv, (size_t)d.nt * DINV_PER_BLOCK * 8, hipMemcpyDeviceToDevice, s));
        if (D > 0)
            HIPCK(ctx, hipMemcpyAsync(f->buf + d.X, ctx->dX, (size_t)N * D * 8, hipMemcpyDeviceToDevice, s));
        HIPCK(ctx, hipMemcpyAsync(f->buf + d.tp, ctx->dtp, sizeof(TermPack), hipMemcpyDeviceToDevice, s));
        HIPCK(ctx, hipStreamSynchronize(s));
        drop.keep = true;
    }
    f->ctx = ctx;
    ctx->fits.push_back(f.get());
    *out = f.release();
    return 0;
}

// Argument checks the queries share; 1: nothing to do (M = 0), 0: go on.
static int fit_query_check(gaplac_fit* f, int64_t M, const double* Xs, int64_t ldxs) {
    if (!f || !f->ctx) return GAPLAC_E_ARG;
    gaplac_ctx* ctx = f->ctx;
    if (M < 0) return set_err(ctx, GAPLAC_E_ARG, "M = %lld < 0", (long long)M);
    if (M > 0 && f->D > 0 && (!Xs || ldxs < M))
        return set_err(ctx, GAPLAC_E_ARG, "Xs NULL or ldxs %lld < M %lld", (long long)ldxs, (long long)M);
    return M == 0 ? 1 : 0;
}

// rows [r0, r0 + m) of the host block Xs into the fit's test inputs (ld m)
static int fit_upload_xs(gaplac_fit* f, int64_t r0, int64_t m, const double* Xs, int64_t ldxs) {
    if (f->D > 0)
        HIPCK(f->ctx, hipMemcpy2DAsync(f->buf + f->d.Xs, (size_t)m * 8, Xs + r0, (size_t)ldxs * 8, (size_t)m * 8,
                                       (size_t)f->D, hipMemcpyHostToDevice, f->ctx->s_main));
    return 0;
}

extern "C" int gaplac_fit_mean(gaplac_fit* f, int64_t M, const double* Xs, int64_t ldxs, double* out_mean) {
    for (int64_t j = 0; out_mean && j < M; ++j) out_mean[j] = NAN;
    int rc = fit_query_check(f, M, Xs, ldxs);
    if (rc) return rc > 0 ? 0 : rc;
    gaplac_ctx* ctx = f->ctx;
    if (!out_mean) return set_err(ctx, GAPLAC_E_ARG, "out_mean is NULL");
    if (f->N == 0) {
        for (int64_t j = 0; j < M; ++j) out_mean[j] = 0.0;
        return 0;
    }
    HIPCK(ctx, hipSetDevice(f->device));
    const FitDims& d = f->d;
    hipStream_t s = ctx->s_main;
    for (int64_t r0 = 0; r0 < M; r0 += d.qc) {
        const int64_t m = std::min(d.qc, M - r0);
        if ((rc = fit_upload_xs(f, r0, m, Xs, ldxs))) return rc;
        if ((rc = guarded_on(ctx, f->buf, (size_t)d.elems, nullptr, 0, [&] { fit_mean_launches(s, d, f->N, m, f->buf); })))
            return rc;
        HIPCK(ctx, hipMemcpyAsync(out_mean + r0, f->buf + d.mean, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIPCK(ctx, hipStreamSynchronize(s));
    }
    return 0;
}

extern "C" int gaplac_fit_mean_var(gaplac_fit* f, int64_t M, const double* Xs, int64_t ldxs, double* out_mean,
                                   double* out_var) {
    if (!out_var) return gaplac_fit_mean(f, M, Xs, ldxs, out_mean);
    for (int64_t j = 0; j < M; ++j) {
        if (out_mean) out_mean[j] = NAN;
        out_var[j] = NAN;
    }
    int rc = fit_query_check(f, M, Xs, ldxs);
    if (rc) return rc > 0 ? 0 : rc;
    gaplac_ctx* ctx = f->ctx;
    if (f->N == 0) {  // the prior
        for (int64_t j = 0; j < M; ++j) {
            if (out_mean) out_mean[j] = 0.0;
            out_var[j] = host_kdiag(f->tp, Xs, ldxs, j);
        }
        return 0;
    }
    HIPCK(ctx, hipSetDevice(f->device));
    const FitDims& d = f->d;
    hipStream_t s = ctx->s_main;
    for (int64_t r0 = 0; r0 < M; r0 += f->cap) {
        const int64_t m = std::min(f->cap, M - r0);
        if ((rc = fit_upload_xs(f, r0, m, Xs, ldxs))) return rc;
        if ((rc = guarded_on(ctx, f->buf, (size_t)d.elems, nullptr, 0,
                             [&] { fit_query_launches(s, d, f->N, m, ctx->spw, f->buf, f->kind == 1); })))
            return rc;
        if (out_mean) HIPCK(ctx, hipMemcpyAsync(out_mean + r0, f->buf + d.mean, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIPCK(ctx, hipMemcpyAsync(out_var + r0, f->buf + d.var, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIPCK(ctx, hipStreamSynchronize(s));
    }
    return 0;
}

// The joint covariance of M <= cap test points from a fit of either kind (§10.15): the query's rows
// and mean, then launch_post_cov + launch_mirror_lower reading the rows from the fit's buffer.
extern "C" int gaplac_fit_mean_cov(gaplac_fit* f, int64_t M, const double* Xs, int64_t ldxs, double noise_s,
                                   double* out_mean, double* out_cov, int64_t ldc) {
    if (!f || !f->ctx) return GAPLAC_E_ARG;
    gaplac_ctx* ctx = f->ctx;
    if (M < 0 || (out_cov && ldc < M))
        return set_err(ctx, GAPLAC_E_ARG, "M = %lld < 0 or ldc %lld < M", (long long)M, (long long)ldc);
    nan_mean_cov(M, out_mean, out_cov, ldc);
    if (M > f->cap)
        return set_err(ctx, GAPLAC_E_ARG, "M = %lld > cap = %lld: the joint covariance takes one chunk of test points",
                       (long long)M, (long long)f->cap);
    int rc = fit_query_check(f, M, Xs, ldxs);
    if (rc < 0) return rc;
    if (!(noise_s >= 0.0) || !std::isfinite(noise_s))
        return set_err(ctx, GAPLAC_E_ARG, "noise_s %g must be finite and >= 0", noise_s);
    if (rc > 0) return 0;
    if (!out_cov) return gaplac_fit_mean(f, M, Xs, ldxs, out_mean);
    if (f->N == 0)  // the prior
        return prior_mean_cov(ctx, f->D, (int32_t)f->terms.size(), f->terms.data(), M, Xs, ldxs, noise_s, out_mean,
                              out_cov, ldc);
    HIPCK(ctx, hipSetDevice(f->device));
    const FitDims& d = f->d;
    hipStream_t s = ctx->s_main;
    const int64_t ldb = round_up(M + 1, NB);
    if ((rc = ensure(ctx, &ctx->B, &ctx->B_elems, (size_t)ldb * (size_t)ldb))) return rc;
    if ((rc = fit_upload_xs(f, 0, M, Xs, ldxs))) return rc;
    TermPack tp = f->tp;
    tp.noise = noise_s;
    *ctx->htp = tp;  // (nothing of the context's is in flight: every entry waits for its own work)
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, s));
    if ((rc = guarded_on(ctx, f->buf, (size_t)d.elems, ctx->B, ctx->B_elems, [&] {
             fit_query_launches(s, d, f->N, M, ctx->spw, f->buf, f->kind == 1);
             fit_cov_launches(s, d, f->N, M, f->buf, ctx->B, ldb, ctx->dtp);
         }))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    return read_mean_cov(ctx, M, ctx->B, ldb, f->buf + d.mean, out_mean, out_cov, ldc);
}

// ---------------------------------------------------------------------------------
// Laplace approximation: Newton's iteration on the host, every vector on
// the device, one factorisation of the prebuilt B per step through eval_device.
// ---------------------------------------------------------------------------------

// Test points per final factorisation (their rows ride below B); further points take a
// factorisation of their own per chunk.
constexpr int64_t LAP_CHUNK = 4096;

// Where the iteration's vectors lie in the context's buffer (offsets in doubles; at / ft, the
// trial point, last: a buffer one element short is reported by the line search's launch), and
// the workspace's size: the matrix with the first chunk's riding rows, then u (N values).
struct LapDims {
    int64_t Np, nb, nkm, qc, ldq;
    int nt;
    int64_t a, f, g, w, sw, b, c, an, fn, diag, part, lpart, out, mean, at, ft, elems;
    int64_t u, a_elems;  // in the workspace
    // the gradient (§10.14): diag B^{-1}, s2, q = K s2, t = Y^T q, r = Y t, launch_alpha's second
    // output, the partial sums (the row scaling's, the products' and the bilinear form's), the
    // implicit parts, and u last (the bilinear form's launch reports a buffer one element short)
    int64_t dbinv, s2, q, tv, yt, dvs, gpart, gimp, ug;
};
static LapDims lap_dims(int64_t N, int64_t M, bool grad = false) {
    LapDims d{};
    d.Np = round_up(N + 1, NB);
    d.nt = (int)(d.Np / NB);
    d.nb = (N + 255) / 256;
    d.nkm = (N + 255) / 256;
    d.qc = std::min(M, LAP_CHUNK);
    d.ldq = d.Np + NB * ((d.qc + NB - 1) / NB);
    int64_t o = 0;
    for (int64_t* p : {&d.a, &d.f, &d.g, &d.w, &d.sw, &d.b, &d.c, &d.an, &d.fn, &d.diag}) {
        *p = o;
        o += N;
    }
    d.part = o;
    o += d.nkm * std::max(N, d.qc);
    d.lpart = o;
    o += 3 * d.nb;
    d.out = o;
    o += 4;
    d.mean = o;
    o += d.qc;
    d.at = o;
    o += N;
    d.ft = o;
    o += N;
    if (grad) {  // (M = 0) the final factorisation carries identity rows: lda = 2 Np
        d.ldq = 2 * d.Np;
        for (int64_t* p : {&d.dbinv, &d.s2, &d.q, &d.tv, &d.yt, &d.dvs}) {
            *p = o;
            o += N;
        }
        d.gpart = o;
        o += std::max(((N + NB - 1) / NB) * N, laplace_grad_bilinear_blocks(N) * (GAPLAC_MAX_TERMS + 1));
        d.gimp = o;
        o += GAPLAC_MAX_TERMS + 1;
        d.ug = o;
        o += N;
    }
    d.elems = o;
    d.u = d.ldq * d.Np;
    d.a_elems = d.u + N;
    return d;
}

// The stages' launches, run by the entries and walked dry by gaplac_plan_check_laplace. Each runs
// under one guard: lap_mf_launches under the vectors' buffer alone (launch_fit_mean checks its
// scratch against the guard's first allocation), the others under the workspace (first), the
// vectors' buffer (second) and the response matrix (third).
// The likelihood at (a, f): g, W, sw, b and the sums.
static void lap_lik_launches(hipStream_t s, const LapDims& d, int64_t N, int lik, double param, const double* y,
                             double* lap) {
    launch_laplace_lik(s, N, lik, param, y, lap + d.a, lap + d.f, lap + d.g, lap + d.w, lap + d.sw, lap + d.b,
                       lap + d.lpart, lap + d.out);
}
// out = K(xs, X) v, matrix-free, without K's diagonal part (m points at Xs, ld ldxs).
static void lap_mf_launches(hipStream_t s, const LapDims& d, int64_t N, int64_t m, const double* X, const double* Xs,
                            int64_t ldxs, const TermPack* dtp, double* lap, int64_t v, int64_t out) {
    launch_fit_mean(s, N, m, X, N, lap + v, Xs, ldxs, dtp, lap + d.part, lap + out);
}
// c = K b finished, the Gram (ld lda) and B over it with the right-hand side sw c in row N.
static void lap_build_launches(hipStream_t s, const LapDims& d, int64_t N, int64_t lda, bool finish_c, double* A,
                               const double* X, const double* y, const TermPack* dtp, double* lap) {
    if (finish_c) launch_laplace_axpy_diag(s, N, lap + d.diag, lap + d.b, lap + d.c);
    launch_gram(s, A, lda, N, d.nt, X, N, y, dtp, 0, 0, nullptr);
    launch_laplace_b_build(s, A, lda, N, d.nt, lap + d.sw, lap + d.c);
}
// After the factorisation (ld Np): z out of row N, u = L^{-T} z, a+ = b - sw u.
static void lap_solve_launches(hipStream_t s, const LapDims& d, int64_t N, double* A, double* lap) {
    launch_copy_z(s, A, d.Np, N, A + d.u);
    launch_fit_backsub(s, A, d.Np, N, A + d.u);
    launch_laplace_anew(s, N, lap + d.b, lap + d.sw, A + d.u, lap + d.an);
}
// f+ = K a+ finished.
static void lap_fnew_launches(hipStream_t s, const LapDims& d, int64_t N, double* lap) {
    launch_laplace_axpy_diag(s, N, lap + d.diag, lap + d.an, lap + d.fn);
}
static void lap_trial_launches(hipStream_t s, const LapDims& d, int64_t N, int lik, double param, double step,
                               const double* y, double* lap) {
    launch_laplace_trial(s, N, lik, param, step, y, lap + d.a, lap + d.f, lap + d.an, lap + d.fn, lap + d.at,
                         lap + d.ft, lap + d.lpart, lap + d.out);
}
// A chunk of m test points (ld m at Xs): the Gram and B with m riding rows' room (ld lda), and the
// response matrix diag(sw) K(X, xs) (ld N).
static void lap_query_launches(hipStream_t s, const LapDims& d, int64_t N, int64_t m, int64_t lda, double* A,
                               const double* X, const double* y, const double* Xs, const TermPack* dtp, double* lap,
                               double* Y) {
    lap_build_launches(s, d, N, lda, false, A, X, y, dtp, lap);
    launch_laplace_cross(s, N, m, X, N, Xs, m, dtp, lap + d.sw, Y, N);
}

// The gradient's stages after the final factorisation with identity rows (ld 2 Np, §10.14).
// Y's rows scaled by sw with diag B^{-1} on the way, and s2.
static void lap_grad_scale_launches(hipStream_t s, const LapDims& d, int64_t N, int lik, double* A, double* lap) {
    launch_laplace_grad_scale(s, A, 2 * d.Np, d.Np, N, lap + d.sw, lap + d.gpart, lap + d.dbinv);
    launch_laplace_grad_s2(s, N, lik, lap + d.f, lap + d.dbinv, lap + d.s2);
}
// q = K s2 finished (its matrix-free part: lap_mf_launches), t = Y^T q, r = Y t, u = s2 - r.
static void lap_grad_solve_launches(hipStream_t s, const LapDims& d, int64_t N, const double* A, double* lap) {
    launch_laplace_axpy_diag(s, N, lap + d.diag, lap + d.s2, lap + d.q);
    launch_laplace_grad_tmv(s, A, 2 * d.Np, d.Np, N, lap + d.q, lap + d.gpart, lap + d.tv);
    launch_alpha(s, A, 2 * d.Np, d.Np, N, lap + d.tv, lap + d.gpart, lap + d.yt, lap + d.dvs);
    launch_laplace_grad_u(s, N, lap + d.s2, lap + d.yt, lap + d.ug);
}
// The implicit part of every parameter and of the jitter.
static void lap_grad_bilinear_launches(hipStream_t s, const LapDims& d, int64_t N, int T, const double* X,
                                       const TermPack* dtp, const GradTermPack* dgp, double* lap) {
    launch_laplace_grad_bilinear(s, N, T, X, N, lap + d.ug, lap + d.a, dtp, dgp, lap + d.gpart, lap + d.gimp);
}

template <typename Launches>
static int lap_on_ws(gaplac_ctx* ctx, Launches&& launches) {
    return guarded_on(ctx, ctx->A, ctx->A_elems, ctx->lap, ctx->lap_elems, launches, ctx->dY, ctx->dY_elems);
}
template <typename Launches>
static int lap_on_vectors(gaplac_ctx* ctx, Launches&& launches) {
    return guarded_on(ctx, ctx->lap, ctx->lap_elems, nullptr, 0, launches);
}

// {sum log p, a^T f, psi, non-finite W count} of the last likelihood / trial launch.
static int lap_read_sums(gaplac_ctx* ctx, const LapDims& d, double* h) {
    HIPCK(ctx, hipMemcpyAsync(h, ctx->lap + d.out, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

static int lap_bad_w(gaplac_ctx* ctx, int64_t N, double count, int64_t* out_info) {
    if (out_info) *out_info = 1;
    return set_err(ctx, 1, "B = I + sqrt(W) K sqrt(W) (order %lld) cannot be formed: W is not finite at %.0f "
                           "observations (exp(f) overflows)", (long long)N, count);
}

static int lap_bad_b(gaplac_ctx* ctx, int64_t N, int info, int64_t* out_info) {
    if (out_info) *out_info = info;
    return set_err(ctx, info, "B = I + sqrt(W) K sqrt(W) (order %lld): its Cholesky factorisation failed at leading "
                              "minor %d, which an indefinite matrix cannot cause (B >= I): W or K is not finite",
                   (long long)N, info);
}

namespace {
// What a Laplace entry is asked, in the entries' argument order (a0 may be NULL; M = 0: no test points).
struct LapRequest {
    int64_t N;
    int32_t D;
    const double* X;
    int64_t ldx;
    int32_t T;
    const gaplac_term* terms;
    double jitter;
    int32_t lik;
    double lik_param;
    const double* y;
    int32_t max_iter;
    double tol;
    const double* a0;
    int64_t M;
    const double* Xs;
    int64_t ldxs;
};

// What it may answer (every pointer but logq may be NULL): what all four entries have, first.
struct LapOut {
    double* logq;
    int32_t *iters, *converged;
    int64_t* info;
    double *f, *a;       // the mode and a = K^{-1} f, N values each
    double *mean, *var;  // at the M test points
    // gaplac_laplace_logpdf_grad (§10.14): the final factorisation carries identity rows
    bool grad;
    double *dparam, *djitter, *implicit;  // T, 1 and T + 1 values
    // gaplac_laplace_fit_create (§10.15): a fit of kind 1 with room for cap test points, out through *fit
    gaplac_fit** fit;
    int64_t cap;
};

struct LapResult {  // what the iteration and the final factorisation leave for the answer
    double logq, logdet, atf;
    int iters;
    bool converged;
};

// The create-time launches of a Laplace fit after the final factorisation: the factor's lower tiles
// out of the workspace A (ld Np) and sw, f, a out of the vectors' buffer (alpha, the buffer's last
// slot, written last: a buffer one element short is reported).
static void lap_fit_create_launches(hipStream_t s, const FitDims& d, const LapDims& ld, int64_t N, const double* A,
                                    const double* lap, double* buf) {
    launch_fit_copy(s, A, d.Np, d.nt, buf + d.L, d.ldl);
    launch_fit_vectors_copy(s, N, lap + ld.sw, lap + ld.f, lap + ld.a, buf + d.sw, buf + d.fhat, buf + d.alpha);
}

// The buffer of a Laplace fit out of the context after the final factorisation of B (ld Np in the
// workspace, M = 0, no identity rows): the factor's lower tiles, Dinv, X and the pack as
// gaplac_fit_create copies them, and sw, f, a out of the vectors' buffer.
static int lap_fit_fill(gaplac_ctx* ctx, gaplac_fit* f, const LapDims& ld) {
    const int64_t N = f->N;
    f->d = fit_dims(N, f->D, f->cap, true);
    const FitDims& d = f->d;
    if (hipMalloc(reinterpret_cast<void**>(&f->buf), (size_t)d.elems * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        f->buf = nullptr;
        return set_err(ctx, GAPLAC_E_OOM, "hipMalloc of the fit's %lld bytes failed", (long long)d.elems * 8);
    }
    hipStream_t s = ctx->s_main;
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(f->buf);
        f->buf = nullptr;
        return rc;
    };
    int rc = guarded_on(ctx, f->buf, (size_t)d.elems, ctx->A, ctx->A_elems,
                        [&] { lap_fit_create_launches(s, d, ld, N, ctx->A, ctx->lap, f->buf); }, ctx->lap, ctx->lap_elems);
    if (rc) return fail(rc);
    const struct {
        int64_t dst;
        const void* src;
        size_t bytes;
    } copies[] = {{d.dinv, ctx->Dinv, (size_t)d.nt * DINV_PER_BLOCK * 8},
                  {d.X, ctx->dX, (size_t)N * f->D * 8},
                  {d.tp, ctx->dtp, sizeof(TermPack)}};
    for (const auto& c : copies)
        if (c.bytes && hipMemcpyAsync(f->buf + c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(set_err(ctx, GAPLAC_E_HIP, "copy into the fit's buffer: %s", hipGetErrorString(hipGetLastError())));
    if (hipStreamSynchronize(s) != hipSuccess)
        return fail(set_err(ctx, GAPLAC_E_HIP, "fit's buffer: %s", hipGetErrorString(hipGetLastError())));
    return 0;
}

// The handle of a finished call, registered with the context and handed out through *o.fit: the
// empty fit (d null, N = 0: the prior at every query), or the one filled by lap_fit_fill.
static int lap_fit_hand_out(gaplac_ctx* ctx, const LapRequest& q, const LapOut& o, const TermPack& tp,
                            const LapDims* d, const LapResult& res) {
    std::unique_ptr<gaplac_fit> f(new gaplac_fit());
    f->device = ctx->device;
    f->N = q.N;
    f->cap = o.cap;
    f->D = q.D;
    f->tp = tp;
    f->tp.noise = q.jitter;
    f->terms.assign(q.terms, q.terms + q.T);
    f->kind = 1;
    f->lik = q.lik;
    f->lik_param = q.lik_param;
    f->jitter = q.jitter;
    f->logpdf = res.logq;
    f->logdet = res.logdet;
    f->quad = res.atf;
    f->iters = res.iters;
    f->converged = res.converged ? 1 : 0;
    int rc;
    if (d && (rc = lap_fit_fill(ctx, f.get(), *d))) return rc;
    f->ctx = ctx;
    ctx->fits.push_back(f.get());
    *o.fit = f.release();
    return 0;
}

// v into every value the entry may write, 0 into its counters: NaN before any check, 0 without observations.
static void lap_fill_out(const LapRequest& q, const LapOut& o, double v) {
    if (o.logq) *o.logq = v;
    if (o.djitter) *o.djitter = v;
    for (int t = 0; o.dparam && t < q.T && t < GAPLAC_MAX_TERMS; ++t) o.dparam[t] = v;
    for (int t = 0; o.implicit && t <= q.T && t <= GAPLAC_MAX_TERMS; ++t) o.implicit[t] = v;
    if (o.iters) *o.iters = 0;
    if (o.converged) *o.converged = 0;
    if (o.info) *o.info = 0;
    for (double* p : {o.f, o.a})
        for (int64_t i = 0; p && i < q.N; ++i) p[i] = v;
    for (double* p : {o.mean, o.var})
        for (int64_t j = 0; p && j < q.M; ++j) p[j] = v;
}

// Whether an observation v lies in the likelihood's support.
static bool lik_supports(int lik, double v) {
    return lik == GAPLAC_LIK_BERNOULLI ? (v == 0.0 || v == 1.0)
           : lik == GAPLAC_LIK_POISSON ? (std::isfinite(v) && v >= 0.0 && v == std::floor(v))
                                       : std::isfinite(v);
}

// The argument checks, the pack and the observations' support.
static int lap_check(gaplac_ctx* ctx, const LapRequest& q, const LapOut& o, TermPack* tp) {
    int rc = check_common(ctx, q.N, q.D, q.X, q.ldx, 0.0, q.y);
    if (rc) return rc;
    if (q.M < 0 || (q.M > 0 && q.D > 0 && (!q.Xs || q.ldxs < q.M)))
        return set_err(ctx, GAPLAC_E_ARG, "M < 0, or Xs NULL / ldxs < M");
    if (!o.logq) return set_err(ctx, GAPLAC_E_ARG, "out_logq is NULL");
    if (o.fit && o.cap < 1) return set_err(ctx, GAPLAC_E_ARG, "cap = %lld < 1", (long long)o.cap);
    if (q.lik != GAPLAC_LIK_GAUSSIAN && q.lik != GAPLAC_LIK_BERNOULLI && q.lik != GAPLAC_LIK_POISSON)
        return set_err(ctx, GAPLAC_E_KIND, "unknown likelihood %d", q.lik);
    if (!(q.jitter >= 0.0) || !std::isfinite(q.jitter))
        return set_err(ctx, GAPLAC_E_PARAM, "jitter %g must be finite and >= 0", q.jitter);
    if (!(q.tol > 0.0) || !std::isfinite(q.tol))
        return set_err(ctx, GAPLAC_E_PARAM, "tol %g must be finite and > 0", q.tol);
    if (q.max_iter < 1) return set_err(ctx, GAPLAC_E_PARAM, "max_iter = %d < 1", q.max_iter);
    if (q.lik == GAPLAC_LIK_GAUSSIAN && (!(q.lik_param > 0.0) || !std::isfinite(q.lik_param)))
        return set_err(ctx, GAPLAC_E_PARAM, "the Gaussian likelihood's variance %g must be finite and > 0", q.lik_param);
    if ((rc = pack_terms(ctx, q.D, q.T, q.terms, tp))) return rc;
    for (int64_t i = 0; i < q.N; ++i)
        if (!lik_supports(q.lik, q.y[i]))
            return set_err(ctx, GAPLAC_E_PARAM, "y[%lld] = %g is outside the likelihood's support", (long long)i, q.y[i]);
    for (int64_t i = 0; q.a0 && i < q.N; ++i)
        if (!std::isfinite(q.a0[i])) return set_err(ctx, GAPLAC_E_PARAM, "a0[%lld] is not finite", (long long)i);
    return 0;
}

// The inputs, the buffers and the packs onto the device, K's diagonal part, and the start:
// a = a0 and f = K a, or both 0. *singletons: the gradient's groups are single terms.
static int lap_upload(gaplac_ctx* ctx, const LapRequest& q, const LapDims& d, const TermPack& tp, bool grad,
                      bool* singletons) {
    int rc;
    const int64_t N = q.N;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, q.D, q.X, q.ldx, q.y))) return rc;
    if ((rc = ensure(ctx, &ctx->A, &ctx->A_elems, (size_t)d.a_elems))) return rc;
    if ((rc = ensure(ctx, &ctx->lap, &ctx->lap_elems, (size_t)d.elems))) return rc;
    if (d.qc > 0 && (rc = ensure(ctx, &ctx->dY, &ctx->dY_elems, (size_t)N * (size_t)d.qc))) return rc;
    hipStream_t s = ctx->s_main;
    double* const lap = ctx->lap;
    *ctx->htp = tp;
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, s));
    if (grad) {  // the product groups' bounds, as gaplac_logpdf_grad packs them
        GradTermPack gp{};
        *singletons = pack_groups(q.T, q.terms, &gp);
        *ctx->hgp = gp;
        HIPCK(ctx, hipMemcpyAsync(ctx->dgp, ctx->hgp, sizeof(GradTermPack), hipMemcpyHostToDevice, s));
    }
    {
        std::vector<double> diag((size_t)N);
        for (int64_t i = 0; i < N; ++i) diag[(size_t)i] = q.jitter + host_kdiag(tp, q.X, q.ldx, i, nullptr, 0, NOISE_GROUPS_ONLY);
        HIPCK(ctx, hipMemcpyAsync(lap + d.diag, diag.data(), (size_t)N * 8, hipMemcpyHostToDevice, s));
        HIPCK(ctx, hipStreamSynchronize(s));  // (diag is the host's: it ends with this block)
    }
    if (!q.a0) {
        HIPCK(ctx, hipMemsetAsync(lap + d.a, 0, (size_t)N * 8, s));
        HIPCK(ctx, hipMemsetAsync(lap + d.f, 0, (size_t)N * 8, s));
        return 0;
    }
    HIPCK(ctx, hipMemcpyAsync(lap + d.a, q.a0, (size_t)N * 8, hipMemcpyHostToDevice, s));
    if ((rc = lap_on_vectors(ctx, [&] { lap_mf_launches(s, d, N, N, ctx->dX, ctx->dX, N, ctx->dtp, lap, d.a, d.f); })))
        return rc;
    return lap_on_ws(ctx, [&] { launch_laplace_axpy_diag(s, N, lap + d.diag, lap + d.a, lap + d.f); });
}

// The likelihood at (a, f) and its sums h; W must be finite.
static int lap_lik_at_iterate(gaplac_ctx* ctx, const LapRequest& q, const LapDims& d, int64_t* out_info, double* h) {
    int rc;
    if ((rc = lap_on_ws(ctx, [&] { lap_lik_launches(ctx->s_main, d, q.N, q.lik, q.lik_param, ctx->dv, ctx->lap); })))
        return rc;
    if ((rc = lap_read_sums(ctx, d, h))) return rc;
    return h[3] > 0.0 ? lap_bad_w(ctx, q.N, h[3], out_info) : 0;
}

// One Newton step from (a, f) with its halving line search. *moved: a step was accepted and is
// the new iterate; *converged: and psi changed by no more than tol (relative).
static int lap_newton_step(gaplac_ctx* ctx, const LapRequest& q, const LapDims& d, const TermPack& tp,
                           int64_t* out_info, bool* moved, bool* converged) {
    int rc;
    const int64_t N = q.N;
    hipStream_t s = ctx->s_main;
    double* const lap = ctx->lap;
    const double* const dy = ctx->dv;
    double h[4];
    EvalResult r;
    *moved = *converged = false;
    // the likelihood at (a, f); c = K b; K and B; the factorisation
    if ((rc = lap_lik_at_iterate(ctx, q, d, out_info, h))) return rc;
    const double psi_old = h[2];
    if ((rc = lap_on_vectors(ctx, [&] { lap_mf_launches(s, d, N, N, ctx->dX, ctx->dX, N, ctx->dtp, lap, d.b, d.c); })))
        return rc;
    if ((rc = lap_on_ws(ctx, [&] { lap_build_launches(s, d, N, d.Np, true, ctx->A, ctx->dX, dy, ctx->dtp, lap); })))
        return rc;
    if ((rc = eval_device(ctx, N, q.D, tp, ExtraRows{}.on_prebuilt(), &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr))) return lap_bad_b(ctx, N, rc, out_info);
    // u = B^{-1} (sw c), a+ = b - sw u, f+ = K a+
    if ((rc = lap_on_ws(ctx, [&] { lap_solve_launches(s, d, N, ctx->A, lap); }))) return rc;
    if ((rc = lap_on_vectors(ctx, [&] { lap_mf_launches(s, d, N, N, ctx->dX, ctx->dX, N, ctx->dtp, lap, d.an, d.fn); })))
        return rc;
    if ((rc = lap_on_ws(ctx, [&] { lap_fnew_launches(s, d, N, lap); }))) return rc;
    // the step: the first s = 1, 1/2, ... whose psi is finite and no worse than psi_old (to rounding)
    double step = 1.0, psi_new = NAN;
    for (int hv = 0; hv <= 20 && !*moved; ++hv, step *= 0.5) {
        if ((rc = lap_on_ws(ctx, [&] { lap_trial_launches(s, d, N, q.lik, q.lik_param, step, dy, lap); }))) return rc;
        if ((rc = lap_read_sums(ctx, d, h))) return rc;
        psi_new = h[2];
        *moved = std::isfinite(psi_new) && psi_new >= psi_old - q.tol * (1.0 + std::fabs(psi_old));
    }
    if (!*moved) return 0;  // no acceptable step: the iterate stays
    HIPCK(ctx, hipMemcpyAsync(lap + d.a, lap + d.at, (size_t)N * 8, hipMemcpyDeviceToDevice, s));
    HIPCK(ctx, hipMemcpyAsync(lap + d.f, lap + d.ft, (size_t)N * 8, hipMemcpyDeviceToDevice, s));
    *converged = std::fabs(psi_new - psi_old) <= q.tol * (1.0 + std::fabs(psi_new));
    return 0;
}

// The final factorisation of B with one chunk of test points riding (rows [r0, r0 + m) of Xs, their mean
// and variance out), or with M = 0 plain (the gradient: with its identity rows, which leave Y = L^{-T}).
static int lap_final_chunk(gaplac_ctx* ctx, const LapRequest& q, const LapOut& o, const LapDims& d,
                           const TermPack& tp, int64_t r0, bool singletons, EvalResult* r) {
    int rc;
    const int64_t N = q.N, m = std::min(LAP_CHUNK, q.M - r0);
    hipStream_t s = ctx->s_main;
    double* const lap = ctx->lap;
    ExtraRows xr;
    if (m > 0) {
        const int64_t lda = d.Np + NB * ((m + NB - 1) / NB);
        if ((rc = upload_test_inputs(ctx, q.D, m, 0, m, q.Xs + r0, q.ldxs))) return rc;
        if ((rc = lap_on_ws(ctx, [&] {
                 lap_query_launches(s, d, N, m, lda, ctx->A, ctx->dX, ctx->dv, ctx->dXs, ctx->dtp, lap, ctx->dY);
             })))
            return rc;
        xr = ExtraRows::responses(m, ctx->dY, N);
    } else {
        if (o.grad) xr = ExtraRows::identity(N, singletons).deferred();
        if ((rc = lap_on_ws(ctx, [&] {
                 lap_build_launches(s, d, N, o.grad ? 2 * d.Np : d.Np, false, ctx->A, ctx->dX, ctx->dv, ctx->dtp, lap);
             })))
            return rc;
    }
    if ((rc = eval_device(ctx, N, q.D, tp, xr.on_prebuilt(), r))) return rc;
    if ((rc = finish(*r, nullptr, nullptr, nullptr))) return lap_bad_b(ctx, N, rc, o.info);
    if (m <= 0) return 0;
    if ((rc = lap_on_vectors(ctx, [&] { lap_mf_launches(s, d, N, m, ctx->dX, ctx->dXs, m, ctx->dtp, lap, d.a, d.mean); })))
        return rc;
    std::vector<double> quad((size_t)m);
    HIPCK(ctx, hipMemcpyAsync(quad.data(), ctx->mres, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    if (o.mean) HIPCK(ctx, hipMemcpyAsync(o.mean + r0, lap + d.mean, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIPCK(ctx, hipStreamSynchronize(s));
    for (int64_t j = 0; o.var && j < m; ++j) o.var[r0 + j] = host_kdiag(tp, q.Xs, q.ldxs, r0 + j) - quad[(size_t)j];
    return 0;
}

// The gradient's stages after the final factorisation with identity rows: Y's rows times sw (Y Y^T = R)
// and diag B^{-1}; s2, q = K s2, u = s2 - R q; the explicit part by the gradient's ending with alpha = a
// (into ctx->hgout); the implicit part matrix-free, into himp (T + 1 values, once s_main has retired).
static int lap_grad_stages(gaplac_ctx* ctx, const LapRequest& q, const LapDims& d, bool singletons, double* himp) {
    int rc, erc = 0;
    const int64_t N = q.N;
    hipStream_t s = ctx->s_main;
    double* const lap = ctx->lap;
    EvalScope scope(ctx, ExtraRows::identity(N, singletons));
    if ((rc = lap_on_ws(ctx, [&] { lap_grad_scale_launches(s, d, N, q.lik, ctx->A, lap); }))) return rc;
    if ((rc = lap_on_vectors(ctx, [&] { lap_mf_launches(s, d, N, N, ctx->dX, ctx->dX, N, ctx->dtp, lap, d.s2, d.q); })))
        return rc;
    if ((rc = lap_on_ws(ctx, [&] { lap_grad_solve_launches(s, d, N, ctx->A, lap); }))) return rc;
    if ((rc = lap_on_ws(ctx, [&] { erc = enqueue_grad_ending(ctx, N, d.Np, 2 * d.Np, lap + d.a); }))) return rc;
    if (erc) return erc;
    if ((rc = lap_on_ws(ctx, [&] { lap_grad_bilinear_launches(s, d, N, q.T, ctx->dX, ctx->dtp, ctx->dgp, lap); })))
        return rc;
    HIPCK(ctx, hipMemcpyAsync(himp, lap + d.gimp, (size_t)(q.T + 1) * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

// Shared body of gaplac_laplace_logpdf, gaplac_laplace_posterior_mean_var (q.M test points),
// gaplac_laplace_logpdf_grad (o.grad) and gaplac_laplace_fit_create (o.fit), phase by phase.
static int laplace_impl(gaplac_ctx* ctx, const LapRequest& q, const LapOut& o) {
    lap_fill_out(q, o, NAN);
    TermPack tp;
    int rc = lap_check(ctx, q, o, &tp);
    if (rc) return rc;
    if (q.N == 0) {  // no observations: log q = 0, a zero gradient, the prior at the test points, the empty fit
        lap_fill_out(q, o, 0.0);
        if (o.converged) *o.converged = 1;
        for (int64_t j = 0; o.var && j < q.M; ++j) o.var[j] = host_kdiag(tp, q.Xs, q.ldxs, j);
        return o.fit ? lap_fit_hand_out(ctx, q, o, tp, nullptr, LapResult{0.0, 0.0, 0.0, 0, true}) : 0;
    }
    tp.noise = q.jitter;
    const int64_t N = q.N;
    const LapDims d = lap_dims(N, q.M, o.grad);
    if ((d.qc + NB - 1) / NB > 65535 || (N + NB - 1) / NB > 65535 || (o.fit && (o.cap + NB - 1) / NB > 65535))
        return set_err(ctx, GAPLAC_E_OOM, "more than 65535 tile rows in one call");
    bool singletons = true;
    if ((rc = lap_upload(ctx, q, d, tp, o.grad, &singletons))) return rc;
    LapResult res{NAN, NAN, NAN, 0, false};
    for (int it = 0; it < q.max_iter && !res.converged; ++it) {
        bool moved;
        if ((rc = lap_newton_step(ctx, q, d, tp, o.info, &moved, &res.converged))) return rc;
        if (!moved) break;  // not converged
        ++res.iters;
    }
    // W at the last iterate, B factored once more (with the first chunk of test points riding)
    double h[4];
    if ((rc = lap_lik_at_iterate(ctx, q, d, o.info, h))) return rc;
    res.atf = h[1];
    for (int64_t r0 = 0; r0 == 0 || r0 < q.M; r0 += LAP_CHUNK) {
        EvalResult r;
        if ((rc = lap_final_chunk(ctx, q, o, d, tp, r0, singletons, &r))) return rc;
        if (r0 == 0) res.logq = h[2] - 0.5 * r.logdet;
        res.logdet = r.logdet;
    }
    double himp[GAPLAC_MAX_TERMS + 1];
    if (o.grad && (rc = lap_grad_stages(ctx, q, d, singletons, himp))) return rc;
    hipStream_t s = ctx->s_main;
    if (o.f) HIPCK(ctx, hipMemcpyAsync(o.f, ctx->lap + d.f, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    if (o.a) HIPCK(ctx, hipMemcpyAsync(o.a, ctx->lap + d.a, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    HIPCK(ctx, hipStreamSynchronize(s));
    // (the fit: M = 0, no gradient: the workspace holds B's factor with ld Np)
    if (o.fit && (rc = lap_fit_hand_out(ctx, q, o, tp, &d, res))) return rc;
    if (o.grad) {  // explicit (ctx->hgout, copied by the ending) + implicit
        for (int t = 0; o.dparam && t < q.T; ++t) o.dparam[t] = ctx->hgout[t] + himp[t];
        if (o.djitter) *o.djitter = ctx->hgout[q.T] + himp[q.T];
        for (int t = 0; o.implicit && t <= q.T; ++t) o.implicit[t] = himp[t];
    }
    *o.logq = res.logq;
    if (o.iters) *o.iters = res.iters;
    if (o.converged) *o.converged = res.converged ? 1 : 0;
    return 0;
}

// ---- parts that several plan checks share ----
// The Laplace entries' two guards over fake regions: the twins of lap_on_ws and lap_on_vectors.
struct LapWalk {
    PlanWalk& w;
    int64_t a_elems, l_elems, y_elems;
    double *const fa = PlanWalk::region(0), *const fl = PlanWalk::region(1), *const fy = PlanWalk::region(2);
    template <typename L> void on_ws(L&& run) { w.on(fa, a_elems, fl, l_elems, run, y_elems ? fy : nullptr, y_elems); }
    template <typename L> void on_vectors(L&& run) { w.on(fl, l_elems, nullptr, 0, run); }
};

// lap_newton_step with one trial point, then the likelihood at the new iterate: both Laplace walks' start.
static void walk_lap_iteration(LapWalk& lw, const LapDims& d, int64_t N) {
    double *const fa = lw.fa, *const fl = lw.fl;
    const int lik = GAPLAC_LIK_POISSON;
    lw.on_ws([&] { lap_lik_launches(nullptr, d, N, lik, 0.0, nullptr, fl); });
    lw.on_vectors([&] { lap_mf_launches(nullptr, d, N, N, nullptr, nullptr, N, nullptr, fl, d.b, d.c); });
    lw.on_ws([&] { lap_build_launches(nullptr, d, N, d.Np, true, fa, nullptr, nullptr, nullptr, fl); });
    lw.w.eval(N, ExtraRows{}.on_prebuilt());
    lw.on_ws([&] { lap_solve_launches(nullptr, d, N, fa, fl); });
    lw.on_vectors([&] { lap_mf_launches(nullptr, d, N, N, nullptr, nullptr, N, nullptr, fl, d.an, d.fn); });
    lw.on_ws([&] { lap_fnew_launches(nullptr, d, N, fl); });
    lw.on_ws([&] { lap_trial_launches(nullptr, d, N, lik, 0.0, 1.0, nullptr, fl); });
    lw.on_ws([&] { lap_lik_launches(nullptr, d, N, lik, 0.0, nullptr, fl); });
}

// The sparse entries' three stages (see gaplac_plan_check_sparse), also the first part of the sparse
// gradient's and the sparse joint walks. false, and nothing walked: the arguments are out of range.
static bool walk_sparse(PlanWalk& w, int64_t N, int64_t Mz, int64_t Ms, int32_t short_ws) {
    if (N < 1 || Mz < 1 || Ms < 0 || w.spw < 1 || w.spw > 8 || short_ws < 0 || short_ws > 2) return false;
    if ((N + Ms + NB - 1) / NB > 65535) return false;
    const SparseDims d = sparse_dims(N, Mz, Ms);
    double *const fa = PlanWalk::region(0), *const fb = PlanWalk::region(1);
    const int64_t a_elems = d.lda * d.Np - (short_ws == 1 ? 1 : 0), b_elems = d.ldb * d.Np - (short_ws == 2 ? 1 : 0);
    w.eval(Mz, ExtraRows::test_points(N + Ms), short_ws == 1 ? 1 : 0);
    w.on(fa, a_elems, fb, b_elems, [&] {
        sparse_s_launches(nullptr, d, N, Mz, fa, nullptr, nullptr, fb, 1.0);
        sparse_rows_launches(nullptr, d, N, Mz, Ms, fa, nullptr);
    });
    const ExtraRows rows = Ms > 0 ? ExtraRows::responses(Ms, nullptr, 0) : ExtraRows{};
    w.eval(Mz, rows.on_prebuilt(), short_ws == 2 ? 1 : 0);
    w.on(fb, b_elems, nullptr, 0, [&] { sparse_post_launches(nullptr, d, Mz, Ms, 1.0, fb, nullptr, nullptr, nullptr); });
    return true;
}
}  // namespace

extern "C" {

int gaplac_abi_version(void) { return GAPLAC_ABI_VERSION; }

const char* gaplac_last_error(const gaplac_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int gaplac_ctx_create(int device, gaplac_ctx** out) {
    if (!out) return GAPLAC_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GAPLAC_E_NODEVICE;
    if (device < 0 || device >= n) return GAPLAC_E_NODEVICE;
    gaplac_ctx* ctx = new gaplac_ctx();
    ctx->device = device;
    // the schedule switches
    if (const char* s = std::getenv("GAPLAC_SERIAL")) ctx->serial = s[0] == '1';
    if (const char* s = std::getenv("GAPLAC_SPW")) ctx->spw = std::max(1, std::min(8, std::atoi(s)));
    if (const char* s = std::getenv("GAPLAC_PAIR_M")) ctx->pair_m = std::max(0, std::atoi(s));
    if (const char* s = std::getenv("GAPLAC_BAND_TILES_M")) ctx->band_tiles_m = std::max(1, std::atoi(s));
    if (const char* s = std::getenv("GAPLAC_TAIL_SIM")) ctx->tail_sim = s[0] == '0' ? 0 : 1;
    if (const char* s = std::getenv("GAPLAC_GRAD_FUSED")) ctx->grad_fused = s[0] != '0';
    if (const char* s = std::getenv("GAPLAC_BATCH_LANES")) ctx->batch_lanes = std::max(1, std::min(16, std::atoi(s)));
    if (const char* s = std::getenv("GAPLAC_TAILK")) ctx->tailk = s[0] != '0';
    if (ctx->tailk) ctx->tail_s = 80;  // the persistent tail (A/B at N = 16384)
    if (const char* s = std::getenv("GAPLAC_TAIL_S")) ctx->tail_s = std::max(0, std::atoi(s));
    if (const char* s = std::getenv("GAPLAC_TAIL_TRACE")) ctx->ttrace_path = s;  // diagnostics
    if (const char* s = std::getenv("GAPLAC_TAIL_FAULT")) {  // tests only: forced expiry
        ctx->tail_fault = std::atoi(s);
        if (ctx->tail_fault >= 0)
            std::fprintf(stderr,
                         "gaplac: GAPLAC_TAIL_FAULT=%d is set (test hook): the persistent tail skips the diagonal "
                         "block of that tail column and evaluations return GAPLAC_E_HIP\n",
                         ctx->tail_fault);
    }
    if (const char* s = std::getenv("GAPLAC_BATCH_W")) ctx->batch_w = std::max(1, std::min(TAIL_MAX_MODELS, std::atoi(s)));
    if (const char* s = std::getenv("GAPLAC_BATCH_LAG")) ctx->batch_lag = std::max(0, std::atoi(s));
    auto fail = [&](const char* what, hipError_t e) {
        std::fprintf(stderr, "gaplac_ctx_create: %s: %s\n", what, hipGetErrorString(e));
        gaplac_ctx_destroy(ctx);
        return GAPLAC_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    // s_panel: highest priority; s_main: lowest priority. A CU mask that
    // keeps CUs free of s_main's workgroups for the chain (the 512-thread diagonal-block
    // kernel cannot share a CU with a bulk workgroup) and hipGraph replay were both measured
    // slower (round 3, N=16384: no mask 28.8 ms, 4/8/16 CUs 29.8-30.1 ms: the masked bulk
    // kernel lost ~15%) and are not kept.
    int ncu = 0;
    if ((e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess)
        return fail("attribute", e);
    if (ncu > 0) ctx->ncu = ncu;
    int least = 0, greatest = 0;
    if ((e = hipDeviceGetStreamPriorityRange(&least, &greatest)) != hipSuccess)
        return fail("priority range", e);
    if ((e = hipStreamCreateWithPriority(&ctx->s_panel, hipStreamNonBlocking, greatest)) != hipSuccess)
        return fail("stream", e);
    if ((e = hipStreamCreateWithPriority(&ctx->s_main, hipStreamNonBlocking, least)) != hipSuccess)
        return fail("stream", e);
    for (hipEvent_t* ev : ctx_events(ctx))
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return fail("event", e);
    for (const Buf& b : ctx_buffers(ctx))
        if (b.fixed && (e = b.pinned ? hipHostMalloc(b.p, b.fixed, 0) : hipMalloc(b.p, b.fixed)) != hipSuccess)
            return fail(b.pinned ? "hipHostMalloc" : "hipMalloc", e);
    *out = ctx;
    return 0;
}

int gaplac_ctx_destroy(gaplac_ctx* ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)sync_streams(ctx);
    for (gaplac_ctx* c : ctx->lanes) gaplac_ctx_destroy(c);
    for (gaplac_fit* f : ctx->fits) {  // the handles stay valid for gaplac_fit_destroy; every other call fails
        if (f->buf) (void)hipFree(f->buf);
        f->buf = nullptr;
        f->ctx = nullptr;
    }
    ctx->fits.clear();
    if (ctx->borrowed_inputs) {
        ctx->dX = nullptr;
        ctx->dv = nullptr;
    }
    for (hipEvent_t* ev : ctx_events(ctx))
        if (*ev) (void)hipEventDestroy(*ev);
    for (hipEvent_t e : ctx->evpool) (void)hipEventDestroy(e);
    for (const Buf& b : ctx_buffers(ctx)) free_buf(b);
    for (hipStream_t s : {ctx->s_main, ctx->s_panel, ctx->s_extra, ctx->s_xrest})
        if (s) (void)hipStreamDestroy(s);
    delete ctx;
    return 0;
}

int gaplac_ctx_release(gaplac_ctx* ctx) {
    if (!ctx) return GAPLAC_E_ARG;
    HIPCK(ctx, hipSetDevice(ctx->device));
    HIPCK(ctx, sync_streams(ctx));
    for (gaplac_ctx* c : ctx->lanes) gaplac_ctx_destroy(c);
    ctx->lanes.clear();
    for (auto& w : ctx->bw) {
        if (w.busy) HIPCK(ctx, hipEventSynchronize(w.ev_done));
        w.busy = false;
    }
    for (const Buf& b : ctx_buffers(ctx))
        if (b.cap) free_buf(b);  // the large ones: the matrices and their diagonal inverses
    return 0;
}

int gaplac_logpdf_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx,
                         int32_t T, const gaplac_term* terms, double noise, const double* dv,
                         double* out_logpdf, double* out_logdet, double* out_quad) {
    return logpdf_impl(ctx, true, N, D, dX, ldx, T, terms, noise, dv, out_logpdf, out_logdet, out_quad);
}

int gaplac_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                  const gaplac_term* terms, double noise, const double* v, double* out_logpdf,
                  double* out_logdet, double* out_quad) {
    return logpdf_impl(ctx, false, N, D, X, ldx, T, terms, noise, v, out_logpdf, out_logdet, out_quad);
}

int gaplac_logpdf_batch(gaplac_ctx* ctx, int32_t nmodels, int64_t N, int32_t D, const double* X,
                        int64_t ldx, const int32_t* term_offset, const gaplac_term* terms,
                        double noise, const double* v, double* out_logpdf, int64_t* out_info) {
    if (!ctx) return GAPLAC_E_ARG;
    if (nmodels < 0 || (nmodels > 0 && (!term_offset || !out_logpdf || !out_info)))
        return set_err(ctx, GAPLAC_E_ARG, "bad batch arguments");
    for (int m = 0; m < nmodels; ++m) {
        out_logpdf[m] = NAN;
        out_info[m] = 0;
    }
    int rc = check_common(ctx, N, D, X, ldx, noise, v);
    if (rc) return rc;
    std::vector<TermPack> packs((size_t)nmodels);
    for (int m = 0; m < nmodels; ++m) {
        const int32_t a = term_offset[m], b = term_offset[m + 1];
        if (a < 0 || b < a) return set_err(ctx, GAPLAC_E_ARG, "model %d: bad term offsets", m);
        if ((rc = pack_terms(ctx, D, b - a, terms + a, &packs[(size_t)m]))) return rc;
    }
    if (N == 0) {
        for (int m = 0; m < nmodels; ++m) out_logpdf[m] = -0.0;
        return 0;
    }
    HIPCK(ctx, hipSetDevice(ctx->device));
    {
        const int nt = (int)(round_up(N + 1, NB) / NB);
        // Models per batched launch, capped by the free device memory: two workspace sets of
        // bw matrices must fit beside everything else on the device (what the sets already
        // hold is reusable). Below two models per set the lane path runs instead.
        int bwid = std::min(ctx->batch_w, std::max(nmodels, 1));
        if (nmodels >= 2 && whole_in_tail(ctx, nt)) {
            const int64_t Np = (int64_t)nt * NB;
            const size_t per = ((size_t)Np * (size_t)Np + (size_t)nt * DINV_PER_BLOCK) * sizeof(double) +
                               sizeof(TailCtl) + sizeof(EvalResult) + sizeof(TermPack);
            size_t freeb = 0, totalb = 0;
            if (hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
                size_t held = 0;
                for (const auto& w : ctx->bw) held += (w.A_elems + w.Dinv_elems) * sizeof(double);
                const size_t margin = (size_t)2 << 30;  // 2 GiB for everything else
                const size_t budget = freeb + held > margin ? freeb + held - margin : 0;
                bwid = (int)std::min<size_t>((size_t)bwid, budget / (2 * per));
            }
        }
        if (nmodels >= 2 && bwid >= 2 && whole_in_tail(ctx, nt)) {  // batched tail
            for (gaplac_ctx* c : ctx->lanes) HIPCK(ctx, hipStreamSynchronize(c->s_main));
            if ((rc = upload(ctx, N, D, X, ldx, v))) return rc;
            HIPCK(ctx, hipStreamSynchronize(ctx->s_main));  // the Grams read X / v on s_panel
            for (int m = 0; m < nmodels; ++m) packs[(size_t)m].noise = noise;
            int p = 0;
            for (int m0 = 0; m0 < nmodels; m0 += bwid, p ^= 1) {
                const int B = std::min(bwid, nmodels - m0);
                if ((rc = batch_tail_enqueue(ctx, N, packs, m0, B, p, out_logpdf, out_info))) break;
            }
            // collect both sets (also after a failure: nothing of this call stays in flight)
            for (int q = 0; q < 2; ++q) {
                const int r2 = batch_tail_finish(ctx, q, out_logpdf, out_info);
                if (!rc) rc = r2;
            }
            return rc;
        }
    }
    // the lanes borrow dX / dv: nothing of an earlier call may still read them
    for (gaplac_ctx* c : ctx->lanes) HIPCK(ctx, hipStreamSynchronize(c->s_main));
    if ((rc = upload(ctx, N, D, X, ldx, v))) return rc;
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));  // lanes read X / v on their own streams
    // Models in flight on up to batch_lanes lanes (lane 0 = this context): an order-8192
    // evaluation alone fills the chip only ~half the time (its panel chain is a
    // latency-bound critical path), so concurrent models fill the gaps.
    int nl = std::max(1, std::min(ctx->batch_lanes, nmodels));
    {
        // every extra lane holds a whole evaluation workspace: keep the extra lanes that fit
        // in the free device memory beside this context's own workspace (the workspaces
        // already held are reusable; 2 GiB kept free for everything else). Lane 0 is this
        // context: it is never refused here (as a single gaplac_logpdf call would not be);
        // if even its workspace does not fit, ensure_workspace reports the real OOM.
        const int64_t Np = round_up(N + 1, NB);
        const size_t per = (size_t)Np * (size_t)Np * sizeof(double) + (size_t)(Np / NB) * DINV_PER_BLOCK * sizeof(double);
        size_t freeb = 0, totalb = 0;
        if (nl > 1 && hipMemGetInfo(&freeb, &totalb) == hipSuccess) {
            const size_t own = ctx->A_elems * sizeof(double);
            size_t held = 0;
            for (size_t l = 0; l + 1 < (size_t)nl && l < ctx->lanes.size(); ++l) held += ctx->lanes[l]->A_elems * sizeof(double);
            const size_t margin = (size_t)2 << 30;
            const size_t own_need = own >= per ? 0 : per - own;  // lane 0's workspace still to allocate
            const size_t avail = freeb + held;
            const size_t budget = avail > margin + own_need ? avail - margin - own_need : 0;
            nl = 1 + (int)std::min<size_t>((size_t)(nl - 1), budget / per);
        }
    }
    while ((int)ctx->lanes.size() < nl - 1) {
        gaplac_ctx* c = nullptr;
        if ((rc = gaplac_ctx_create(ctx->device, &c))) return set_err(ctx, rc, "batch lane creation failed");
        c->borrowed_inputs = true;
        ctx->lanes.push_back(c);
    }
    std::vector<gaplac_ctx*> lane((size_t)nl, ctx);
    for (int l = 1; l < nl; ++l) {
        gaplac_ctx* c = ctx->lanes[(size_t)l - 1];
        c->dX = ctx->dX;
        c->dX_elems = ctx->dX_elems;
        c->dv = ctx->dv;
        c->dv_elems = ctx->dv_elems;
        lane[(size_t)l] = c;
    }
    for (int l = 0; l < nl; ++l) lane[(size_t)l]->tail_share = nl;
    struct ShareReset {
        std::vector<gaplac_ctx*>& ls;
        ~ShareReset() {
            for (gaplac_ctx* c : ls) c->tail_share = 1;
        }
    } share_reset{lane};
    std::vector<int> pending((size_t)nl, -1);
    auto drain = [&](int l) -> int {
        const int m = pending[(size_t)l];
        if (m < 0) return 0;
        EvalResult r;
        int e = eval_wait(lane[(size_t)l], &r);
        if (e) return set_err(ctx, e, "batch lane %d: %s", l, lane[(size_t)l]->err.c_str());
        out_info[m] = finish(r, &out_logpdf[m], nullptr, nullptr);
        pending[(size_t)l] = -1;
        return 0;
    };
    // on an error, wait for every lane still in flight before returning: they read the
    // borrowed dX / dv, which the next call's upload overwrites
    auto quiesce = [&](int code) -> int {
        for (int l = 0; l < nl; ++l) (void)sync_streams(lane[(size_t)l]);
        return code;
    };
    for (int m = 0; m < nmodels; ++m) {
        const int l = m % nl;
        if ((rc = drain(l))) return quiesce(rc);
        packs[(size_t)m].noise = noise;
        if ((rc = eval_enqueue(lane[(size_t)l], N, D, packs[(size_t)m])))
            return quiesce(set_err(ctx, rc, "batch lane %d: %s", l, lane[(size_t)l]->err.c_str()));
        pending[(size_t)l] = m;
    }
    for (int l = 0; l < nl; ++l)
        if ((rc = drain(l))) return quiesce(rc);
    return 0;
}

int gaplac_gram(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                const gaplac_term* terms, double noise, double* out_C, int64_t ldc) {
    int rc = check_common(ctx, N, D, X, ldx, noise, X /* v unused */);
    if (rc && N > 0) return rc;
    if (N == 0) return 0;
    if (!out_C || ldc < N) return set_err(ctx, GAPLAC_E_ARG, "out_C NULL or ldc < N");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    std::vector<double> zeros((size_t)N, 0.0);
    if ((rc = upload(ctx, N, D, X, ldx, zeros.data()))) return rc;
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    if ((rc = ensure(ctx, &ctx->A, &ctx->A_elems, (size_t)Np * Np))) return rc;
    tp.noise = noise;
    *ctx->htp = tp;
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    if ((rc = guarded(ctx, false, [&] {
             launch_gram(ctx->s_main, ctx->A, Np, N, nt, ctx->dX, N, ctx->dv, ctx->dtp, 0, 0, nullptr);
         })))
        return rc;
    HIPCK(ctx, hipMemcpy2DAsync(out_C, (size_t)ldc * 8, ctx->A, (size_t)Np * 8, (size_t)N * 8,
                                (size_t)N, hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    // only the lower triangle is built on the device; mirror it
    for (int64_t j = 0; j < N; ++j)
        for (int64_t i = 0; i < j; ++i) out_C[j * ldc + i] = out_C[i * ldc + j];
    return 0;
}

int gaplac_gram_time(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                     const gaplac_term* terms, double noise, const double* v, int32_t reps, double* best_ms,
                     double* bytes) {
    int rc = check_common(ctx, N, D, X, ldx, noise, v);
    if (rc) return rc;
    if (N == 0 || reps < 1 || !best_ms || !bytes) return set_err(ctx, GAPLAC_E_ARG, "N = 0, reps < 1 or NULL outputs");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, v))) return rc;
    const int64_t Np = round_up(N + 1, NB);
    const int nt = (int)(Np / NB);
    if ((rc = ensure(ctx, &ctx->A, &ctx->A_elems, (size_t)Np * Np))) return rc;
    tp.noise = noise;
    *ctx->htp = tp;
    HIPCK(ctx, hipMemcpyAsync(ctx->dtp, ctx->htp, sizeof(TermPack), hipMemcpyHostToDevice, ctx->s_main));
    hipEvent_t e0, e1;
    HIPCK(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return set_err(ctx, GAPLAC_E_HIP, "hipEventCreate failed");
    }
    double best = 1e300;
    {
        LaunchGuard g;
        g.base = ctx->A;
        g.elems = (int64_t)ctx->A_elems;
        GuardScope scope(&g);
        for (int r = 0; r < reps && rc == 0; ++r) {
            float ms = 0.f;
            if (hipEventRecord(e0, ctx->s_main) != hipSuccess) rc = GAPLAC_E_HIP;
            launch_gram(ctx->s_main, ctx->A, Np, N, nt, ctx->dX, N, ctx->dv, ctx->dtp, 0, 0, nullptr);
            if (rc == 0 && (hipEventRecord(e1, ctx->s_main) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                            hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
                rc = GAPLAC_E_HIP;
            if (rc == 0) best = std::min(best, (double)ms);
        }
        if (g.violations) rc = GAPLAC_E_ARG;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return set_err(ctx, rc, "gram timing failed");
    *best_ms = best;
    *bytes = 8.0 * (double)Np * (double)(Np + 1) / 2.0 + 8.0 * (double)N * (D + 1);
    return 0;
}

int gaplac_factor(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                  const gaplac_term* terms, double noise, const double* v, double* out_L,
                  int64_t ldl, double* out_z) {
    int rc = check_common(ctx, N, D, X, ldx, noise, v);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!out_L || ldl < N || !out_z) return set_err(ctx, GAPLAC_E_ARG, "bad output buffers");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, v))) return rc;
    tp.noise = noise;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows{}, &r))) return rc;
    const int64_t Np = round_up(N + 1, NB);
    HIPCK(ctx, hipMemcpy2D(out_L, (size_t)ldl * 8, ctx->A, (size_t)Np * 8, (size_t)N * 8, (size_t)N,
                           hipMemcpyDeviceToHost));
    HIPCK(ctx, hipMemcpy2D(out_z, 8, ctx->A + N, (size_t)Np * 8, 8, (size_t)N, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < N; ++j)
        for (int64_t i = 0; i < j; ++i) out_L[j * ldl + i] = 0.0;
    return finish(r, nullptr, nullptr, nullptr);
}

int gaplac_logpdf_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                       const gaplac_term* terms, double noise, const double* v, double* out_logpdf,
                       double* out_dv, double* out_dparam, double* out_dnoise) {
    return logpdf_grad_impl(ctx, false, N, D, X, ldx, T, terms, noise, v, out_logpdf, out_dv, out_dparam,
                            out_dnoise);
}

int gaplac_logpdf_grad_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double noise, const double* dv, double* out_logpdf,
                              double* out_dv, double* out_dparam, double* out_dnoise) {
    return logpdf_grad_impl(ctx, true, N, D, dX, ldx, T, terms, noise, dv, out_logpdf, out_dv, out_dparam,
                            out_dnoise);
}

int gaplac_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double noise, const double* y, int64_t M,
                              const double* Xs, int64_t ldxs, double* out_mean, double* out_var) {
    return posterior_impl(ctx, N, D, X, ldx, T, terms, noise, y, M, Xs, ldxs, out_mean, out_var);
}

int gaplac_posterior_components(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                                int64_t ldxs, int32_t G, const int32_t* comp, double* out_mean, int64_t ldm,
                                double* out_var, int64_t ldv) {
    return posterior_components_impl(ctx, N, D, X, ldx, T, terms, noise, y, M, Xs, ldxs, G, comp, out_mean, ldm,
                                     out_var, ldv);
}

int gaplac_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                const gaplac_term* terms, double noise, const double* z, double* out) {
    if (out)
        for (int64_t i = 0; i < N; ++i) out[i] = NAN;
    int rc = check_common(ctx, N, D, X, ldx, noise, z);
    if (rc) return rc;
    if (N > 0 && !out) return set_err(ctx, GAPLAC_E_ARG, "out is NULL");
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (N == 0) return 0;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, z))) return rc;  // z also rides in the v row (unused)
    tp.noise = noise;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows{}, &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr))) return rc;
    const size_t nk = (size_t)((N + 511) / 512);
    if ((rc = ensure(ctx, &ctx->gpart, &ctx->gpart_elems, nk * (size_t)N))) return rc;
    if ((rc = ensure(ctx, &ctx->gdv, &ctx->gdv_elems, (size_t)N))) return rc;
    const int64_t Np = round_up(N + 1, NB);
    if ((rc = guarded(ctx, false,
                      [&] { launch_lower_mv(ctx->s_main, ctx->A, Np, N, ctx->dv, ctx->gpart, ctx->gdv); })))
        return rc;
    HIPCK(ctx, hipMemcpyAsync(out, ctx->gdv, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

int gaplac_logpdf_multi(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                        const gaplac_term* terms, double noise, int64_t R, const double* Y, int64_t ldy,
                        double* out_logpdf, double* out_logdet, double* out_quad) {
    return logpdf_multi_impl(ctx, false, N, D, X, ldx, T, terms, noise, R, Y, ldy, out_logpdf, out_logdet, out_quad);
}

int gaplac_logpdf_multi_device(gaplac_ctx* ctx, int64_t N, int32_t D, const double* dX, int64_t ldx, int32_t T,
                               const gaplac_term* terms, double noise, int64_t R, const double* dY, int64_t ldy,
                               double* out_logpdf, double* out_logdet, double* out_quad) {
    return logpdf_multi_impl(ctx, true, N, D, dX, ldx, T, terms, noise, R, dY, ldy, out_logpdf, out_logdet, out_quad);
}

int gaplac_rand_multi(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                      const gaplac_term* terms, double noise, int64_t R, const double* Z, int64_t ldz, double* out,
                      int64_t ldo) {
    if (!ctx) return GAPLAC_E_ARG;
    if (R < 0 || !out || ldz < N || ldo < N || (R > 0 && N > 0 && !Z))
        return set_err(ctx, GAPLAC_E_ARG, "R < 0, Z / out NULL, or ldz / ldo < N");
    for (int64_t r = 0; r < R; ++r)  // (rows N .. ldo-1 of out are the caller's)
        for (int64_t i = 0; i < N; ++i) out[r * ldo + i] = NAN;
    int rc = check_common(ctx, N, D, X, ldx, noise, ctx /* v: Z is checked above */);
    if (rc) return rc;
    TermPack tp;
    if ((rc = pack_terms(ctx, D, T, terms, &tp))) return rc;
    if (N == 0 || R == 0) return 0;
    HIPCK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload(ctx, N, D, X, ldx, Z))) return rc;  // column 0 also rides in the v row (unused)
    const int64_t Np = round_up(N + 1, NB);
    if ((rc = ensure(ctx, &ctx->dZ, &ctx->dZ_elems, (size_t)Np * (size_t)R))) return rc;
    if ((rc = ensure(ctx, &ctx->dO, &ctx->dO_elems, (size_t)N * (size_t)R))) return rc;
    HIPCK(ctx, hipMemcpy2DAsync(ctx->dZ, (size_t)Np * 8, Z, (size_t)ldz * 8, (size_t)N * 8, (size_t)R,
                                hipMemcpyHostToDevice, ctx->s_main));
    tp.noise = noise;
    EvalResult r;
    if ((rc = eval_device(ctx, N, D, tp, ExtraRows{}, &r))) return rc;
    if ((rc = finish(r, nullptr, nullptr, nullptr))) return rc;
    // <trace path>.lz: "N R ms" of the L Z launch alone
    rc = trace_timed(ctx, ".lz", N, R, [&] {
        return guarded(ctx, false,
                       [&] { draws_launches(ctx->s_main, ctx->A, Np, N, ctx->dZ, R, ctx->dO, nullptr); });
    });
    if (rc) return rc;
    HIPCK(ctx, hipMemcpy2DAsync(out, (size_t)ldo * 8, ctx->dO, (size_t)N * 8, (size_t)N * 8, (size_t)R,
                                hipMemcpyDeviceToHost, ctx->s_main));
    HIPCK(ctx, hipStreamSynchronize(ctx->s_main));
    return 0;
}

int gaplac_posterior_mean_cov(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                              int64_t ldxs, double noise_s, double* out_mean, double* out_cov, int64_t ldc) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y};
    return joint_mean_cov(ctx, m, M, Xs, ldxs, noise_s, out_mean, out_cov, ldc);
}

int gaplac_posterior_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                          const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                          int64_t ldxs, double noise_s, int64_t R, const double* Z, int64_t ldz, double* out,
                          int64_t ldo) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y};
    return joint_rand(ctx, m, M, Xs, ldxs, noise_s, R, Z, ldz, out, ldo);
}

int gaplac_posterior_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                            const gaplac_term* terms, double noise, const double* y, int64_t M, const double* Xs,
                            int64_t ldxs, double noise_s, int64_t R, const double* Ys, int64_t ldys,
                            double* out_logpdf, double* out_logdet, double* out_quad) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y};
    return joint_logpdf(ctx, m, M, Xs, ldxs, noise_s, R, Ys, ldys, out_logpdf, out_logdet, out_quad);
}

int gaplac_sparse_elbo(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                       const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                       int64_t ldz, double jitter, double* out_elbo, double* out_dtc, double* out_trace,
                       double* out_logdet, double* out_quad) {
    return sparse_elbo_impl(ctx, N, D, X, ldx, T, terms, noise, y, Mz, Z, ldz, jitter, out_elbo, out_dtc, out_trace,
                            out_logdet, out_quad);
}

int gaplac_sparse_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                     const gaplac_term* terms, double noise, const double* y, int64_t Mz,
                                     const double* Z, int64_t ldz, double jitter, int64_t Ms, const double* Xs,
                                     int64_t ldxs, double* out_mean, double* out_var) {
    return sparse_posterior_impl(ctx, N, D, X, ldx, T, terms, noise, y, Mz, Z, ldz, jitter, Ms, Xs, ldxs, out_mean,
                                 out_var);
}

int gaplac_sparse_elbo_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                            const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                            int64_t ldz, double jitter, double* out_elbo, double* out_dy, double* out_dparam,
                            double* out_dnoise, double* out_djitter) {
    return sparse_elbo_grad_impl(ctx, N, D, X, ldx, T, terms, noise, y, Mz, Z, ldz, jitter, out_elbo, out_dy,
                                 out_dparam, out_dnoise, out_djitter);
}

int gaplac_sparse_elbo_grad_z(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                              int64_t ldz, double jitter, double* out_elbo, double* out_dy, double* out_dparam,
                              double* out_dnoise, double* out_djitter, double* out_dZ, int64_t lddz) {
    return sparse_elbo_grad_impl(ctx, N, D, X, ldx, T, terms, noise, y, Mz, Z, ldz, jitter, out_elbo, out_dy,
                                 out_dparam, out_dnoise, out_djitter, out_dZ, lddz);
}

int gaplac_sparse_posterior_mean_cov(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                     const gaplac_term* terms, double noise, const double* y, int64_t Mz,
                                     const double* Z, int64_t ldz, double jitter, int64_t Ms, const double* Xs,
                                     int64_t ldxs, double noise_s, double* out_mean, double* out_cov, int64_t ldc) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y, true, Mz, Z, ldz, jitter};
    return joint_mean_cov(ctx, m, Ms, Xs, ldxs, noise_s, out_mean, out_cov, ldc);
}

int gaplac_sparse_posterior_rand(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                 const gaplac_term* terms, double noise, const double* y, int64_t Mz, const double* Z,
                                 int64_t ldz, double jitter, int64_t Ms, const double* Xs, int64_t ldxs,
                                 double noise_s, int64_t R, const double* E, int64_t lde, double* out, int64_t ldo) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y, true, Mz, Z, ldz, jitter};
    return joint_rand(ctx, m, Ms, Xs, ldxs, noise_s, R, E, lde, out, ldo);
}

int gaplac_sparse_posterior_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                   const gaplac_term* terms, double noise, const double* y, int64_t Mz,
                                   const double* Z, int64_t ldz, double jitter, int64_t Ms, const double* Xs,
                                   int64_t ldxs, double noise_s, int64_t R, const double* Ys, int64_t ldys,
                                   double* out_logpdf, double* out_logdet, double* out_quad) {
    const JointModel m{N, D, X, ldx, T, terms, noise, y, true, Mz, Z, ldz, jitter};
    return joint_logpdf(ctx, m, Ms, Xs, ldxs, noise_s, R, Ys, ldys, out_logpdf, out_logdet, out_quad);
}

int gaplac_fit_destroy(gaplac_fit* fit) {
    if (!fit) return 0;
    if (fit->ctx) {
        (void)hipSetDevice(fit->device);
        (void)hipStreamSynchronize(fit->ctx->s_main);
        fit_unregister(fit);
    }
    if (fit->buf) (void)hipFree(fit->buf);
    delete fit;
    return 0;
}

int gaplac_fit_info(const gaplac_fit* fit, int64_t* out_N, int64_t* out_cap, double* out_logpdf, double* out_logdet,
                    double* out_quad) {
    if (!fit) return GAPLAC_E_ARG;
    if (out_N) *out_N = fit->N;
    if (out_cap) *out_cap = fit->cap;
    if (out_logpdf) *out_logpdf = fit->logpdf;
    if (out_logdet) *out_logdet = fit->logdet;
    if (out_quad) *out_quad = fit->quad;
    return 0;
}

int gaplac_fit_alpha(gaplac_fit* fit, double* out_alpha) {
    if (!fit) return GAPLAC_E_ARG;
    for (int64_t i = 0; out_alpha && i < fit->N; ++i) out_alpha[i] = NAN;
    if (!fit->ctx) return GAPLAC_E_ARG;
    if (fit->N == 0) return 0;
    if (!out_alpha) return set_err(fit->ctx, GAPLAC_E_ARG, "out_alpha is NULL");
    HIPCK(fit->ctx, hipSetDevice(fit->device));
    HIPCK(fit->ctx, hipMemcpy(out_alpha, fit->buf + fit->d.alpha, (size_t)fit->N * 8, hipMemcpyDeviceToHost));
    return 0;
}

int gaplac_fit_mode(gaplac_fit* fit, double* out_f) {
    if (!fit) return GAPLAC_E_ARG;
    for (int64_t i = 0; out_f && i < fit->N; ++i) out_f[i] = NAN;
    if (!fit->ctx) return GAPLAC_E_ARG;
    if (fit->kind != 1) return set_err(fit->ctx, GAPLAC_E_ARG, "the fit is exact: it has no mode");
    if (fit->N == 0) return 0;
    if (!out_f) return set_err(fit->ctx, GAPLAC_E_ARG, "out_f is NULL");
    HIPCK(fit->ctx, hipSetDevice(fit->device));
    HIPCK(fit->ctx, hipMemcpy(out_f, fit->buf + fit->d.fhat, (size_t)fit->N * 8, hipMemcpyDeviceToHost));
    return 0;
}

int gaplac_fit_laplace_info(const gaplac_fit* fit, int32_t* out_lik, double* out_lik_param, double* out_jitter,
                            int32_t* out_iters, int32_t* out_converged) {
    if (!fit || fit->kind != 1) return GAPLAC_E_ARG;
    if (out_lik) *out_lik = fit->lik;
    if (out_lik_param) *out_lik_param = fit->lik_param;
    if (out_jitter) *out_jitter = fit->jitter;
    if (out_iters) *out_iters = fit->iters;
    if (out_converged) *out_converged = fit->converged;
    return 0;
}

int gaplac_laplace_fit_create(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                              const gaplac_term* terms, double jitter, int32_t lik, double lik_param, const double* y,
                              int32_t max_iter, double tol, const double* a0, int64_t cap, gaplac_fit** out,
                              int32_t* out_iters, int32_t* out_converged, int64_t* out_info) {
    if (out) *out = nullptr;
    if (!ctx) return GAPLAC_E_ARG;
    if (!out) return set_err(ctx, GAPLAC_E_ARG, "out is NULL");
    const LapRequest q{N, D, X, ldx, T, terms, jitter, lik, lik_param, y, max_iter, tol, a0};
    double logq;
    LapOut o{&logq, out_iters, out_converged, out_info};
    o.fit = out;
    o.cap = cap;
    return laplace_impl(ctx, q, o);
}

// Host-only walk of a Laplace fit (no device needed; the iteration and its final factorisation are
// gaplac_plan_check_laplace's): the create-time launches against the fit's buffer, one
// mean-and-variance query of M points in chunks of cap (the scaled build, the rows' solve, the
// norms and the matrix-free mean), one matrix-free mean query and one joint covariance of
// min(M, cap) points against the context's second workspace, every launch through the functions
// the entries call. short_ws 1: the fit's buffer one element short; 2: the covariance workspace.
int gaplac_plan_check_laplace_fit(int64_t N, int64_t cap, int64_t M, int32_t spw, int32_t short_ws,
                                  int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || cap < 1 || M < 0 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 2) return GAPLAC_E_ARG;
    if ((cap + NB - 1) / NB > 65535) return GAPLAC_E_ARG;
    const FitDims d = fit_dims(N, 1, cap, true);
    const LapDims ld = lap_dims(N, 0);
    const int64_t mc = std::min(M, cap), ldb = round_up(mc + 1, NB);
    double* const fb = PlanWalk::region(0);  // the fit's buffer
    double* const fa = PlanWalk::region(1);  // the workspace
    double* const fl = PlanWalk::region(2);  // the vectors
    double* const fB = PlanWalk::region(3);  // the second workspace
    const int64_t b_elems = d.elems - (short_ws == 1 ? 1 : 0), B_elems = ldb * ldb - (short_ws == 2 ? 1 : 0);
    PlanWalk w{spw};
    w.on(fb, b_elems, fa, ld.a_elems, [&] { lap_fit_create_launches(nullptr, d, ld, N, fa, fl, fb); }, fl, ld.elems);
    w.on(fb, b_elems, fB, B_elems, [&] {
        for (int64_t r0 = 0; r0 < M; r0 += cap)
            fit_query_launches(nullptr, d, N, std::min(cap, M - r0), spw, fb, true);
        for (int64_t r0 = 0; r0 < M; r0 += d.qc) fit_mean_launches(nullptr, d, N, std::min(d.qc, M - r0), fb);
        if (mc > 0) {
            fit_query_launches(nullptr, d, N, mc, spw, fb, true);
            fit_cov_launches(nullptr, d, N, mc, fb, fB, ldb, nullptr);
        }
    });
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only walk of a fit (no device needed): the create-time copy, z and the back-substitution
// against the fit's buffer (the evaluation before them is gaplac_plan_check's mode 0), then one
// mean-and-variance query of M points in chunks of cap and one matrix-free mean query, every
// launch through the functions the entries call. short_ws 1: the buffer one element short.
int gaplac_plan_check_fit(int64_t N, int64_t cap, int64_t M, int32_t spw, int32_t short_ws, int64_t* out_launches,
                          int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || cap < 1 || M < 0 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 1) return GAPLAC_E_ARG;
    if ((cap + NB - 1) / NB > 65535) return GAPLAC_E_ARG;
    const FitDims d = fit_dims(N, 1, cap);
    double *const fb = PlanWalk::region(0), *const fa = PlanWalk::region(1);
    PlanWalk w{spw};
    w.on(fb, d.elems - (short_ws == 1 ? 1 : 0), fa, d.Np * d.Np, [&] {
        fit_create_launches(nullptr, d, N, fa, d.Np, fb);
        for (int64_t r0 = 0; r0 < M; r0 += cap) fit_query_launches(nullptr, d, N, std::min(cap, M - r0), spw, fb);
        for (int64_t r0 = 0; r0 < M; r0 += d.qc) fit_mean_launches(nullptr, d, N, std::min(d.qc, M - r0), fb);
    });
    return w.report(out_launches, out_violations, msg, msglen);
}

int gaplac_laplace_logpdf(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                          const gaplac_term* terms, double jitter, int32_t lik, double lik_param, const double* y,
                          int32_t max_iter, double tol, const double* a0, double* out_logq, double* out_f,
                          double* out_a, int32_t* out_iters, int32_t* out_converged, int64_t* out_info) {
    const LapRequest q{N, D, X, ldx, T, terms, jitter, lik, lik_param, y, max_iter, tol, a0};
    LapOut o{out_logq, out_iters, out_converged, out_info};
    o.f = out_f;
    o.a = out_a;
    return laplace_impl(ctx, q, o);
}

int gaplac_laplace_posterior_mean_var(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                                      const gaplac_term* terms, double jitter, int32_t lik, double lik_param,
                                      const double* y, int32_t max_iter, double tol, const double* a0, int64_t M,
                                      const double* Xs, int64_t ldxs, double* out_logq, double* out_mean,
                                      double* out_var, int32_t* out_iters, int32_t* out_converged, int64_t* out_info) {
    const LapRequest q{N, D, X, ldx, T, terms, jitter, lik, lik_param, y, max_iter, tol, a0, M, Xs, ldxs};
    LapOut o{out_logq, out_iters, out_converged, out_info};
    o.mean = out_mean;
    o.var = out_var;
    return laplace_impl(ctx, q, o);
}

int gaplac_laplace_logpdf_grad(gaplac_ctx* ctx, int64_t N, int32_t D, const double* X, int64_t ldx, int32_t T,
                               const gaplac_term* terms, double jitter, int32_t lik, double lik_param,
                               const double* y, int32_t max_iter, double tol, const double* a0, double* out_logq,
                               double* out_f, double* out_a, int32_t* out_iters, int32_t* out_converged,
                               int64_t* out_info, double* out_dparam, double* out_djitter, double* out_implicit) {
    const LapRequest q{N, D, X, ldx, T, terms, jitter, lik, lik_param, y, max_iter, tol, a0};
    double logq;
    LapOut o{&logq, out_iters, out_converged, out_info};  // (out_logq may be NULL here)
    o.f = out_f;
    o.a = out_a;
    o.grad = true;
    o.dparam = out_dparam;
    o.djitter = out_djitter;
    o.implicit = out_implicit;
    const int rc = laplace_impl(ctx, q, o);
    if (out_logq) *out_logq = logq;
    return rc;
}

// Host-only walk of gaplac_laplace_logpdf_grad: one Newton step with one trial point, the final
// factorisation with identity rows and the gradient's stages and ending, every launch through
// the functions the entry calls. short_ws 1: the workspace one element short; 2: the vectors' buffer.
int gaplac_plan_check_laplace_grad(int64_t N, int32_t spw, int32_t short_ws, int64_t* out_launches,
                                   int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 2) return GAPLAC_E_ARG;
    const LapDims d = lap_dims(N, 0, true);
    PlanWalk w{spw};
    LapWalk lw{w, d.a_elems - (short_ws == 1 ? 1 : 0), d.elems - (short_ws == 2 ? 1 : 0), 0};
    double *const fa = lw.fa, *const fl = lw.fl;
    walk_lap_iteration(lw, d, N);
    lw.on_ws([&] { lap_build_launches(nullptr, d, N, 2 * d.Np, false, fa, nullptr, nullptr, nullptr, fl); });
    // the final factorisation; then, in its (dry) context, the gradient's stages: the stages under
    // the entry's guards, the ending under the walk's own (the workspace of 2 Np x Np elements)
    // (twice: single-term groups, the fused contraction; product groups, its two-launch form). The vectors
    // are the evaluation's second region for the ending; the step's evaluation, with no `after`, needs none.
    for (bool singletons : {true, false})
        w.eval(N, ExtraRows::identity(N, singletons).deferred().on_prebuilt(), 0, [&](gaplac_ctx& c) {
            lw.on_ws([&] { lap_grad_scale_launches(nullptr, d, N, GAPLAC_LIK_POISSON, fa, fl); });
            lw.on_vectors([&] { lap_mf_launches(nullptr, d, N, N, nullptr, nullptr, N, nullptr, fl, d.s2, d.q); });
            lw.on_ws([&] { lap_grad_solve_launches(nullptr, d, N, fa, fl); });
            const int e = enqueue_grad_ending(&c, N, d.Np, 2 * d.Np, fl + d.a);
            lw.on_ws([&] { lap_grad_bilinear_launches(nullptr, d, N, 1, nullptr, nullptr, nullptr, fl); });
            return e;
        }, fl, lw.l_elems);
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only walk of the Laplace entries (no device needed): one Newton step with one trial point,
// the final factorisation, and with M > 0 the posterior query in its chunks, every launch through
// the functions the entries call. short_ws 1: the workspace and the vectors' buffer one element
// short.
int gaplac_plan_check_laplace(int64_t N, int64_t M, int32_t spw, int32_t short_ws, int64_t* out_launches,
                              int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || M < 0 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 1) return GAPLAC_E_ARG;
    const LapDims d = lap_dims(N, M);
    PlanWalk w{spw};
    LapWalk lw{w, d.a_elems - short_ws, d.elems - short_ws, N * d.qc};
    double *const fa = lw.fa, *const fl = lw.fl;
    walk_lap_iteration(lw, d, N);
    for (int64_t r0 = 0; r0 == 0 || r0 < M; r0 += LAP_CHUNK) {
        const int64_t m = std::min(LAP_CHUNK, M - r0);
        if (m > 0) {
            const int64_t lda = d.Np + NB * ((m + NB - 1) / NB);
            lw.on_ws([&] { lap_query_launches(nullptr, d, N, m, lda, fa, nullptr, nullptr, nullptr, nullptr, fl, lw.fy); });
            w.eval(N, ExtraRows::responses(m, nullptr, 0).on_prebuilt());
            lw.on_vectors([&] { lap_mf_launches(nullptr, d, N, m, nullptr, nullptr, m, nullptr, fl, d.a, d.mean); });
        } else {
            lw.on_ws([&] { lap_build_launches(nullptr, d, N, d.Np, false, fa, nullptr, nullptr, nullptr, fl); });
            w.eval(N, ExtraRows{}.on_prebuilt());
        }
    }
    return w.report(out_launches, out_violations, msg, msglen);
}

int gaplac_sparse_split(int64_t N, int64_t Mz, int64_t* out_chunks, int64_t* out_chunk_rows) {
    if (N < 0 || Mz < 0 || !out_chunks || !out_chunk_rows) return GAPLAC_E_ARG;
    sparse_split(N, Mz, out_chunks, out_chunk_rows);
    return 0;
}

// Host-only walk of the sparse entries' three stages (no device needed): the posterior
// evaluation of order Mz with N + Ms riding rows, the stage-2 launches and the transposing copy
// against both workspaces, and the prebuilt factorisation of order Mz, plain (Ms = 0,
// gaplac_sparse_elbo) or with Ms riding rows (gaplac_sparse_posterior_mean_var), and the rows'
// reduction. The launches between the evaluations are the entries' own functions, run dry; the
// walk takes the copy and the reduction at Ms = 0 too, where the entries have neither. short_ws
// 1 / 2: the stage-1 / stage-3 workspace one element short (negative controls).
int gaplac_plan_check_sparse(int64_t N, int64_t Mz, int64_t Ms, int32_t spw, int32_t short_ws, int64_t* out_launches,
                             int64_t* out_violations, char* msg, int64_t msglen) {
    PlanWalk w{spw};
    if (!walk_sparse(w, N, Mz, Ms, short_ws)) return GAPLAC_E_ARG;
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only walk of gaplac_sparse_elbo_grad: the three stages of the value (gaplac_plan_check_sparse
// at Ms = 0), then the gradient's own launches run dry: the order-Mz launches against the
// scratch, the N-long launches (alpha, the product kernel) against the first workspace and the
// scratch as its second region. short_ws 1: the first workspace one element short (the value's
// walk and the product kernel's riding rows both leave it); 2: the second workspace of the value
// and the gradient's scratch one element short (negative controls).
// With Tz > 0 it is gaplac_sparse_elbo_grad_z's walk (§10.10): the product kernel's dZ variant in
// the product's place and the dZ launches after it, the buffer of dZ's partials as the third
// region, one element short with short_ws 3.
static int plan_sparse_grad(int64_t N, int64_t Mz, int32_t Tz, int32_t spw, int32_t short_ws, int64_t* out_launches,
                            int64_t* out_violations, char* msg, int64_t msglen) {
    PlanWalk w{spw};
    if (!walk_sparse(w, N, Mz, 0, short_ws == 3 ? 0 : short_ws)) return GAPLAC_E_ARG;
    const SparseDims d = sparse_dims(N, Mz, 0);
    const SparseGradDims g = sparse_grad_dims(Mz);
    double* const fa = PlanWalk::region(0);
    double* const fg = PlanWalk::region(1);
    double* const fv = PlanWalk::region(2);  // vectors, partials, Dinv: never guarded
    // (one column of Z: the finishing step's store is the buffer's last element for any D)
    double* const fz = Tz > 0 ? PlanWalk::region(3) : nullptr;
    const int64_t g_elems = 3 * g.ld * g.Np - (short_ws == 2 ? 1 : 0);
    const int64_t z_elems = fz ? sparse_dz_dims(N, Mz, Tz, 1).elems - (short_ws == 3 ? 1 : 0) : 0;
    w.on(fg, g_elems, nullptr, 0,
         [&] { sparse_grad_mz_launches(nullptr, g, Mz, fg, fv, fv, fv, fv, 1.0, nullptr, nullptr, nullptr, 1); });
    w.on(fa, d.lda * d.Np - (short_ws == 1 ? 1 : 0), fg, g_elems, [&] {
        sparse_grad_alpha_launches(nullptr, d, g, N, Mz, fa, fv, fv, 1.0, nullptr);
        sparse_grad_uf_launches(nullptr, d, g, N, Mz, fa, fg, fv, fv, nullptr, nullptr, nullptr, nullptr, false,
                                fz ? Tz : 1, fz, 1);
    }, fz, z_elems);
    return w.report(out_launches, out_violations, msg, msglen);
}

int gaplac_plan_check_sparse_grad(int64_t N, int64_t Mz, int32_t spw, int32_t short_ws, int64_t* out_launches,
                                  int64_t* out_violations, char* msg, int64_t msglen) {
    if (short_ws == 3) return GAPLAC_E_ARG;
    return plan_sparse_grad(N, Mz, 0, spw, short_ws, out_launches, out_violations, msg, msglen);
}

int gaplac_plan_check_sparse_grad_z(int64_t N, int64_t Mz, int32_t T, int32_t spw, int32_t short_ws,
                                    int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen) {
    if (T < 1 || T > GAPLAC_MAX_TERMS || short_ws < 0 || short_ws > 3) return GAPLAC_E_ARG;
    return plan_sparse_grad(N, Mz, T, spw, short_ws, out_launches, out_violations, msg, msglen);
}

// Host-only walk of the sparse joint entries (§10.11, no device needed): gaplac_plan_check_sparse
// with Ms test points (the three stages and the mean's reduction), the copy of the a rows against
// the first workspace, the covariance launches (zeroing, sparse_post_cov_kernel, the mirroring
// pass) against the second and third, and the prebuilt factorisation of order Ms in the third,
// with R > 0 carrying R riding rows (gaplac_sparse_posterior_logpdf), else plain
// (gaplac_sparse_posterior_rand). The launches between the evaluations are the entries' own
// functions, run dry; the copy of the a rows (never short) is a guarded region of both. Gaps
// against the entries: the walk takes the copy after the first two factorisations (the entries
// before the second), the mirroring pass always (the entries for gaplac_sparse_posterior_mean_cov
// only), and gaplac_sparse_posterior_rand's draws_launches are in no walk.
// short_ws 1 / 2 / 3: that workspace one element short (negative controls).
int gaplac_plan_check_sparse_joint(int64_t N, int64_t Mz, int64_t Ms, int64_t R, int32_t spw, int32_t short_ws,
                                   int64_t* out_launches, int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || Mz < 1 || Ms < 1 || R < 0 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 3) return GAPLAC_E_ARG;
    if ((N + Ms + NB - 1) / NB > 65535 || (R + NB - 1) / NB > 65535) return GAPLAC_E_ARG;
    PlanWalk w{spw};
    if (!walk_sparse(w, N, Mz, Ms, short_ws == 3 ? 0 : short_ws)) return GAPLAC_E_ARG;
    const SparseDims d = sparse_dims(N, Mz, Ms);
    const SparseJointDims j = sparse_joint_dims(Ms, R);
    double* const fa = PlanWalk::region(0);
    double* const fb = PlanWalk::region(1);
    double* const fc = PlanWalk::region(2);
    double* const fr = PlanWalk::region(3);
    const int64_t a_elems = d.lda * d.Np - (short_ws == 1 ? 1 : 0), b_elems = d.ldb * d.Np - (short_ws == 2 ? 1 : 0);
    const int64_t c_elems = j.ldc * j.Msp - (short_ws == 3 ? 1 : 0), r_elems = d.Np * j.ldr;
    w.on(fa, a_elems, fr, r_elems, [&] { sparse_joint_copy_launches(nullptr, d, j, N, Mz, Ms, fa, fr); });
    w.on(fb, b_elems, fc, c_elems, [&] {
        sparse_joint_cov_launches(nullptr, d, j, Mz, Ms, fb, fr, fc, nullptr, 0, nullptr, nullptr, 1.0, true);
    }, fr, r_elems);
    const ExtraRows rows = R > 0 ? ExtraRows::responses(R, nullptr, 0) : ExtraRows{};
    w.eval(Ms, rows.on_prebuilt(), short_ws == 3 ? 1 : 0);
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only walk of the joint posterior's three stages (no device needed): the posterior
// evaluation of order N with M test points, the covariance launches (zeroing, post_cov_kernel,
// the mirroring pass) against both workspaces, and the prebuilt factorisation of order M, with
// R > 0 carrying R riding rows (gaplac_posterior_logpdf), else plain (gaplac_posterior_rand).
// The covariance launches are the entries' own function, run dry. Two gaps against the entries:
// the walk takes the mirroring pass whenever R = 0, the entries when a covariance is asked for
// (gaplac_posterior_mean_cov with out_cov; gaplac_posterior_rand has none); and
// gaplac_posterior_rand's draws_launches after stage 3 are in no walk.
// short_ws 1 / 2: the order-N / order-M workspace one element short (negative controls).
int gaplac_plan_check_joint(int64_t N, int64_t M, int64_t R, int32_t spw, int32_t short_ws, int64_t* out_launches,
                            int64_t* out_violations, char* msg, int64_t msglen) {
    if (N < 1 || M < 1 || R < 0 || spw < 1 || spw > 8 || short_ws < 0 || short_ws > 2) return GAPLAC_E_ARG;
    const JointDims d = joint_dims(N, M, R);
    double *const fa = PlanWalk::region(0), *const fb = PlanWalk::region(1);
    PlanWalk w{spw};
    w.eval(N, ExtraRows::test_points(M), short_ws == 1 ? 1 : 0);
    w.on(fa, d.lda * d.Np - (short_ws == 1 ? 1 : 0), fb, d.ldb * d.Mp - (short_ws == 2 ? 1 : 0),
         [&] { joint_cov_launches(nullptr, d, N, M, fa, fb, nullptr, nullptr, nullptr, R == 0); });
    const ExtraRows rows = R > 0 ? ExtraRows::responses(R, nullptr, 0) : ExtraRows{};
    w.eval(M, rows.on_prebuilt(), short_ws == 2 ? 1 : 0);
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only walk of one evaluation's schedule (no device needed): every launch's element
// range is checked against the workspace ensure_workspace would allocate for N.
// mode 0: logpdf; 1: logpdf + gradient (identity rows); 2: posterior at M test points;
// 3: logpdf_multi of M responses (the transposing launch, the rows, the per-row reduction).
int gaplac_plan_check(int64_t N, int32_t mode, int64_t M, int32_t spw, int64_t* out_launches,
                      int64_t* out_violations, char* msg, int64_t msglen) {
    const bool short_ws = mode >= 8;  // negative control: a workspace one element short
    if (short_ws) mode -= 8;
    if (N < 1 || mode < 0 || mode > 3 || (mode >= 2 && M < 1) || spw < 1 || spw > 8) return GAPLAC_E_ARG;
    {
        // every tail length the library can launch: the task list is a topological order
        static std::string tail_bad = [] {
            for (int T = 1; T <= TAIL_TMAX; ++T)
                for (int gw : {4, 8})
                    for (int near : {2, 3, 4, 8})
                    for (int ql : {0, 7, 24, 40, TAIL_TMAX})
                    for (int wp : {0, 1, 2, 3, 4, 5}) {
                        std::vector<uint32_t> l;
                        build_tail_tasks(T, l, nullptr, gw, near, ql, (wp & 1) != 0, 1 << (wp >> 1));
                        std::string why;
                        if (!check_tail_tasks(T, l, &why)) return why + " (gw " + std::to_string(gw) + ", near " +
                                                                  std::to_string(near) + ")";
                    }
            // single evaluations with the critical sub-diagonal quadrants, with and without the
            // posterior's extra rows
            for (int T = 1; T <= TAIL_TMAX; ++T)
                for (int ql : {GAPLAC_QUAD_LAST, TAIL_TMAX})
                    for (int cq : {0, 1, 2})
                        for (int X : {0, 2}) {
                            if (T + X > TAIL_TMAX) continue;  // (the launch condition)
                            std::vector<uint32_t> l;
                            build_tail_tasks(T, l, nullptr, 4, 4, ql, false, GAPLAC_SINGLE_GROUP, X, cq);
                            std::string why;
                            if (!check_tail_tasks(T, l, &why, X))
                                return why + " (quad_last " + std::to_string(ql) + ", crit_quads " + std::to_string(cq) +
                                       ", extra rows " + std::to_string(X) + ")";
                        }
            // the simulated order (GAPLAC_TAIL_SIM) must come out reordered and checked
            for (int T : {2, 9, 33, 65, 80, 128})
                for (int ql : {GAPLAC_QUAD_LAST, TAIL_TMAX}) {
                    std::vector<uint32_t> l;
                    build_tail_tasks(T, l, nullptr, 4, 4, ql, false, GAPLAC_SINGLE_GROUP, 0, 1);
                    const int st = sim_order_tail_tasks(T, l, 256);
                    if (st != 0)
                        return "simulated tail order (T = " + std::to_string(T) + ", quad_last " + std::to_string(ql) +
                               ") " + (st == 1 ? "stalled" : "failed the dependency check");
                }
            // batched launches: each model's tasks, read out of the interleaved list, are
            // its single list in order (so each is a topological order of its own dataflow)
            for (int T : {1, 2, 9, 33, 65, 80})
                for (int B : {1, 3, 32})
                    for (int lag : {0, 1, 6, 16}) {
                        std::vector<uint32_t> one, all;
                        std::vector<size_t> cs;
                        build_tail_tasks(T, one, &cs);
                        interleave_tail_tasks(one, cs, B, lag, all);
                        std::vector<size_t> at((size_t)B, 0);
                        char b[128];
                        std::snprintf(b, sizeof b, "interleaved tail list (T = %d, B = %d, lag = %d) breaks a model's order",
                                      T, B, lag);
                        if (all.size() != one.size() * (size_t)B) return std::string(b);
                        for (uint32_t e : all) {
                            const size_t m = e >> TAIL_MODEL_SHIFT;
                            if (m >= (size_t)B || at[m] >= one.size() ||
                                (e & ((1u << TAIL_MODEL_SHIFT) - 1)) != one[at[m]++])
                                return std::string(b);
                        }
                    }
            return std::string();
        }();
        if (!tail_bad.empty()) {
            if (msg && msglen > 0) std::snprintf(msg, (size_t)msglen, "%s", tail_bad.c_str());
            return GAPLAC_E_ARG;
        }
    }
    const ExtraRows xr = mode == 1   ? ExtraRows::identity(N)
                         : mode == 2 ? ExtraRows::test_points(M)
                         : mode == 3 ? ExtraRows::responses(M, nullptr, 0)
                                     : ExtraRows{};
    PlanWalk w{spw};
    w.eval(N, xr, short_ws ? 1 : 0);
    return w.report(out_launches, out_violations, msg, msglen);
}

// Host-only accounting of the single-GPU schedule: a dry walk of one
// evaluation of order N with the given deferral depth / band extension / cut-off, whose
// launchers record every update (tile columns x panel columns) and every column's
// factorisation in enqueue order (LaunchGuard::acct). Checks that every tile column gets
// every earlier panel column exactly once, in increasing order, before its diagonal block
// (or before the persistent tail that factors it), and that every update reads panel
// columns already factored. 0, or GAPLAC_E_ARG with the first violation in msg.
int gaplac_plan_check_schedule(int64_t N, int32_t spw, int32_t depth, int32_t pair_ext, int32_t pair_m,
                               int64_t* out_records, char* msg, int64_t msglen) {
    if (N < 1 || spw < 1 || spw > 8 || depth < 0 || depth > 8 || pair_ext < 0 || pair_ext > 1 || pair_m < 0)
        return GAPLAC_E_ARG;
    gaplac_ctx c;
    c.spw = spw;
    c.pair_depth = depth;
    c.pair_ext = pair_ext;
    c.pair_m = pair_m;
    const int nt = (int)(round_up(N + 1, NB) / NB);
    LaunchGuard g;
    std::vector<int> acct;
    g.acct = &acct;
    const int rc = dry_walk(c, N, ExtraRows{}, g);
    std::string why;
    char b[200];
    if (rc) why = "the dry walk failed";
    if (g.violations && why.empty()) why = g.first;
    std::vector<int> next((size_t)nt, 0);       // next panel column tile column j must receive
    std::vector<char> done((size_t)nt, 0);      // factored (or handed to the tail)
    for (size_t i = 0; i + 5 <= acct.size() && why.empty(); i += 5) {
        const int kind = acct[i], j0 = acct[i + 1], j1 = acct[i + 2], k0 = acct[i + 3], k1 = acct[i + 4];
        if (kind == 0) {
            for (int k = k0; k < k1 && why.empty(); ++k)
                if (k < 0 || k >= nt || !done[(size_t)k]) {
                    std::snprintf(b, sizeof b, "an update reads panel column %d before it is factored", k);
                    why = b;
                }
            for (int j = j0; j < j1 && why.empty(); ++j) {
                if (j < 0 || j >= nt || done[(size_t)j] || next[(size_t)j] != k0 || k1 > j) {
                    std::snprintf(b, sizeof b, "tile column %d gets panel columns %d..%d (expected from %d%s)", j, k0,
                                  k1 - 1, j >= 0 && j < nt ? next[(size_t)j] : -1,
                                  j >= 0 && j < nt && done[(size_t)j] ? ", after its factorisation" : "");
                    why = b;
                } else {
                    next[(size_t)j] = k1;
                }
            }
        } else if (kind == 1) {
            if (j0 < 0 || j0 >= nt) continue;
            if (!done[(size_t)j0] && next[(size_t)j0] != j0) {
                std::snprintf(b, sizeof b, "tile column %d factored with panel columns < %d only", j0,
                              next[(size_t)j0]);
                why = b;
            }
            done[(size_t)j0] = 1;
        } else {
            for (int j = j0; j < nt && why.empty(); ++j) {
                if (done[(size_t)j] || next[(size_t)j] != j0) {
                    std::snprintf(b, sizeof b, "the tail from %d starts with tile column %d at panel %d", j0, j,
                                  next[(size_t)j]);
                    why = b;
                }
                done[(size_t)j] = 1;
            }
        }
    }
    for (int j = 0; j < nt && why.empty(); ++j)
        if (!done[(size_t)j]) {
            std::snprintf(b, sizeof b, "tile column %d never factored", j);
            why = b;
        }
    if (out_records) *out_records = (int64_t)(acct.size() / 5);
    if (msg && msglen > 0) std::snprintf(msg, (size_t)msglen, "%s", why.c_str());
    return why.empty() ? 0 : GAPLAC_E_ARG;
}

int gaplac_set_profiling(gaplac_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return GAPLAC_E_ARG;
    ctx->prof_mode = mode;
    return 0;
}

int gaplac_get_stats(gaplac_ctx* ctx, gaplac_stats* out) {
    if (!ctx || !out) return GAPLAC_E_ARG;
    if (!ctx->evpairs.empty()) {  // fold the event-timed bulk launches in
        HIPCK(ctx, hipSetDevice(ctx->device));
        std::vector<std::pair<double, double>> iv;  // bulk-type launch intervals, ms after the first event
        const hipEvent_t ref = ctx->evpool[ctx->evpairs.front().i0];
        for (const auto& p : ctx->evpairs) {
            float ms = 0.f;
            // (the pair's launch retired: pairs lie on s_main, s_panel and the split's s_xrest,
            // each stream in order, so no other stream or context is waited for)
            HIPCK(ctx, hipEventSynchronize(ctx->evpool[p.i0 + 1]));
            HIPCK(ctx, hipEventElapsedTime(&ms, ctx->evpool[p.i0], ctx->evpool[p.i0 + 1]));
            if (p.kind == 8) {
                ctx->stats.cinv_ms += ms;
                ctx->stats.cinv_launches += 1;
                continue;
            }
            float t0 = 0.f;
            HIPCK(ctx, hipEventElapsedTime(&t0, ref, ctx->evpool[p.i0]));
            iv.push_back({(double)t0, (double)t0 + ms});
            ctx->stats.bulk_flops += p.flops;
            ctx->stats.bulk_launches += 1;
            if (p.kind == 5) continue;  // bands, heads, lookaheads: the union only
            ctx->stats.syrk_ms += ms;
            ctx->stats.syrk_flops += p.flops;
            ctx->stats.syrk_bytes += p.bytes;
            ctx->stats.syrk_launches += 1;
        }
        // union of the intervals: the time some bulk-type launch was in flight
        std::sort(iv.begin(), iv.end());
        double cs = -1.0, ce = -1.0;
        for (const auto& x : iv) {
            if (x.first > ce) {
                if (ce > cs) ctx->stats.bulk_union_ms += ce - cs;
                cs = x.first;
                ce = x.second;
            } else {
                ce = std::max(ce, x.second);
            }
        }
        if (ce > cs) ctx->stats.bulk_union_ms += ce - cs;
        ctx->evpairs.clear();
    }
    *out = ctx->stats;
    return 0;
}

int gaplac_reset_stats(gaplac_ctx* ctx) {
    if (!ctx) return GAPLAC_E_ARG;
    ctx->stats = gaplac_stats{};
    ctx->evpairs.clear();
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// Observation-space predictions of the Laplace posterior: O(M) host
// arithmetic, no context and no device.
// ---------------------------------------------------------------------------------
namespace {

constexpr int GH_MAX_Q = 64;

// Physicists' Gauss-Hermite rule of order Q (weight e^{-x^2}), ascending nodes: Newton on the
// orthonormal Hermite recurrence in long double, from the largest root down (the usual asymptotic
// first guesses), the negative half by symmetry.
void gauss_hermite_ld(int Q, long double* x, long double* w) {
    const long double pim4 = 0.7511255444649425L;  // pi^{-1/4}
    const int half = (Q + 1) / 2;
    long double z = 0.0L;
    for (int i = 0; i < half; ++i) {
        if (i == 0)
            z = std::sqrt((long double)(2 * Q + 1)) - 1.85575L * std::pow((long double)(2 * Q + 1), -1.0L / 6.0L);
        else if (i == 1)
            z -= 1.14L * std::pow((long double)Q, 0.426L) / z;
        else if (i == 2)
            z = 1.86L * z - 0.86L * x[Q - 1];
        else if (i == 3)
            z = 1.91L * z - 0.91L * x[Q - 2];
        else
            z = 2.0L * z - x[Q + 1 - i];
        long double pp = 1.0L;
        for (int it = 0; it < 100; ++it) {
            long double p1 = pim4, p2 = 0.0L;
            for (int j = 0; j < Q; ++j) {
                const long double p3 = p2;
                p2 = p1;
                p1 = z * std::sqrt(2.0L / (j + 1)) * p2 - std::sqrt((long double)j / (j + 1)) * p3;
            }
            pp = std::sqrt((long double)(2 * Q)) * p2;
            const long double dz = p1 / pp;
            z -= dz;
            if (std::fabs(dz) <= 1e-19L * (1.0L + std::fabs(z))) break;
        }
        if (2 * i + 1 == Q) z = 0.0L;  // the middle node of an odd rule
        {  // the derivative at the converged node
            long double p1 = pim4, p2 = 0.0L;
            for (int j = 0; j < Q; ++j) {
                const long double p3 = p2;
                p2 = p1;
                p1 = z * std::sqrt(2.0L / (j + 1)) * p2 - std::sqrt((long double)j / (j + 1)) * p3;
            }
            pp = std::sqrt((long double)(2 * Q)) * p2;
        }
        x[Q - 1 - i] = z;
        x[i] = -z;
        w[i] = w[Q - 1 - i] = 2.0L / (pp * pp);
    }
}

// Nodes and log weights of order Q in double, computed once per Q.
struct GhRule {
    bool ready = false;
    double x[GH_MAX_Q], w[GH_MAX_Q], logw[GH_MAX_Q];
};
const GhRule& gh_rule(int Q) {
    static GhRule rules[GH_MAX_Q + 1];
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    GhRule& r = rules[Q];
    if (!r.ready) {
        long double x[GH_MAX_Q], w[GH_MAX_Q];
        gauss_hermite_ld(Q, x, w);
        for (int q = 0; q < Q; ++q) {
            r.x[q] = (double)x[q];
            r.w[q] = (double)w[q];
            r.logw[q] = (double)std::log(w[q]);
        }
        r.ready = true;
    }
    return r;
}

// log p(y | f) of the two non-Gaussian likelihoods, in the stable forms of the device's lik_eval.
double host_lik_logp(int lik, double y, double f) {
    if (lik == GAPLAC_LIK_BERNOULLI) return y * f - ((f > 0.0 ? f : 0.0) + std::log1p(std::exp(-std::fabs(f))));
    return y * f - std::exp(f) - std::lgamma(y + 1.0);
}
double host_sigmoid(double f) {
    const double e = std::exp(-std::fabs(f));
    return f >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

}  // namespace

extern "C" {

int gaplac_gauss_hermite(int32_t Q, double* nodes, double* weights) {
    if (Q < 1 || Q > GH_MAX_Q) return GAPLAC_E_ARG;
    const GhRule& r = gh_rule(Q);
    for (int q = 0; q < Q; ++q) {
        if (nodes) nodes[q] = r.x[q];
        if (weights) weights[q] = r.w[q];
    }
    return 0;
}

int gaplac_laplace_predict(int32_t lik, double lik_param, int64_t M, const double* mean, const double* var,
                           const double* ys, int32_t Q, double* out_ymean, double* out_yvar, double* out_logp) {
    if (M < 0) return GAPLAC_E_ARG;
    for (int64_t j = 0; j < M; ++j) {
        if (out_ymean) out_ymean[j] = NAN;
        if (out_yvar) out_yvar[j] = NAN;
        if (out_logp) out_logp[j] = NAN;
    }
    if (lik != GAPLAC_LIK_GAUSSIAN && lik != GAPLAC_LIK_BERNOULLI && lik != GAPLAC_LIK_POISSON) return GAPLAC_E_KIND;
    if (M > 0 && (!mean || !var)) return GAPLAC_E_ARG;
    if (lik == GAPLAC_LIK_GAUSSIAN) {
        if (!(lik_param >= 0.0) || !std::isfinite(lik_param)) return GAPLAC_E_PARAM;
    } else if (Q < 1 || Q > GH_MAX_Q) {
        return GAPLAC_E_ARG;
    }
    for (int64_t j = 0; ys && j < M; ++j)
        if (!lik_supports(lik, ys[j])) return GAPLAC_E_PARAM;
    const bool score = ys && out_logp;
    const GhRule* rule = lik == GAPLAC_LIK_GAUSSIAN ? nullptr : &gh_rule(Q);
    const double sqrt_pi = 1.7724538509055160273, half_log_pi = 0.57236494292470008707;
    for (int64_t j = 0; j < M; ++j) {
        const double mu = mean[j];
        if (!std::isfinite(mu) || !std::isfinite(var[j])) continue;  // NaN at this point
        const double v = var[j] > 0.0 ? var[j] : 0.0, sd = std::sqrt(v);
        if (lik == GAPLAC_LIK_GAUSSIAN) {
            const double s2 = v + lik_param, r = score ? ys[j] - mu : 0.0;
            if (out_ymean) out_ymean[j] = mu;
            if (out_yvar) out_yvar[j] = s2;
            if (score) out_logp[j] = -0.5 * (1.8378770664093453 + std::log(s2)) - 0.5 * r * r / s2;
            continue;
        }
        if (lik == GAPLAC_LIK_POISSON) {
            const double ym = std::exp(mu + 0.5 * v);
            if (out_ymean) out_ymean[j] = ym;
            if (out_yvar) out_yvar[j] = ym + std::expm1(v) * ym * ym;
        }
        const bool need_p = lik == GAPLAC_LIK_BERNOULLI && (out_ymean || out_yvar);
        if (sd == 0.0) {  // a point mass: the likelihood at mu itself
            if (need_p) {
                const double p = host_sigmoid(mu);
                if (out_ymean) out_ymean[j] = p;
                if (out_yvar) out_yvar[j] = p * (1.0 - p);
            }
            if (score) out_logp[j] = host_lik_logp(lik, ys[j], mu);
            continue;
        }
        double t[GH_MAX_Q], tmax = -INFINITY, p = 0.0;
        const double step = 1.4142135623730951 * sd;
        for (int q = 0; q < Q; ++q) {
            const double f = mu + step * rule->x[q];
            if (need_p) p += rule->w[q] * host_sigmoid(f);
            if (score) {
                t[q] = rule->logw[q] + host_lik_logp(lik, ys[j], f);
                tmax = t[q] > tmax ? t[q] : tmax;
            }
        }
        if (need_p) {
            p /= sqrt_pi;
            if (out_ymean) out_ymean[j] = p;
            if (out_yvar) out_yvar[j] = p * (1.0 - p);
        }
        if (score) {
            double acc = 0.0;
            for (int q = 0; q < Q; ++q) acc += std::exp(t[q] - tmax);
            out_logp[j] = tmax + std::log(acc) - half_log_pi;
        }
    }
    return 0;
}

}  // extern "C"
