// mvtv_admm.cpp — the ADMM loop: mvtv_admm_run, and the parts of an iteration and of a device-controlled run that it
// shares with the slab loop (mvtv_slab.cpp). Declarations in mvtv_problem.h.
//
// An iteration is a theta-solve (mvtv_capi.cpp), then the edge pass below: z-update and dual update over all edges,
// D^T alpha and D^T u, and the sums the stopping tests and adapt_step need. The loop follows the reference variants
// line by line at the level of scalars (adapt_step, stopping tests, counters):
//   B  rcpp-code/MultivarTV/src/solvers.cpp:96-136   (admm_update, adapt_step :77-94)
//   A  cpp-code/solvers.cpp:90-130                    (admm_update, adapt_step :70-88)
//   C  code/solvers.py:53-76                          (mbs_one's loop)
// With the spectral theta-solve the decisions of every iteration are taken on the device (k_admm_control, AdmmCtl)
// and the host enqueues iterations ahead; otherwise (PCG, or MVTV_ADMM_SYNC set) the host reads back 7 scalars per
// iteration and decides itself.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mvtv/mvtv.h"
#include "mvtv_internal.h"
#include "mvtv_problem.h"

namespace mvtv {

// ============================================================================================ one edge pass
namespace {
// sums of `nparts` partial rows; the last reduction of an iteration may carry the control step
mvtv_status reduce(mvtv_problem* P, const EdgePass& e, int nparts, int nr, int nmax, double* out, bool last) {
    const int h = e.timed_red ? P->tstart(MVTV_K_REDUCE) : -1;
    const bool step = last && e.ctl_step;
    HIP_TRY(launch_finalize(P->stream, P->partials, nparts, nr, nmax, 0, out, P->st, 0.0, 0, e.ctl,
                            step ? P->ctl : nullptr, step ? P->red : nullptr));
    P->tstop(h);
    return MVTV_OK;
}
}  // namespace

mvtv_status edge_stage(mvtv_problem* P, const EdgePass& e) {
    const Launch L = P->L();
    if (P->f3d) {   // edge update + gather in one pass, z ping-pongs between the edge buffers
        const int h = P->tstart(MVTV_K_ADMM_FUSED);
        int np = 0;
        HIP_TRY(launch_admm3d(P->g, P->order, e.umode, L.stream, P->theta, e.z_old, e.z_new, e.t_old, e.c_old, e.t_new,
                              e.c_prev, e.theta_old, P->ga, e.g_new, e.g_prev, P->partials, &np, e.ctl, e.fold, e.twin));
        P->tstop(h);
        return reduce(P, e, np, ER_N + GR_N, -(1 << ER_DTH), P->red, true);
    }
    int np = L.grid;
    if (P->f4d) {   // 4-D: edge update + the gather's pass A in one pass (z ping-pong); pass B in the gather stage
        const int h = P->tstart(MVTV_K_ADMM_FUSED4);
        HIP_TRY(launch_admm4a(P->g, P->order, e.umode, L.stream, P->theta, e.z_old, e.z_new, e.t_old, e.c_old, e.t_new,
                              e.theta_old, P->g4, P->partials, &np, e.ctl, e.twin));
        P->tstop(h);
    } else {   // z-update (soft threshold) and dual update over all edges, in place
        const int h = P->tstart(MVTV_K_EDGE_UPDATE);
        if (P->e3d)
            HIP_TRY(launch_edge3d(P->g, P->order, e.umode, L.stream, P->theta, e.z_new, e.t_old, e.c_old, e.t_new,
                                  e.theta_old, P->partials, &np, e.ctl));
        else
            HIP_TRY(launch_edge_update(P->g, P->order, e.umode, L, P->theta, e.z_new, e.t_old, e.c_old, e.t_new,
                                       e.theta_old, P->partials, e.ctl));
        P->tstop(h);
    }
    return reduce(P, e, np, ER_N, 1, P->red, false);
}

mvtv_status gather_stage(mvtv_problem* P, const EdgePass& e) {
    if (P->f3d) return MVTV_OK;
    const Launch L = P->L();
    int np = L.grid;
    if (P->f4d) {
        const int h = P->tstart(MVTV_K_GATHER4B);
        HIP_TRY(launch_gather4b(P->g, U_FROM_Z, L.stream, P->ga, e.g_new, e.g_prev, e.c_prev, P->partials, &np, e.ctl,
                                P->g4, e.fold));
        P->tstop(h);
    } else {   // D^T alpha, D^T u and the dual residual norms, from the z just formed (threshold t_new)
        const int h = P->tstart(MVTV_K_GATHER);
        const int hb = P->tstart_b(MVTV_K_GATHER4B);
        if (P->e3d)
            HIP_TRY(launch_gather3d(P->g, P->order, U_FROM_Z, L.stream, e.z_new, e.t_new, P->ga, e.g_new, e.g_prev,
                                    e.c_prev, P->partials, &np, e.ctl, P->g4, e.fold));
        else
            HIP_TRY(launch_gather(P->g, P->order, U_FROM_Z, L, e.z_new, e.t_new, P->ga, e.g_new, e.g_prev, e.c_prev,
                                  P->partials, e.ctl));
        P->tstop(h);
        P->tstop_b(hb);
    }
    return reduce(P, e, np, GR_N, 0, P->red + ER_N, true);
}

// ============================================================================ a device-controlled run's frame
mvtv_status admm_ctl_start(mvtv_problem* P, int variant, int fixed_iters, int max_counter, double tol, double lambda,
                           double rho, double sigma, double c_prev, double t_z, double dtheta, double sqrtN,
                           double sqrtE) {
    AdmmCtl& c = *P->host_ctl;
    std::memset(&c, 0, sizeof(c));
    c.variant = variant;
    c.fixed_iters = fixed_iters > 0 ? fixed_iters : 0;
    c.max_counter = max_counter;
    c.lambda = lambda;
    c.tol = tol;
    c.sqrtN = sqrtN;
    c.sqrtE = sqrtE;
    c.rho = rho;
    c.sigma = sigma;
    c.c_prev = c_prev;
    c.t_z = t_z;
    c.t_next = rho != 0.0 ? lambda / rho : INFINITY;
    c.counter = 1;
    c.dtheta = dtheta;
    c.dual_norm = c.primal_norm = 1.0;
    c.eps_dual = c.eps_pri = tol;
    HIP_TRY(hipMemcpyAsync(P->ctl, &c, sizeof(AdmmCtl), hipMemcpyHostToDevice, P->stream));
    return MVTV_OK;
}

mvtv_status admm_enqueue_ahead(mvtv_problem* P, const std::function<mvtv_status(int)>& enqueue, int fixed_iters,
                               int limit, bool single, std::vector<size_t>& mark) {
    int target = single ? 1 : (fixed_iters > 0 ? fixed_iters : (P->admm_hint > 0 ? P->admm_hint : 16));
    int enq = 0;
    for (;;) {
        while (enq < target && enq < limit) {
            mark.push_back(P->pending.size());
            MVTV_TRY(enqueue(enq++));
        }
        HIP_TRY(hipMemcpyAsync(P->host_ctl, P->ctl, sizeof(AdmmCtl), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        if (P->host_ctl->done || enq >= limit) return MVTV_OK;
        target = single ? enq + 1 : enq + std::max(4, enq / 4);
    }
}

mvtv_admm_stats admm_finish(mvtv_problem* P, const std::vector<size_t>& mark, int fixed_iters, bool fold,
                            bool pingpong) {
    const AdmmCtl& c = *P->host_ctl;
    const int it_done = c.it;
    if (P->timing && it_done < int(mark.size()))   // iterations enqueued past the stop did no work
        for (size_t e = mark[size_t(it_done)]; e < P->pending.size(); ++e) P->pending[e].kid = -1;
    P->harvest();
    if (P->timing && fold) P->fold_fix += c.nfix;
    if (fixed_iters <= 0 && c.status == 0) P->admm_hint = it_done + 1;
    if (it_done & 1) {   // P->guprev holds D^T u of the current state, P->edges its z
        std::swap(P->guprev, P->gu);
        if (pingpong) std::swap(P->edges, P->edges2);
    }
    if (it_done > 0) {
        P->edge_mode = U_FROM_Z;
        P->t_z = c.t_z;
    }
    P->c_state = c.c_prev;
    P->rho = c.rho;
    mvtv_admm_stats S{};
    S.iters = it_done;
    S.rho = c.rho;
    S.r_norm = c.r_norm;
    S.s_norm = c.s_norm;
    if (c.variant == MVTV_VARIANT_RCPP) {
        S.eps_pri = c.eps_pri;
        S.eps_dual = c.eps_dual;
    }
    S.dtheta_max = c.dtheta;
    S.status = c.status ? MVTV_MAXITER : MVTV_OK;
    return S;
}

// ============================================================================================ twins, z pair
// The fused 3-D kernel may skip the twin block (mvtv_internal.h twin_block): one GPU, equal twin weights and state.
// MVTV_TWIN_OFF=1 (probe builds) keeps both.
bool twin_ready(const mvtv_problem* P) {
    if (P->slab || !P->twin_ok || probe_env("MVTV_TWIN_OFF")) return false;
    if (!((P->g.p == 3 && P->f3d) || (P->g.p == 4 && P->f4d))) return false;
    return twin_weights_equal(P->g, P->order);
}

// edge words the twins leave out (the twin blocks' lengths)
double twin_edges(const mvtv_problem* P) {
    double t = 0.0;
    for (int k = 0; k < P->g.nb; ++k)
        if (twin_of(k, P->g.p, P->order) != k) t += double(P->blk_len[k]);
    return t;
}

// Placement-aware z ping-pong: the fused 3-D kernel's time depends on WHICH physical
// edge buffer it reads z from and writes to (profiles/r01/v12_zflip_probe.txt: up to 4.70 against
// 4.15 ms for the two directions of one pair). Once per problem, for 3-D meshes of >= 2^24 nodes, time
// every ordered pair of four candidate buffers (candidate 0 = edges2, 1..3 = new allocations; `edges`
// holds the state and is not a candidate) with side-effect-free launches of the steady-state kernel
// (zeroed z, scratch outputs, no control block), keep the pair with the lowest round-trip cost, move z into
// it and free the rest. Best effort: any failure (allocation, launch) leaves the allocation-order pair in
// place, frees everything the probe allocated and clears HIP's error state. MVTV_ZPICK=0 turns it off
// (MVTV_ZPICK=fail: allocate, then take the failure path; tests/test_gpu_zpick.py).
mvtv_status pick_zpair(mvtv_problem* P, bool track_theta, bool twin) {
    P->zpicked = true;
    const char* env = std::getenv("MVTV_ZPICK");
    if ((env && std::atoi(env) == 0) || P->g.p != 3 || P->g.N < (size_t(1) << 24) || !P->edges2) return MVTV_OK;
    const size_t ne = size_t(P->g.nb) * P->g.N, bytes = ne * sizeof(double);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < 3 * bytes + (size_t(16) << 30)) {
        (void)hipGetLastError();
        return MVTV_OK;
    }
    constexpr int K = 4, R = 3;
    double* cand[K] = {P->edges2, nullptr, nullptr, nullptr};
    double* tmp[3] = {nullptr, nullptr, nullptr};   // the probes' g_alpha / g_u outputs and theta_old input
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ok = true;
    auto hip = [&](hipError_t e) {
        if (e != hipSuccess) ok = false;
        return ok;
    };
    for (int i = 1; i < K && ok; ++i) hip(hipMalloc(reinterpret_cast<void**>(&cand[i]), bytes));
    for (int i = 0; i < 3 && ok; ++i) hip(hipMalloc(reinterpret_cast<void**>(&tmp[i]), size_t(P->g.N) * sizeof(double)));
    for (int i = 0; i < K && ok; ++i) hip(hipMemsetAsync(cand[i], 0, bytes, P->stream));
    if (ok) hip(hipMemsetAsync(tmp[2], 0, size_t(P->g.N) * sizeof(double), P->stream));
    if (ok) hip(hipEventCreate(&ev[0]));
    if (ok) hip(hipEventCreate(&ev[1]));
    if (env && std::strcmp(env, "fail") == 0) ok = false;   // test hook: take the failure path after allocating
    double cost[K][K] = {};
    for (int rep = 0; rep <= R && ok; ++rep)   // rep 0 warms up
        for (int i = 0; i < K && ok; ++i)
            for (int j = 0; j < K && ok; ++j) {
                if (i == j) continue;
                int np = 0;
                float ms = 0.f;
                if (hip(hipEventRecord(ev[0], P->stream)) &&
                    hip(launch_admm3d(P->g, P->order, U_FROM_Z, P->stream, P->theta, cand[i], cand[j], 0.0, 1.0, 0.0,
                                      1.0, track_theta ? tmp[2] : nullptr, tmp[0], tmp[1], P->guprev, P->partials,
                                      &np, nullptr, false, twin)) &&
                    hip(hipEventRecord(ev[1], P->stream)) && hip(hipEventSynchronize(ev[1])) &&
                    hip(hipEventElapsedTime(&ms, ev[0], ev[1])) && rep > 0)
                    cost[i][j] += ms;
            }
    int a = 0, b = 1;
    if (ok) {
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j)
                if (cost[i][j] + cost[j][i] < cost[a][b] + cost[b][a]) a = i, b = j;
        // the probes wrote only the candidates, tmp and the partials (scratch until the next reduction)
        ok = hip(hipMemcpyAsync(cand[a], P->edges, bytes, hipMemcpyDeviceToDevice, P->stream)) &&
             hip(hipStreamSynchronize(P->stream));
    }
    (void)hipStreamSynchronize(P->stream);
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    for (auto t : tmp)
        if (t) (void)hipFree(t);
    if (!ok) {   // keep (edges, edges2); the candidates' contents were never used
        for (int i = 1; i < K; ++i)
            if (cand[i]) (void)hipFree(cand[i]);
        (void)hipGetLastError();
        return MVTV_OK;
    }
    (void)hipFree(P->edges);
    for (int i = 0; i < K; ++i)
        if (i != a && i != b) (void)hipFree(cand[i]);
    P->edges = cand[a];
    P->edges2 = cand[b];
    if (probe_env("MVTV_ZPICK_LOG"))
        std::fprintf(stderr, "[mvtv] z pair %d,%d: %.3f / %.3f ms (candidate 0 = edges2, 1-3 new; pair 0,1: %.3f / %.3f)\n",
                     a, b, cost[a][b] / R, cost[b][a] / R, cost[0][1] / R, cost[1][0] / R);
    return MVTV_OK;
}

// ============================================================================================ mvtv_admm_run
namespace {

// what the prologue settles for either loop
struct AdmmSetup {
    mvtv_admm_opts o;
    double lambda, tol, rtol;
    int max_counter, pcg_maxit;
    bool spectral, pcg_spec;   // the theta-solver: exact spectral, PCG with the spectral preconditioner, else Jacobi-PCG
    bool track_theta;          // variants A and C stop on max|theta - theta_old|
    bool pingpong, twin;
    double rho, sigma, c_prev, t_z, dtheta;
    int mode;                  // how the edge buffer holds u0
    std::chrono::steady_clock::time_point t0;
    mvtv_admm_stats* stats;    // the caller's, or null

    // a loop's normal exit (an early error return leaves the caller's stats alone)
    mvtv_status report(mvtv_admm_stats& S) const {
        S.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = S;
        return mvtv_status(S.status);
    }
};

// An early return (MVTV_TRY / HIP_TRY) after twin-skipping iterations must not leave a stale twin block behind
// twin_ok: fill the twins of both edge buffers (whichever holds the state), best effort; the normal exits fill
// them themselves and disarm
struct TwinGuard {
    mvtv_problem* P;
    bool armed;
    ~TwinGuard() {
        if (!armed) return;
        (void)fill_twins(P->g, P->order, P->stream, P->edges);
        if (P->edges2) (void)fill_twins(P->g, P->order, P->stream, P->edges2);
        (void)hipStreamSynchronize(P->stream);
        (void)hipGetLastError();
    }
};

// options, solver, rho and sigma; u0 explicit in the edge buffer with D^T u0 formed, or the resident z form;
// g_alpha = D^T D theta0; the second edge buffer and its placement; the initial max|theta - theta_old|
mvtv_status admm_prologue(mvtv_problem* P, const mvtv_admm_opts& o, double lambda, AdmmSetup& A) {
    const int variant = o.variant;
    if (variant < 0 || variant > 2) return fail(MVTV_BAD_ARG, "variant");
    A.o = o;
    A.lambda = lambda;
    A.tol = variant_tol(o);
    A.max_counter = variant_maxc(o);
    A.rtol = o.pcg_rtol > 0 ? o.pcg_rtol : 1e-10;
    A.pcg_maxit = o.pcg_max_iter > 0 ? o.pcg_max_iter : 20000;
    const Launch L = P->L();
    if (o.theta_solver < MVTV_SOLVER_AUTO || o.theta_solver > MVTV_SOLVER_PCG_SPECTRAL)
        return fail(MVTV_BAD_ARG, "theta_solver");
    if (o.theta_solver == MVTV_SOLVER_SPECTRAL && !spectral_ok(P))
        return fail(MVTV_BAD_ARG, "spectral theta-solve needs W = I and every m_j, j < p - 1, <= 4096 or a product of two 2-3-5-7-smooth factors <= 4096");
    if (o.theta_solver == MVTV_SOLVER_PCG_SPECTRAL && (!P->spec_mesh || P->wmode == W_NONE))
        return fail(MVTV_BAD_ARG, "spectral preconditioner needs every m_j, j < p - 1, <= 4096 or a product of two 2-3-5-7-smooth factors <= 4096");
    A.spectral = o.theta_solver == MVTV_SOLVER_SPECTRAL || (o.theta_solver == MVTV_SOLVER_AUTO && spectral_ok(P));
    // AUTO with W != I on a spectral mesh: PCG with the spectral preconditioner (K an order of magnitude
    // below Jacobi's once sigma D^T D dominates); other meshes: Jacobi-PCG
    A.pcg_spec = o.theta_solver == MVTV_SOLVER_PCG_SPECTRAL ||
                 (o.theta_solver == MVTV_SOLVER_AUTO && !A.spectral && P->spec_mesh && P->wmode != W_NONE && !P->slab);

    // ---- initial state: u explicit in the edge buffer, alpha_0 = D theta_0 ------------------
    if (variant == MVTV_VARIANT_RCPP) A.rho = P->rho;                      // rho_init (:100)
    else if (variant == MVTV_VARIANT_CPP) A.rho = double(int(lambda));     // int rho = lambda (:108)
    else A.rho = lambda;                                                   // rho = tune (py :55)
    A.sigma = std::isnan(o.sigma) ? (variant == MVTV_VARIANT_RCPP ? A.rho : lambda) : o.sigma;
    A.c_prev = 1.0;
    A.t_z = 0.0;
    A.mode = U_EXPLICIT;
    int h = -1;
    if (P->edge_mode == U_FROM_Z) {
        // resume from the resident state of the previous call: u0 = -c clamp(z, t_z) is read straight
        // from z by the first edge update, and P->guprev already holds D^T clamp-part of it (scale c)
        A.mode = U_FROM_Z;
        A.t_z = P->t_z;
        A.c_prev = P->c_state;
    } else {
        if (P->u_default) {
            const double u0 = variant == MVTV_VARIANT_RCPP ? 0.0 : 1.0 / lambda;   // A :101, C :62
            HIP_TRY(launch_edges_fill_valid(P->g, P->order, L, P->edges, u0));
            P->u_default = false;
        }
        // g_uprev = D^T u0
        h = P->tstart(MVTV_K_GATHER);
        int np0 = L.grid;
        if (P->e3d)
            HIP_TRY(launch_gather3d(P->g, P->order, U_EXPLICIT, P->stream, P->edges, 0.0, nullptr, P->guprev, nullptr,
                                    1.0, P->partials, &np0, nullptr, P->g4));
        else
            HIP_TRY(launch_gather(P->g, P->order, U_EXPLICIT, L, P->edges, 0.0, nullptr, P->guprev, nullptr, 1.0,
                                  P->partials));
        P->tstop(h);
    }
    // g_alpha = D^T D theta0 (alpha0 = D theta0, rcpp…/solvers.cpp:101)  ->  b_1 = oty + rho D^T (alpha0 + u0)
    h = P->tstart(MVTV_K_OTHER);
    HIP_TRY(launch_apply_A(P->g, L, 1.0, W_NONE, nullptr, P->theta, P->ga, nullptr, nullptr));
    P->tstop(h);

    A.track_theta = variant != MVTV_VARIANT_RCPP;
    const bool fused = P->f3d;
    A.pingpong = P->f3d || P->f4d;   // z ping-pongs between two edge buffers under the fused passes
    if (A.pingpong && !P->edges2) MVTV_TRY(alloc(&P->edges2, size_t(P->g.nb) * P->g.N));
    // MVTV_ZFLIP (probe only, tools/zflip_probe.py): move z to the other edge buffer before this run,
    // so the g_u ping-pong meets the z ping-pong in the other pairing of physical buffers
    if (fused && probe_env("MVTV_ZFLIP")) {
        HIP_TRY(hipMemcpyAsync(P->edges2, P->edges, size_t(P->g.nb) * P->g.N * sizeof(double),
                               hipMemcpyDeviceToDevice, P->stream));
        std::swap(P->edges, P->edges2);
    }
    if (fused && probe_env("MVTV_GFLIP")) {   // probe only: the same for the g_u ping-pong
        HIP_TRY(hipMemcpyAsync(P->gu, P->guprev, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToDevice,
                               P->stream));
        std::swap(P->gu, P->guprev);
    }
    // the twin blocks are skipped by the fused kernels and filled from their group's first block when the run ends
    A.twin = A.pingpong && twin_ready(P);
    if (P->timing && A.pingpong) P->twin_timed = A.twin;
    if (fused && A.spectral && !P->zpicked) MVTV_TRY(pick_zpair(P, A.track_theta, A.twin));
    A.dtheta = 0.0;
    if (A.track_theta) {
        if (!P->thold) MVTV_TRY(alloc(&P->thold, P->g.N));
        HIP_TRY(launch_fill(P->stream, P->thold, o.ymean - (variant == MVTV_VARIANT_CPP ? 0.1 : 1.0), P->g.N));
        HIP_TRY(launch_maxabsdiff(P->g, L, P->theta, P->thold, P->partials));
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 1, 0, P->red, P->st));
        HIP_TRY(hipMemcpyAsync(P->host_red, P->red, sizeof(double), hipMemcpyDeviceToHost, P->stream));
        MVTV_TRY(P->sync());
        A.dtheta = P->host_red[0];
    }
    return MVTV_OK;
}

// ---- asynchronous loop (spectral theta-solve): the decisions of every iteration are taken on the device by
// k_admm_control, the host enqueues iterations ahead and polls the done flag
mvtv_status admm_device_loop(mvtv_problem* P, const AdmmSetup& A, TwinGuard& guard) {
    const mvtv_admm_opts& o = A.o;
    const int variant = o.variant;
    MVTV_TRY(admm_ctl_start(P, variant, o.fixed_iters, A.max_counter, A.tol, A.lambda, A.rho, A.sigma, A.c_prev, A.t_z,
                            A.dtheta, std::sqrt(double(P->g.N)), std::sqrt(double(P->E))));
    double* gbuf[2] = {P->guprev, P->gu};
    double* ebuf[2] = {P->edges, A.pingpong ? P->edges2 : P->edges};
    // FOLD (variant B): the fused 3-D kernel stores s = rho (D^T alpha + D^T u) in P->ga instead of D^T alpha, so
    // the next solve's first pass reads oty and s (2N words) instead of oty, D^T alpha and D^T u (3N); after a
    // control step that changed rho it forms oty + (rho'/rho) s + rho' (c - 1) D^T u (AdmmCtl::fold_ka / _kb)
    // (the first pass transforms dim 0)
    const uint32_t m0 = P->g.m[0];
    const bool fold_path = P->f3d ? (P->g.p == 2 || P->g.p == 3)
                                  : (P->g.p == 4 && P->e3d && P->g4 != nullptr && gather4_ok(P->g));   // two-pass 4-D
    const bool fold = fold_path && variant == MVTV_VARIANT_RCPP && m0 >= 8 && m0 <= 4096 && (m0 & (m0 - 1)) == 0 &&
                      !split_on(P) && !probe_env("MVTV_FOLD_OFF") && !probe_env("MVTV_DCT_LDS");
    auto enqueue = [&](int j) -> mvtv_status {
        if (A.track_theta)
            HIP_TRY(hipMemcpyAsync(P->thold, P->theta, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToDevice,
                                   P->stream));
        MVTV_TRY(spectral_solve(P, A.sigma, P->oty, P->ga, A.rho, gbuf[j & 1], A.rho, P->theta, P->ctl, 1.0, nullptr,
                                fold && j > 0));
        EdgePass e;
        e.umode = j == 0 ? A.mode : U_FROM_Z;
        e.z_old = ebuf[j & 1];
        e.z_new = ebuf[(j + 1) & 1];
        e.g_prev = gbuf[j & 1];
        e.g_new = gbuf[(j + 1) & 1];
        e.theta_old = A.track_theta ? P->thold : nullptr;
        e.ctl = P->ctl;
        e.fold = fold;
        e.twin = A.twin;
        e.timed_red = e.ctl_step = true;
        MVTV_TRY(edge_stage(P, e));
        return gather_stage(P, e);
    };
    const int limit = o.fixed_iters > 0 ? o.fixed_iters : (variant == MVTV_VARIANT_PY ? A.max_counter : A.max_counter + 1);
    std::vector<size_t> mark;
    MVTV_TRY(admm_enqueue_ahead(P, enqueue, o.fixed_iters, limit, false, mark));
    mvtv_admm_stats S = admm_finish(P, mark, o.fixed_iters, fold, A.pingpong);
    guard.armed = false;
    if (A.twin) HIP_TRY(fill_twins(P->g, P->order, P->stream, P->edges));
    S.theta_solver = MVTV_SOLVER_SPECTRAL;
    if (S.status == MVTV_MAXITER) {
        if (variant == MVTV_VARIANT_CPP) fail(MVTV_MAXITER, "Failed to converge!");
        else if (variant == MVTV_VARIANT_RCPP && o.verbose) std::printf("ADMM reached max_counter at lambda = %g\n", A.lambda);
    }
    if (o.verbose) std::printf("Lambda= %g, Counter = %d\n", A.lambda, P->host_ctl->counter);
    return A.report(S);
}

// ---- synchronous loop (PCG theta-solves, or MVTV_ADMM_SYNC): the host reads the sums of every iteration and takes
// the reference's decisions itself
mvtv_status admm_host_loop(mvtv_problem* P, const AdmmSetup& A, TwinGuard& guard) {
    const mvtv_admm_opts& o = A.o;
    const int variant = o.variant;
    const double lambda = A.lambda, tol = A.tol, N = double(P->g.N), E = double(P->E);
    double rho = A.rho, sigma = A.sigma, c_prev = A.c_prev, t_z = A.t_z, dtheta = A.dtheta;
    double* gprev = P->guprev;
    double* gnew = P->gu;
    int mode = A.mode;
    mvtv_admm_stats S{};
    S.status = MVTV_OK;
    double dual_norm = 1.0, primal_norm = 1.0, eps_dual = tol, eps_primal = tol;
    int counter = 1, it = 0;
    mvtv_status status = MVTV_OK;
    for (;;) {
        // ---- loop condition, evaluated at the top as in the reference -----------------------
        if (o.fixed_iters > 0) {
            if (it >= o.fixed_iters) break;
        } else if (variant == MVTV_VARIANT_RCPP) {
            if (!(dual_norm > eps_dual || primal_norm > eps_primal)) break;   // :110
        } else {
            if (!(dtheta > tol)) break;   // any(|theta - thetaold| > TOL): A :113, C :69
            if (variant == MVTV_VARIANT_PY && it >= A.max_counter) {
                status = MVTV_MAXITER;
                break;
            }
        }
        if (A.track_theta) HIP_TRY(hipMemcpyAsync(P->thold, P->theta, size_t(P->g.N) * sizeof(double),
                                                  hipMemcpyDeviceToDevice, P->stream));
        // ---- theta-update: (W + sigma D^T D) theta = oty + rho D^T (alpha + u) ----------------
        int pit = 0;
        double relres = 0.0;
        if (A.spectral)
            MVTV_TRY(spectral_solve(P, sigma, P->oty, P->ga, rho, gprev, rho * c_prev, P->theta));
        else if (A.pcg_spec)
            MVTV_TRY(pcgs_solve(P, sigma, P->oty, P->ga, rho, gprev, rho * c_prev, P->theta, A.rtol, A.pcg_maxit, &pit,
                                &relres));
        else
            MVTV_TRY(pcg_solve(P, sigma, P->oty, P->ga, rho, gprev, rho * c_prev, P->theta, A.rtol, A.pcg_maxit, &pit,
                               &relres));
        S.pcg_iters += pit;
        S.pcg_iters_max = std::max(S.pcg_iters_max, pit);
        if (!A.spectral && pit >= A.pcg_maxit && !(relres <= A.rtol)) {
            S.pcg_unconverged += 1;
            if (o.pcg_strict) {
                status = MVTV_PCG_NOT_CONVERGED;
                fail(status, "PCG hit pcg_max_iter");
                break;
            }
        }
        // ---- the edge pass, thresholds and scales by value; z ping-pongs in place of P->edges / P->edges2
        EdgePass e;
        e.umode = mode;
        e.z_old = P->edges;
        e.z_new = A.pingpong ? P->edges2 : P->edges;
        e.g_new = gnew;
        e.g_prev = gprev;
        e.theta_old = A.track_theta ? P->thold : nullptr;
        e.t_old = t_z;
        e.c_old = e.c_prev = c_prev;
        e.t_new = rho != 0.0 ? lambda / rho : INFINITY;
        e.twin = A.twin;
        e.timed_red = true;
        MVTV_TRY(edge_stage(P, e));
        if (A.pingpong) std::swap(P->edges, P->edges2);
        MVTV_TRY(gather_stage(P, e));
        mode = U_FROM_Z;
        t_z = e.t_new;
        HIP_TRY(hipMemcpyAsync(P->host_red, P->red, (ER_N + GR_N) * sizeof(double), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));   // timing events are harvested after the loop
        const double* R = P->host_red;
        const double r_norm = std::sqrt(R[ER_R2]);
        it += 1;
        counter += 1;
        double c_next = 1.0, rho_next = rho;
        if (variant == MVTV_VARIANT_RCPP) {
            // :117-125
            dual_norm = std::fabs(rho) * std::sqrt(R[ER_N + GR_S2B]);
            primal_norm = r_norm;
            eps_dual = tol * (std::sqrt(N) + std::sqrt(R[ER_N + GR_GU2]));
            eps_primal = tol * (std::sqrt(E) + std::max(std::sqrt(R[ER_D2]), std::sqrt(R[ER_A2])));
            const double tau = 2.0;
            if (primal_norm > 10 * dual_norm) {
                rho_next = tau * rho;
                c_next = 1.0 / tau;
            } else if (dual_norm > 10 * primal_norm) {
                rho_next = 1.0 / tau * rho;
                c_next = tau;
            }
            S.s_norm = dual_norm;
            S.eps_pri = eps_primal;
            S.eps_dual = eps_dual;
        } else if (variant == MVTV_VARIANT_CPP) {
            // :118-126 — s uses the new alpha and the old u; rho is an int
            const double s_norm = std::fabs(rho) * std::sqrt(R[ER_N + GR_S2A]);
            dtheta = R[ER_DTH];
            S.s_norm = s_norm;
            if (o.fixed_iters <= 0 && counter > A.max_counter) {
                status = MVTV_MAXITER;
                fail(status, "Failed to converge!");
                rho_next = rho;
            } else {
                if (r_norm > 20 * s_norm) {
                    rho_next = 20 * rho;
                    c_next = 0.05;
                } else if (s_norm > 20 * r_norm) {
                    rho_next = 0.1 * rho;
                    c_next = 10.0;
                }
                rho_next = double(int(rho_next));
            }
        } else {
            dtheta = R[ER_DTH];
        }
        S.r_norm = r_norm;
        S.dtheta_max = dtheta;
        std::swap(gprev, gnew);
        c_prev = c_next;
        rho = rho_next;
        if (variant == MVTV_VARIANT_RCPP) sigma = rho;   // spcrosses = crossO + rho crossD (:126)
        if (status == MVTV_MAXITER) break;
        if (variant == MVTV_VARIANT_RCPP && o.fixed_iters <= 0 && counter > A.max_counter) {
            if (o.verbose) std::printf("ADMM reached max_counter at lambda = %g\n", lambda);
            status = MVTV_MAXITER;
            break;
        }
    }
    P->harvest();   // the stream is idle here (last iteration synchronised)
    guard.armed = false;
    if (A.twin) {
        HIP_TRY(fill_twins(P->g, P->order, P->stream, P->edges));
        HIP_TRY(hipStreamSynchronize(P->stream));
    }
    if (o.verbose) std::printf("Lambda= %g, Counter = %d\n", lambda, counter);
    // keep the resident state consistent: g_uprev buffer is P->guprev
    if (gprev != P->guprev) std::swap(P->guprev, P->gu);
    P->edge_mode = mode;
    P->t_z = t_z;
    P->c_state = c_prev;
    P->rho = rho;
    S.iters = it;
    S.theta_solver = A.spectral ? MVTV_SOLVER_SPECTRAL : (A.pcg_spec ? MVTV_SOLVER_PCG_SPECTRAL : MVTV_SOLVER_PCG);
    S.rho = rho;
    S.status = status;
    return A.report(S);
}

}  // namespace
}  // namespace mvtv

extern "C" mvtv_status mvtv_admm_run(mvtv_problem* P, const mvtv_admm_opts* opts, double lambda,
                                     mvtv_admm_stats* stats) {
    if (!P || !opts) return fail(MVTV_BAD_ARG, "null problem/opts");
    MVTV_TRY(ensure_state(P));
    if (!(lambda >= 0.0)) return fail(MVTV_BAD_ARG, "lambda must be >= 0");
    AdmmSetup A;
    A.t0 = std::chrono::steady_clock::now();
    A.stats = stats;
    DeviceGuard dg(P->device);
    MVTV_TRY(admm_prologue(P, *opts, lambda, A));
    TwinGuard guard{P, A.twin};
    // the device-controlled loop always runs its first iteration; a run whose loop condition fails at once goes to
    // the host loop, whose top test ends it. MVTV_ADMM_SYNC is read at every call (tests flip it between calls)
    const bool first_runs = A.o.fixed_iters > 0 || A.o.variant == MVTV_VARIANT_RCPP ||
                            (A.dtheta > A.tol && !(A.o.variant == MVTV_VARIANT_PY && A.max_counter <= 0));
    if (A.spectral && first_runs && !std::getenv("MVTV_ADMM_SYNC")) return admm_device_loop(P, A, guard);
    return admm_host_loop(P, A, guard);
}
