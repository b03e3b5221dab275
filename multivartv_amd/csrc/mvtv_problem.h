// mvtv_problem.h — the mvtv_problem handle and host helpers shared by the C-ABI translation units
// (mvtv_capi.cpp: setup, theta-solves, operators, batch calls, instrumentation; mvtv_admm.cpp: the ADMM loop of one
// GPU and the parts of an iteration it shares with the slab loop; mvtv_slab.cpp: the slab-decomposed loop over RCCL).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "mvtv/mvtv.h"
#include "mvtv_internal.h"

namespace mvtv {
extern thread_local std::string g_last_error;

inline mvtv_status fail(mvtv_status s, const std::string& msg) {
    g_last_error = msg;
    return s;
}
}  // namespace mvtv

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return mvtv::fail(_e == hipErrorOutOfMemory ? MVTV_OUT_OF_MEMORY : MVTV_HIP_ERROR,        \
                              std::string(#expr) + ": " + hipGetErrorString(_e));                     \
    } while (0)

#define MVTV_TRY(expr)                        \
    do {                                      \
        mvtv_status _s = (expr);              \
        if (_s != MVTV_OK) return _s;         \
    } while (0)

namespace mvtv {
constexpr int kPcgPoll = 8;   // PCG iterations enqueued between host polls of the done flag

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline mvtv_status alloc(double** ptr, size_t n) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(ptr), std::max<size_t>(n, 1) * sizeof(double)));
    return MVTV_OK;
}
}  // namespace mvtv

using namespace mvtv;   // the handle's members use the device-side types

struct mvtv_problem {
    int device = 0;
    hipStream_t stream = nullptr;
    Geom g{};
    int order = 0, weighted = 1, wmode = W_IDENTITY;
    double deltas[MVTV_MAX_DIMS] = {0, 0, 0, 0};
    int codes[kMaxBlocks] = {0};
    int sprime[kMaxBlocks] = {0};
    uint64_t blk_len[kMaxBlocks] = {0};
    int64_t E = 0;
    int grid = 1;
    bool fused3d = true;   // fused Chronopoulos-Gear PCG for p = 3 (MVTV_PCG=classic disables)
    int pcg_hint = 0;      // PCG iterations of the last theta-solve (poll schedule)

    double *oty = nullptr, *wdiag = nullptr;
    double *theta = nullptr, *edges = nullptr, *ga = nullptr, *gu = nullptr, *guprev = nullptr;
    double *r = nullptr, *p = nullptr, *q = nullptr, *thold = nullptr, *p2 = nullptr;
    double *partials = nullptr, *red = nullptr;
    PcgState* st = nullptr;
    double* stage = nullptr;
    size_t stage_n = 0;
    double* host_red = nullptr;   // pinned: reductions + PcgState mirror
    PcgState* host_st = nullptr;
    SpecPlan spec;                // spectral theta-solve tables (allocated when the mesh allows it)
    bool spec_mesh = false;       // spectral solve: every dimension j < p - 1 has a transform (m_j <= 4096, or a two-pass
                                  // split); a slab rank: m_j <= 4096 for every j
    int32_t split_forced[kMaxDims] = {0, 0, 0, 0};   // mvtv_problem_dct_split: the first factor per dimension, 0 automatic
    // mvtv_problem_dct_chirp: the convolution's factors (a, b) per dimension; a = -1 the library's, 0 off
    int32_t chirp_forced[kMaxDims][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    bool spec_long = false;       // ... with a last dimension longer than 4096 (the blocked line solve, spec.lb)
    bool spec_pow2 = false;       // ... and a power of two (k_dct8 / k_trir passes)
    bool spec_lead = false;       // dims 0..p-2 have a transform (the slab loop: the last dimension may have any length)
    bool e3d = false;             // z-marching 3-D edge kernels
    bool f3d = false;             // fused 3-D edge update + gather (needs the second edge buffer)
    bool f4d = false;             // fused 4-D edge update + gather pass A (k_admm4a; second edge buffer, g4)
    double* edges2 = nullptr;     // ping-pong partner of edges for the fused kernel
    bool zpicked = false;         // the z ping-pong pair was chosen by timed probes (pick_zpair)
    double* pcg_b = nullptr;      // right-hand side of the spectrally preconditioned PCG
    double* g4 = nullptr;         // 4 N-arrays: the two-pass 4-D gather's partial sums
    double wmean = 1.0;           // mean(W): the preconditioner's identity weight
    double wstd = 0.0;            // std(W): chooses the diagonally scaled spectral preconditioner
    double wsum_own = 0.0, wsum2_own = 0.0;   // sum W, sum W^2 over the nodes [ibeg, iend) (slab: owned planes)
    double* pcg_s = nullptr;      // 1/s of the scaled spectral preconditioner
    double* pcg_t = nullptr;      // r / s, the preconditioner's input
    // the marching line sweeps of the 3-D spectral solve (k_sweep; mvtv_problem_line_sweep)
    int ls_mode = -1;             // -1 auto (the gate), 0 off, 1 on wherever the shape admits it
    int ls_chunks = 0;            // chunks over dim 2 in use; 0: the five-pass solve
    double *ls_coef = nullptr, *ls_lr = nullptr;   // the chunks' pairs and carries, ls_cap chunks each
    int ls_cap = 0;
    AdmmCtl* ctl = nullptr;       // device control block of the asynchronous ADMM loop
    AdmmCtl* host_ctl = nullptr;  // pinned mirror
    int admm_hint = 0;            // ADMM iterations of the last converged run (enqueue-ahead depth)

    // batched small-mesh fits (mvtv_path_batch, mvtv_solve_batch)
    int batch_cos = 0;            // mvtv_problem_batch_cosine: 0 Jacobi-PCG for all, 1 exact cosine solve for W = I
                                  // members, 2 also cosine-preconditioned PCG for the others
    CosPlan cos;                  // the in-workgroup cosine solve's plan and device tables (cos.ld < 0: not built)
    void* batch_buf = nullptr;    // the batched calls' device buffers, kept between calls and grown on demand
    size_t batch_cap = 0;

    // slab decomposition (mvtv_problem_create_slab): this problem holds planes [zb, ze) of dim p-1
    // of a mesh with m_global planes, plus ghost planes below / above
    bool slab = false;
    int64_t m_global = 0, zb = 0, ze = 0;
    int g_lo = 0, g_hi = 0;
    double* slab_iface = nullptr;  // mvtv_slab_run: interface numbers of the distributed line solves (16 per line)
    hipStream_t comm_stream = nullptr;   // mvtv_slab_run: the collectives' stream (overlapped with `stream`)

    // resident ADMM state
    bool have_state = false;
    bool u_default = true;
    // the twin blocks (mvtv_internal.h twin_block) hold equal u: true for the variant defaults, checked on import
    bool twin_ok = true;
    bool twin_timed = false;   // the timed fused launches skipped the twin block (its bytes are not counted)
    int edge_mode = U_EXPLICIT;
    double t_z = 0.0, c_state = 1.0, rho = 0.0;

    // instrumentation
    bool timing = false;
    struct Pending {
        hipEvent_t a, b;
        int kid;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
    double ms[MVTV_K_COUNT] = {0};
    int64_t launches[MVTV_K_COUNT] = {0};
    int64_t fold_fix = 0;   // timed folded first passes that also read g_u (a rho change before them)
    int64_t pcg_xmoves = 0;   // timed fused PCG iterations that also moved x (the odd ones)

    Launch L() const { return Launch{stream, grid}; }

    hipEvent_t get_event() {
        if (!ev_pool.empty()) {
            hipEvent_t e = ev_pool.back();
            ev_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    int tstart(int kid) {
        if (!timing) return -1;
        Pending pd{get_event(), get_event(), kid};
        g_timed = TimedLaunch{pd.a, pd.b};   // stamped by the next kernel dispatch (klaunch)
        pending.push_back(pd);
        return int(pending.size()) - 1;
    }
    void tstop(int h) {
        if (h >= 0 && g_timed.start) pending[h].kid = -1;   // the launcher enqueued nothing
        g_timed = TimedLaunch{};
    }
    // second launch of a two-kernel launcher (armed in g_timed_b, moved to g_timed by the launcher)
    int tstart_b(int kid) {
        if (!timing) return -1;
        Pending pd{get_event(), get_event(), kid};
        g_timed_b = TimedLaunch{pd.a, pd.b};
        pending.push_back(pd);
        return int(pending.size()) - 1;
    }
    void tstop_b(int h) {
        if (h >= 0 && g_timed_b.start) pending[h].kid = -1;
        g_timed_b = TimedLaunch{};
    }
    void harvest() {  // call after a stream sync
        for (auto& pd : pending) {
            float t = 0.f;
            if (pd.kid >= 0 && hipEventElapsedTime(&t, pd.a, pd.b) == hipSuccess) {
                ms[pd.kid] += t;
                launches[pd.kid] += 1;
            }
            ev_pool.push_back(pd.a);
            ev_pool.push_back(pd.b);
        }
        pending.clear();
    }
    mvtv_status sync() {
        HIP_TRY(hipStreamSynchronize(stream));
        harvest();
        return MVTV_OK;
    }
};

namespace mvtv {
// ---- mvtv_capi.cpp: what the ADMM loop needs of the setup and the theta-solves
double variant_tol(const mvtv_admm_opts& o);
int variant_maxc(const mvtv_admm_opts& o);
mvtv_status ensure_state(mvtv_problem* P);
bool spectral_ok(const mvtv_problem* P);
bool split_on(const mvtv_problem* P);
mvtv_status spectral_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                           const double* gb, double cb, double* x, const AdmmCtl* ctl = nullptr, double w0 = 1.0,
                           const int32_t* skip = nullptr, bool fold = false);
mvtv_status pcgs_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                       const double* gb, double cb, double* x, double rtol, int maxit, int* iters, double* relres);
mvtv_status pcg_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                      const double* gb, double cb, double* x, double rtol, int maxit, int* iters, double* relres);

// ---- mvtv_admm.cpp: the part of an ADMM iteration after the theta-solve, shared by the device-controlled loop, the
// host-controlled loop and the slab loop. The edge work of one iteration:
struct EdgePass {
    int umode = U_FROM_Z;                        // how the edge buffer holds u on entry (U_EXPLICIT: a run's first pass)
    const double* z_old = nullptr;               // z ping-pong; z_new == z_old where the layout updates in place
    double* z_new = nullptr;
    double* g_new = nullptr;                     // D^T u of this iteration, and the previous one's
    const double* g_prev = nullptr;
    const double* theta_old = nullptr;           // max|theta - theta_old| wanted (variants A, C), or null
    const AdmmCtl* ctl = nullptr;                // the kernels take thresholds and scales from the control block, and skip
                                                 // once it says done; then the by-value scalars keep these neutral values
    double t_old = 0.0, c_old = 1.0, t_new = 0.0, c_prev = 1.0;
    bool fold = false, twin = false;
    bool timed_red = false;                      // the reductions are counted under MVTV_K_REDUCE
    bool ctl_step = false;                       // the last reduction also runs the control step on P->ctl
};
// edge stage: the edge update (fused with the gather, or with its pass A, where the mesh allows) and its sums into
// P->red; gather stage: what is left of D^T alpha and D^T u, and its sums into P->red + ER_N. Two calls, so that the
// slab loop can move its z halo between them.
mvtv_status edge_stage(mvtv_problem* P, const EdgePass& e);
mvtv_status gather_stage(mvtv_problem* P, const EdgePass& e);

// the device-controlled loops (one GPU's and the slab's): the control block at the start of a run, enqueued on P->stream
mvtv_status admm_ctl_start(mvtv_problem* P, int variant, int fixed_iters, int max_counter, double tol, double lambda,
                           double rho, double sigma, double c_prev, double t_z, double dtheta, double sqrtN,
                           double sqrtE);
// enqueue iterations ahead of the device's decisions and poll the control block (left in P->host_ctl) until it says
// done or `limit` iterations are enqueued. First poll after fixed_iters, else the last converged run's count, else 16;
// then every max(4, enq / 4). single: one iteration per poll. mark: the first timing entry of each iteration
mvtv_status admm_enqueue_ahead(mvtv_problem* P, const std::function<mvtv_status(int)>& enqueue, int fixed_iters,
                               int limit, bool single, std::vector<size_t>& mark);
// after the last poll: timing entries of the iterations past the stop dropped and the rest harvested, the ping-pong
// parities (D^T u; z with `pingpong`) put back so that P->guprev and P->edges hold the state, the resident scalars and
// the stats the control block gives. The caller adds the solver, its PCG counts and the seconds
mvtv_admm_stats admm_finish(mvtv_problem* P, const std::vector<size_t>& mark, int fixed_iters, bool fold, bool pingpong);

// The fused kernels may skip the twin blocks (mvtv_internal.h twin_block) of a one-GPU problem; their edge words
bool twin_ready(const mvtv_problem* P);
double twin_edges(const mvtv_problem* P);
// timed choice of the fused 3-D kernel's z ping-pong buffer pair, once per problem
mvtv_status pick_zpair(mvtv_problem* P, bool track_theta, bool twin);
}  // namespace mvtv
