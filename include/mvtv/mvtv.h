/*
 * mvtv.h — C ABI of the MI355X-native mesh-TV ADMM solver (libmvtv.so).
 *
 * This is the drop-in boundary for the reference's ADMM hot path. Every entry
 * point replaces one reference interface (cited as path:line under
 * /root/reference) and uses only plain pointers, sizes and PODs: no Armadillo,
 * Rcpp or torch types. Host buffers are caller-owned; device buffers are owned
 * by the opaque mvtv_problem handle (one handle per GPU; handles are
 * thread-safe with respect to each other, a single handle is not).
 *
 * Layouts (identical to the reference):
 *   theta  [N]  mesh values, column-major, dim 0 fastest (cpp-code/utils.cpp:40-52)
 *   u      [E]  scaled dual, blocks concatenated in the D row order of the
 *               caller (C++ create_D: all-ones block first; Python create_D:
 *               b = 1..), each block a column-major reduced grid
 *               (cpp-code/utils.cpp:103-134, 245-269; code/utils.py:138-149)
 *
 * Errors never cross the ABI as exceptions: every call returns mvtv_status and
 * leaves a message readable through mvtv_last_error() (thread-local).
 */
#ifndef MVTV_MVTV_H
#define MVTV_MVTV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVTV_MAX_DIMS 4
#define MVTV_MAX_BLOCKS 15

typedef enum mvtv_status {
    MVTV_OK = 0,
    MVTV_MAXITER = 1,        /* A: "Failed to converge!" (cpp-code/solvers.cpp:122-124); B: max_counter break (rcpp…/solvers.cpp:129-132) */
    MVTV_BAD_ARG = 2,
    MVTV_DIM_MISMATCH = 3,   /* reference's mixed-partial product fails for this mesh */
    MVTV_HIP_ERROR = 4,
    MVTV_NO_DEVICE = 5,
    MVTV_OUT_OF_MEMORY = 6,
    MVTV_PCG_NOT_CONVERGED = 7 /* only reported when opts.pcg_strict != 0 */
} mvtv_status;

/* Which reference implementation's ADMM semantics to follow. */
typedef enum mvtv_variant {
    MVTV_VARIANT_RCPP = 0,   /* B: rcpp-code/MultivarTV/src/solvers.cpp:96-136 (released package) */
    MVTV_VARIANT_CPP = 1,    /* A: cpp-code/solvers.cpp:90-130 (int rho, theta-change stop) */
    MVTV_VARIANT_PY = 2      /* C: code/solvers.py:53-76 (fixed rho = lambda, threshold 1) */
} mvtv_variant;

/* Row-block order of D (low bit) and the rule that gives a block its difference set (bit 1).
 * Orders 0 and 1 follow the reference: its mixedpartial differences along dim 0 first, so a mixed block whose
 * set S misses dim 0 acts as S' = (S \ {min S}) + {0}, and a mesh with m_0 != m_{min S} is refused
 * (MVTV_DIM_MISMATCH): every 3-D mesh with m_0 != m_1, every 4-D mesh unless m_0 = m_1 = m_2.
 * Orders 2 and 3 keep the row order, the weights and the leading / dropped all-ones block of 0 and 1 and
 * difference block b along exactly the dims whose bit is set in b (true mixed partials, D^T D =
 * sum_S w_S^2 (x)_{j in S} L_j): any m_j >= 2 is accepted, no two blocks share a set, and E, the block
 * lengths, mvtv_problem_block_info and the layout of u follow these sets. For p <= 2 both rules give the
 * same D and orders 2, 3 compute bit for bit what 0, 1 compute. mvtv_problem_create_slab takes orders 0, 1 only. */
typedef enum mvtv_block_order {
    MVTV_ORDER_CPP = 0,      /* C++ create_D: [all-ones, w=1] + b=1..2^p-2 (cpp-code/utils.cpp:245-269) */
    MVTV_ORDER_PY = 1,       /* Python create_D: b=1..2^p-1 unweighted, or b=1..2^p-2 weighted (code/utils.py:138-149) */
    MVTV_ORDER_CPP_NOMINAL = 2, /* rows and weights of MVTV_ORDER_CPP, nominal difference sets */
    MVTV_ORDER_PY_NOMINAL = 3   /* rows and weights of MVTV_ORDER_PY, nominal difference sets */
} mvtv_block_order;

/* Replaces the mbs_cache / mbs_one_inits bundles (rcpp…/solvers.hpp:30-50,
 * cpp-code/solvers.hpp:25-43): instead of sparse O, D, D^T D the problem is the
 * mesh shape, the block weights and the diagonal W = O^T O with O^T y. */
typedef struct mvtv_problem_desc {
    int32_t p;                       /* 1..4 dimensions */
    int64_t m[MVTV_MAX_DIMS];        /* mesh points per dimension (each >= 2) */
    int32_t block_order;             /* mvtv_block_order */
    int32_t weighted;                /* 1: w_b = prod_{j not in b} deltas_j; 0: every w = 1 */
    double deltas[MVTV_MAX_DIMS];    /* mesh widths (create_deltas, rcpp…/utils.cpp:256-263) */
    const double* oty;               /* [N] O^T y (required) */
    const double* wdiag;             /* [N] diag(O^T O), or NULL for W = I (mesh == data) */
    int32_t device;                  /* HIP device ordinal */
} mvtv_problem_desc;

typedef struct mvtv_admm_opts {
    int32_t variant;        /* mvtv_variant */
    double tol;             /* <= 0: variant default (B 1e-4 rcpp…/solvers.hpp:19; A 1e-3 cpp-code/solvers.hpp:14; C 1e-3) */
    int32_t max_counter;    /* <= 0: variant default (B 3000, A 2000, C 1000000 — the reference's C guard is dead) */
    int32_t fixed_iters;    /* > 0: run exactly this many iterations, stopping test disabled (trajectory / bench mode) */
    double sigma;           /* solve-matrix scalar W + sigma D^T D at entry; NaN: variant default (B rho, A lambda, C lambda) */
    double ymean;           /* mean(y): A and C initialise theta_old from it (cpp-code/solvers.cpp:103, code/solvers.py:63) */
    double pcg_rtol;        /* <= 0: 1e-10 (relative to ||b||) */
    int32_t pcg_max_iter;   /* <= 0: 20000 */
    int32_t pcg_strict;     /* != 0: report MVTV_PCG_NOT_CONVERGED when a theta-solve stops at pcg_max_iter */
    int32_t verbose;        /* != 0: print "Lambda= .., Counter = .." like rcpp…/solvers.cpp:134 */
    int32_t theta_solver;   /* mvtv_theta_solver: how spsolve(spcrosses, b) (rcpp…/solvers.cpp:113) is replaced */
} mvtv_admm_opts;

/* theta-solve of (W + sigma D^T D) theta = b. The reference factorises with SuperLU every
 * iteration (rcpp…/solvers.cpp:113, cpp-code/solvers.cpp:116, code/solvers.py:72). */
typedef enum mvtv_theta_solver {
    MVTV_SOLVER_AUTO = 0,      /* SPECTRAL where it is exact; else PCG_SPECTRAL on the same meshes; else PCG */
    MVTV_SOLVER_PCG = 1,       /* Jacobi-PCG on the 3^p-point stencil, warm-started, pcg_rtol */
    MVTV_SOLVER_SPECTRAL = 2,  /* direct: cosine transforms + a tridiagonal solve along the last dim. Exact for
                                  W = I (mesh == data) with, for j < p - 1, m_j <= 4096 (FFT plans for lengths with
                                  prime factors 2, 3, 5, 7, Bluestein's chirp-z for any other) or m_j = a * b with
                                  both factors <= 4096 and 2-3-5-7-smooth (two passes, one GPU), or any m_j under
                                  mvtv_problem_dct_chirp (opt-in, one GPU), and a last dimension
                                  of any length (never transformed: a line solve, in blocks past 4096 rows);
                                  MVTV_BAD_ARG otherwise */
    MVTV_SOLVER_PCG_SPECTRAL = 3 /* PCG preconditioned by S (mean(W) I + sigma D^T D) S, its middle factor inverted
                                  exactly by cosine transforms, S = I or a Jacobi-like diagonal scaling when W varies
                                  strongly against sigma D^T D's diagonal: for W != I (scattered data, CV folds) on
                                  the meshes SPECTRAL accepts */
} mvtv_theta_solver;

typedef struct mvtv_admm_stats {
    int32_t iters;          /* ADMM iterations executed */
    int32_t status;         /* mvtv_status of the run */
    double r_norm, s_norm;  /* last primal / dual residual norms */
    double eps_pri, eps_dual;
    double rho;             /* final rho (after the last adaptation) */
    double dtheta_max;      /* last max|theta - theta_old| (A, C) */
    int64_t pcg_iters;      /* total PCG iterations */
    int32_t pcg_iters_max;  /* max PCG iterations in one theta-solve */
    int32_t pcg_unconverged;/* theta-solves that hit pcg_max_iter */
    double seconds;         /* wall time of the call */
    int32_t theta_solver;   /* the solver that ran (MVTV_SOLVER_PCG or MVTV_SOLVER_SPECTRAL) */
} mvtv_admm_stats;

typedef struct mvtv_problem mvtv_problem;

/* ---- library -------------------------------------------------------------------- */
const char* mvtv_version(void);
const char* mvtv_status_string(int32_t status);
const char* mvtv_last_error(void);
int32_t mvtv_device_count(void);
void mvtv_default_opts(mvtv_admm_opts* opts, int32_t variant);

/* ---- problem (replaces create_cache_objects / fill_cache / use_cache,
 *      rcpp…/solvers.cpp:36-69; cpp-code/solvers.cpp:31-62) ------------------------ */
mvtv_status mvtv_problem_create(const mvtv_problem_desc* desc, mvtv_problem** out);
void mvtv_problem_destroy(mvtv_problem* prob);
int64_t mvtv_problem_nodes(const mvtv_problem* prob);   /* N = ntheta (rcpp…/solvers.hpp:36) */
int64_t mvtv_problem_edges(const mvtv_problem* prob);   /* E = rowsD (rcpp…/solvers.hpp:35) */
int32_t mvtv_problem_blocks(const mvtv_problem* prob);
/* block k's binary code, difference set (bit j = dim j: S' under orders 0 and 1, the code's own dims under the
 * nominal orders) and weight */
mvtv_status mvtv_problem_block_info(const mvtv_problem* prob, int32_t k, int32_t* code, int32_t* sprime, double* weight);
/* new O^T y and W for the same mesh (CV folds re-run create_cache_objects, rcpp…/solvers.cpp:347-348) */
mvtv_status mvtv_problem_set_data(mvtv_problem* prob, const double* oty, const double* wdiag);
/* 1 if MVTV_SOLVER_SPECTRAL applies to this problem (W = I; every m_j, j < p - 1, <= 4096 or, on one GPU, a product of
 * two 2-3-5-7-smooth factors <= 4096; the last dimension any length on one GPU), else 0. What is refused by default: a
 * leading dimension above 4096 with a prime factor >= 11 (4099, 4100 = 2^2 5^2 41), which mvtv_problem_dct_chirp or
 * MVTV_DCT_CHIRP=1 switches on; what stays refused: any dimension above 4096 on a slab rank but the last of G >= 2. */
int32_t mvtv_problem_spectral_ok(const mvtv_problem* prob);
/* The line solve along the last dimension in `blocks` blocks [floor(m k / blocks), floor(m (k + 1) / blocks)) of every
 * line: per-block recursion sums, an interface step that gives every block its carries and closes the mirror, and a
 * rerun from the carries (three launches, 3N words instead of the 2N of a line that fits one workgroup). blocks 0:
 * automatic (the default): the one-workgroup kernels where m_last <= 4096, the library's block count beyond. blocks
 * >= 2: that many blocks at any m_last (tests; an A/B against the one-workgroup kernels; the marching line sweeps
 * rest meanwhile). MVTV_BAD_ARG for blocks < 0, 1, > m_last, a block longer than a workgroup takes (4096 rows at
 * p = 1; 1024 at p >= 2, 2048 with fewer than 16 lines), a slab rank, or a mesh the spectral solve does not accept. Waits for the problem's stream;
 * (re)allocates 4 * blocks * N / m_last doubles of scratch. */
mvtv_status mvtv_problem_line_blocks(mvtv_problem* prob, int32_t blocks);
/* Cosine transforms along dimension dim (< p - 1) in two passes over the factorisation m_dim = a * (m_dim / a).
 * a = 0: automatic (the default: only where m_dim > 4096, the library's factorisation). a >= 2: that first
 * factor at any m_dim (tests; an A/B against the one-workgroup kernels; the passes that hold a whole line of a leading
 * dimension in one workgroup, the marching line sweeps, the fused plane pass, the folded right-hand side and the
 * PCG-fused passes, rest meanwhile). The frequencies of a split dimension stay in the order position
 * (m_dim / a) * k1 + k2 <-> k = k1 + a * k2 between the forward and the inverse pass. MVTV_BAD_ARG for dim < 0 or
 * >= p - 1, a = 1, a < 0, a that does not divide m_dim, a factor above 4096 or with a prime factor >= 11, a slab
 * rank, or a mesh the spectral solve does not accept. Waits for the problem's stream; (re)allocates the splits' tables
 * (32 B * (4096 + m_dim / 1024) + 20 B * (a + b) a dimension) and one scratch vector of <= N + m_dim doubles. */
mvtv_status mvtv_problem_dct_split(mvtv_problem* prob, int32_t dim, int32_t a);
/* Cosine transforms along dimension dim (< p - 1) by Bluestein's chirp-z identity with the length-M circular
 * convolution, M = a * b >= 2 m_dim - 1, run as a two-pass FFT: any m_dim, so also a leading dimension above 4096 with
 * a prime factor >= 11 (three launches a transform: columns in, fused rows, columns out). a = b = 0: off for that
 * dimension (the default; a dimension that then has no transform makes the mesh refused again, and the scratch, the
 * blocked line solve's and the line sweeps' buffers are released). a = -1 (b ignored): the library's M, the smallest 2-3-5-7-smooth M >= 2 m_dim - 1 with a factorisation into two factors <= 4096, a the
 * largest such divisor <= sqrt(M). a, b >= 2: that M at any m_dim >= 2, both factors 2-3-5-7-smooth and <= 4096 (tests;
 * the passes that rest under mvtv_problem_dct_split rest here too). The frequencies stay in natural order.
 * MVTV_BAD_ARG for dim < 0 or >= p - 1, a factor above 4096 or with a prime factor >= 11, a * b < 2 m_dim - 1, a slab
 * rank, a dimension with a forced mvtv_problem_dct_split (and dct_split(dim, a >= 2) on a dimension under chirp),
 * a = -1 where no M exists (m_dim > (4096^2 + 1) / 2). Waits for the problem's stream, re-evaluates which solvers
 * the mesh admits (mvtv_problem_spectral_ok, MVTV_SOLVER_AUTO) and (re)builds what a spectral problem owns: the tables
 * (16 B * (2 m_dim + M) and the factor tables a dimension) and one scratch vector of 2 * ceil(lines / 2) * M doubles,
 * about 2N; when that fails (MVTV_OUT_OF_MEMORY) the problem keeps the mode it had. The environment variable
 * MVTV_DCT_CHIRP=1, read at problem creation, starts every leading dimension above 4096 without a two-pass
 * factorisation (and with an M) in the automatic mode (not on a slab rank). */
mvtv_status mvtv_problem_dct_chirp(mvtv_problem* prob, int32_t dim, int32_t a, int32_t b);
/* the factors in use along dim (the automatic choice included); 0, 0: the dimension is not under chirp */
mvtv_status mvtv_problem_dct_chirp_get(const mvtv_problem* prob, int32_t dim, int32_t* a, int32_t* b);
/* The marching line sweeps of the 3-D spectral solve (m_1 = 512, m_0 a multiple of 16, one GPU): the dim-1 transforms
 * fused into the dim-2 line solve, two passes over the vector and an interface step over `chunks` chunks of dim 2 in
 * place of three passes. mode -1: automatic (the default: meshes of more than 2^24 nodes that fill the GPU with
 * chunks of >= 8 planes), 0: off, 1: on wherever the shape admits it (any size; other shapes keep the five-pass solve).
 * chunks 0: chosen by the library's cost model; mode 1 accepts 1 <= chunks <= min(m_2, 64). Waits for the problem's
 * stream; (re)allocates 4 * chunks * m_0 * m_1 doubles of scratch. The environment variable MVTV_LINE_SWEEP=0, read
 * when a problem is created, starts it in mode 0. */
mvtv_status mvtv_problem_line_sweep(mvtv_problem* prob, int32_t mode, int32_t chunks);

/* ---- the hot path ------------------------------------------------------------------ */
/* Drop-in for admm_update:
 *   B: void admm_update(vec y, mbs_one_inits, vec& theta_init, double lambda, bool verbose,
 *                       vec& u_init, double& rho_init, admm_out&)   rcpp…/solvers.hpp:100
 *   A: vec admm_update(vec y, mbs_one_inits, vec* theta_init, double lambda)  cpp-code/solvers.hpp:85
 *   C: the while-loop of mbs_one                                     code/solvers.py:53-76
 * theta_inout [N]: theta_init in, theta out. u_inout [E]: u_init in / u out, or NULL for the
 * variant's own u0 (B 0, A and C 1/lambda) with u not returned. rho_inout: rho_init in /
 * rho out (B; A and C derive rho from lambda and return the final one). */
mvtv_status mvtv_admm(mvtv_problem* prob, const mvtv_admm_opts* opts, double lambda,
                      double* theta_inout, double* u_inout, double* rho_inout, mvtv_admm_stats* stats);

/* Resident form of the same loop for callers that keep the state in HBM across calls
 * (lambda paths with warm start rcpp…/solvers.cpp:212-220, benchmarks). */
mvtv_status mvtv_state_set(mvtv_problem* prob, const double* theta, const double* u, double rho);
mvtv_status mvtv_state_get(mvtv_problem* prob, double* theta, double* u, double* rho);
mvtv_status mvtv_admm_run(mvtv_problem* prob, const mvtv_admm_opts* opts, double lambda, mvtv_admm_stats* stats);
/* mbs_path's lambda loop (rcpp…/solvers.cpp:204-222) in one call: from theta_init [N], the variant's
 * u0 and rho_init, the ADMM state (theta, u, rho) is carried on the device from each lambda to the
 * next (:217-219). thetas_out [n_lambda x N] (may be NULL): theta after each lambda, lambda-major.
 * rhos_out, stats [n_lambda] (may be NULL). The state stays resident (mvtv_state_get reads the last).
 * Returns MVTV_MAXITER when some lambda hit max_counter (the loop goes on, as B breaks and goes on). */
mvtv_status mvtv_path(mvtv_problem* prob, const mvtv_admm_opts* opts, const double* lambdas, int32_t n_lambda,
                      const double* theta_init, double rho_init, double* thetas_out, double* rhos_out,
                      mvtv_admm_stats* stats);
/* Batched small-mesh fits: nbatch independent paths on the problem's mesh in one call, each member run start to
 * finish by one workgroup with no host in its ADMM loop (variant B, u0 = 0; theta-solve: Jacobi-PCG on W + rho D^T D,
 * warm-started, the stopping rule of MVTV_SOLVER_PCG). prob supplies only the geometry (p, m, deltas, block order,
 * weights), the device and the stream; its own data and resident state are not touched. A member's result does not
 * depend on its position in the batch or on the batch size.
 * mvtv_problem_batch_ok: 1 when the mesh is admitted: not a slab rank, N <= 4096 for p <= 3, N <= 1296 for p = 4.
 * Members are member-major in every array; (theta, u, rho) are carried from each lambda to the next per member, as
 * mvtv_path does, and the next lambda starts once every member has finished the current one. n_lambda = 1 is the
 * batched single fit. Honoured options: fixed_iters, tol, max_counter, pcg_rtol, pcg_max_iter, pcg_strict.
 * MVTV_BAD_ARG (before any launch) for: a mesh that is not admitted; a variant other than MVTV_VARIANT_RCPP; a
 * theta_solver other than AUTO or PCG (but see mvtv_problem_batch_cosine); a non-NaN opts.sigma; nbatch < 1 or n_lambda < 1; a lambda < 0; a rho_init that is
 * not positive and finite; a member whose W has a negative entry or no positive one. stats[b, l] holds that member's own iters, status, norms, eps, rho and
 * PCG counts (theta_solver = MVTV_SOLVER_PCG unless mvtv_problem_batch_cosine says otherwise; seconds: the call's wall time). Returns MVTV_MAXITER when some (member,
 * lambda) hit max_counter (the others are unaffected), MVTV_PCG_NOT_CONVERGED under pcg_strict likewise. */
int32_t mvtv_problem_batch_ok(const mvtv_problem* prob);
mvtv_status mvtv_path_batch(mvtv_problem* prob, const mvtv_admm_opts* opts, int32_t nbatch,
                            const double* oty,        /* [nbatch x N] */
                            const double* wdiag,      /* [nbatch x N], or NULL: W = I for every member */
                            const double* lambdas,    /* [nbatch x n_lambda], member-major */
                            int32_t n_lambda,
                            const double* theta_init, /* [nbatch x N] */
                            const double* rho_init,   /* [nbatch] */
                            double* thetas_out,       /* [nbatch x n_lambda x N], may be NULL */
                            double* u_out,            /* [nbatch x E], u after the last lambda in the problem's D row order, may be NULL */
                            double* rhos_out,         /* [nbatch x n_lambda], may be NULL */
                            mvtv_admm_stats* stats);  /* [nbatch x n_lambda], may be NULL */
/* The batched fits' cosine theta-solve, opt-in per problem (mvtv_small_cos.hip): the cosine-transform solve inside the
 * member's workgroup, dense transforms along every dimension but the longest and the factorised line solve along
 * that one. mode 0 (the default): mvtv_path_batch as described above in every respect. mode 1: members with W = I
 * (wdiag NULL, or a wdiag row of all ones) take the exact solve theta = (I + rho D^T D)^-1 b in place of the PCG loop
 * (pcg_iters stays 0); the others run Jacobi-PCG as under mode 0. mode 2: the others run PCG preconditioned by
 * S (mean(W) I + rho D^T D)^-1 S, the preconditioner and the scaling rule of MVTV_SOLVER_PCG_SPECTRAL evaluated per
 * member with the current rho, under the stopping rule and counters of MVTV_SOLVER_PCG.
 * With mode >= 1, opts.theta_solver means: AUTO as above, per member; PCG: Jacobi-PCG for every member; SPECTRAL:
 * accepted when every member has W = I, else MVTV_BAD_ARG; PCG_SPECTRAL: needs mode 2 (else MVTV_BAD_ARG) and runs
 * the preconditioned PCG for every member. stats.theta_solver reports what the member ran (MVTV_SOLVER_PCG,
 * _SPECTRAL or _PCG_SPECTRAL). MVTV_BAD_ARG for a mode outside 0..2 and on a mesh mvtv_problem_batch_ok refuses. */
mvtv_status mvtv_problem_batch_cosine(mvtv_problem* prob, int32_t mode);
mvtv_status mvtv_problem_batch_cosine_get(const mvtv_problem* prob, int32_t* mode);
/* x[b] = (shift[b] I + sigma[b] D^T D)^-1 f[b] for b < nbatch by that solve alone, one workgroup a member, whatever
 * the problem's batch_cosine mode. sigma [nbatch] >= 0; shift [nbatch] > 0, or NULL: 1; f, x [nbatch x N], member-major
 * (x may be f). MVTV_BAD_ARG on a mesh mvtv_problem_batch_ok refuses. */
mvtv_status mvtv_solve_batch(mvtv_problem* prob, int32_t nbatch, const double* sigma, const double* shift,
                             const double* f, double* x);
/* fitted values O theta for n points given their mesh index (fill_output_mbs_one, rcpp…/solvers.cpp:73) */
mvtv_status mvtv_fitted(mvtv_problem* prob, const int64_t* mesh_index, int64_t n, double* fitted);

/* ---- scattered data on the device ----------------------------------------------------
 * axes: the mesh's sorted axis values, m[0] values of dim 0, then m[1] of dim 1, ... (the linspace
 * axes of create_mesh, rcpp…/utils.cpp:234-254; mesh rows in column-major order). data: n x p,
 * column-major (arma::mat). mesh_index_out [n] (may be NULL): the column-major mesh node of each
 * point, i.e. the column of the 1 in row i of O.
 * Every coordinate must be finite (NaN or +-inf: MVTV_BAD_ARG; the reference maps an infinite point to node 0).
 * The indices equal the reference's brute-force scan for every point with, on every axis j,
 *     g_j (2 r_j + g_j) >= 4 (p + 2) 2^-53 sum_i R_i^2
 * g_j: smallest spacing of axis j; r_j: distance from x_j to its nearest node of axis j; R_i: distance from x_i to
 * the farther end of the axis-i cell that holds it (to the nearest node when x_i lies outside the axis). That is
 * every point inside the mesh box when the spacings lie within 2^25 / sqrt(p (p + 2)) of one another, and points
 * outside it up to about 2^25.5 / sqrt(p + 2) smallest spacings away; farther out float64 absorbs the other axes'
 * squared distances, whole rows of nodes tie, and the scan's first minimum need not be a corner of the point's cell. */
/* nearest1 / nearest_interp_matrix (rcpp…/utils.cpp:267-304): first nearest mesh row per point */
mvtv_status mvtv_nearest(mvtv_problem* prob, const double* axes, const double* data, int64_t n,
                         int64_t* mesh_index_out);
/* create_cache_objects (rcpp…/solvers.cpp:36-44) on the device: O from mvtv_nearest, then
 * W = diag(O^T O) and O^T y (summed per node in data order) installed as the problem's data, as by
 * mvtv_problem_set_data (W = I when every node holds exactly one point). */
mvtv_status mvtv_problem_set_scattered(mvtv_problem* prob, const double* axes, const double* data, int64_t n,
                                       const double* y, int64_t* mesh_index_out);
/* mbs_predict (rcpp…/solvers.cpp:161-165): O(data) theta of the resident state, fits [n] */
mvtv_status mvtv_predict(mvtv_problem* prob, const double* axes, const double* data, int64_t n, double* fits);
/* The whole k-fold CV of mbs_impl (rcpp…/solvers.cpp:305-376) for a mesh mvtv_problem_batch_ok admits, in one call:
 * the nearest-node map of the n points (one pass, as mvtv_nearest), every member's W, O^T y and constant start, all
 * paths as mvtv_path_batch runs them, and the test MSEs, on the device. Member 0 is the final path on all n points;
 * with folds >= 2, member f + 1 is trained on the points with fold[i] != f: members = 1 + (folds >= 2 ? folds : 0).
 * A member's W and O^T y are what create_cache_objects gives on its training subset, O^T y summed per node in data
 * order (bit-identical to mvtv_problem_set_scattered on that subset). Every member runs mvtv_path_batch's path on the
 * shared grid `lambdas` from theta = theta0[member], u = 0, rho = rho_init: variant B with (theta, u, rho) carried
 * from lambda to lambda, the theta-solver kinds of mvtv_problem_batch_cosine (each member's kind, mean(W) and std(W)
 * from mvtv_path_batch's own scan of the W built here), the same honoured options, per-(member, lambda) stats and
 * return status (MVTV_MAXITER, MVTV_PCG_NOT_CONVERGED under pcg_strict).
 *   mse_mat[l, f]  = mean over the points with fold[i] == f of (theta_{f+1,l}[node_i] - y_i)^2   (test_mse, :278-288);
 *                    with folds <= 1 the one column is member 0's mean over all points against y (:413)
 *   model_mses[l]  = member 0's mean over all points against ref (the path models' mbs_mse, :214)
 * each a deterministic sum within (k + 4) 2^-53 relative of the exact mean of its k terms. The call does not select a
 * lambda. prob supplies the geometry, the device and the stream; its own data and resident state are not touched.
 * Host <-> device traffic: the inputs once, the per-lambda poll of mvtv_path_batch, under a batch_cosine mode the
 * members' W for that scan, and one download of the results asked for.
 * MVTV_BAD_ARG, before any launch, for: everything mvtv_path_batch refuses (except SPECTRAL with a member whose W is
 * not I, found after the setup kernels); a NaN or infinite coordinate or axis value; folds >= 2 with fold NULL; a label
 * outside [0, folds); a fold with no test point; a member with no training point; n < 1 or n >= 2^32.
 * MVTV_OUT_OF_MEMORY when the problem's batch buffer cannot grow (the problem stays usable). */
mvtv_status mvtv_cv_batch(mvtv_problem* prob, const mvtv_admm_opts* opts,
                          const double* axes, const double* data, int64_t n, const double* y, /* as mvtv_problem_set_scattered */
                          const int32_t* fold,      /* [n] labels in [0, folds); may be NULL when folds <= 1 */
                          int32_t folds,
                          const double* ref,        /* [n] what model_mses is taken against (ftrue); NULL: y */
                          const double* lambdas, int32_t n_lambda,   /* one grid, shared by every member */
                          const double* theta0,     /* [members] each member's constant start; NULL: the mean of its y, summed in data order */
                          double rho_init,          /* NaN: lambdas[0] / 5 (rcpp…/solvers.cpp:209) */
                          double* mse_mat_out,      /* [n_lambda x max(folds, 1)], lambda-major */
                          double* model_mses_out,   /* [n_lambda], may be NULL */
                          double* thetas_out,       /* [n_lambda x N] the final path, may be NULL */
                          double* fold_thetas_out,  /* [folds x n_lambda x N], may be NULL (tests) */
                          double* rhos_out,         /* [members x n_lambda], may be NULL */
                          int64_t* mesh_index_out,  /* [n], may be NULL */
                          mvtv_admm_stats* stats);  /* [members x n_lambda], may be NULL */

/* ---- operators (inits.D*theta, inits.Dt*v, spcrosses*x, spsolve(spcrosses, b):
 *      rcpp…/solvers.cpp:112-126) ----------------------------------------------------- */
mvtv_status mvtv_apply_D(mvtv_problem* prob, const double* theta, double* d_out);        /* [N] -> [E] */
mvtv_status mvtv_apply_Dt(mvtv_problem* prob, const double* v, double* g_out);           /* [E] -> [N] */
mvtv_status mvtv_apply_A(mvtv_problem* prob, double sigma, const double* x, double* q_out); /* (W + sigma D^T D) x */
mvtv_status mvtv_solve(mvtv_problem* prob, double sigma, const double* b, double* x_inout,
                       double rtol, int32_t max_iter, int32_t* iters, double* relres);
/* lam_max_pinv (rcpp…/utils.cpp:306-355, called by create_lambdas rcpp…/solvers.cpp:186-200):
 * 5 ||D x||_inf with x from the reference's CG on D^T D x = O^T y (relative stop 1e-4, at most
 * min(N, 2000) iterations), its recurrences reproduced step by step on the GPU. */
mvtv_status mvtv_lambda_max(mvtv_problem* prob, double* out, int32_t* iters);
/* lam_max_pinv of variant A (cpp-code/utils.cpp:354-404, called by create_lambdas cpp-code/solvers.cpp:
 * 179-192): ||D x||_inf with x from cg(D^T D, O^T y): x0 = mean(O^T y), absolute stop ||r|| < 0.01, at most
 * 500 iterations (N < 400) or 100 */
mvtv_status mvtv_lambda_max_cpp(mvtv_problem* prob, double* out, int32_t* iters);
/* direct theta-solve (I + sigma D^T D) x = b by cosine transforms (MVTV_SOLVER_SPECTRAL) */
mvtv_status mvtv_solve_spectral(mvtv_problem* prob, double sigma, const double* b, double* x_out);

/* ---- slab decomposition of one mesh over ranks (the metric at 2-8 GPUs) ---------
 * Rank r holds planes [z_begin, z_end) of the last dimension plus one ghost plane below (unless
 * z_begin = 0) and above (unless z_end = m_global); desc->m[p-1] counts owned + ghost planes and
 * desc->oty (and desc->wdiag, if any) cover them (ghost values are not used). Rank r owns planes
 * [floor(m r / G), floor(m (r+1) / G)). mvtv_slab_run is the whole variant-B loop of one rank
 * (rcpp…/solvers.cpp:110-133) with its collectives on a communication stream: the substructured line solves'
 * two all-to-alls of 2 and 2 numbers per line (each block's two recursion sums, then its two carries), halo
 * planes of theta and of the edge state, one 7-value all-reduce per iteration feeding the device-side
 * adapt_step / stopping decision. With W != I (desc->wdiag)
 * the theta-solve is PCG with the spectral preconditioner of mean(W) I + sigma D^T D (opts pcg_rtol,
 * pcg_max_iter, pcg_strict as mvtv_admm_run), distributed: a halo of the search direction per iteration and
 * one all-reduce per dot product; the loop then polls once per ADMM iteration. Supported: variant B, W = I
 * or diagonal, u0 = 0, m_j <= 4096 for j < p - 1; the last dimension any length when G >= 2 (its line solves
 * are substructured over the ranks; each rank's plane count must be 1..64 segments of <= 32 rows, e.g. any
 * count <= 64 or with a divisor in 2..32 giving <= 64 segments: checked on every rank before the first
 * collective, MVTV_BAD_ARG on all of them otherwise), <= 4096 when G = 1. */
typedef struct mvtv_slab_desc {
    int64_t m_global;          /* planes of dim p-1 in the whole mesh */
    int64_t z_begin, z_end;    /* owned planes */
    int32_t ghost_lo, ghost_hi;
} mvtv_slab_desc;
typedef struct mvtv_comm mvtv_comm;
mvtv_status mvtv_problem_create_slab(const mvtv_problem_desc* desc, const mvtv_slab_desc* slab, mvtv_problem** out);
/* RCCL transport (one process per GPU): rank 0 makes the id, every rank passes the same 128 bytes. The first
 * mvtv_slab_run on a communicator with MVTV_RCCL_SPLIT=1 splits off a second RCCL communicator (ncclCommSplit,
 * collective) for the halos, so they can run beside the critical-path collectives issued on the problem's stream; the
 * ranks all-reduce the split's outcome before use and all keep one communicator unless every split succeeded.
 * Without it (the default) every collective goes on the communication stream. */
mvtv_status mvtv_comm_unique_id(uint8_t* id128);
mvtv_status mvtv_comm_create_rccl(const uint8_t* id128, int32_t nranks, int32_t rank, int32_t device, mvtv_comm** out);
/* in-process loopback group of nranks handles (comms[0..nranks-1]): each rank's mvtv_slab_run on its own
 * host thread, transfers as device copies (rehearsal of the decomposition on one GPU) */
mvtv_status mvtv_comm_create_local(int32_t nranks, mvtv_comm** comms);
/* inter-process group over HIP IPC memory (one process per rank; the ranks' devices one GPU or peers of one
 * node): transfers are device-to-device copies out of the sender's buffer (hipIpcOpenMemHandle), ordered through
 * a POSIX shared-memory rendezvous segment `name` ("/..."; rank 0 creates it, every rank passes the same name,
 * it is unlinked once all nranks <= 16 have attached). Host-synchronous inside each collective (no overlap of
 * the z halo): the multi-process path without RCCL, e.g. several ranks on one GPU, where RCCL refuses. Waits give
 * up after MVTV_IPC_TIMEOUT seconds (default 300) or when a peer's loop failed. */
mvtv_status mvtv_comm_create_ipc(const char* name, int32_t nranks, int32_t rank, int32_t device, mvtv_comm** out);
void mvtv_comm_destroy(mvtv_comm* comm);
int32_t mvtv_comm_rank(const mvtv_comm* comm);
int32_t mvtv_comm_size(const mvtv_comm* comm);
/* sum of n <= 64 host doubles over an RCCL or ipc communicator, in place (the global residual all-reduce of
 * independent fits); blocking */
mvtv_status mvtv_comm_allreduce_host(mvtv_comm* comm, double* vals, int32_t n);
/* the file RCCL was resolved from (ROCm's librccl, which shares libmvtv's HIP runtime); "" when RCCL is
 * unavailable */
const char* mvtv_comm_library(void);
/* admm_update B from theta = theta0 on every node, u = 0, rho = rho0 (rcpp…/solvers.cpp:207-209); collective
 * over the communicator. stats hold the global norms; theta of the owned planes: mvtv_state_get (ghosts
 * included, planes as desc->m) */
mvtv_status mvtv_slab_run(mvtv_problem* prob, mvtv_comm* comm, const mvtv_admm_opts* opts, double lambda,
                          double theta0, double rho0, mvtv_admm_stats* stats);
mvtv_status mvtv_sync(mvtv_problem* prob);

/* ---- instrumentation (HIP events on the solver's stream) ---------------------------- */
typedef enum mvtv_kernel_id {
    MVTV_K_EDGE_UPDATE = 0,   /* D theta, soft-threshold, dual update, |r|,|D theta|,|alpha| */
    MVTV_K_GATHER = 1,        /* D^T alpha, D^T u and the dual-residual norms */
    MVTV_K_PCG_INIT = 2,      /* b and r0 = b - A theta */
    MVTV_K_PCG_APPLY = 3,     /* q = A p, p.q */
    MVTV_K_PCG_UPDATE = 4,    /* x += a p, r -= a q, r.z */
    MVTV_K_PCG_DIRECTION = 5, /* p = z + b p */
    MVTV_K_REDUCE = 6,        /* partial-sum finalisation / PCG scalars */
    MVTV_K_OTHER = 7,
    MVTV_K_PCG_FUSED = 8,     /* 3-D fused Chronopoulos-Gear iteration: p, A p, r, A M^-1 r, x in one pass */
    MVTV_K_DCT_FIRST = 9,     /* spectral solve, first pass: b formed on load, DCT along dim 0 */
    MVTV_K_DCT = 10,          /* spectral solve, other passes (DCT / divide / inverse DCT along one dim) */
    MVTV_K_ADMM_FUSED = 11,   /* 3-D: edge update + D^T gather in one pass over the edge state */
    MVTV_K_GATHER4B = 12,     /* 4-D two-pass gather, second pass (the first is MVTV_K_GATHER) */
    MVTV_K_DCT_FOLD = 13,     /* spectral solve, first pass from the folded s (b = oty + s; + D^T u after a rho change) */
    MVTV_K_ADMM_FUSED4 = 14,  /* 4-D: edge update + the gather's first pass in one pass over the edge state */
    MVTV_K_COUNT = 15
} mvtv_kernel_id;
mvtv_status mvtv_timing_enable(mvtv_problem* prob, int32_t on);
mvtv_status mvtv_timing_get(mvtv_problem* prob, int32_t kernel_id, double* total_ms, int64_t* launches,
                            double* bytes_per_launch);
const char* mvtv_kernel_name(int32_t kernel_id);

/* Launch log (tests; off by default, per calling thread). on != 0: clear the log and record the kernel, grid and
 * block of every launch this thread makes from now on (the last 8192 are kept); on == 0: stop and clear.
 * mvtv_launch_log_read writes the log as text, one launch per line in launch order,
 *   "<kernel name with template arguments>\t<grid x y z>\t<block x y z>\n",
 * NUL-terminated and cut to cap bytes, and returns the length of the whole text (call with cap = 0 to size it). */
void mvtv_launch_log_enable(int32_t on);
int64_t mvtv_launch_log_read(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MVTV_MVTV_H */
