// mvtv_small.hip — batched small-mesh fits: the whole variant-B ADMM loop of one batch member in one workgroup.
//
// k_admm_small<P, NT, ZLDS>: grid = batch members, NT threads each, no workgroup reads another member's data and none
// waits for another. Per ADMM iteration (rcpp-code/MultivarTV/src/solvers.cpp:110-133):
//   b = O^T y + rho (D^T alpha + c D^T u)                       from the node-owned D^T alpha, D^T u of the last gather
//   theta = (W + rho D^T D)^-1 b                                Jacobi-PCG, warm-started, the rule of MVTV_SOLVER_PCG
//   z = D theta - u_old, alpha = soft(z, lambda / rho), r, u    one pass over the member's edge state
//   D^T alpha, D^T u, s = rho D^T (u - u_old)                   one gather per node
//   the five norms, eps, adapt_step, the stopping test          every thread, from the same reduced numbers
// State. A thread owns the nodes tid + q NT (q < KPT) and keeps their theta, PCG residual and direction and W in
// registers; their D^T alpha and D^T u, read and written once an ADMM iteration by the owner alone, stay in the
// member's HBM scratch (where an unfinished member needs them anyway). What neighbours read goes through LDS: one
// vector `sv` [N] (theta for D theta and the first residual, the PCG direction inside the solve) and the edge state
// z [nb][N] in the padded layout of mvtv_kernels.hip (u = -c clamp(z, t_z), alpha = z - clamp(z, t_z)); z stays in the
// member's HBM scratch when nb N exceeds kSmallZLds. Reductions: a shuffle tree in each wave, then a fixed tree over
// the waves' sums in every lane, so each thread holds the same bits and takes the same branches. The two reduction
// buffers alternate: a buffer is rewritten only after the barrier of the next reduction, which every thread reaches
// after its reads of the first.
// A launch runs at most kSmallChunk iterations; theta, z, D^T alpha, D^T u and SmallCtl round-trip through HBM.
#include "mvtv_device.h"

namespace mvtv {

namespace {

// a value every lane holds, moved to scalar registers (branches on it are wave-uniform for the compiler too)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// The same value behind an empty asm: what is derived from it (a node's multi-index, its stencil offsets, its D^T D
// diagonal) is recomputed where it is used instead of being hoisted out of the loops into registers that the
// 128-register budget of a 1024-thread workgroup does not have.
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}

// (D^T D x)_i as stencil_DtD, for p >= 3 one hyperplane of the last dimension at a time: 9 or 27 loads in flight
// instead of 27 or 81, which is what fits beside the node state in 128 registers.
template <int P>
__device__ __forceinline__ double stencil_small(const Geom& g, const double* __restrict__ x, uint32_t i,
                                                const uint32_t (&c)[kMaxDims], const double* __restrict__ K) {
    if constexpr (P <= 2) {
        return stencil_DtD<P>(g, x, i, c, K);
    } else {
        constexpr int L = P - 1;
        constexpr int NL = (P == 3) ? 9 : 27;
        int32_t lo[L], hi[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            lo[j] = c[j] > 0 ? -int32_t(g.stride[j]) : 0;
            hi[j] = c[j] + 1 < g.m[j] ? int32_t(g.stride[j]) : 0;
        }
        const int32_t pl[3] = {c[L] > 0 ? -int32_t(g.stride[L]) : 0, 0, c[L] + 1 < g.m[L] ? int32_t(g.stride[L]) : 0};
        double acc = 0.0;
#pragma unroll 1
        for (int o = 0; o < 3; ++o) {
            const int64_t base = int64_t(i) + (o == 0 ? pl[0] : (o == 1 ? pl[1] : pl[2]));
            const double* __restrict__ Kp = K + o * NL;
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                int32_t off = 0;
                int tt = t;
#pragma unroll
                for (int j = 0; j < L; ++j) {
                    const int oj = tt % 3;
                    tt /= 3;
                    off += (oj == 0) ? lo[j] : (oj == 2 ? hi[j] : 0);
                }
                acc = fma(Kp[t], x[base + off], acc);
            }
        }
        return acc;
    }
}

// Sums v over the workgroup in a fixed order; every thread returns with the same totals.
template <int NR, int NT>
__device__ __forceinline__ void wg_sum(double (&v)[NR], double* __restrict__ sm, int& flip) {
    constexpr int NW = NT / 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NR; ++k) v[k] += __shfl_down(v[k], off, 64);
    }
    double* buf = sm + flip * (NW * 3);
    flip ^= 1;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) buf[wid * 3 + k] = v[k];
    }
    __syncthreads();
    // lane l takes wave (l mod NW)'s sum; an xor butterfly over NW lanes adds the same pairs in every lane
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        double acc = buf[(lane & (NW - 1)) * 3 + k];
#pragma unroll
        for (int off = NW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        v[k] = uni(acc);
    }
}

}  // namespace

template <int P, int NT, bool ZLDS>
__global__ __launch_bounds__(NT) void k_admm_small(Geom g, StencilK sk, SmallArgs a) {
    constexpr int KPT = (P == 4 && NT == 1024) ? 2 : 4;   // nodes a thread: 4096 / 1024, 1024 / 256, 256 / 64; 1296 / 1024
    constexpr int NC = 1 << P;
    constexpr int NW = NT / 64;
    extern __shared__ double lds[];
    const uint32_t mb = blockIdx.x, tid = threadIdx.x, N = g.N;
    const int nb = g.nb;
    SmallCtl* const cp = a.ctl + mb;
    SmallCtl c = *cp;
    if (c.cur_l == a.li && c.done) return;   // finished members return at once

    double* const sv = lds;
    double* const sm = sv + N;
    double* const zl = sm + 2 * NW * 3;
    const double* const oty = a.oty + size_t(mb) * N;
    const double* const wd = a.wdiag ? a.wdiag + size_t(mb) * N : nullptr;
    double* const theta = a.theta + size_t(mb) * N;
    double* const zg = a.z + size_t(mb) * nb * N;
    double* const gg = a.gag + size_t(mb) * 2 * N;
    auto zld = [&](uint32_t e) -> double {
        if constexpr (ZLDS) return zl[e];
        else return zg[e];
    };
    auto zst = [&](uint32_t e, double v) {
        if constexpr (ZLDS) zl[e] = v;
        else zg[e] = v;
    };

    const bool entry = c.cur_l != a.li;   // a new lambda: alpha = D theta, u carried (admm_update :100-101)
    if (entry) {
        c.cur_l = a.li;
        c.done = c.status = c.it = 0;
        c.counter = 1;
        c.pcg_max = c.pcg_unconv = 0;
        c.pcg_iters = 0;
        c.lambda = a.lambdas[size_t(mb) * a.n_lambda + a.li];
        c.dual = c.primal = 1.0;
        c.eps_d = c.eps_p = a.tol;
    }

    double x[KPT], wv[KPT];
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        x[q] = 0.0, wv[q] = 1.0;
        if (i < N) {
            x[q] = theta[i];
            wv[q] = wd ? wd[i] : 1.0;
            sv[i] = x[q];
        }
    }
    if constexpr (ZLDS)
        for (uint32_t e = tid; e < uint32_t(nb) * N; e += NT) zl[e] = zg[e];
    __syncthreads();

    // D^T alpha and D^T u (u unscaled: -clamp(z, t)) at node i from the edge state, as k_gather does
    auto gather = [&](uint32_t i, const uint32_t (&cc)[kMaxDims], double t, double& oa, double& ou) {
        oa = 0.0, ou = 0.0;
        for (int k = 0; k < nb; ++k) {
            const int S = a.sp[k];
            double aa = 0.0, au = 0.0;
#pragma unroll
            for (int T = 0; T < NC; ++T) {
                if ((T & ~S) != 0) continue;
                bool ok = true;
                uint32_t idx = i;
#pragma unroll
                for (int j = 0; j < P; ++j)
                    if ((T >> j) & 1) {
                        ok = ok && (cc[j] > 0);
                        idx -= g.stride[j];
                    }
                const double vv = zld(uint32_t(k) * N + (ok ? idx : i));
                const double v = ok ? vv : 0.0;
                const double cl = clampd(v, t);
                const double al = v - cl;
                if (__builtin_popcount(T) & 1) aa -= al, au += cl;
                else aa += al, au -= cl;
            }
            oa = fma(g.w[k], aa, oa);
            ou = fma(g.w[k], au, ou);
        }
    };

    if (entry) {
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            if (i < N) {
                uint32_t cc[kMaxDims];
                decode<P>(g, i, cc);
                double unused, gu0;
                gather(i, cc, c.t_z, unused, gu0);
                gg[i] = stencil_small<P>(g, sv, i, cc, sk.K);   // D^T alpha_0 = D^T D theta_0
                gg[N + i] = gu0;
            }
        }
    }

    int flip = 0, nl = 0;
    for (;;) {
        // ---- the loop condition, at the top as in the reference (:110) ----
        const bool stop = a.fixed_iters > 0 ? c.it >= a.fixed_iters : !(c.dual > c.eps_d || c.primal > c.eps_p);
        if (uni(int(stop))) {
            c.done = 1;
            break;
        }
        if (nl == kSmallChunk) break;
        ++nl;
        const double rho = c.rho;
        // ---- theta-solve: Jacobi-PCG on W + rho D^T D from the previous theta (sv holds theta) ----
        double r[KPT], pd[KPT], zz[KPT];
        double r3[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            r[q] = pd[q] = zz[q] = 0.0;
            if (i < N) {
                uint32_t cc[kMaxDims];
                decode<P>(g, i, cc);
                const double b = fma(rho * c.c, gg[N + i], fma(rho, gg[i], oty[i]));
                const double ax = fma(rho, stencil_small<P>(g, sv, i, cc, sk.K), wv[q] * x[q]);
                r[q] = b - ax;
                pd[q] = r[q] / fma(rho, jacobi_diag<P, W_NONE>(g, 1.0, nullptr, i, cc), wv[q]);
                r3[PR_B2] = fma(b, b, r3[PR_B2]);
                r3[PR_RZ] = fma(r[q], pd[q], r3[PR_RZ]);
                r3[PR_R2] = fma(r[q], r[q], r3[PR_R2]);
            }
        }
        wg_sum<3, NT>(r3, sm, flip);
        const double b2 = r3[PR_B2];
        double gamma = r3[PR_RZ], r2 = r3[PR_R2];
        int pit = 0;
        bool pdone = (r2 <= a.rtol2 * b2) || a.pcg_maxit <= 0;
        while (!uni(int(pdone))) {   // at most pcg_maxit passes
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                if (i < N) sv[i] = pd[q];
            }
            __syncthreads();
            double qv[KPT];
            double r1[1] = {0.0};
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                qv[q] = 0.0;
                if (i < N) {
                    uint32_t cc[kMaxDims];
                    decode<P>(g, i, cc);
                    qv[q] = fma(rho, stencil_small<P>(g, sv, i, cc, sk.K), wv[q] * pd[q]);
                    r1[0] = fma(pd[q], qv[q], r1[0]);
                }
            }
            wg_sum<1, NT>(r1, sm, flip);
            const double alpha = gamma / r1[0];
            double r2v[2] = {0.0, 0.0};
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                if (i < N) {
                    uint32_t cc[kMaxDims];
                    decode<P>(g, i, cc);
                    x[q] = fma(alpha, pd[q], x[q]);
                    r[q] = fma(-alpha, qv[q], r[q]);
                    zz[q] = r[q] / fma(rho, jacobi_diag<P, W_NONE>(g, 1.0, nullptr, i, cc), wv[q]);
                    r2v[0] = fma(r[q], zz[q], r2v[0]);
                    r2v[1] = fma(r[q], r[q], r2v[1]);
                }
            }
            wg_sum<2, NT>(r2v, sm, flip);
            const double beta = r2v[0] / gamma;
            gamma = r2v[0];
            r2 = r2v[1];
            ++pit;
            pdone = (r2 <= a.rtol2 * b2) || pit >= a.pcg_maxit;
#pragma unroll
            for (int q = 0; q < KPT; ++q) pd[q] = fma(beta, pd[q], zz[q]);
        }
        c.pcg_iters += pit;
        c.pcg_max = pit > c.pcg_max ? pit : c.pcg_max;
        if (pit >= a.pcg_maxit && !(r2 <= a.rtol2 * b2)) {
            c.pcg_unconv += 1;
            if (a.pcg_strict) {
                c.status = 7;   // MVTV_PCG_NOT_CONVERGED
                c.done = 1;
                break;
            }
        }
        // ---- z-update, dual update (:114-116) ----
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            if (i < N) sv[i] = x[q];
        }
        __syncthreads();
        const double t_new = rho != 0.0 ? c.lambda / rho : INFINITY;
        double e3[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            if (i < N) {
                uint32_t cc[kMaxDims];
                decode<P>(g, i, cc);
                double av[NC];
#pragma unroll
                for (int T = 0; T < NC; ++T) {
                    uint32_t idx = i;
#pragma unroll
                    for (int j = 0; j < P; ++j)
                        if ((T >> j) & 1) idx += (cc[j] + 1 < g.m[j]) ? g.stride[j] : 0u;
                    av[T] = sv[idx];
                }
#pragma unroll
                for (int j = 0; j < P; ++j) {
#pragma unroll
                    for (int T = 0; T < NC; ++T)
                        if (!((T >> j) & 1)) av[T | (1 << j)] = av[T] - av[T | (1 << j)];
                }
                for (int k = 0; k < nb; ++k) {
                    const int S = a.sp[k];
                    double ds = 0.0;
#pragma unroll
                    for (int T = 1; T < NC; ++T) ds = (T == S) ? av[T] : ds;
                    const double d = g.w[k] * ds;
                    const uint32_t e = uint32_t(k) * N + i;
                    const double uo = -c.c * clampd(zld(e), c.t_z);
                    const double z = d - uo;
                    const double al = z - clampd(z, t_new);
                    const double rr = al - d;
                    zst(e, z);
                    e3[ER_R2] = fma(rr, rr, e3[ER_R2]);
                    e3[ER_D2] = fma(d, d, e3[ER_D2]);
                    e3[ER_A2] = fma(al, al, e3[ER_A2]);
                }
            }
        }
        wg_sum<3, NT>(e3, sm, flip);   // its barrier also orders the z stores before the gather's loads
        // ---- D^T alpha, D^T u and the dual residual s = rho D^T (u - u_old) (:117-121) ----
        double g2[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            if (i < N) {
                uint32_t cc[kMaxDims];
                decode<P>(g, i, cc);
                double na, nu;
                gather(i, cc, t_new, na, nu);
                const double db = nu - c.c * gg[N + i];
                gg[i] = na, gg[N + i] = nu;
                g2[0] = fma(nu, nu, g2[0]);
                g2[1] = fma(db, db, g2[1]);
            }
        }
        wg_sum<2, NT>(g2, sm, flip);
        // ---- norms, adapt_step (tau 2, mu 10, :77-94), counter (:127-132): as admm_control_step ----
        c.it += 1;
        c.counter += 1;
        c.dual = fabs(rho) * sqrt(g2[1]);
        c.primal = sqrt(e3[ER_R2]);
        c.eps_d = a.tol * (a.sqrtN + sqrt(g2[0]));
        c.eps_p = a.tol * (a.sqrtE + fmax(sqrt(e3[ER_D2]), sqrt(e3[ER_A2])));
        double c_next = 1.0, rho_next = rho;
        if (c.primal > 10 * c.dual) {
            rho_next = 2.0 * rho;
            c_next = 0.5;
        } else if (c.dual > 10 * c.primal) {
            rho_next = 0.5 * rho;
            c_next = 2.0;
        }
        c.t_z = t_new;
        c.c = c_next;
        c.rho = rho_next;
        if (a.fixed_iters <= 0 && c.counter > a.max_counter) {
            c.status = 1;   // MVTV_MAXITER
            c.done = 1;
            break;
        }
    }

    // ---- state back to HBM ----
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        if (i < N) {
            theta[i] = x[q];
            if (c.done && a.thetas_out) a.thetas_out[(size_t(mb) * a.n_lambda + a.li) * N + i] = x[q];
        }
    }
    if constexpr (ZLDS) {
        __syncthreads();
        for (uint32_t e = tid; e < uint32_t(nb) * N; e += NT) zg[e] = zl[e];
    }
    if (tid == 0) {
        *cp = c;
        if (c.done) {
            a.log[size_t(mb) * a.n_lambda + a.li] = c;
            atomicSub(a.remaining + a.li, 1);
        }
    }
}

hipError_t launch_admm_small(const Geom& g, hipStream_t s, int nbatch, const SmallArgs& a) {
    if (!small_ok(g) || nbatch < 1) return hipErrorInvalidValue;
    const StencilK sk = make_stencil(g);
    const int nt = small_nt(g.N);
    const bool zlds = small_zlds(g.nb, g.N);
    const size_t smem = small_lds_bytes(g);
    auto go = [&](auto kern) {
        if (smem > 65536) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, int(smem));
            if (e != hipSuccess) return e;
        }
        klaunch(kern, dim3(uint32_t(nbatch)), dim3(uint32_t(nt)), uint32_t(smem), s, g, sk, a);
        return hipGetLastError();
    };
    // Every (P, NT, ZLDS) the admission and the two rules can reach (nb <= 1, 3, 7, 15 for p = 1..4): z leaves LDS
    // at p = 3 for N > 2048 (2389 with six blocks) and at p = 4 for nb N > 14336, which is N > 955 with fifteen blocks
    // (so also at NT = 256) and every N > 1024. A combination outside the list is refused, never run with the other
    // kernel's LDS size.
    const int key = g.p * 10000 + nt * 2 + (zlds ? 1 : 0);
    switch (key) {
        case 10000 + 64 * 2 + 1: return go(k_admm_small<1, 64, true>);
        case 10000 + 256 * 2 + 1: return go(k_admm_small<1, 256, true>);
        case 10000 + 1024 * 2 + 1: return go(k_admm_small<1, 1024, true>);
        case 20000 + 64 * 2 + 1: return go(k_admm_small<2, 64, true>);
        case 20000 + 256 * 2 + 1: return go(k_admm_small<2, 256, true>);
        case 20000 + 1024 * 2 + 1: return go(k_admm_small<2, 1024, true>);
        case 30000 + 64 * 2 + 1: return go(k_admm_small<3, 64, true>);
        case 30000 + 256 * 2 + 1: return go(k_admm_small<3, 256, true>);
        case 30000 + 1024 * 2 + 1: return go(k_admm_small<3, 1024, true>);
        case 30000 + 1024 * 2 + 0: return go(k_admm_small<3, 1024, false>);
        case 40000 + 64 * 2 + 1: return go(k_admm_small<4, 64, true>);
        case 40000 + 256 * 2 + 1: return go(k_admm_small<4, 256, true>);
        case 40000 + 256 * 2 + 0: return go(k_admm_small<4, 256, false>);
        case 40000 + 1024 * 2 + 0: return go(k_admm_small<4, 1024, false>);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mvtv
