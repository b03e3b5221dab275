// mvtv_small_dev.h — the batched small-mesh ADMM loop of one member in one workgroup, as a device function over its
// theta-solve, for k_admm_cos (mvtv_small_cos.hip). The loop, its state and its reductions are those of k_admm_small
// and are described at the top of mvtv_small.hip, which keeps its own copy of the loop in the kernel body: built
// from this function k_admm_small came out 10 VGPRs heavier, and at p = 4 with the 81 stencil coefficients copied to
// scratch (656 B a lane), so the two are kept in step by hand (the helpers here are mvtv_small.hip's, verbatim).
#pragma once
#include "mvtv_device.h"

namespace mvtv {
namespace small {

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

// nodes a thread: 4096 / 1024, 1024 / 256, 256 / 64; 1296 / 1024
template <int P, int NT>
constexpr int kpt() {
    return (P == 4 && NT == 1024) ? 2 : 4;
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

// What a theta-solve sees of its member: the neighbour-read vector sv [N] (holding theta on entry, and again on
// return), the reduction buffers, the member's right-hand-side terms. A solve is called by every thread with
// (ctx, c, rho, x, wv): the thread's nodes' theta in x (in and out) and W in wv; it adds its counts to c and returns
// true when the member must stop (c.status set).
struct SolveCtx {
    double* sv;
    double* sm;
    const double* oty;
    const double* gg;   // [2][N]: D^T alpha, D^T u
    uint32_t N, tid, mb;
};

// the right-hand side b = O^T y + rho (D^T alpha + c D^T u) at node i
__device__ __forceinline__ double small_rhs(const SolveCtx& s, const SmallCtl& c, double rho, uint32_t i) {
    return fma(rho * c.c, s.gg[s.N + i], fma(rho, s.gg[i], s.oty[i]));
}

// The loop of one member. KIND: the member kind this kernel runs (SmallArgs::kind; every member when that is null).
// sv [N], sm [2][NT / 64][3] and zl [nb][N] (ZLDS) are the workgroup's LDS.
template <int P, int NT, bool ZLDS, int KIND, class Solve>
__device__ __forceinline__ void admm_small_loop(const Geom& g, const double* __restrict__ K, const SmallArgs& a, double* const sv,
                                                double* const sm, double* const zl, const Solve& solve) {
    constexpr int KPT = kpt<P, NT>();
    constexpr int NC = 1 << P;
    const uint32_t mb = blockIdx.x, tid = threadIdx.x, N = g.N;
    const int nb = g.nb;
    if (a.kind && a.kind[mb] != KIND) return;   // another kernel's member
    SmallCtl* const cp = a.ctl + mb;
    SmallCtl c = *cp;
    if (c.cur_l == a.li && c.done) return;   // finished members return at once

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
                gg[i] = stencil_small<P>(g, sv, i, cc, K);   // D^T alpha_0 = D^T D theta_0
                gg[N + i] = gu0;
            }
        }
    }

    int flip = 0, nl = 0;
    const SolveCtx sctx{sv, sm, oty, gg, N, tid, mb};
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
        // ---- theta-solve: leaves theta in x and, behind a barrier, in sv ----
        if (solve(g, K, a, sctx, flip, c, rho, x, wv)) {
            c.done = 1;
            break;
        }
        // ---- z-update, dual update (:114-116) ----
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
        if constexpr (Solve::kScalarCtl) {
            // the control block's doubles, computed in vector registers (there is no scalar fp64), back into scalar
            // ones: 16 registers a lane that a solve with more state of its own needs
            c.dual = uni(c.dual), c.primal = uni(c.primal), c.eps_d = uni(c.eps_d), c.eps_p = uni(c.eps_p);
            c.t_z = uni(c.t_z), c.c = uni(c.c), c.rho = uni(c.rho);
        }
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

}  // namespace small
}  // namespace mvtv
