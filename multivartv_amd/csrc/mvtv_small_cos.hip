// mvtv_small_cos.hip — the cosine theta-solve of the batched small-mesh fits, inside the member's workgroup.
//
// cos_solve<P, NT>: (shift I + sigma D^T D) x = f in place on a vector in LDS, every thread of the workgroup calling.
// D^T D = sum_S cS[S] (x)_{j in S} L_j, so after cosine transforms along every dimension but one (the line dimension,
// the longest) each line of that dimension is a tridiagonal system c0 I + c1 L with c0 = shift + sigma a(k'),
// c1 = sigma b(k'); a and b per line come from the host (long double, rounded), rho changes inside the kernel.
//   Transforms. A thread owns the nodes tid + q NT as in the loop. Along dimension j it forms its nodes' transformed
//   values as dense products with the orthonormal DCT-II matrix C_j (<= 64 x 64, in LDS at an odd row pitch: thread k
//   reads row k in the forward product and column n in the inverse one, both free of bank conflicts along dimension 0,
//   and a broadcast along the others), holds them over a barrier and stores them.
//   Line solve. A line gets tpl threads (a power of two), thread s of them the rows [s sl, (s + 1) sl) (the last
//   segments shorter or empty). The factorised operator of DESIGN.md §4.1: both first-order recursions over the
//   segment from zero, the segments' sums combined by a weighted scan over the line's threads (shuffles in a wave,
//   the waves' pairs through LDS where a line spans several), the mirror closure on the totals, and the rerun from
//   the carries: the backward recursion leaves B_i in place, the forward one emits (B_i + r F_{i-1}) / D. r and 1 - r
//   by the cancellation-free formulas, every multiplier a pair h + l (mvtv_device.h Mul2).
// Every loop is bounded by the mesh or by pcg_maxit; no workgroup waits for another; no floating-point atomics.
//
// k_solve_cos<P, NT>: the solve alone, one member a workgroup (mvtv_solve_batch).
// k_admm_cos<P, NT, ZLDS, PC>: the loop of k_admm_small (mvtv_small_dev.h) with this theta-solve. PC = false: theta =
// cos_solve(b) with shift 1, sigma rho, exact for W = I. PC = true: PCG on W + rho D^T D by the rule of
// MVTV_SOLVER_PCG, preconditioned by M^-1 = S A0^-1 S, A0 = mean(W) I + rho D^T D, S = I unless
// std(W) >= 0.1 (mean(W) + rho cmean), then S = diag(sqrt(dbar / d)), d the Jacobi diagonal (pcgs_solve); S is
// recomputed where it is used, which keeps the kernel inside 128 registers at NT = 1024.
#include "mvtv_small_dev.h"

namespace mvtv {

namespace {

using small::kpt;
using small::opaque;
using small::uni;
using small::wg_sum;

// what a thread keeps of its line segment for the whole kernel
struct CosSeg {
    uint32_t base;   // its first row's node
    int rows;        // 0: no rows (an empty segment, or a thread beyond the last line)
    double la, lb;   // the line's a, b
};

__device__ __forceinline__ CosSeg cos_seg(const CosPlan& cp, uint32_t lm, uint32_t lstride) {
    const uint32_t tid = threadIdx.x;
    const uint32_t line = tid / uint32_t(cp.tpl), seg = tid & uint32_t(cp.tpl - 1);
    CosSeg s{0u, 0, 0.0, 0.0};
    if (line < cp.nlines) {
        const uint32_t r0 = seg * uint32_t(cp.sl);
        const uint32_t hi = line / lstride, lo = line - hi * lstride;
        s.rows = r0 < lm ? int(min(uint32_t(cp.sl), lm - r0)) : 0;
        s.base = lo + hi * lstride * lm + r0 * lstride;
        s.la = cp.ab[line];
        s.lb = cp.ab[cp.nlines + line];
    }
    return s;
}

// Exclusive weighted scan over each line's tpl threads in order (REV: from the line's last thread down): v the
// thread's sum from a zero carry, p its multiplier r^rows; (ev, ep) what the line's threads before it make of a zero
// carry and their multiplier, tv the line's total. sc: [3][NT / 64] of LDS. Every thread of the workgroup calls it.
template <int NT, bool REV>
__device__ __forceinline__ void seg_scan(double v, Mul2 p, int tpl, double* sc, double& ev, Mul2& ep, double& tv) {
    constexpr int NW = NT / 64;
    const int lane = int(threadIdx.x) & 63;
    const int gl = tpl < 64 ? tpl : 64;   // the line's threads in this wave
    const int pos = lane & (gl - 1);
    auto from = [&](double x, int off) { return REV ? __shfl_down(x, off, 64) : __shfl_up(x, off, 64); };
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        if (off < gl) {   // workgroup-uniform
            const double lv = from(v, off);
            const Mul2 lp{from(p.h, off), from(p.l, off)};
            if (REV ? pos + off < gl : pos >= off) {
                v = mul2_mac(p, lv, v);
                p = mul2_mul(p, lp);
            }
        }
    }
    double xv = from(v, 1);
    Mul2 xp{from(p.h, 1), from(p.l, 1)};
    if (pos == (REV ? gl - 1 : 0)) {
        xv = 0.0;
        xp = Mul2{1.0, 0.0};
    }
    if (NW == 1 || tpl <= 64) {
        ev = xv;
        ep = xp;
        tv = __shfl(v, REV ? (lane & ~(gl - 1)) : (lane | (gl - 1)), 64);
    } else {
        const int w = int(threadIdx.x) >> 6, nwl = tpl >> 6, w0 = w & ~(nwl - 1);
        if (lane == (REV ? 0 : 63)) {
            sc[w] = v;
            sc[NW + w] = p.h;
            sc[2 * NW + w] = p.l;
        }
        __syncthreads();
        double wv = 0.0;
        Mul2 wp{1.0, 0.0}, tp{1.0, 0.0};
        tv = 0.0;
        for (int k = 0; k < nwl; ++k) {   // nwl <= NW
            const int kk = REV ? w0 + nwl - 1 - k : w0 + k;
            if (kk == w) {
                wv = tv;
                wp = tp;
            }
            const Mul2 pk{sc[NW + kk], sc[2 * NW + kk]};
            tv = mul2_mac(pk, tv, sc[kk]);
            tp = mul2_mul(tp, pk);
        }
        ev = mul2_mac(xp, wv, xv);
        ep = mul2_mul(wp, xp);
        __syncthreads();
    }
}

// the dense transform along dimension J of the thread's nodes: forward (INV = false) out_k = sum_n C[k][n] v_n,
// inverse out_n = sum_k C[k][n] v_k
template <int P, int NT, int J, bool INV>
__device__ __forceinline__ void cos_dim(const Geom& g, const CosPlan& cp, double* __restrict__ sv,
                                        const double* __restrict__ tl) {
    constexpr int KPT = kpt<P, NT>();
    const uint32_t tid = threadIdx.x, N = g.N, mj = g.m[J], st = g.stride[J], pitch = cp.pitch[J];
    const double* __restrict__ T = tl + cp.toff[J];
    double out[KPT];
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        out[q] = 0.0;
        if (i < N) {
            uint32_t cc[kMaxDims];
            decode<P>(g, i, cc);
            const uint32_t cj = cc[J], base = i - cj * st;
            double acc = 0.0;
#pragma unroll 4
            for (uint32_t n = 0; n < mj; ++n)
                acc = fma(INV ? T[n * pitch + cj] : T[cj * pitch + n], sv[base + n * st], acc);
            out[q] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        if (i < N) sv[i] = out[q];
    }
    __syncthreads();
}

// (shift I + sigma D^T D) x = f in place on sv [N]; the caller's stores of f need no barrier of their own, and sv is
// readable by every thread on return. sc: [3][NT / 64]; tl: the tables in LDS. shift > 0, sigma >= 0.
template <int P, int NT>
__device__ __forceinline__ void cos_solve(const Geom& g, const CosPlan& cp, const CosSeg& cs, uint32_t lm,
                                          uint32_t lstride, double shift, double sigma, double* __restrict__ sv,
                                          double* sc, const double* __restrict__ tl) {
    __syncthreads();
    static_for<0, P>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if (J != cp.ld) cos_dim<P, NT, J, false>(g, cp, sv, tl);
    });
    {
        const double c0 = fma(sigma, cs.la, shift), c1 = sigma * cs.lb;
        const double D = sqrt(c0 * fma(4.0, c1, c0));
        const double den = 1.0 / (fma(2.0, c1, c0) + D);
        const double t1 = (c0 + D) * den;   // 1 - r, r = 2 c1 den
        const Mul2 r = mul2_from_t(t1);
        double* const row = sv + cs.base;
        double fl = 0.0, bl = 0.0;
#pragma unroll 2
        for (int i = 0; i < cs.rows; ++i) {
            fl = mul2_mac(r, fl, row[uint32_t(i) * lstride]);
            bl = mul2_mac(r, bl, row[uint32_t(cs.rows - 1 - i) * lstride]);
        }
        const Mul2 pr = mul2_from_t(tpow(t1, uint32_t(cs.rows)));   // r^rows, 1 for no rows
        double fin = 0.0, bin = 0.0;
        if (cp.tpl > 1) {   // workgroup-uniform
            double fev, ftv, bev, btv;
            Mul2 fep, bep;
            seg_scan<NT, false>(fl, pr, cp.tpl, sc, fev, fep, ftv);
            seg_scan<NT, true>(bl, pr, cp.tpl, sc, bev, bep, btv);
            const double tm = tpow(t1, lm), pm = 1.0 - tm, idet = 1.0 / (tm * (2.0 - tm));   // r^m, 1 / (1 - r^2m)
            fin = mul2_mac(fep, fma(pm, ftv, btv) * idet, fev);
            bin = mul2_mac(bep, fma(pm, btv, ftv) * idet, bev);
        } else {
            const double tm = tpow(t1, lm), pm = 1.0 - tm, idet = 1.0 / (tm * (2.0 - tm));
            fin = fma(pm, fl, bl) * idet;
            bin = fma(pm, bl, fl) * idet;
        }
        // a thread touches its own rows only: B_i in place, then x_i = (B_i + r F_{i-1}) / D, F_i = B_i + r (F_{i-1} - B_{i+1})
        double bv = bin;
#pragma unroll 2
        for (int i = cs.rows - 1; i >= 0; --i) {
            bv = mul2_mac(r, bv, row[uint32_t(i) * lstride]);
            row[uint32_t(i) * lstride] = bv;
        }
        const double sd = 1.0 / D;
        double fv = fin, gi = cs.rows > 0 ? row[0] : 0.0;
#pragma unroll 2
        for (int i = 0; i < cs.rows; ++i) {
            const double gn = i + 1 < cs.rows ? row[uint32_t(i + 1) * lstride] : bin;
            row[uint32_t(i) * lstride] = sd * mul2_mac(r, fv, gi);
            fv = mul2_mac(r, fv - gn, gi);
            gi = gn;
        }
    }
    __syncthreads();
    static_for<0, P>([&](auto jc) {
        constexpr int J = P - 1 - decltype(jc)::value;
        if (J != cp.ld) cos_dim<P, NT, J, true>(g, cp, sv, tl);
    });
}

// the tables into LDS (visible after the next barrier)
template <int NT>
__device__ __forceinline__ void cos_tables(const CosPlan& cp, double* __restrict__ tl) {
    for (uint32_t e = threadIdx.x; e < cp.tab_words; e += NT) tl[e] = cp.tab[e];
}

// theta = (I + rho D^T D)^-1 b: the exact solve of a W = I member; no PCG iteration is counted
template <int P, int NT>
struct CosExact {
    static constexpr int KPT = kpt<P, NT>();
    static constexpr bool kScalarCtl = true;
    const CosPlan& cp;
    const CosSeg& cs;
    uint32_t lm, lstride;
    double* sc;
    const double* tl;
    __device__ __forceinline__ bool operator()(const Geom& g, const double*, const SmallArgs&,
                                               const small::SolveCtx& s, int&, SmallCtl& c, double rho,
                                               double (&x)[KPT], const double (&)[KPT]) const {
        __syncthreads();   // the last neighbour reads of theta in sv (the entry's stencil)
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(s.tid + q * NT);
            if (i < s.N) s.sv[i] = small::small_rhs(s, c, rho, i);
        }
        cos_solve<P, NT>(g, cp, cs, lm, lstride, 1.0, rho, s.sv, sc, tl);
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(s.tid + q * NT);
            if (i < s.N) x[q] = s.sv[i];
        }
        return false;
    }
};

// PCG on W + rho D^T D from the previous theta with the cosine preconditioner, the rule of MVTV_SOLVER_PCG
template <int P, int NT>
struct CosPcg {
    static constexpr int KPT = kpt<P, NT>();
    static constexpr bool kScalarCtl = true;
    const CosPlan& cp;
    const CosSeg& cs;
    uint32_t lm, lstride;
    double* sc;
    const double* tl;
    double cmean;   // mean over the mesh of D^T D's diagonal
    __device__ __forceinline__ bool operator()(const Geom& g, const double* __restrict__ K, const SmallArgs& a,
                                               const small::SolveCtx& s, int& flip, SmallCtl& c, double rho,
                                               double (&x)[KPT], const double (&)[KPT]) const {
        // The thread's W and theta are not held in registers over the solve: W is read again where it is used and
        // theta moves through the member's theta array in HBM (its owner alone touches it), which is what keeps
        // r, the direction and the cosine solve inside 128 registers at NT = 1024.
        double* const sv = s.sv;
        const uint32_t tid = s.tid, N = s.N;
        const double wmean = a.wstat ? a.wstat[2 * s.mb] : 1.0, wstd = a.wstat ? a.wstat[2 * s.mb + 1] : 0.0;
        const double w0 = wmean > 0.0 ? wmean : 1.0;
        const double* const wd = a.wdiag ? a.wdiag + size_t(s.mb) * N : nullptr;
        double* const xg = a.theta + size_t(s.mb) * N;
        auto wat = [&](uint32_t i) -> double { return wd ? wd[i] : 1.0; };
        const double dbar = uni(fma(rho, cmean, w0));
        const bool scaled = wstd >= 0.1 * dbar;   // the same for every thread
        // 1 / s at node i: sqrt(dbar / d_i), d the Jacobi diagonal
        auto sinv = [&](uint32_t i, double w) -> double {
            if (!scaled) return 1.0;
            uint32_t cc[kMaxDims];
            decode<P>(g, i, cc);
            return sqrt(dbar / fma(rho, jacobi_diag<P, W_NONE>(g, 1.0, nullptr, i, cc), w));
        };
        double r[KPT], pd[KPT];
        double r2v[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            r[q] = pd[q] = 0.0;
            if (i < N) {
                uint32_t cc[kMaxDims];
                decode<P>(g, i, cc);
                const double b = small::small_rhs(s, c, rho, i);
                const double ax = fma(rho, small::stencil_small<P>(g, sv, i, cc, K), wat(i) * x[q]);
                r[q] = b - ax;
                xg[i] = x[q];
                r2v[0] = fma(b, b, r2v[0]);
                r2v[1] = fma(r[q], r[q], r2v[1]);
            }
        }
        wg_sum<2, NT>(r2v, s.sm, flip);
        const double b2 = r2v[0];
        double r2 = r2v[1], gamma = 0.0;
        int pit = 0;
        bool pdone = (r2 <= a.rtol2 * b2) || a.pcg_maxit <= 0;
        // z = M^-1 r = S A0^-1 S r, and r.z
        auto precond = [&](double (&zz)[KPT]) -> double {
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                if (i < N) sv[i] = sinv(i, wat(i)) * r[q];
            }
            cos_solve<P, NT>(g, cp, cs, lm, lstride, w0, rho, sv, sc, tl);
            double rz[1] = {0.0};
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                zz[q] = 0.0;
                if (i < N) {
                    zz[q] = sinv(i, wat(i)) * sv[i];
                    rz[0] = fma(r[q], zz[q], rz[0]);
                }
            }
            wg_sum<1, NT>(rz, s.sm, flip);
            return rz[0];
        };
        if (!uni(int(pdone))) gamma = precond(pd);
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
                    qv[q] = fma(rho, small::stencil_small<P>(g, sv, i, cc, K), wat(i) * pd[q]);
                    r1[0] = fma(pd[q], qv[q], r1[0]);
                }
            }
            wg_sum<1, NT>(r1, s.sm, flip);
            const double alpha = uni(gamma / r1[0]);
            double rr[1] = {0.0};
#pragma unroll
            for (int q = 0; q < KPT; ++q) {
                const uint32_t i = opaque(tid + q * NT);
                if (i < N) {
                    xg[i] = fma(alpha, pd[q], xg[i]);
                    r[q] = fma(-alpha, qv[q], r[q]);
                    rr[0] = fma(r[q], r[q], rr[0]);
                }
            }
            wg_sum<1, NT>(rr, s.sm, flip);
            r2 = rr[0];
            ++pit;
            pdone = (r2 <= a.rtol2 * b2) || pit >= a.pcg_maxit;
            if (uni(int(pdone))) break;
            double zz[KPT];
            const double rz = precond(zz);
            const double beta = uni(rz / gamma);
            gamma = rz;
#pragma unroll
            for (int q = 0; q < KPT; ++q) pd[q] = fma(beta, pd[q], zz[q]);
        }
        c.pcg_iters += pit;
        c.pcg_max = pit > c.pcg_max ? pit : c.pcg_max;
        if (pit >= a.pcg_maxit && !(r2 <= a.rtol2 * b2)) {
            c.pcg_unconv += 1;
            if (a.pcg_strict) {
                c.status = 7;   // MVTV_PCG_NOT_CONVERGED
                return true;
            }
        }
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const uint32_t i = opaque(tid + q * NT);
            if (i < N) {
                x[q] = xg[i];
                sv[i] = x[q];
            }
        }
        __syncthreads();
        return false;
    }
};

}  // namespace

template <int P, int NT, bool ZLDS, bool PC>
__global__ __launch_bounds__(NT) void k_admm_cos(Geom g, StencilK sk, SmallArgs a, CosPlan cp, uint32_t lm,
                                                 uint32_t lstride, double cmean) {
    constexpr int NW = NT / 64;
    extern __shared__ double lds[];
    if (a.kind && a.kind[blockIdx.x] != (PC ? SMALL_KIND_COS_PCG : SMALL_KIND_COS)) return;
    double* const sv = lds;
    double* const sm = sv + g.N;
    double* const sc = sm + 2 * NW * 3;
    double* const tl = sc + 3 * NW;
    double* const zl = tl + cp.tab_words;
    cos_tables<NT>(cp, tl);   // visible after the loop's first barrier
    const CosSeg cs = cos_seg(cp, lm, lstride);
    if constexpr (PC)
        small::admm_small_loop<P, NT, ZLDS, SMALL_KIND_COS_PCG>(g, sk.K, a, sv, sm, zl,
                                                               CosPcg<P, NT>{cp, cs, lm, lstride, sc, tl, cmean});
    else
        small::admm_small_loop<P, NT, ZLDS, SMALL_KIND_COS>(g, sk.K, a, sv, sm, zl,
                                                           CosExact<P, NT>{cp, cs, lm, lstride, sc, tl});
}

template <int P, int NT>
__global__ __launch_bounds__(NT) void k_solve_cos(Geom g, CosPlan cp, uint32_t lm, uint32_t lstride,
                                                  const double* __restrict__ sigma, const double* __restrict__ shift,
                                                  const double* __restrict__ f, double* __restrict__ x) {
    constexpr int NW = NT / 64;
    constexpr int KPT = kpt<P, NT>();
    extern __shared__ double lds[];
    double* const sv = lds;
    double* const sc = sv + g.N + 2 * NW * 3;
    double* const tl = sc + 3 * NW;
    const uint32_t mb = blockIdx.x, tid = threadIdx.x, N = g.N;
    cos_tables<NT>(cp, tl);
    const CosSeg cs = cos_seg(cp, lm, lstride);
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        if (i < N) sv[i] = f[size_t(mb) * N + i];
    }
    cos_solve<P, NT>(g, cp, cs, lm, lstride, shift ? shift[mb] : 1.0, sigma[mb], sv, sc, tl);
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const uint32_t i = opaque(tid + q * NT);
        if (i < N) x[size_t(mb) * N + i] = sv[i];
    }
}

bool small_cos_shape(const Geom& g, CosPlan* cp) {
    if (!small_ok(g) || g.p < 1 || g.p > kMaxDims) return false;
    int ld = 0;
    for (int j = 1; j < g.p; ++j)
        if (g.m[j] >= g.m[ld]) ld = j;   // the longest; ties: the last
    const uint32_t nt = uint32_t(small_nt(g.N)), nlines = g.N / g.m[ld];
    if (nlines > nt) return false;   // cannot happen under small_ok: nlines <= N^(1 - 1/p) <= NT
    CosPlan c;
    c.ld = ld;
    c.nlines = nlines;
    uint32_t tpl = 1;
    while (tpl * 2 * nlines <= nt) tpl *= 2;
    c.tpl = int32_t(tpl);
    c.sl = int32_t((g.m[ld] + tpl - 1) / tpl);
    uint32_t off = 0;
    for (int j = 0; j < g.p; ++j) {
        if (j == ld) continue;
        if (g.m[j] > kSmallCosMaxT) return false;   // cannot happen either: (second longest)^2 <= N
        c.toff[j] = off;
        c.pitch[j] = g.m[j] | 1u;
        off += g.m[j] * c.pitch[j];
    }
    c.tab_words = off;
    *cp = c;
    return true;
}

namespace {
// mean over the mesh of D^T D's diagonal: sum_S cS[S] prod_{j in S} mean(l_j), l_j = 1 at the ends, 2 inside
double cos_cmean(const Geom& g) {
    double cmean = 0.0;
    for (int S = 1; S < (1 << g.p); ++S) {
        double prod = g.cS[S];
        for (int j = 0; j < g.p; ++j)
            if ((S >> j) & 1) prod *= 2.0 * double(g.m[j] - 1) / double(g.m[j]);
        cmean += prod;
    }
    return cmean;
}

template <class K>
hipError_t cos_attr(K kern, size_t smem) {
    if (smem > 160u * 1024u) return hipErrorInvalidValue;
    if (smem <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(smem));
}
}  // namespace

hipError_t launch_admm_cos(const Geom& g, const CosPlan& cp, hipStream_t s, int nbatch, const SmallArgs& a, bool pc) {
    if (!small_ok(g) || nbatch < 1 || cp.ld < 0 || !cp.ab || (cp.tab_words && !cp.tab)) return hipErrorInvalidValue;
    const StencilK sk = make_stencil(g);
    const int nt = small_nt(g.N);
    const bool zlds = small_cos_zlds(g.nb, g.N);
    const size_t smem = small_cos_lds_bytes(g, cp, true);
    const uint32_t lm = g.m[cp.ld], lstride = g.stride[cp.ld];
    const double cmean = cos_cmean(g);
    auto go = [&](auto kern) {
        const hipError_t e = cos_attr(kern, smem);
        if (e != hipSuccess) return e;
        klaunch(kern, dim3(uint32_t(nbatch)), dim3(uint32_t(nt)), uint32_t(smem), s, g, sk, a, cp, lm, lstride, cmean);
        return hipGetLastError();
    };
    // Every (P, NT, ZLDS) the admission and small_cos_zlds can reach (nb <= 1, 3, 7, 15 for p = 1..4): z leaves LDS at
    // p = 2 for N > 3754 with three blocks, at p = 3 for N > 1609 with seven, at p = 4 for N > 750 with fifteen (so
    // also at NT = 256) and every N > 1024.
    const int key = g.p * 10000 + nt * 2 + (zlds ? 1 : 0);
#define MVTV_COS_GO(P_, NT_, Z_) \
    case P_ * 10000 + NT_ * 2 + (Z_ ? 1 : 0): return pc ? go(k_admm_cos<P_, NT_, Z_, true>) : go(k_admm_cos<P_, NT_, Z_, false>)
    switch (key) {
        MVTV_COS_GO(1, 64, true);
        MVTV_COS_GO(1, 256, true);
        MVTV_COS_GO(1, 1024, true);
        MVTV_COS_GO(2, 64, true);
        MVTV_COS_GO(2, 256, true);
        MVTV_COS_GO(2, 1024, true);
        MVTV_COS_GO(2, 1024, false);
        MVTV_COS_GO(3, 64, true);
        MVTV_COS_GO(3, 256, true);
        MVTV_COS_GO(3, 1024, true);
        MVTV_COS_GO(3, 1024, false);
        MVTV_COS_GO(4, 64, true);
        MVTV_COS_GO(4, 256, true);
        MVTV_COS_GO(4, 256, false);
        MVTV_COS_GO(4, 1024, false);
        default: return hipErrorInvalidValue;
    }
#undef MVTV_COS_GO
}

hipError_t launch_solve_cos(const Geom& g, const CosPlan& cp, hipStream_t s, int nbatch, const double* sigma,
                            const double* shift, const double* f, double* x) {
    if (!small_ok(g) || nbatch < 1 || cp.ld < 0 || !cp.ab || (cp.tab_words && !cp.tab)) return hipErrorInvalidValue;
    const int nt = small_nt(g.N);
    const size_t smem = small_cos_lds_bytes(g, cp, false);
    const uint32_t lm = g.m[cp.ld], lstride = g.stride[cp.ld];
    auto go = [&](auto kern) {
        const hipError_t e = cos_attr(kern, smem);
        if (e != hipSuccess) return e;
        klaunch(kern, dim3(uint32_t(nbatch)), dim3(uint32_t(nt)), uint32_t(smem), s, g, cp, lm, lstride, sigma, shift, f,
                x);
        return hipGetLastError();
    };
    switch (g.p * 10000 + nt) {
        case 10000 + 64: return go(k_solve_cos<1, 64>);
        case 10000 + 256: return go(k_solve_cos<1, 256>);
        case 10000 + 1024: return go(k_solve_cos<1, 1024>);
        case 20000 + 64: return go(k_solve_cos<2, 64>);
        case 20000 + 256: return go(k_solve_cos<2, 256>);
        case 20000 + 1024: return go(k_solve_cos<2, 1024>);
        case 30000 + 64: return go(k_solve_cos<3, 64>);
        case 30000 + 256: return go(k_solve_cos<3, 256>);
        case 30000 + 1024: return go(k_solve_cos<3, 1024>);
        case 40000 + 64: return go(k_solve_cos<4, 64>);
        case 40000 + 256: return go(k_solve_cos<4, 256>);
        case 40000 + 1024: return go(k_solve_cos<4, 1024>);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mvtv
