// mvtv_device.h — device helpers shared by the kernel translation units.
#pragma once
#include <type_traits>

#include "mvtv_internal.h"

namespace mvtv {

template <int K, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (K < N) {
        f(std::integral_constant<int, K>{});
        static_for<K + 1, N>(f);
    }
}

__device__ __forceinline__ double clampd(double z, double t) { return fmin(fmax(z, -t), t); }

// Workgroup barrier that orders LDS only: __syncthreads() also waits for every outstanding
// global load (s_waitcnt vmcnt(0)), which would drain a prefetch issued before the barrier.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Wave (64-lane) shuffle reduction, then across the block's waves through LDS. The last NMAX
// slots are max-reductions, the others sums. Thread 0 writes this block's partials.
template <int NR, int NMAX, int NT = kThreads>
__device__ __forceinline__ void block_reduce_store(double (&v)[NR], double* __restrict__ partials) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            double o = __shfl_down(v[k], off, 64);
            v[k] = (k < NR - NMAX) ? v[k] + o : fmax(v[k], o);
        }
    }
    __shared__ double sm[NT / 64][NR];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) sm[wid][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            double acc = sm[0][k];
            for (int w = 1; w < NT / 64; ++w) acc = (k < NR - NMAX) ? acc + sm[w][k] : fmax(acc, sm[w][k]);
            partials[blockIdx.x * NR + k] = acc;
        }
    }
}

// The line solves' multipliers (mvtv_spectral.hip "Multipliers", mvtv_small_cos.hip): t_n = 1 - r^n from t = 1 - r
// alone (t_{a+b} = t_a + t_b - t_a t_b: a few eps relative for any n), and r^n as the pair h + l with h = 1 - t
// rounded and l = (1 - h) - t, exact where h >= 1/2.
__device__ __forceinline__ double tpow(double t, uint32_t n) {   // 1 - r^n from t = 1 - r
    double y = 0.0, x = t;
    while (n) {
        if (n & 1u) y = fma(-y, x, y + x);
        x = fma(-x, x, x + x);
        n >>= 1;
    }
    return y;
}
struct Mul2 {
    double h, l;
};
__device__ __forceinline__ Mul2 mul2_from_t(double t) {
    const double h = 1.0 - t;
    return {h, h >= 0.5 ? (1.0 - h) - t : 0.0};
}
__device__ __forceinline__ double mul2_mac(Mul2 m, double acc, double f) { return fma(m.h, acc, fma(m.l, acc, f)); }
__device__ __forceinline__ Mul2 mul2_mul(Mul2 a, Mul2 b) {
    const double h = a.h * b.h;
    return {h, fma(a.h, b.h, -h) + fma(a.h, b.l, a.l * b.h)};
}

// 3^p stencil coefficients of D^T D (mvtv_kernels.hip make_stencil), passed to kernels by value
struct StencilK {
    double K[81];
};
StencilK make_stencil(const Geom& g);

// Jacobi diagonal of W + sigma * sum_S cS[S] (x)_{j in S} L_j at a node with multi-index c:
// the 1-D Neumann Laplacian's diagonal is (c > 0) + (c < m - 1).
template <int P, int WM>
__device__ __forceinline__ double jacobi_diag(const Geom& g, double sigma, const double* __restrict__ wdiag,
                                              uint32_t i, const uint32_t (&c)[kMaxDims]) {
    double l[P];
#pragma unroll
    for (int j = 0; j < P; ++j) l[j] = double(c[j] > 0) + double(c[j] + 1 < g.m[j]);
    double acc = 0.0;
#pragma unroll
    for (int S = 1; S < (1 << P); ++S) {
        double prod = g.cS[S];
#pragma unroll
        for (int j = 0; j < P; ++j)
            if ((S >> j) & 1) prod *= l[j];
        acc += prod;
    }
    double wv = (WM == W_DIAG) ? wdiag[i] : (WM == W_IDENTITY ? 1.0 : 0.0);
    return wv + sigma * acc;
}

// K-weighted 3^P-point stencil with per-dimension clamped neighbours: (D^T D x)_i.
template <int P>
__device__ __forceinline__ double stencil_DtD(const Geom& g, const double* __restrict__ x, uint32_t i,
                                              const uint32_t (&c)[kMaxDims], const double* __restrict__ K) {
    int32_t lo[P], hi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        lo[j] = c[j] > 0 ? -int32_t(g.stride[j]) : 0;
        hi[j] = c[j] + 1 < g.m[j] ? int32_t(g.stride[j]) : 0;
    }
    double acc = 0.0;
    constexpr int NT = (P == 1) ? 3 : (P == 2) ? 9 : (P == 3) ? 27 : 81;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int32_t off = 0;
        int tt = t;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int o = tt % 3;
            tt /= 3;
            off += (o == 0) ? lo[j] : (o == 2 ? hi[j] : 0);
        }
        acc = fma(K[t], x[int64_t(i) + off], acc);
    }
    return acc;
}

}  // namespace mvtv
