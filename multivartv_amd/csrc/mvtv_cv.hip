// The k-fold CV of a batched small-mesh fit on the device (mvtv_cv_batch): member setup and scoring around the
// loop kernels of mvtv_small.hip / mvtv_small_cos.hip. Member 0 is the final path on all n points, member f + 1 is
// trained on the points whose fold label is not f (mbs_impl, rcpp-code/MultivarTV/src/solvers.cpp:305-376).
//
// Setup. A point's nearest node does not depend on the subset it is in, so k_nearest (mvtv_scatter.hip) runs once
// over all n points. The pairs (node, point position) are sorted by node with one stable radix sort (rocPRIM):
// inside a run of equal nodes the positions ascend, i.e. they stand in data order. k_fold_sums then has the first
// element of every run walk it left to right once per member, skipping the points of the member's own fold: a
// member's O^T y adds the same values in the same order as the reference's sparse product (and numpy's bincount) on
// that member's training subset, bit for bit, as k_run_sums does for one data set. No floating-point atomics.
//
// Scoring. k_cv_mse: one workgroup per (lambda, member) sums (theta[node_i] - y_i)^2 over the member's test points,
// each thread over its points in a fixed strided order, a shuffle tree per wave, a fixed tree over the four waves:
// deterministic, and within (k + 4) 2^-53 relative of the exact mean of the k terms (one rounding for the
// difference, one for the square, at most k - 1 for the sum, one for the division; no fused multiply-add).
//
// Every loop here is bounded by n, N or the member count; no kernel waits for another workgroup.
#include <rocprim/device/device_radix_sort.hpp>

#include "mvtv/mvtv.h"
#include "mvtv_device.h"
#include "mvtv_internal.h"

namespace mvtv {

// pos[i] = i (the sort's values) and every member's constant start theta[b][.] = theta0[b]
__global__ __launch_bounds__(256) void k_cv_fill(uint32_t* __restrict__ pos, int64_t n,
                                                 const double* __restrict__ theta0, double* __restrict__ theta,
                                                 uint32_t N, int64_t members) {
    const int64_t step = int64_t(gridDim.x) * blockDim.x, t0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n; i += step) pos[i] = uint32_t(i);
    for (int64_t i = t0; i < members * int64_t(N); i += step) theta[i] = theta0[i / N];
}

// key, pos: the sorted pairs. Grid (runs' elements, members): the first element of a run of equal keys walks the run
// for member b = blockIdx.y, b + gridDim.y, ...; oty and wdiag [members][N] were zeroed (nodes without a point).
__global__ __launch_bounds__(256) void k_fold_sums(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pos,
                                                   const double* __restrict__ y, const int32_t* __restrict__ fold,
                                                   int64_t n, uint32_t N, int32_t members, double* __restrict__ oty,
                                                   double* __restrict__ wdiag) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        const uint32_t k = key[i];
        if (i > 0 && key[i - 1] == k) continue;
        for (int32_t b = int32_t(blockIdx.y); b < members; b += int32_t(gridDim.y)) {
            double s = 0.0;
            int64_t cnt = 0;
            for (int64_t j = i; j < n && key[j] == k; ++j) {
                const uint32_t q = pos[j];
                if (b > 0 && fold[q] == b - 1) continue;   // the member's own fold is its test set
                s = s + y[q];
                ++cnt;
            }
            oty[size_t(b) * N + k] = s;
            wdiag[size_t(b) * N + k] = double(cnt);
        }
    }
}

// sum over the block of (v, c), thread 0 holds the result: lanes by a shuffle tree, the four waves in a fixed order
__device__ __forceinline__ void cv_block_sum(double& v, unsigned long long& c, double* sv, unsigned long long* sc) {
    for (int off = 32; off > 0; off >>= 1) {
        v = v + __shfl_down(v, off, 64);
        c += __shfl_down(c, off, 64);
    }
    __syncthreads();   // the buffers' previous use
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = v;
        sc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    v = (sv[0] + sv[1]) + (sv[2] + sv[3]);
    c = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// Workgroup blockIdx.x = l * members + b. thetas [members][n_lambda][N]. b >= 1: mse_mat[l][b - 1] over the points
// of fold b - 1 against y. b = 0: model_mses[l] over all points against ref, and with fcols == 1 and members == 1
// (no folds) mse_mat[l][0] over all points against y.
__global__ __launch_bounds__(256) void k_cv_mse(const double* __restrict__ thetas, const int64_t* __restrict__ node,
                                                const double* __restrict__ y, const double* __restrict__ ref,
                                                const int32_t* __restrict__ fold, int64_t n, uint32_t N,
                                                int32_t n_lambda, int32_t members, double* __restrict__ mse_mat,
                                                double* __restrict__ model_mses) {
#pragma clang fp contract(off)
    __shared__ double sv[4];
    __shared__ unsigned long long sc[4];
    const int32_t l = int32_t(blockIdx.x / uint32_t(members)), b = int32_t(blockIdx.x % uint32_t(members));
    const double* th = thetas + (size_t(b) * size_t(n_lambda) + size_t(l)) * N;
    const int32_t fcols = members > 1 ? members - 1 : 1;
    if (b > 0) {
        double acc = 0.0;
        unsigned long long cnt = 0;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
            if (fold[i] != b - 1) continue;
            const double d = th[node[i]] - y[i];
            acc = acc + d * d;
            ++cnt;
        }
        cv_block_sum(acc, cnt, sv, sc);
        if (threadIdx.x == 0) mse_mat[size_t(l) * fcols + (b - 1)] = acc / double(cnt);
        return;
    }
    double acc = 0.0, acc_y = 0.0;
    unsigned long long cnt = 0, cnt_y = 0;
    const bool with_y = members == 1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double t = th[node[i]];
        const double d = t - ref[i];
        acc = acc + d * d;
        ++cnt;
        if (with_y) {
            const double e = t - y[i];
            acc_y = acc_y + e * e;
            ++cnt_y;
        }
    }
    cv_block_sum(acc, cnt, sv, sc);
    if (threadIdx.x == 0) model_mses[l] = acc / double(cnt);
    if (with_y) {
        cv_block_sum(acc_y, cnt_y, sv, sc);
        if (threadIdx.x == 0) mse_mat[l] = acc_y / double(cnt_y);
    }
}

namespace {
unsigned cv_grid_for(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return unsigned(std::max<int64_t>(1, std::min<int64_t>(b, 65536)));
}
unsigned cv_end_bit(uint32_t N) {
    unsigned end_bit = 1;
    while (end_bit < 32 && (uint64_t(1) << end_bit) < uint64_t(N)) ++end_bit;
    return end_bit;
}
}  // namespace

hipError_t cv_sort_temp_bytes(int64_t n, uint32_t N, size_t* bytes) {
    uint32_t *k = nullptr, *v = nullptr;
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, k, k, v, v, size_t(n), 0u, cv_end_bit(N), hipStream_t(nullptr));
}

hipError_t launch_cv_fill(hipStream_t s, uint32_t* pos, int64_t n, const double* theta0, double* theta, uint32_t N,
                          int32_t members) {
    klaunch(k_cv_fill, dim3(cv_grid_for(std::max<int64_t>(n, int64_t(members) * N))), dim3(256), 0, s, pos, n, theta0,
            theta, N, int64_t(members));
    return hipGetLastError();
}

// key, pos (consumed) -> key2, pos2 sorted by key, then oty, wdiag [members][N] (zeroed here)
hipError_t launch_cv_fold_sums(hipStream_t s, uint32_t* key, uint32_t* pos, uint32_t* key2, uint32_t* pos2, void* tmp,
                               size_t tmp_bytes, const double* y, const int32_t* fold, int64_t n, uint32_t N,
                               int32_t members, double* oty, double* wdiag) {
    hipError_t e = hipMemsetAsync(oty, 0, size_t(members) * N * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(wdiag, 0, size_t(members) * N * sizeof(double), s);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(tmp, tmp_bytes, key, key2, pos, pos2, size_t(n), 0u, cv_end_bit(N), s);
    if (e != hipSuccess) return e;
    const dim3 grid(cv_grid_for(n), unsigned(std::min<int32_t>(members, 1024)));
    klaunch(k_fold_sums, grid, dim3(256), 0, s, static_cast<const uint32_t*>(key2), static_cast<const uint32_t*>(pos2), y,
            fold, n, N, members, oty, wdiag);
    return hipGetLastError();
}

hipError_t launch_cv_mse(hipStream_t s, const double* thetas, const int64_t* node, const double* y, const double* ref,
                         const int32_t* fold, int64_t n, uint32_t N, int32_t n_lambda, int32_t members, double* mse_mat,
                         double* model_mses) {
    klaunch(k_cv_mse, dim3(unsigned(n_lambda) * unsigned(members)), dim3(256), 0, s, thetas, node, y, ref, fold, n, N,
            n_lambda, members, mse_mat, model_mses);
    return hipGetLastError();
}

}  // namespace mvtv
