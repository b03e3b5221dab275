// mvtv_capi.cpp — the C ABI declared in include/mvtv/mvtv.h, apart from the ADMM loop (mvtv_admm.cpp) and the slab
// loop (mvtv_slab.cpp): problem set-up, the theta-solves, operators, batch calls, instrumentation.
//
// One mvtv_problem = one GPU, one HIP stream, all vectors resident in HBM; every vector operation is a kernel
// from the .hip files. The PCG theta-solve keeps its scalars on the device and is polled every few iterations.
#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <complex>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mvtv/mvtv.h"
#include "mvtv_internal.h"
#include "mvtv_problem.h"

using namespace mvtv;

namespace mvtv {
thread_local std::string g_last_error;
}  // namespace mvtv

namespace {

int popcount(int x) { return __builtin_popcount(unsigned(x)); }

// Readable name of a kernel from its host function pointer (the launch log): the runtime's registered device symbol,
// else the host stub's own symbol, demangled and cut down to the name with its template arguments, e.g.
// "k_trir<10, 32, 32>" from "void mvtv::k_trir<10, 32, 32>(double*, ...)".
std::string kernel_display_name(const void* fn) {
    const char* sym = hipKernelNameRefByPtr(fn, nullptr);
    Dl_info info;
    if (!sym || !*sym) {
        (void)hipGetLastError();   // the failed lookup's error only: a pending launch error stays for its caller
        if (dladdr(fn, &info) && info.dli_sname) sym = info.dli_sname;
    }
    if (!sym || !*sym) {
        char p[32];
        std::snprintf(p, sizeof p, "%p", fn);
        return p;
    }
    int status = 0;
    char* dem = abi::__cxa_demangle(sym, nullptr, nullptr, &status);
    std::string s = (status == 0 && dem) ? dem : sym;
    std::free(dem);
    // the parameter list starts at the first '(' outside template brackets; the name at the last space before it
    int depth = 0;
    size_t start = 0, end = s.size();
    for (size_t i = 0; i < s.size(); ++i) {
        const char c = s[i];
        if (c == '<') ++depth;
        else if (c == '>') --depth;
        else if (depth == 0 && c == ' ') start = i + 1;
        else if (depth == 0 && c == '(' && s.compare(i, 21, "(anonymous namespace)") == 0) i += 20;
        else if (depth == 0 && c == '(') { end = i; break; }
    }
    s = s.substr(start, end - start);
    for (const char* prefix : {"mvtv::", "__device_stub__"})
        if (s.compare(0, std::strlen(prefix), prefix) == 0) s.erase(0, std::strlen(prefix));
    return s;
}

void free_all(mvtv_problem* P) {
    double** bufs[] = {&P->oty, &P->wdiag, &P->theta, &P->edges, &P->ga, &P->gu, &P->guprev, &P->r,
                       &P->p, &P->q, &P->thold, &P->p2, &P->partials, &P->red, &P->stage, &P->slab_iface,
                       &P->edges2, &P->pcg_b, &P->g4, &P->pcg_s, &P->pcg_t, &P->ls_coef, &P->ls_lr};
    for (double** b : bufs)
        if (*b) {
            (void)hipFree(*b);
            *b = nullptr;
        }
    if (P->batch_buf) (void)hipFree(P->batch_buf);
    P->batch_buf = nullptr;
    P->batch_cap = 0;
    if (P->cos.tab) (void)hipFree(const_cast<double*>(P->cos.tab));
    if (P->cos.ab) (void)hipFree(const_cast<double*>(P->cos.ab));
    P->cos = CosPlan{};
    if (P->st) (void)hipFree(P->st);
    if (P->ctl) (void)hipFree(P->ctl);
    if (P->host_ctl) (void)hipHostFree(P->host_ctl);
    for (double* t : {P->spec.tw, P->spec.twq, P->spec.lam, P->spec.blu, P->spec.lb_coef, P->spec.lb_lr, P->spec.stw,
                      P->spec.sscr})
        if (t) (void)hipFree(t);
    if (P->spec.perm) (void)hipFree(P->spec.perm);
    if (P->spec.srev) (void)hipFree(P->spec.srev);
    P->spec = SpecPlan{};
    if (P->host_red) (void)hipHostFree(P->host_red);
    for (auto& pd : P->pending) {
        (void)hipEventDestroy(pd.a);
        (void)hipEventDestroy(pd.b);
    }
    for (auto e : P->ev_pool) (void)hipEventDestroy(e);
    if (P->stream) (void)hipStreamDestroy(P->stream);
    if (P->comm_stream) (void)hipStreamDestroy(P->comm_stream);
}

}  // namespace
// (namespace mvtv, here and below: declared in mvtv_problem.h for the ADMM loop of mvtv_admm.cpp)
namespace mvtv {
double variant_tol(const mvtv_admm_opts& o) {
    if (o.tol > 0) return o.tol;
    return o.variant == MVTV_VARIANT_RCPP ? 1e-4 : 1e-3;
}
int variant_maxc(const mvtv_admm_opts& o) {
    if (o.max_counter > 0) return o.max_counter;
    return o.variant == MVTV_VARIANT_RCPP ? 3000 : (o.variant == MVTV_VARIANT_CPP ? 2000 : 1000000);
}
}  // namespace mvtv
namespace {

// Copy a compact [E] edge vector (reference block layout) into the padded device layout.
mvtv_status import_edges(mvtv_problem* P, const double* host_u, double* padded) {
    HIP_TRY(hipMemsetAsync(padded, 0, size_t(P->g.nb) * P->g.N * sizeof(double), P->stream));
    if (!P->stage) {
        P->stage_n = std::min<size_t>(size_t(P->E), size_t(1) << 24);
        MVTV_TRY(alloc(&P->stage, P->stage_n));
    }
    uint64_t off = 0;
    for (int k = 0; k < P->g.nb; ++k) {
        for (uint64_t e0 = 0; e0 < P->blk_len[k]; e0 += P->stage_n) {
            const uint64_t cnt = std::min<uint64_t>(P->stage_n, P->blk_len[k] - e0);
            HIP_TRY(hipMemcpyAsync(P->stage, host_u + off + e0, cnt * sizeof(double), hipMemcpyHostToDevice, P->stream));
            HIP_TRY(launch_edges_import(P->g, P->order, P->stream, k, e0, cnt, P->stage, padded));
        }
        off += P->blk_len[k];
    }
    HIP_TRY(hipStreamSynchronize(P->stream));
    return MVTV_OK;
}

mvtv_status export_edges(mvtv_problem* P, const double* padded, double* host_u, int umode, double t, double c) {
    if (!P->stage) {
        P->stage_n = std::min<size_t>(size_t(P->E), size_t(1) << 24);
        MVTV_TRY(alloc(&P->stage, P->stage_n));
    }
    uint64_t off = 0;
    for (int k = 0; k < P->g.nb; ++k) {
        for (uint64_t e0 = 0; e0 < P->blk_len[k]; e0 += P->stage_n) {
            const uint64_t cnt = std::min<uint64_t>(P->stage_n, P->blk_len[k] - e0);
            HIP_TRY(launch_edges_export(P->g, P->order, P->stream, k, e0, cnt, padded, P->stage, umode, t, c));
            HIP_TRY(hipMemcpyAsync(host_u + off + e0, P->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, P->stream));
            HIP_TRY(hipStreamSynchronize(P->stream));
        }
        off += P->blk_len[k];
    }
    return MVTV_OK;
}

// PCG iterations enqueued before the first poll: the last solve's count plus this (probe: MVTV_PCG_AHEAD).
// Config 4's work item (2048^2 fold, one stream): -2 327, 0 335, +2 326, +4 325 ADMM it/s on one box
// (profiles/r03/v5_cv_tuning)
int pcg_ahead() {
    static const int v = [] {
        const char* e = probe_env("MVTV_PCG_AHEAD");
        return e ? std::atoi(e) : 0;
    }();
    return v;
}
}  // namespace

namespace mvtv {
// Solve (W + sigma D^T D) x = b, b = oty + ca*ga + cb*gb, by Jacobi-PCG warm-started at x.
mvtv_status pcg_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                      const double* gb, double cb, double* x, double rtol, int maxit, int* iters, double* relres) {
    const Launch L = P->L();
    const double* w = P->wdiag;
    const bool fused = P->g.p == 3 && P->fused3d && P->wmode != W_NONE;
    // fused 3-D: r and p ping-pong between two buffers (a launch reads neighbour halos of r_i and
    // p_{i-1} that their owning workgroups overwrite, so outputs must not alias inputs)
    if (fused && !P->p2) MVTV_TRY(alloc(&P->p2, P->g.N));
    double* rb[2] = {P->r, P->q};
    double* pb[2] = {P->p, P->p2};
    int nb = 0;
    int h = P->tstart(MVTV_K_PCG_INIT);
    if (fused)
        HIP_TRY(launch_cg3d(P->g, P->stream, 0, sigma, P->wmode, w, x, nullptr, nullptr, rb[0], nullptr, oty, ga, ca,
                            gb, cb, P->st, P->partials, &nb));
    else
        HIP_TRY(launch_pcg_init(P->g, L, sigma, P->wmode, w, oty, ga, ca, gb, cb, x, P->r, P->p, P->partials));
    P->tstop(h);
    h = P->tstart(MVTV_K_REDUCE);
    if (fused)
        HIP_TRY(launch_finalize(P->stream, P->partials, nb, 4, 0, 4, nullptr, P->st, rtol * rtol, maxit));
    else
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, PR_N, 0, 1, nullptr, P->st, rtol * rtol, maxit));
    P->tstop(h);

    // one PCG iteration; kernels enqueued after convergence return at once (device done flag)
    auto enqueue = [&](int j) -> mvtv_status {
        if (fused) {
            int hh = P->tstart(MVTV_K_PCG_FUSED);
            // x moves in odd iterations only (both steps, k_cg3d); k_cg_xflush applies an even last one's
            HIP_TRY(launch_cg3d(P->g, P->stream, j == 0 ? 1 : ((j & 1) ? 3 : 2), sigma, P->wmode, w, x, rb[j & 1],
                                pb[j & 1], rb[(j + 1) & 1], pb[(j + 1) & 1], oty, ga, ca, gb, cb, P->st, P->partials,
                                &nb));
            P->tstop(hh);
            hh = P->tstart(MVTV_K_REDUCE);
            HIP_TRY(launch_finalize(P->stream, P->partials, nb, 4, 0, 5, nullptr, P->st));
            P->tstop(hh);
            return MVTV_OK;
        }
        int hh = P->tstart(MVTV_K_PCG_APPLY);
        HIP_TRY(launch_apply_A(P->g, L, sigma, P->wmode, w, P->p, P->q, P->partials, P->st));
        P->tstop(hh);
        hh = P->tstart(MVTV_K_REDUCE);
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 0, 2, nullptr, P->st));
        P->tstop(hh);
        hh = P->tstart(MVTV_K_PCG_UPDATE);
        HIP_TRY(launch_pcg_update(P->g, L, sigma, P->wmode, w, x, P->r, P->p, P->q, P->st, P->partials));
        P->tstop(hh);
        hh = P->tstart(MVTV_K_REDUCE);
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 2, 0, 3, nullptr, P->st));
        P->tstop(hh);
        hh = P->tstart(MVTV_K_PCG_DIRECTION);
        HIP_TRY(launch_pcg_pupdate(P->g, L, sigma, P->wmode, w, P->r, P->p, P->st));
        P->tstop(hh);
        return MVTV_OK;
    };
    // Poll schedule: the previous solve's count predicts this one (warm starts change it slowly),
    // so the first poll comes just before it and later polls every 2 iterations.
    std::vector<size_t> mark;   // first timing entry of each enqueued iteration
    int enq = 0;
    int batch = P->pcg_hint > 0 ? std::max(2, P->pcg_hint + pcg_ahead()) : kPcgPoll;
    for (;;) {
        for (int b = 0; b < batch && enq < maxit; ++b, ++enq) {
            mark.push_back(P->pending.size());
            MVTV_TRY(enqueue(enq));
        }
        HIP_TRY(hipMemcpyAsync(P->host_st, P->st, sizeof(PcgState), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        const int done_iters = P->host_st->iter;
        if (P->timing && done_iters < int(mark.size()))   // launches past convergence did no work
            for (size_t e = mark[size_t(done_iters)]; e < P->pending.size(); ++e) P->pending[e].kid = -1;
        P->harvest();
        if (P->host_st->done || enq >= maxit) break;
        batch = 2;
    }
    if (fused) {   // an even last iteration's x step (p_i of an even i is in pb[1])
        h = P->tstart(MVTV_K_OTHER);
        HIP_TRY(launch_cg_xflush(P->stream, P->g.N, x, pb[1], P->st));
        P->tstop(h);
        if (P->timing) P->pcg_xmoves += P->host_st->iter / 2;
    }
    *iters = P->host_st->iter;
    P->pcg_hint = *iters;
    *relres = P->host_st->bnorm2 > 0 ? std::sqrt(P->host_st->rnorm2 / P->host_st->bnorm2) : 0.0;
    return MVTV_OK;
}

bool spectral_ok(const mvtv_problem* P) { return P->spec_mesh && P->wmode == W_IDENTITY; }
}  // namespace mvtv

namespace {
// M = 2^ceil(log2(2m - 1)): the circular convolution length of Bluestein's identity for length m
uint32_t bluestein_length(uint32_t m) {
    uint32_t M = 1;
    while (M < 2 * m - 1) M <<= 1;
    return M;
}

// In-place radix-2 DFT (sign -1, unnormalised) in long double: the convolution kernels' transforms, once per
// problem (twiddles from exact angles 2 pi (k mod M) / M)
void fft_ld(std::vector<std::complex<long double>>& x) {
    const size_t M = x.size();
    const long double pi = 3.141592653589793238462643383279502884L;
    for (size_t i = 1, j = 0; i < M; ++i) {
        size_t bit = M >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(x[i], x[j]);
    }
    for (size_t len = 2; len <= M; len <<= 1) {
        for (size_t i = 0; i < M; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const long double ang = -2.0L * pi * (long double)(k * (M / len)) / (long double)M;
                const std::complex<long double> w(cosl(ang), sinl(ang));
                const std::complex<long double> u = x[i + k], v = x[i + k + len / 2] * w;
                x[i + k] = u + v;
                x[i + k + len / 2] = u - v;
            }
    }
}

// Bluestein tables of one dimension (SpecPlan::blu layout): chirp c[n] = e^{-i pi n^2/m} (n^2 mod 2m exactly), the
// transforms / M of the kernels b_f[j] = conj c[|j|] (forward DFT, s = -1) and b_i[j] = c[|j|] (inverse, s = +1)
// wrapped to length M, and the length-M twiddles e^{-2 pi i k/M}, k < M
void bluestein_tables(uint32_t m, uint32_t M, std::vector<double>& out) {
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<std::complex<long double>> c(m), bf(M, 0.0L), bi(M, 0.0L);
    for (uint32_t n = 0; n < m; ++n) {
        const uint64_t r = (uint64_t(n) * n) % (2 * uint64_t(m));
        const long double ang = -pi * (long double)r / (long double)m;
        c[n] = std::complex<long double>(cosl(ang), sinl(ang));
    }
    for (uint32_t j = 0; j < m; ++j) {
        bf[j] = std::conj(c[j]);
        bi[j] = c[j];
        if (j > 0) {
            bf[M - j] = std::conj(c[j]);
            bi[M - j] = c[j];
        }
    }
    fft_ld(bf);
    fft_ld(bi);
    for (uint32_t n = 0; n < m; ++n) {
        out.push_back(double(c[n].real()));
        out.push_back(double(c[n].imag()));
    }
    for (auto* v : {&bf, &bi})
        for (uint32_t k = 0; k < M; ++k) {
            out.push_back(double((*v)[k].real() / (long double)M));
            out.push_back(double((*v)[k].imag() / (long double)M));
        }
    for (uint32_t k = 0; k < M; ++k) {   // (k_dctb8's radix-8 stages read k < M)
        const long double ang = -2.0L * pi * (long double)k / (long double)M;
        out.push_back(double(cosl(ang)));
        out.push_back(double(sinl(ang)));
    }
}

// Device tables of the spectral solve. Twiddles and eigenvalues are evaluated in long double.
mvtv_status spectral_plan(mvtv_problem* P) {
    std::vector<double> tw, twq, lam;
    std::vector<uint32_t> perm;
    SpecPlan& sp = P->spec;
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int j = 0; j < P->g.p; ++j) {
        const uint32_t m = (P->slab && j == P->g.p - 1) ? uint32_t(P->m_global) : P->g.m[j];
        sp.tw_off[j] = uint32_t(tw.size());
        sp.twq_off[j] = uint32_t(twq.size());
        sp.lam_off[j] = uint32_t(lam.size());
        sp.perm_off[j] = uint32_t(perm.size());
        // a last dimension longer than 4096 is never transformed (the blocked line solve reads no table of it)
        if (P->spec_long && j == P->g.p - 1) continue;
        // a leading dimension longer than 4096 takes the two-pass transform (dct_split_setup: its tables, and this
        // dimension's eigenvalues in its frequency order): no length-m twiddle table
        if (m > kSplitMax) {
            lam.resize(lam.size() + m, 0.0);
            continue;
        }
        for (uint32_t k = 0; k < m; ++k) {
            const long double a = -2.0L * pi * k / m;
            tw.push_back(double(cosl(a)));
            tw.push_back(double(sinl(a)));
        }
        for (uint32_t k = 0; k < m; ++k) {
            const long double a = -pi * k / (2.0L * m);
            twq.push_back(double(cosl(a)));
            twq.push_back(double(sinl(a)));
            const long double sn = sinl(pi * k / (2.0L * m));
            lam.push_back(double(4.0L * sn * sn));
        }
        // k_dctg's input order: sample k goes to Makhoul position n (x[2n], x[2(m-1-n)+1]) at its
        // digit-reversed place for the radix plan (n = sum of digits d_s, most significant first in
        // stage order reversed; position = sum d_s prod_{u<s} rad[u])
        int rad[8], nrad = 0;
        const bool planned = dct_radix_plan(m, rad, &nrad);
        for (uint32_t k = 0; k < m; ++k) {
            uint32_t n = (k & 1u) ? m - 1u - (k >> 1) : (k >> 1), pos = 0;
            if (planned) {
                for (int st = nrad - 1; st >= 0; --st) {
                    uint32_t mul = 1;
                    for (int u = 0; u < st; ++u) mul *= uint32_t(rad[u]);
                    pos += (n % uint32_t(rad[st])) * mul;
                    n /= uint32_t(rad[st]);
                }
            }
            perm.push_back(pos);
        }
    }
    // Bluestein tables of the lengths without a 2-3-5-7 plan (k_dctb8; mvtv_spectral.hip)
    std::vector<double> blu;
    for (int j = 0; j < P->g.p; ++j) {
        const uint32_t m = (P->slab && j == P->g.p - 1) ? uint32_t(P->m_global) : P->g.m[j];
        int rad[8], nrad = 0;
        sp.blu_M[j] = 0;
        if (m > 4096 || dct_radix_plan(m, rad, &nrad)) continue;
        const uint32_t M = bluestein_length(m);
        sp.blu_M[j] = M;
        sp.blu_off[j] = uint32_t(blu.size());
        bluestein_tables(m, M, blu);
    }
    auto up = [&](double** dst, const std::vector<double>& v) -> mvtv_status {
        MVTV_TRY(alloc(dst, v.size()));
        HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
        return MVTV_OK;
    };
    if (!blu.empty()) MVTV_TRY(up(&sp.blu, blu));
    if (tw.empty()) {   // only long dimensions (p = 1 with a long line: no table at all): the passes still take the pointers
        tw.assign(2, 0.0);
        twq.assign(2, 0.0);
        perm.assign(1, 0u);
    }
    if (lam.empty()) lam.assign(1, 0.0);
    MVTV_TRY(up(&sp.tw, tw));
    MVTV_TRY(up(&sp.twq, twq));
    MVTV_TRY(up(&sp.lam, lam));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&sp.perm), perm.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(sp.perm, perm.data(), perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return MVTV_OK;
}

// The marching line sweeps of a 3-D solve (mvtv_spectral.hip k_sweep): which problems take them, with how many chunks
// over dim 2, and their scratch. mode -1: the gate (not a slab rank, N > 2^24 nodes, a grid of >= one workgroup per CU
// with chunks of >= 8 planes); 1: wherever the shape has an instantiation; 0: off. chunks 0: the cost model's count.
mvtv_status line_sweep_setup(mvtv_problem* P, int mode, int chunks) {
    if (mode < -1 || mode > 1 || chunks < 0 || chunks > kLineSweepMaxChunks)
        return fail(MVTV_BAD_ARG, "line_sweep: mode in {-1, 0, 1}, 0 <= chunks <= 64");
    int C = 0;
    if (mode != 0 && !P->slab && P->spec_mesh && !P->spec_long && line_sweep_shape_ok(P->g)) {
        if (mode == 1) {
            if (chunks > int(P->g.m[2])) return fail(MVTV_BAD_ARG, "line_sweep: more chunks than planes");
            C = chunks > 0 ? chunks : line_sweep_chunks(P->g, false);
        } else if (uint64_t(P->g.N) > (uint64_t(1) << 24)) {
            C = line_sweep_chunks(P->g, true);
        }
    }
    HIP_TRY(hipStreamSynchronize(P->stream));   // no launch may still read the scratch
    if (C > P->ls_cap) {
        for (double** b : {&P->ls_coef, &P->ls_lr})
            if (*b) {
                (void)hipFree(*b);
                *b = nullptr;
            }
        P->ls_cap = 0;
        P->ls_chunks = 0;
        const size_t words = 2 * size_t(C) * P->g.m[0] * P->g.m[1];
        MVTV_TRY(alloc(&P->ls_coef, words));
        MVTV_TRY(alloc(&P->ls_lr, words));
        P->ls_cap = C;
    }
    P->ls_mode = mode;
    P->ls_chunks = C;
    return MVTV_OK;
}

// The blocked line solve along the last dimension (mvtv_spectral.hip k_trib / k_tri1): blocks 0: only where the last
// dimension is longer than 4096, with the library's block count; >= 2: that many blocks at any length. The blocks'
// pairs and carries live in the plan, allocated here when the solve is in use.
mvtv_status line_blocks_setup(mvtv_problem* P, int blocks) {
    if (P->slab || !P->spec_mesh)
        return fail(MVTV_BAD_ARG, "line_blocks: not a slab rank, and every m_j, j < p - 1, <= 4096 or a product of two 2-3-5-7-smooth factors <= 4096");
    const uint32_t mlast = P->g.m[P->g.p - 1];
    if (blocks < 0 || blocks == 1 || uint32_t(blocks) > mlast)
        return fail(MVTV_BAD_ARG, "line_blocks: 0 or 2 <= blocks <= m_last");
    LineBlocks lb;
    if ((blocks > 0 || P->spec_long) && !line_blocks_plan(P->g, blocks, &lb))
        return fail(MVTV_BAD_ARG, "line_blocks: a block of the last dimension does not fit a workgroup's segments");
    HIP_TRY(hipStreamSynchronize(P->stream));   // no launch may still read the scratch
    SpecPlan& sp = P->spec;
    const size_t words = 2 * size_t(lb.nblk) * size_t(P->g.N / mlast);
    if (words > sp.lb_cap) {
        for (double** b : {&sp.lb_coef, &sp.lb_lr})
            if (*b) {
                (void)hipFree(*b);
                *b = nullptr;
            }
        sp.lb_cap = 0;
        sp.lb = LineBlocks{};
        MVTV_TRY(alloc(&sp.lb_coef, words));
        MVTV_TRY(alloc(&sp.lb_lr, words));
        sp.lb_cap = words;
    }
    sp.lb = lb;   // (forced blocks on a line-sweep mesh: the five-pass solve while they are on, sweeps_on)
    return MVTV_OK;
}

// DFT of any 2-3-5-7-smooth length (sign -1, unnormalised) in long double, decimation in time over the smallest prime
// first; w: the M twiddles e^{-2 pi i k/M} from exact angles. out and in do not overlap.
void fft_smooth_ld(const std::complex<long double>* in, size_t stride, size_t n, std::complex<long double>* out,
                   const std::vector<std::complex<long double>>& w) {
    if (n == 1) {
        out[0] = in[0];
        return;
    }
    const size_t M = w.size();
    size_t r = 7;
    for (size_t q : {2, 3, 5})
        if (n % q == 0) {
            r = q;
            break;
        }
    const size_t sub = n / r;
    for (size_t q = 0; q < r; ++q) fft_smooth_ld(in + q * stride, stride * r, sub, out + q * sub, w);
    std::complex<long double> t[7];
    for (size_t k = 0; k < sub; ++k) {
        for (size_t q = 0; q < r; ++q) t[q] = out[q * sub + k] * w[(q * k * (M / n)) % M];
        for (size_t pp = 0; pp < r; ++pp) {
            std::complex<long double> acc = t[0];
            for (size_t q = 1; q < r; ++q) acc += t[q] * w[((q * pp) % r) * (M / r)];
            out[k + pp * sub] = acc;
        }
    }
}

// Tables of one chirp dimension, appended to tw at dc's offsets: the chirp c[n] = e^{-i pi n^2/m} (n^2 mod 2m exactly),
// the quarter wave e^{-i pi k/2m}, and H = FFT_M(h) / M of h[j] = conj c[|j|] wrapped to M = a b, stored where the
// row pass meets frequency k1 + a k2: position b k1 + k2. h is symmetric, so the inverse transform (taken as the
// conjugate of a forward one) reads the same H.
void chirp_tables(uint32_t m, uint32_t a, uint32_t b, DctChirp* dc, std::vector<double>& tw) {
    const long double pi = 3.141592653589793238462643383279502884L;
    const size_t M = size_t(a) * b;
    std::vector<std::complex<long double>> c(m), h(M, 0.0L), Hh(M), w(M);
    for (uint32_t n = 0; n < m; ++n) {
        const uint64_t r = (uint64_t(n) * n) % (2 * uint64_t(m));
        const long double ang = -pi * (long double)r / (long double)m;
        c[n] = std::complex<long double>(cosl(ang), sinl(ang));
    }
    for (size_t k = 0; k < M; ++k) {
        const long double ang = -2.0L * pi * (long double)k / (long double)M;
        w[k] = std::complex<long double>(cosl(ang), sinl(ang));
    }
    for (uint32_t j = 0; j < m; ++j) {
        h[j] = std::conj(c[j]);
        if (j > 0) h[M - j] = std::conj(c[j]);
    }
    fft_smooth_ld(h.data(), 1, M, Hh.data(), w);
    dc->chirp = uint32_t(tw.size());
    for (uint32_t n = 0; n < m; ++n) {
        tw.push_back(double(c[n].real()));
        tw.push_back(double(c[n].imag()));
    }
    dc->qw = uint32_t(tw.size());
    for (uint32_t k = 0; k < m; ++k) {
        const long double ang = -pi * k / (2.0L * m);
        tw.push_back(double(cosl(ang)));
        tw.push_back(double(sinl(ang)));
    }
    dc->H = uint32_t(tw.size());
    for (uint32_t k1 = 0; k1 < a; ++k1)
        for (uint32_t k2 = 0; k2 < b; ++k2) {
            const std::complex<long double> v = Hh[k1 + size_t(a) * k2] / (long double)M;
            tw.push_back(double(v.real()));
            tw.push_back(double(v.imag()));
        }
}

// a factor of a split: 2 <= n <= 4096 with a 2-3-5-7 plan
bool split_factor_ok(uint32_t n) {
    int rad[8], nrad = 0;
    return n >= 2 && n <= kSplitMax && dct_radix_plan(n, rad, &nrad);
}

// The two-pass cosine transforms of the leading dimensions (mvtv_spectral.hip k_dsc / k_dsr): dimension j takes
// m_j = a (m_j / a) with a = split_forced[j], or the library's factorisation where m_j > 4096. (Re)builds the splits'
// tables (evaluated in long double) and their scratch, and stores lam_j of every leading dimension in the order its
// forward pass leaves the frequencies: position b k1 + k2 holds k = k1 + a k2 (the natural order without a split).
mvtv_status dct_split_setup(mvtv_problem* P) {
    SpecPlan& sp = P->spec;
    const int p = P->g.p;
    const long double pi = 3.141592653589793238462643383279502884L;
    HIP_TRY(hipStreamSynchronize(P->stream));   // no launch may still read the tables or the scratch
    if (sp.stw) (void)hipFree(sp.stw);
    if (sp.srev) (void)hipFree(sp.srev);
    sp.stw = nullptr;
    sp.srev = nullptr;
    std::vector<double> tw;
    std::vector<uint32_t> rev;
    size_t scratch = 0;
    auto fft_tables = [&](uint32_t n, uint32_t* tw_off, uint32_t* rev_off) {
        *tw_off = uint32_t(tw.size());
        *rev_off = uint32_t(rev.size());
        int rad[8], nrad = 0;
        (void)dct_radix_plan(n, rad, &nrad);
        for (uint32_t k = 0; k < n; ++k) {
            const long double ang = -2.0L * pi * k / n;
            tw.push_back(double(cosl(ang)));
            tw.push_back(double(sinl(ang)));
            uint32_t r = k, pos = 0;   // digit-reversed place of sample k (spectral_plan's rule)
            for (int st = nrad - 1; st >= 0; --st) {
                uint32_t mul = 1;
                for (int u = 0; u < st; ++u) mul *= uint32_t(rad[u]);
                pos += (r % uint32_t(rad[st])) * mul;
                r /= uint32_t(rad[st]);
            }
            rev.push_back(pos);
        }
    };
    auto hilo = [&](uint64_t J, uint64_t M4) {   // e^{-2 pi i J / M4} as (re, im) hi then lo
        const long double ang = -2.0L * pi * (long double)(J % M4) / (long double)M4;
        const long double c = cosl(ang), sn = sinl(ang);
        const double ch = double(c), sh = double(sn);
        tw.push_back(ch);
        tw.push_back(sh);
        tw.push_back(double(c - (long double)ch));
        tw.push_back(double(sn - (long double)sh));
    };
    for (int j = 0; j < p - 1; ++j) {
        const uint32_t m = P->g.m[j];
        DctSplit& ds = sp.split[j];
        ds = DctSplit{};
        DctChirp& dc = sp.chirp[j];
        dc = DctChirp{};
        if (P->chirp_forced[j][0] != 0) {   // the chirp-z transform: natural frequency order, its own tables
            std::vector<double> lam(m);
            for (uint32_t k = 0; k < m; ++k) {
                const long double sn = sinl(pi * k / (2.0L * m));
                lam[k] = double(4.0L * sn * sn);
            }
            HIP_TRY(hipMemcpy(sp.lam + sp.lam_off[j], lam.data(), size_t(m) * sizeof(double), hipMemcpyHostToDevice));
            uint32_t ca = uint32_t(P->chirp_forced[j][0]), cb = uint32_t(P->chirp_forced[j][1]);
            if (P->chirp_forced[j][0] < 0 && !dct_chirp_auto(m, &ca, &cb))
                return fail(MVTV_BAD_ARG, "dct_chirp: no convolution length");
            dc.a = ca;
            dc.b = cb;
            const uint64_t M = uint64_t(ca) * cb;
            fft_tables(dc.a, &dc.twa, &dc.reva);
            fft_tables(dc.b, &dc.twb, &dc.revb);
            dc.t1 = uint32_t(tw.size());
            for (uint64_t i = 0; i * 4096 < M; ++i) hilo(i * 4096, M);
            dc.t2 = uint32_t(tw.size());
            for (uint64_t i = 0; i < 4096; ++i) hilo(i, M);
            chirp_tables(m, ca, cb, &dc, tw);
            scratch = std::max(scratch, 2 * ((size_t(P->g.N / m) + 1) / 2) * size_t(M));
            continue;
        }
        const uint32_t a = P->split_forced[j] ? uint32_t(P->split_forced[j]) : (m > kSplitMax ? dct_split_auto(m) : 0u);
        if (m > kSplitMax && a == 0) return fail(MVTV_BAD_ARG, "dct_split: no factorisation");
        std::vector<double> lam(m);
        for (uint32_t pos = 0; pos < m; ++pos) {
            const uint32_t k = a ? pos / (m / a) + a * (pos % (m / a)) : pos;
            const long double sn = sinl(pi * k / (2.0L * m));
            lam[pos] = double(4.0L * sn * sn);
        }
        HIP_TRY(hipMemcpy(sp.lam + sp.lam_off[j], lam.data(), size_t(m) * sizeof(double), hipMemcpyHostToDevice));
        if (a == 0) continue;
        ds.a = a;
        ds.b = m / a;
        fft_tables(ds.a, &ds.twa, &ds.reva);
        fft_tables(ds.b, &ds.twb, &ds.revb);
        const uint64_t M4 = 4 * uint64_t(m);
        ds.t1 = uint32_t(tw.size());
        for (uint64_t i = 0; i * 4096 < M4; ++i) hilo(i * 4096, M4);
        ds.t2 = uint32_t(tw.size());
        for (uint64_t i = 0; i < 4096; ++i) hilo(i, M4);
        const size_t nlines = P->g.N / m;
        scratch = std::max(scratch, 2 * ((nlines + 1) / 2) * size_t(m));
    }
    if (scratch > sp.sscr_cap || scratch == 0) {
        if (sp.sscr) (void)hipFree(sp.sscr);
        sp.sscr = nullptr;
        sp.sscr_cap = 0;
        if (scratch) {
            MVTV_TRY(alloc(&sp.sscr, scratch));
            sp.sscr_cap = scratch;
        }
    }
    if (tw.empty()) return MVTV_OK;
    MVTV_TRY(alloc(&sp.stw, tw.size()));
    HIP_TRY(hipMemcpy(sp.stw, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&sp.srev), rev.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(sp.srev, rev.data(), rev.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return MVTV_OK;
}

// a leading dimension runs in two passes (or the chirp transform's three): the passes that hold a whole line of it in
// one workgroup rest
}  // namespace
bool mvtv::split_on(const mvtv_problem* P) {
    for (int j = 0; j < P->g.p - 1; ++j)
        if (P->spec.split[j].a > 0 || P->spec.chirp[j].a > 0) return true;
    return false;
}
namespace {

// Which meshes the spectral solve takes. Cosine transforms of any length <= 4096: FFT plans for 2-3-5-7 lengths,
// Bluestein (k_dctb8) for the rest; a longer leading dimension with a factorisation a * b, both 2-3-5-7-smooth and
// <= 4096, in two passes, and any leading dimension under mvtv_problem_dct_chirp (dct_split_setup). The last dimension
// is never transformed: on one GPU it may have any length (spec_long: the blocked line solve); a slab rank keeps the
// old rule for every dimension (its loop has the substructured solve over the ranks)
void spectral_gate(mvtv_problem* P) {
    const int p = P->g.p;
    P->spec_mesh = P->spec_pow2 = P->spec_lead = true;
    P->spec_long = false;
    for (int j = 0; j < p; ++j) {
        const uint32_t mj = (P->slab && j == p - 1) ? uint32_t(P->m_global) : P->g.m[j];
        if (mj > 4096) {
            const bool split = j < p - 1 && !P->slab && (P->chirp_forced[j][0] != 0 || dct_split_auto(mj) != 0);
            if (j < p - 1 && !split) P->spec_lead = false;
            if (j == p - 1 && !P->slab) P->spec_long = true;
            else if (!split) P->spec_mesh = false;
        }
        if ((mj & (mj - 1)) != 0) P->spec_pow2 = false;
    }
    if (!P->spec_mesh) P->spec_long = false;
    if (!P->spec_mesh || P->spec_long) P->spec_pow2 = false;
}

// Everything a spectral mesh owns, in order: the resident tables (once; they depend on the mesh alone), the marching
// line sweeps' gate (MVTV_LINE_SWEEP=0 off), the blocked last-dimension solve where that dimension is long, the
// two-pass and chirp transforms' tables and scratch. Shared by problem creation and mvtv_problem_dct_chirp, which can
// make a refused mesh spectral later.
mvtv_status spectral_setup(mvtv_problem* P) {
    const int p = P->g.p;
    const bool first = !P->spec.tw;
    if (first && (P->spec_mesh || (P->slab && P->spec_lead && p >= 2))) MVTV_TRY(spectral_plan(P));
    if (first && P->spec_mesh && !P->slab) {
        const char* e = std::getenv("MVTV_LINE_SWEEP");
        MVTV_TRY(line_sweep_setup(P, (e && std::atoi(e) == 0) ? 0 : -1, 0));
    }
    if (P->spec_long && P->spec.lb.nblk == 0) MVTV_TRY(line_blocks_setup(P, 0));
    if (P->spec_mesh && !P->slab) MVTV_TRY(dct_split_setup(P));
    return MVTV_OK;
}

// a mesh that is refused (again): no transform is in use, and what the spectral period allocated beyond the mesh's
// own resident tables goes back: the transforms' scratch, the blocked line solve's and the line sweeps' buffers (which
// mvtv_problem_line_blocks / _line_sweep could no longer reach on a refused mesh)
void spectral_release(mvtv_problem* P) {
    SpecPlan& sp = P->spec;
    for (int j = 0; j < kMaxDims; ++j) {
        sp.split[j] = DctSplit{};
        sp.chirp[j] = DctChirp{};
    }
    for (double** b : {&sp.sscr, &sp.lb_coef, &sp.lb_lr, &P->ls_coef, &P->ls_lr})
        if (*b) {
            (void)hipFree(*b);
            *b = nullptr;
        }
    sp.sscr_cap = 0;
    sp.lb_cap = 0;
    sp.lb = LineBlocks{};
    P->ls_cap = 0;
    P->ls_chunks = 0;
}

// the mesh gate for the current chirp_forced / split_forced, and what follows from it
mvtv_status chirp_apply(mvtv_problem* P) {
    spectral_gate(P);
    if (P->spec_mesh) return spectral_setup(P);
    spectral_release(P);
    return MVTV_OK;
}

bool sweeps_on(const mvtv_problem* P) { return P->ls_chunks > 0 && P->spec.lb.nblk == 0 && !split_on(P); }

// down sweep, interface, up sweep, in place on x (the dim-0 coefficients of the right-hand side, then of the solve)
mvtv_status line_sweeps(mvtv_problem* P, double* x, double sigma, double w0, const AdmmCtl* ctl, const int32_t* skip) {
    for (int phase = 0; phase < 3; ++phase) {
        const int h = P->tstart(phase == 1 ? MVTV_K_REDUCE : MVTV_K_DCT);
        HIP_TRY(launch_line_sweep(P->spec, P->g, P->stream, phase, x, P->ls_coef, P->ls_lr, P->ls_chunks, sigma, w0, ctl,
                                  skip));
        P->tstop(h);
    }
    return MVTV_OK;
}

}  // namespace

namespace mvtv {
// Direct solve (I + sigma D^T D) x = oty + ca*ga + cb*gb: forward DCT along dims 0..p-2, the
// last dim's forward/divide/inverse in one pass, inverse DCT along dims p-2..0. All in place on x.
// fold: b = oty + fold_ka ga + fold_kb gb from the control block (ga = the fused kernel's folded
// s = rho (D^T alpha + D^T u), gb = D^T u)
mvtv_status spectral_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                           const double* gb, double cb, double* x, const AdmmCtl* ctl, double w0, const int32_t* skip,
                           bool fold) {
    const int p = P->g.p;
    // the first pass of a solve, along dim 0 (p = 1: the only one, mode 2): oty into x, b formed on load when ga is
    // given (fold: b = oty + fold_ka s + fold_kb g_u, g_u read after a rho change)
    auto first_pass = [&](int mode) -> hipError_t {
        if (ga && fold)
            return launch_dct_pass(P->spec, P->g, P->stream, mode, 0, oty, ga, 1.0, gb, 0.0, x, sigma, w0, ctl, 0, 0.0,
                                   skip, nullptr, true);
        if (ga)
            return launch_dct_pass(P->spec, P->g, P->stream, mode, 0, oty, ga, ca, gb ? gb : ga, gb ? cb : 0.0, x, sigma,
                                   w0, ctl, 0, 0.0, skip);
        return launch_dct_pass(P->spec, P->g, P->stream, mode, 0, oty, nullptr, 0.0, nullptr, 0.0, x, sigma, w0, ctl, 0,
                               0.0, skip);
    };
    // 3-D, m1 = 512: dim-0 forward (b formed on load), the down sweep, the chunk interface, the up sweep, dim-0
    // inverse: 9N words and the chunks' carries instead of 11N (line_sweep_setup chose ls_chunks)
    if (!P->slab && sweeps_on(P)) {
        int h = P->tstart(ga ? (fold ? MVTV_K_DCT_FOLD : MVTV_K_DCT_FIRST) : MVTV_K_DCT);
        HIP_TRY(first_pass(0));
        P->tstop(h);
        MVTV_TRY(line_sweeps(P, x, sigma, w0, ctl, skip));
        h = P->tstart(MVTV_K_DCT);
        HIP_TRY(launch_dct_pass(P->spec, P->g, P->stream, 1, 0, x, nullptr, 0.0, nullptr, 0.0, x, sigma, w0, ctl, 0, 0.0,
                                skip));
        P->tstop(h);
        return MVTV_OK;
    }
    // m0 = m1 <= 128: dims 0 and 1 in one pass each way (k_plane8: the plane stays on chip between them)
    const bool plane = plane_pass_ok(P->g) && !split_on(P);
    if (plane) {
        const int h = P->tstart(ga ? (fold ? MVTV_K_DCT_FOLD : MVTV_K_DCT_FIRST) : MVTV_K_DCT);
        if (ga && fold)
            HIP_TRY(launch_plane_pass(P->spec, P->g, P->stream, 0, oty, ga, 1.0, gb, 0.0, x, ctl, skip, true));
        else if (ga)
            HIP_TRY(launch_plane_pass(P->spec, P->g, P->stream, 0, oty, ga, ca, gb, cb, x, ctl, skip));
        else
            HIP_TRY(launch_plane_pass(P->spec, P->g, P->stream, 0, oty, nullptr, 0.0, nullptr, 0.0, x, ctl, skip));
        P->tstop(h);
    }
    for (int d = plane ? 2 : 0; d < p; ++d) {
        const int mode = d == p - 1 ? 2 : 0;
        const int h = P->tstart(d == 0 ? (fold ? MVTV_K_DCT_FOLD : MVTV_K_DCT_FIRST) : MVTV_K_DCT);
        if (d == 0)
            HIP_TRY(first_pass(mode));
        else
            HIP_TRY(launch_dct_pass(P->spec, P->g, P->stream, mode, d, x, nullptr, 0.0, nullptr, 0.0, x, sigma, w0, ctl, 0,
                                    0.0, skip));
        P->tstop(h);
    }
    for (int d = p - 2; d >= (plane ? 2 : 0); --d) {
        const int h = P->tstart(MVTV_K_DCT);
        HIP_TRY(launch_dct_pass(P->spec, P->g, P->stream, 1, d, x, nullptr, 0.0, nullptr, 0.0, x, sigma, w0, ctl, 0, 0.0,
                                skip));
        P->tstop(h);
    }
    if (plane) {
        const int h = P->tstart(MVTV_K_DCT);
        HIP_TRY(launch_plane_pass(P->spec, P->g, P->stream, 1, x, nullptr, 0.0, nullptr, 0.0, x, ctl, skip));
        P->tstop(h);
    }
    return MVTV_OK;
}

// (W + sigma D^T D) x = oty + ca*ga + cb*gb by PCG with the spectral preconditioner M = S A0 S,
// A0 = mean(W) I + sigma D^T D applied exactly by the cosine-transform solve. S = I when W is nearly
// constant against sigma D^T D's diagonal d (std(W) < 0.1 mean(d)); otherwise S = diag(sqrt(d / mean d)),
// which turns M into the Jacobi preconditioner as sigma -> 0 and into A0 as sigma grows (PCG counts to
// rtol 1e-10 from zero, 128^2 / 256^2: CV-fold mask at sigma = 6: Jacobi 187-192, M 19; scattered counts
// at sigma = 0.04: Jacobi 115, scaled M 95, unscaled 297). Scalars stay on the device
// (PcgState, k_finalize ops 1-3); iterations enqueued after convergence return at once (st->done).
mvtv_status pcgs_solve(mvtv_problem* P, double sigma, const double* oty, const double* ga, double ca,
                       const double* gb, double cb, double* x, double rtol, int maxit, int* iters, double* relres) {
    const Launch L = P->L();
    if (!P->p2) MVTV_TRY(alloc(&P->p2, P->g.N));
    if (!P->pcg_b) MVTV_TRY(alloc(&P->pcg_b, P->g.N));
    double *r = P->r, *z = P->q, *p = P->p, *q = P->p2, *b = P->pcg_b;
    const double w0 = P->wmean > 0.0 ? P->wmean : 1.0;
    // mean over the mesh of D^T D's diagonal: sum_S cS[S] prod_{j in S} mean(l_j), l_j = 1 at the ends, 2 inside
    double cmean = 0.0;
    for (int S = 1; S < (1 << P->g.p); ++S) {
        double prod = P->g.cS[S];
        for (int j = 0; j < P->g.p; ++j)
            if ((S >> j) & 1) prod *= 2.0 * double(P->g.m[j] - 1) / double(P->g.m[j]);
        cmean += prod;
    }
    const double dbar = w0 + sigma * cmean;
    const bool scaled = P->wmode == W_DIAG && P->wstd >= 0.1 * dbar;
    double *sinv = nullptr, *t = nullptr;
    if (scaled) {
        if (!P->pcg_s) MVTV_TRY(alloc(&P->pcg_s, P->g.N));
        if (!P->pcg_t) MVTV_TRY(alloc(&P->pcg_t, P->g.N));
        sinv = P->pcg_s;
        t = P->pcg_t;
        HIP_TRY(launch_pcgs_sinv(P->g, L, sigma, P->wmode, P->wdiag, dbar, sinv));
    }
    const double* rin = scaled ? t : r;
    int h = P->tstart(MVTV_K_PCG_INIT);
    HIP_TRY(launch_apply_A(P->g, L, sigma, P->wmode, P->wdiag, x, q, nullptr, nullptr));
    P->tstop(h);
    HIP_TRY(launch_pcgs_vec(P->g, L, 0, oty, ga, ca, gb, cb, x, r, p, q, nullptr, b, sinv, t, P->st, nullptr, 0));
    MVTV_TRY(spectral_solve(P, sigma, rin, nullptr, 0.0, nullptr, 0.0, z, nullptr, w0, nullptr));
    HIP_TRY(launch_pcgs_vec(P->g, L, 2, nullptr, nullptr, 0.0, nullptr, 0.0, x, r, p, q, z, b, sinv, nullptr, P->st,
                            P->partials, 1));
    HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 3, 0, 1, nullptr, P->st, rtol * rtol, maxit));
    HIP_TRY(hipMemcpyAsync(p, z, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToDevice, P->stream));
    const int32_t* skip = &P->st->done;
    // power-of-two m_0 >= 64: the x / r update rides on the preconditioner's first (d = 0) pass and the
    // s^-1 scaling with r.z, |r|^2 on its last, seven launches per iteration instead of nine
    const size_t pwords = size_t(std::max(kMaxGrid, kMaxCgBlocks)) * kMaxRed;
    const bool fused7 = dct_pcg_fusable(P->g, pwords) && !split_on(P);
    auto enqueue7 = [&]() -> mvtv_status {
        const int pdim = P->g.p;
        int np_last = 0;
        for (int t = 0; t < 2 * pdim - 1; ++t) {
            const int d = t < pdim ? t : 2 * pdim - 2 - t;
            const int mode = t < pdim - 1 ? 0 : (t == pdim - 1 ? 2 : 1);
            if (sweeps_on(P) && t >= 1 && t <= 3) {   // the sweeps in place of the three middle passes
                if (t == 1) MVTV_TRY(line_sweeps(P, z, sigma, w0, nullptr, skip));
                continue;
            }
            PcgFuse f;
            if (t == 0 || t == 2 * pdim - 2) {
                f.mode = t == 0 ? 1 : 2;
                f.st = P->st;
                f.x = x;
                f.r = r;
                f.p = p;
                f.q = q;
                f.sinv = sinv;
                f.partials = P->partials;
                f.cap = pwords;
                f.nparts = &np_last;
            }
            const int hh = P->tstart(t == 0 ? MVTV_K_DCT_FIRST : MVTV_K_DCT);
            HIP_TRY(launch_dct_pass(P->spec, P->g, P->stream, mode, d, t == 0 ? r : z, nullptr, 0.0, nullptr, 0.0, z,
                                    sigma, w0, nullptr, 0, 0.0, skip, f.mode ? &f : nullptr));
            P->tstop(hh);
        }
        HIP_TRY(launch_finalize(P->stream, P->partials, np_last, 2, 0, 3, nullptr, P->st));        // beta, done
        return MVTV_OK;
    };
    auto enqueue = [&]() -> mvtv_status {
        int hh = P->tstart(MVTV_K_PCG_APPLY);
        int npa = L.grid;
        HIP_TRY(launch_apply_A(P->g, L, sigma, P->wmode, P->wdiag, p, q, P->partials, P->st, &npa));   // q = A p, p.q
        P->tstop(hh);
        HIP_TRY(launch_finalize(P->stream, P->partials, npa, 1, 0, 2, nullptr, P->st));              // alpha
        if (fused7) {
            MVTV_TRY(enqueue7());
            hh = P->tstart(MVTV_K_PCG_DIRECTION);
            HIP_TRY(launch_pcgs_vec(P->g, L, 3, nullptr, nullptr, 0.0, nullptr, 0.0, x, r, p, q, z, b, nullptr, nullptr,
                                    P->st, nullptr, 0));
            P->tstop(hh);
            return MVTV_OK;
        }
        hh = P->tstart(MVTV_K_PCG_UPDATE);
        HIP_TRY(launch_pcgs_vec(P->g, L, 1, nullptr, nullptr, 0.0, nullptr, 0.0, x, r, p, q, nullptr, b, sinv, t,
                                P->st, nullptr, 0));
        P->tstop(hh);
        MVTV_TRY(spectral_solve(P, sigma, rin, nullptr, 0.0, nullptr, 0.0, z, nullptr, w0, skip));   // z = M^-1 r
        HIP_TRY(launch_pcgs_vec(P->g, L, 2, nullptr, nullptr, 0.0, nullptr, 0.0, x, r, p, q, z, b, sinv, nullptr,
                                P->st, P->partials, 0));
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 3, 0, 3, nullptr, P->st));         // beta, done
        hh = P->tstart(MVTV_K_PCG_DIRECTION);
        HIP_TRY(launch_pcgs_vec(P->g, L, 3, nullptr, nullptr, 0.0, nullptr, 0.0, x, r, p, q, z, b, nullptr, nullptr,
                                P->st, nullptr, 0));
        P->tstop(hh);
        return MVTV_OK;
    };
    std::vector<size_t> mark;
    int enq = 0;
    int batch = P->pcg_hint > 0 ? std::max(2, P->pcg_hint + pcg_ahead()) : kPcgPoll;
    for (;;) {
        for (int bb = 0; bb < batch && enq < maxit; ++bb, ++enq) {
            mark.push_back(P->pending.size());
            MVTV_TRY(enqueue());
        }
        HIP_TRY(hipMemcpyAsync(P->host_st, P->st, sizeof(PcgState), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        const int done_iters = P->host_st->iter;
        if (P->timing && done_iters < int(mark.size()))
            for (size_t e = mark[size_t(done_iters)]; e < P->pending.size(); ++e) P->pending[e].kid = -1;
        P->harvest();
        if (P->host_st->done || enq >= maxit) break;
        batch = 2;
    }
    *iters = P->host_st->iter;
    P->pcg_hint = *iters;
    *relres = P->host_st->bnorm2 > 0 ? std::sqrt(P->host_st->rnorm2 / P->host_st->bnorm2) : 0.0;
    return MVTV_OK;
}

mvtv_status ensure_state(mvtv_problem* P) {
    if (!P->have_state) return fail(MVTV_BAD_ARG, "no ADMM state: call mvtv_state_set first");
    return MVTV_OK;
}

}  // namespace mvtv

// =================================================================================== C ABI
extern "C" {

const char* mvtv_version(void) { return "multivartv_amd 0.1.0 (gfx950)"; }

const char* mvtv_status_string(int32_t s) {
    switch (s) {
        case MVTV_OK: return "ok";
        case MVTV_MAXITER: return "maximum ADMM iterations reached";
        case MVTV_BAD_ARG: return "bad argument";
        case MVTV_DIM_MISMATCH: return "dimension mismatch (mixed-partial construction)";
        case MVTV_HIP_ERROR: return "HIP error";
        case MVTV_NO_DEVICE: return "no HIP device";
        case MVTV_OUT_OF_MEMORY: return "out of device memory";
        case MVTV_PCG_NOT_CONVERGED: return "PCG theta-solve did not converge";
        default: return "unknown status";
    }
}

const char* mvtv_last_error(void) { return g_last_error.c_str(); }

int32_t mvtv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mvtv_default_opts(mvtv_admm_opts* o, int32_t variant) {
    std::memset(o, 0, sizeof(*o));
    o->variant = variant;
    o->sigma = std::nan("");
    o->ymean = 0.0;
}

}  // extern "C"

namespace {
mvtv_status problem_create_impl(const mvtv_problem_desc* d, const mvtv_slab_desc* sl, mvtv_problem** out) {
    if (!d || !out) return fail(MVTV_BAD_ARG, "null descriptor/output");
    *out = nullptr;
    if (d->p < 1 || d->p > MVTV_MAX_DIMS) return fail(MVTV_BAD_ARG, "p must be in 1..4");
    if (!d->oty) return fail(MVTV_BAD_ARG, "oty is required");
    if (d->block_order < MVTV_ORDER_CPP || d->block_order > MVTV_ORDER_PY_NOMINAL) return fail(MVTV_BAD_ARG, "block_order");
    if (sl && order_nominal(d->block_order))
        return fail(MVTV_BAD_ARG, "slab decomposition takes the reference difference sets only (MVTV_ORDER_CPP / MVTV_ORDER_PY)");
    const int p = d->p;
    uint64_t N = 1;
    // slab: the mesh is validated (and D built) with the global extent of dim p-1
    int64_t mg[MVTV_MAX_DIMS];
    for (int j = 0; j < MVTV_MAX_DIMS; ++j) mg[j] = d->m[j];
    if (sl) {
        if (p < 2) return fail(MVTV_BAD_ARG, "slab decomposition needs p >= 2");
        if (sl->z_begin < 0 || sl->z_end <= sl->z_begin || sl->z_end > sl->m_global)
            return fail(MVTV_BAD_ARG, "slab plane range");
        if ((sl->ghost_lo != 0) != (sl->z_begin > 0) || (sl->ghost_hi != 0) != (sl->z_end < sl->m_global))
            return fail(MVTV_BAD_ARG, "slab ghosts: one plane below unless z_begin = 0, one above unless z_end = m");
        if (d->m[p - 1] != sl->z_end - sl->z_begin + (sl->ghost_lo ? 1 : 0) + (sl->ghost_hi ? 1 : 0))
            return fail(MVTV_BAD_ARG, "local m[p-1] must be owned planes + ghosts");
        mg[p - 1] = sl->m_global;
    }
    for (int j = 0; j < p; ++j) {
        if (d->m[j] < 2 && !(sl && j == p - 1)) return fail(MVTV_BAD_ARG, "every m_j must be >= 2");
        if (mg[j] < 2) return fail(MVTV_BAD_ARG, "every m_j must be >= 2");
        N *= uint64_t(d->m[j]);
    }
    if (N >= (uint64_t(1) << 31)) return fail(MVTV_BAD_ARG, "N >= 2^31 nodes on one GPU");
    const int full = (1 << p) - 1;
    int nb;
    if ((d->block_order & 1) == MVTV_ORDER_CPP) nb = full;
    else nb = d->weighted ? full - 1 : full;
    if (nb <= 0) return fail(MVTV_BAD_ARG, "empty D (Python create_D with deltas at p = 1)");
    int ndev = mvtv_device_count();
    if (ndev <= 0) return fail(MVTV_NO_DEVICE, "no HIP device visible");
    if (d->device < 0 || d->device >= ndev) return fail(MVTV_BAD_ARG, "device ordinal out of range");

    auto* P = new mvtv_problem();
    P->device = d->device;
    P->order = d->block_order;
    P->weighted = d->weighted;
    Geom& g = P->g;
    g.p = p;
    g.nb = nb;
    g.N = uint32_t(N);
    uint32_t stride = 1;
    for (int j = 0; j < MVTV_MAX_DIMS; ++j) {
        g.m[j] = j < p ? uint32_t(d->m[j]) : 1u;
        g.stride[j] = stride;
        if (j < p) stride *= g.m[j];
        P->deltas[j] = j < p ? d->deltas[j] : 0.0;
    }
    for (int j = 0; j < MVTV_MAX_DIMS - 1; ++j) g.fd[j] = FastDiv(g.m[j]);
    for (int S = 0; S < 16; ++S) g.cS[S] = 0.0;
    P->E = 0;
    for (int k = 0; k < nb; ++k) {
        const int b = block_code(k, p, P->order);
        const int S = diff_mask(k, p, P->order);
        // reference mixedpartial: a mixed block with min S > 0 multiplies incompatible
        // matrices unless m_0 == m_{min S} (code/utils.py:102-129); the nominal
        // orders difference along the block's own dims and take any extents
        const int nominal = nominal_mask(b, p);
        if (!order_nominal(P->order) && popcount(nominal) >= 2 && !(nominal & 1)) {
            int lo = 0;
            while (!((nominal >> lo) & 1)) ++lo;
            if (mg[0] != mg[lo]) {
                delete P;
                return fail(MVTV_DIM_MISMATCH, "mixed partial of block " + std::to_string(b) +
                                                   ": m[0] != m[" + std::to_string(lo) + "]");
            }
        }
        double w = 1.0;
        if (d->weighted)
            for (int j = 0; j < p; ++j)
                if (!((b >> (p - 1 - j)) & 1)) w *= d->deltas[j];
        g.w[k] = w;
        g.cS[S] += w * w;
        P->codes[k] = b;
        P->sprime[k] = S;
        uint64_t len = 1;
        for (int j = 0; j < p; ++j) len *= uint64_t(g.m[j] - ((S >> j) & 1));
        P->blk_len[k] = len;
        P->E += int64_t(len);
    }
    for (int k = nb; k < kMaxBlocks; ++k) g.w[k] = 0.0;
    g.ibeg = 0;
    g.iend = uint32_t(N);
    if (sl) {
        const uint32_t plane = uint32_t(N / uint64_t(d->m[p - 1]));
        P->slab = true;
        P->m_global = sl->m_global;
        P->zb = sl->z_begin;
        P->ze = sl->z_end;
        P->g_lo = sl->ghost_lo ? 1 : 0;
        P->g_hi = sl->ghost_hi ? 1 : 0;
        g.ibeg = uint32_t(P->g_lo) * plane;
        g.iend = uint32_t(N) - uint32_t(P->g_hi) * plane;
    }
    P->grid = int(std::min<uint64_t>((N + kThreads - 1) / kThreads, kMaxGrid));
    if (const char* env = std::getenv("MVTV_PCG")) P->fused3d = std::strcmp(env, "classic") != 0;

    DeviceGuard dg(P->device);
    mvtv_status s = MVTV_OK;
    auto A = [&](double** ptr, size_t n) {
        if (s == MVTV_OK) s = alloc(ptr, n);
    };
    if (hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking) != hipSuccess) {
        delete P;
        return fail(MVTV_HIP_ERROR, "hipStreamCreate failed");
    }
    A(&P->oty, N);
    A(&P->theta, N);
    A(&P->edges, size_t(nb) * N);
    A(&P->ga, N);
    A(&P->gu, N);
    A(&P->guprev, N);
    A(&P->r, N);
    A(&P->p, N);
    A(&P->q, N);
    A(&P->partials, size_t(std::max(kMaxGrid, kMaxCgBlocks)) * kMaxRed);
    A(&P->red, 16);
    if (s == MVTV_OK && hipMalloc(reinterpret_cast<void**>(&P->st), sizeof(PcgState)) != hipSuccess)
        s = fail(MVTV_OUT_OF_MEMORY, "hipMalloc(PcgState)");
    if (s == MVTV_OK && hipHostMalloc(reinterpret_cast<void**>(&P->host_red), 16 * sizeof(double) + sizeof(PcgState)) != hipSuccess)
        s = fail(MVTV_OUT_OF_MEMORY, "hipHostMalloc");
    if (s == MVTV_OK && (hipMalloc(reinterpret_cast<void**>(&P->ctl), sizeof(AdmmCtl)) != hipSuccess ||
                         hipHostMalloc(reinterpret_cast<void**>(&P->host_ctl), sizeof(AdmmCtl)) != hipSuccess))
        s = fail(MVTV_OUT_OF_MEMORY, "control block");
    if (s != MVTV_OK) {
        free_all(P);
        delete P;
        return s;
    }
    P->host_st = reinterpret_cast<PcgState*>(P->host_red + 16);
    // MVTV_DCT_CHIRP=1: every leading dimension above 4096 without a two-pass factorisation starts under the chirp
    // transform with the library's convolution length (not on a slab rank); unset or 0: such a mesh is refused
    if (const char* e = std::getenv("MVTV_DCT_CHIRP"); e && std::atoi(e) != 0 && !P->slab)
        for (int j = 0; j < p - 1; ++j) {
            uint32_t ca = 0, cb = 0;
            if (g.m[j] > kSplitMax && dct_split_auto(g.m[j]) == 0 && dct_chirp_auto(g.m[j], &ca, &cb))
                P->chirp_forced[j][0] = -1;
        }
    // which meshes the spectral solve takes, and what such a problem owns (a slab problem's last dimension is solved
    // by the substructured line solves, any length: its tables are needed for the transforms along dims 0..p-2 only)
    spectral_gate(P);
    s = spectral_setup(P);
    P->e3d = edge3d_ok(g);
    if (s == MVTV_OK && P->e3d && g.p == 4 && gather4_ok(g)) s = alloc(&P->g4, 4 * size_t(N));
    P->f3d = fused3d_ok(g);   // slab problems too: the fused pass runs on the owned planes (Geom.ibeg/iend)
    P->f4d = P->e3d && g.p == 4 && P->g4 != nullptr && fused4_ok(g);   // slab ranks: on the owned planes
    {   // chunked edge layout for the 3-D fused path (MVTV_EAOS=0 keeps block-major): the fused kernel's
        // launches 2-4 % shorter at 512^3 on the same box (4.21 -> 4.13 ms, 5.2-5.36 -> 5.13 ms)
        const char* e = probe_env("MVTV_EAOS");
        const bool want = e ? std::atoi(e) != 0 : true;
        // a slab rank decides from its plane size, which every rank shares (its N counts its own ghost
        // planes): the z halo moves whole planes, one contiguous run per plane only when planes are whole
        // 64-node chunks, so every rank must pick the same layout
        const uint64_t plane = g.N / g.m[g.p - 1];
        const bool chunks = P->slab ? plane % 64 == 0 : g.N % 64 == 0;
        g.eaos = (want && ((P->f3d && g.p == 3) || (P->e3d && g.p == 4)) && chunks) ? 1u : 0u;
    }
    if (s == MVTV_OK) s = mvtv_problem_set_data(P, d->oty, d->wdiag);
    if (s != MVTV_OK) {
        free_all(P);
        delete P;
        return s;
    }
    *out = P;
    return MVTV_OK;
}
}  // namespace

extern "C" {

mvtv_status mvtv_problem_create(const mvtv_problem_desc* d, mvtv_problem** out) {
    return problem_create_impl(d, nullptr, out);
}

mvtv_status mvtv_problem_create_slab(const mvtv_problem_desc* d, const mvtv_slab_desc* slab, mvtv_problem** out) {
    if (!slab) return fail(MVTV_BAD_ARG, "null slab descriptor");
    return problem_create_impl(d, slab, out);
}

void mvtv_problem_destroy(mvtv_problem* P) {
    if (!P) return;
    DeviceGuard dg(P->device);
    (void)hipStreamSynchronize(P->stream);
    free_all(P);
    delete P;
}

int64_t mvtv_problem_nodes(const mvtv_problem* P) { return P ? int64_t(P->g.N) : 0; }
int64_t mvtv_problem_edges(const mvtv_problem* P) { return P ? P->E : 0; }
int32_t mvtv_problem_blocks(const mvtv_problem* P) { return P ? P->g.nb : 0; }
int32_t mvtv_problem_spectral_ok(const mvtv_problem* P) { return P && spectral_ok(P) ? 1 : 0; }

mvtv_status mvtv_problem_line_sweep(mvtv_problem* P, int32_t mode, int32_t chunks) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    return line_sweep_setup(P, mode, chunks);
}

mvtv_status mvtv_problem_line_blocks(mvtv_problem* P, int32_t blocks) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    return line_blocks_setup(P, blocks);
}

mvtv_status mvtv_problem_dct_split(mvtv_problem* P, int32_t dim, int32_t a) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    if (P->slab || !P->spec_mesh)
        return fail(MVTV_BAD_ARG, "dct_split: not a slab rank, and a mesh the spectral solve accepts");
    if (dim < 0 || dim >= P->g.p - 1) return fail(MVTV_BAD_ARG, "dct_split: 0 <= dim < p - 1");
    const uint32_t m = P->g.m[dim];
    if (a != 0 && (a < 2 || uint32_t(a) >= m || m % uint32_t(a) != 0 || !split_factor_ok(uint32_t(a)) ||
                   !split_factor_ok(m / uint32_t(a))))
        return fail(MVTV_BAD_ARG, "dct_split: a = 0, or m_dim = a * b with both factors 2-3-5-7-smooth in [2, 4096]");
    if (a != 0 && P->chirp_forced[dim][0] != 0)
        return fail(MVTV_BAD_ARG, "dct_split: the dimension is under dct_chirp");
    P->split_forced[dim] = a;
    return dct_split_setup(P);
}

mvtv_status mvtv_problem_dct_chirp(mvtv_problem* P, int32_t dim, int32_t a, int32_t b) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    if (P->slab) return fail(MVTV_BAD_ARG, "dct_chirp: not a slab rank");
    if (dim < 0 || dim >= P->g.p - 1) return fail(MVTV_BAD_ARG, "dct_chirp: 0 <= dim < p - 1");
    const uint32_t m = P->g.m[dim];
    if (a == -1) {
        uint32_t ca = 0, cb = 0;
        if (!dct_chirp_auto(m, &ca, &cb)) return fail(MVTV_BAD_ARG, "dct_chirp: no convolution length for this m");
        b = 0;
    } else if (a != 0 || b != 0) {
        if (a < 2 || b < 2 || !split_factor_ok(uint32_t(a)) || !split_factor_ok(uint32_t(b)) ||
            uint64_t(a) * uint64_t(b) + 1 < 2 * uint64_t(m))
            return fail(MVTV_BAD_ARG,
                        "dct_chirp: a = b = 0, a = -1, or a * b >= 2 m_dim - 1 with both factors 2-3-5-7-smooth in [2, 4096]");
    }
    if (a != 0 && P->split_forced[dim] != 0)
        return fail(MVTV_BAD_ARG, "dct_chirp: the dimension has a forced dct_split");
    HIP_TRY(hipStreamSynchronize(P->stream));
    const int32_t old_a = P->chirp_forced[dim][0], old_b = P->chirp_forced[dim][1];
    P->chirp_forced[dim][0] = a;
    P->chirp_forced[dim][1] = b;
    const mvtv_status s = chirp_apply(P);
    if (s != MVTV_OK) {   // e.g. no memory for the ~2N scratch: back to the mode before the call
        P->chirp_forced[dim][0] = old_a;
        P->chirp_forced[dim][1] = old_b;
        if (chirp_apply(P) != MVTV_OK) {   // nor for that one: nothing spectral stays in use (Jacobi-PCG)
            P->spec_mesh = P->spec_long = P->spec_pow2 = false;
            spectral_release(P);
        }
    }
    return s;
}

mvtv_status mvtv_problem_dct_chirp_get(const mvtv_problem* P, int32_t dim, int32_t* a, int32_t* b) {
    if (!P || dim < 0 || dim >= P->g.p - 1) return fail(MVTV_BAD_ARG, "dct_chirp_get: 0 <= dim < p - 1");
    if (a) *a = int32_t(P->spec.chirp[dim].a);
    if (b) *b = int32_t(P->spec.chirp[dim].b);
    return MVTV_OK;
}

mvtv_status mvtv_problem_block_info(const mvtv_problem* P, int32_t k, int32_t* code, int32_t* sprime, double* weight) {
    if (!P || k < 0 || k >= P->g.nb) return fail(MVTV_BAD_ARG, "block index");
    if (code) *code = P->codes[k];
    if (sprime) *sprime = P->sprime[k];
    if (weight) *weight = P->g.w[k];
    return MVTV_OK;
}

mvtv_status mvtv_problem_set_data(mvtv_problem* P, const double* oty, const double* wdiag) {
    if (!P || !oty) return fail(MVTV_BAD_ARG, "null problem/oty");
    DeviceGuard dg(P->device);
    const size_t bytes = size_t(P->g.N) * sizeof(double);
    HIP_TRY(hipMemcpyAsync(P->oty, oty, bytes, hipMemcpyHostToDevice, P->stream));
    if (wdiag) {
        if (!P->wdiag) MVTV_TRY(alloc(&P->wdiag, P->g.N));
        HIP_TRY(hipMemcpyAsync(P->wdiag, wdiag, bytes, hipMemcpyHostToDevice, P->stream));
        P->wmode = W_DIAG;
        double acc = 0.0, acc2 = 0.0;
        for (uint32_t i = 0; i < P->g.N; ++i) acc += wdiag[i];
        P->wmean = acc / double(P->g.N);
        for (uint32_t i = 0; i < P->g.N; ++i) acc2 += (wdiag[i] - P->wmean) * (wdiag[i] - P->wmean);
        P->wstd = std::sqrt(acc2 / double(P->g.N));
        // a slab rank's share of the global mean / spread (its owned planes), summed over the ranks by mvtv_slab_run
        P->wsum_own = P->wsum2_own = 0.0;
        for (uint32_t i = P->g.ibeg; i < P->g.iend; ++i) {
            P->wsum_own += wdiag[i];
            P->wsum2_own += wdiag[i] * wdiag[i];
        }
    } else {
        P->wmode = W_IDENTITY;
        P->wmean = 1.0;
        P->wstd = 0.0;
        P->wsum_own = P->wsum2_own = double(P->g.iend - P->g.ibeg);
    }
    HIP_TRY(hipStreamSynchronize(P->stream));
    return MVTV_OK;
}

mvtv_status mvtv_state_set(mvtv_problem* P, const double* theta, const double* u, double rho) {
    if (!P || !theta) return fail(MVTV_BAD_ARG, "null problem/theta");
    DeviceGuard dg(P->device);
    HIP_TRY(hipMemcpyAsync(P->theta, theta, size_t(P->g.N) * sizeof(double), hipMemcpyHostToDevice, P->stream));
    P->twin_ok = true;
    if (u) {
        MVTV_TRY(import_edges(P, u, P->edges));
        P->u_default = false;
        uint64_t off[kMaxBlocks + 1] = {0};   // the twin blocks of the caller's u (reference block layout)
        for (int k = 0; k < P->g.nb; ++k) off[k + 1] = off[k] + P->blk_len[k];
        for (int k = 0; k < P->g.nb && P->twin_ok; ++k) {
            const int c = twin_of(k, P->g.p, P->order);
            if (c != k)
                P->twin_ok = P->blk_len[k] == P->blk_len[c] &&
                             std::memcmp(u + off[k], u + off[c], size_t(P->blk_len[k]) * sizeof(double)) == 0;
        }
    } else {
        P->u_default = true;
    }
    HIP_TRY(hipStreamSynchronize(P->stream));
    P->edge_mode = U_EXPLICIT;
    P->t_z = 0.0;
    P->c_state = 1.0;
    P->rho = rho;
    P->have_state = true;
    return MVTV_OK;
}

mvtv_status mvtv_state_get(mvtv_problem* P, double* theta, double* u, double* rho) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    MVTV_TRY(ensure_state(P));
    DeviceGuard dg(P->device);
    if (theta) {
        HIP_TRY(hipMemcpyAsync(theta, P->theta, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
    }
    if (u) {
        if (P->u_default) return fail(MVTV_BAD_ARG, "u is the variant default and has not been formed yet");
        MVTV_TRY(export_edges(P, P->edges, u, P->edge_mode, P->t_z, P->c_state));
    }
    if (rho) *rho = P->rho;
    return MVTV_OK;
}

mvtv_status mvtv_admm(mvtv_problem* P, const mvtv_admm_opts* opts, double lambda, double* theta_inout,
                      double* u_inout, double* rho_inout, mvtv_admm_stats* stats) {
    if (!P || !opts || !theta_inout) return fail(MVTV_BAD_ARG, "null problem/opts/theta");
    const double rho0 = rho_inout ? *rho_inout : lambda / 5.0;
    MVTV_TRY(mvtv_state_set(P, theta_inout, u_inout, rho0));
    mvtv_status s = mvtv_admm_run(P, opts, lambda, stats);
    if (s != MVTV_OK && s != MVTV_MAXITER) return s;
    mvtv_status g = mvtv_state_get(P, theta_inout, u_inout, rho_inout);
    if (g != MVTV_OK) return g;
    return s;
}

mvtv_status mvtv_path(mvtv_problem* P, const mvtv_admm_opts* opts, const double* lambdas, int32_t n_lambda,
                      const double* theta_init, double rho_init, double* thetas_out, double* rhos_out,
                      mvtv_admm_stats* stats) {
    if (!P || !opts || !theta_init || n_lambda < 0 || (n_lambda > 0 && !lambdas))
        return fail(MVTV_BAD_ARG, "null argument");
    MVTV_TRY(mvtv_state_set(P, theta_init, nullptr, rho_init));
    mvtv_status worst = MVTV_OK;
    for (int32_t i = 0; i < n_lambda; ++i) {
        mvtv_admm_stats st{};
        const mvtv_status s = mvtv_admm_run(P, opts, lambdas[i], &st);
        if (s == MVTV_MAXITER) worst = MVTV_MAXITER;
        else if (s != MVTV_OK) return s;
        if (stats) stats[i] = st;
        if (thetas_out) MVTV_TRY(mvtv_state_get(P, thetas_out + size_t(i) * P->g.N, nullptr, nullptr));
        if (rhos_out) rhos_out[i] = P->rho;
    }
    return worst;
}

int32_t mvtv_problem_batch_ok(const mvtv_problem* P) { return P && !P->slab && small_ok(P->g) ? 1 : 0; }

} // extern "C"

namespace {
// The batched calls' device buffers: one allocation kept on the problem, grown when a call needs more, carved into
// 256-byte aligned pieces in the order they are asked for.
struct BatchArena {
    mvtv_problem* P;
    size_t need = 0;
    std::vector<std::pair<void**, size_t>> parts;
    template <class T>
    void add(T** ptr, size_t n) {
        parts.emplace_back(reinterpret_cast<void**>(ptr), need);
        need += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~size_t(255);
    }
    mvtv_status commit() {
        if (need > P->batch_cap) {
            HIP_TRY(hipStreamSynchronize(P->stream));
            if (P->batch_buf) (void)hipFree(P->batch_buf);
            P->batch_buf = nullptr;
            P->batch_cap = 0;
            HIP_TRY(hipMalloc(&P->batch_buf, need));
            P->batch_cap = need;
        }
        for (auto& pr : parts) *pr.first = static_cast<char*>(P->batch_buf) + pr.second;
        return MVTV_OK;
    }
};

// The in-workgroup cosine solve's tables (mvtv_small_cos.hip), built once per problem in long double and rounded:
// per transformed dimension the orthonormal DCT-II matrix at the plan's pitch, per line of the line dimension
// a = sum_{S without ld} cS[S] prod_{j in S} lam_j(k_j) and b = sum_{S with ld} cS[S] prod_{j in S, j != ld} lam_j(k_j),
// lam_j(k) = 4 sin^2(pi k / 2 m_j), cS[S] the sum of w_k^2 over the blocks with S'(k) = S.
mvtv_status cos_plan_setup(mvtv_problem* P) {
    if (P->cos.ld >= 0) return MVTV_OK;
    Geom g = P->g;
    CosPlan cp;
    if (!small_cos_shape(g, &cp)) return fail(MVTV_BAD_ARG, "the mesh does not admit the in-workgroup cosine solve");
    const long double pi = 4.0L * std::atan(1.0L);
    std::vector<double> tab(std::max<uint32_t>(cp.tab_words, 1), 0.0), ab(2 * size_t(cp.nlines));
    std::vector<std::vector<long double>> lam(g.p);
    for (int j = 0; j < g.p; ++j) {
        const uint32_t m = g.m[j];
        lam[j].resize(m);
        for (uint32_t k = 0; k < m; ++k) {
            const long double sn = std::sin(pi * (long double)k / (long double)(2 * m));
            lam[j][k] = 4.0L * sn * sn;
        }
        if (j == cp.ld) continue;
        const long double s0 = std::sqrt(1.0L / (long double)m), s1 = std::sqrt(2.0L / (long double)m);
        for (uint32_t k = 0; k < m; ++k)
            for (uint32_t n = 0; n < m; ++n) {
                const uint32_t arg = uint32_t((uint64_t(2 * n + 1) * k) % (4 * m));   // the angle's period is 4m
                tab[cp.toff[j] + size_t(k) * cp.pitch[j] + n] =
                    double((k == 0 ? s0 : s1) * std::cos(pi * (long double)arg / (long double)(2 * m)));
            }
    }
    long double cS[16] = {0};
    for (int k = 0; k < g.nb; ++k) cS[P->sprime[k]] += (long double)g.w[k] * (long double)g.w[k];
    const uint32_t lstride = g.stride[cp.ld], lm = g.m[cp.ld];
    for (uint32_t line = 0; line < cp.nlines; ++line) {
        const uint32_t hi = line / lstride, lo = line - hi * lstride;
        uint32_t rest = lo + hi * lstride * lm, c[kMaxDims] = {0, 0, 0, 0};
        for (int j = 0; j < g.p; ++j) {
            c[j] = j < g.p - 1 ? rest % g.m[j] : rest;
            rest /= g.m[j];
        }
        long double a = 0.0L, b = 0.0L;
        for (int S = 1; S < (1 << g.p); ++S) {
            long double prod = cS[S];
            for (int j = 0; j < g.p; ++j)
                if (((S >> j) & 1) && j != cp.ld) prod *= lam[j][c[j]];
            if ((S >> cp.ld) & 1) b += prod;
            else a += prod;
        }
        ab[line] = double(a);
        ab[cp.nlines + line] = double(b);
    }
    double *d_tab = nullptr, *d_ab = nullptr;
    MVTV_TRY(alloc(&d_tab, tab.size()));
    if (alloc(&d_ab, ab.size()) != MVTV_OK) {
        (void)hipFree(d_tab);
        return MVTV_OUT_OF_MEMORY;
    }
    cp.tab = d_tab;
    cp.ab = d_ab;
    P->cos = cp;   // owned from here on (free_all)
    HIP_TRY(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ab, ab.data(), ab.size() * sizeof(double), hipMemcpyHostToDevice));
    return MVTV_OK;
}
}  // namespace

extern "C" {

mvtv_status mvtv_problem_batch_cosine(mvtv_problem* P, int32_t mode) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    if (!mvtv_problem_batch_ok(P))
        return fail(MVTV_BAD_ARG, "batch_cosine: batched fits need one GPU's whole mesh of at most 4096 nodes (p = 4: 1296)");
    if (mode < 0 || mode > 2) return fail(MVTV_BAD_ARG, "batch_cosine: mode 0, 1 or 2");
    DeviceGuard dg(P->device);
    if (mode > 0) MVTV_TRY(cos_plan_setup(P));
    P->batch_cos = mode;
    return MVTV_OK;
}

mvtv_status mvtv_problem_batch_cosine_get(const mvtv_problem* P, int32_t* mode) {
    if (!P || !mode) return fail(MVTV_BAD_ARG, "batch_cosine_get: null argument");
    *mode = P->batch_cos;
    return MVTV_OK;
}

mvtv_status mvtv_solve_batch(mvtv_problem* P, int32_t nbatch, const double* sigma, const double* shift, const double* f,
                             double* x) {
    if (!P || !sigma || !f || !x) return fail(MVTV_BAD_ARG, "null argument");
    if (!mvtv_problem_batch_ok(P))
        return fail(MVTV_BAD_ARG, "solve_batch: needs one GPU's whole mesh of at most 4096 nodes (p = 4: 1296)");
    if (nbatch < 1) return fail(MVTV_BAD_ARG, "nbatch must be >= 1");
    for (int32_t b = 0; b < nbatch; ++b) {
        if (!(sigma[b] >= 0.0) || std::isinf(sigma[b])) return fail(MVTV_BAD_ARG, "sigma must be >= 0 and finite");
        if (shift && (!(shift[b] > 0.0) || std::isinf(shift[b]))) return fail(MVTV_BAD_ARG, "shift must be positive and finite");
    }
    DeviceGuard dg(P->device);
    MVTV_TRY(cos_plan_setup(P));
    const size_t N = P->g.N, B = size_t(nbatch);
    double *d_sigma = nullptr, *d_shift = nullptr, *d_x = nullptr;
    BatchArena ar{P};
    ar.add(&d_sigma, B);
    ar.add(&d_shift, B);
    ar.add(&d_x, B * N);
    MVTV_TRY(ar.commit());
    hipStream_t s = P->stream;
    HIP_TRY(hipMemcpyAsync(d_sigma, sigma, B * sizeof(double), hipMemcpyHostToDevice, s));
    if (shift) HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_x, f, B * N * sizeof(double), hipMemcpyHostToDevice, s));
    Geom g = P->g;
    g.eaos = 0;
    HIP_TRY(launch_solve_cos(g, P->cos, s, nbatch, d_sigma, shift ? d_shift : nullptr, d_x, d_x));
    HIP_TRY(hipMemcpyAsync(x, d_x, B * N * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MVTV_OK;
}

}  // extern "C"

namespace {
// ---- what mvtv_path_batch and mvtv_cv_batch share: the checks, the members' kinds, the lambda loop and the stats ----
// the refusals that depend on the problem, the options and the counts alone
mvtv_status batch_check(const mvtv_problem* P, const mvtv_admm_opts& o, int64_t nbatch, int32_t n_lambda) {
    if (!mvtv_problem_batch_ok(P))
        return fail(MVTV_BAD_ARG, "batched fits need one GPU's whole mesh of at most 4096 nodes (p = 4: 1296)");
    if (o.variant != MVTV_VARIANT_RCPP) return fail(MVTV_BAD_ARG, "batched fits run variant B only");
    const int cosm = P->batch_cos;
    if (cosm == 0) {
        if (o.theta_solver != MVTV_SOLVER_AUTO && o.theta_solver != MVTV_SOLVER_PCG)
            return fail(MVTV_BAD_ARG, "batched fits solve for theta by PCG");
    } else {
        if (o.theta_solver < MVTV_SOLVER_AUTO || o.theta_solver > MVTV_SOLVER_PCG_SPECTRAL)
            return fail(MVTV_BAD_ARG, "unknown theta_solver");
        if (o.theta_solver == MVTV_SOLVER_PCG_SPECTRAL && cosm < 2)
            return fail(MVTV_BAD_ARG, "batched fits: PCG_SPECTRAL needs batch_cosine mode 2");
    }
    if (!std::isnan(o.sigma)) return fail(MVTV_BAD_ARG, "batched fits take the matrix scalar rho (sigma must be NaN)");
    if (nbatch < 1 || n_lambda < 1) return fail(MVTV_BAD_ARG, "nbatch and n_lambda must be >= 1");
    return MVTV_OK;
}

// the validation scan of W also gives each member's kind (a row of all ones is W = I) and mean(W), std(W)
mvtv_status batch_scan_w(const double* wdiag, size_t B, size_t N, int cosm, std::vector<int32_t>& kind,
                         std::vector<double>& wstat) {
    if (cosm > 0) {
        kind.assign(B, SMALL_KIND_COS);
        wstat.assign(2 * B, 0.0);
        for (size_t b = 0; b < B; ++b) wstat[2 * b] = 1.0;
    }
    if (wdiag)
        for (size_t b = 0; b < B; ++b) {
            bool pos = false, ones = true;
            double sum = 0.0, sum2 = 0.0;
            for (size_t i = 0; i < N; ++i) {
                const double w = wdiag[b * N + i];
                if (!(w >= 0.0)) return fail(MVTV_BAD_ARG, "W must be >= 0");
                pos = pos || w > 0.0;
                ones = ones && w == 1.0;
                sum += w;
                sum2 += w * w;
            }
            if (!pos) return fail(MVTV_BAD_ARG, "a member's W has no positive entry");
            if (cosm > 0 && !ones) {
                const double mean = sum / double(N);
                kind[b] = SMALL_KIND_COS_PCG;
                wstat[2 * b] = mean;
                wstat[2 * b + 1] = std::sqrt(std::max(0.0, sum2 / double(N) - mean * mean));
            }
        }
    return MVTV_OK;
}

// the kernel each member runs under the problem's batch_cosine mode and opts.theta_solver; has[k]: kind k is present
mvtv_status batch_kinds(mvtv_problem* P, const mvtv_admm_opts& o, std::vector<int32_t>& kind, bool (&has)[3]) {
    const int cosm = P->batch_cos;
    has[0] = cosm == 0, has[1] = has[2] = false;
    if (cosm > 0) {
        for (int32_t& k : kind) {
            if (o.theta_solver == MVTV_SOLVER_SPECTRAL && k != SMALL_KIND_COS)
                return fail(MVTV_BAD_ARG, "batched fits: SPECTRAL needs W = I for every member");
            if (o.theta_solver == MVTV_SOLVER_PCG) k = SMALL_KIND_JACOBI;
            else if (o.theta_solver == MVTV_SOLVER_PCG_SPECTRAL) k = SMALL_KIND_COS_PCG;
            else if (k == SMALL_KIND_COS_PCG && cosm < 2) k = SMALL_KIND_JACOBI;
            has[k] = true;
        }
        MVTV_TRY(cos_plan_setup(P));
    }
    return MVTV_OK;
}

// the members' device-resident inputs and state, carved from the problem's batch arena
struct BatchDev {
    double *oty = nullptr, *w = nullptr, *lam = nullptr, *theta = nullptr, *z = nullptr, *gag = nullptr,
           *thetas = nullptr, *wstat = nullptr;
    SmallCtl *ctl = nullptr, *log = nullptr;
    int32_t *rem = nullptr, *kind = nullptr;
};

void batch_arena_add(BatchArena& ar, BatchDev& d, const mvtv_problem* P, size_t B, size_t NL, bool with_w,
                     bool with_thetas) {
    const size_t N = P->g.N, nbN = size_t(P->g.nb) * N;
    ar.add(&d.oty, B * N);
    if (with_w) ar.add(&d.w, B * N);
    ar.add(&d.lam, B * NL);
    ar.add(&d.theta, B * N);
    ar.add(&d.z, B * nbN);
    ar.add(&d.gag, B * 2 * N);
    if (with_thetas) ar.add(&d.thetas, B * NL * N);
    ar.add(&d.ctl, B);
    ar.add(&d.log, B * NL);
    ar.add(&d.rem, NL);
    if (P->batch_cos > 0) {
        ar.add(&d.kind, B);
        ar.add(&d.wstat, 2 * B);
    }
}

// u0 = 0 (z = 0), every member's control block from its rho_init, the unfinished-member counters, the kinds. The
// copies are asynchronous: hs, kind and wstat must outlive the caller's next stream synchronisation.
struct BatchHostState {
    std::vector<SmallCtl> ctl;
    std::vector<int32_t> rem;
};
mvtv_status batch_upload_state(mvtv_problem* P, const BatchDev& d, size_t B, size_t NL, const double* rho_init,
                               const std::vector<int32_t>& kind, const std::vector<double>& wstat, BatchHostState& hs) {
    const size_t nbN = size_t(P->g.nb) * P->g.N;
    std::vector<SmallCtl>& ctl = hs.ctl;
    ctl.resize(B);
    for (size_t b = 0; b < B; ++b) {
        ctl[b] = SmallCtl{};
        ctl[b].cur_l = -1;
        ctl[b].rho = rho_init[b];
        ctl[b].c = 1.0;   // u0 = 0: z = 0, t_z = 0
    }
    hs.rem.assign(NL, int32_t(B));
    const std::vector<int32_t>& rem = hs.rem;
    hipStream_t s = P->stream;
    HIP_TRY(hipMemsetAsync(d.z, 0, B * nbN * sizeof(double), s));
    HIP_TRY(hipMemcpyAsync(d.ctl, ctl.data(), B * sizeof(SmallCtl), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.rem, rem.data(), NL * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (P->batch_cos > 0) {
        HIP_TRY(hipMemcpyAsync(d.kind, kind.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d.wstat, wstat.data(), 2 * B * sizeof(double), hipMemcpyHostToDevice, s));
    }
    return MVTV_OK;
}

// The lambda loop over device-resident members: per lambda the launches of the loop kernels (one per member kind
// present) are enqueued two rounds at a time and the device counter of members that have not finished that lambda is
// read after each pair.
mvtv_status batch_loop(mvtv_problem* P, const mvtv_admm_opts& o, int32_t nbatch, int32_t n_lambda, const BatchDev& d,
                       const bool (&has)[3]) {
    hipStream_t s = P->stream;
    Geom g = P->g;
    g.eaos = 0;
    SmallArgs a{};
    a.oty = d.oty, a.wdiag = d.w, a.lambdas = d.lam, a.theta = d.theta, a.z = d.z, a.gag = d.gag;
    a.ctl = d.ctl, a.log = d.log, a.thetas_out = d.thetas, a.remaining = d.rem;
    a.kind = d.kind, a.wstat = d.wstat;
    a.n_lambda = n_lambda;
    a.fixed_iters = o.fixed_iters;
    a.max_counter = variant_maxc(o);
    a.pcg_maxit = o.pcg_max_iter > 0 ? o.pcg_max_iter : 20000;
    a.pcg_strict = o.pcg_strict;
    a.tol = variant_tol(o);
    const double rtol = o.pcg_rtol > 0 ? o.pcg_rtol : 1e-10;
    a.rtol2 = rtol * rtol;
    a.sqrtN = std::sqrt(double(P->g.N));
    a.sqrtE = std::sqrt(double(P->E));
    for (int k = 0; k < P->g.nb; ++k) a.sp[k] = P->sprime[k];
    // launches that can be needed for one lambda: the iteration bound in chunks, and the pair's second
    const int64_t it_cap = o.fixed_iters > 0 ? o.fixed_iters : a.max_counter;
    const int64_t launch_cap = (it_cap + kSmallChunk - 1) / kSmallChunk + 2;
    for (int32_t li = 0; li < n_lambda; ++li) {
        a.li = li;
        int32_t left = nbatch;
        for (int64_t done = 0; left > 0; done += 2) {
            if (done >= launch_cap) return fail(MVTV_HIP_ERROR, "batched fits: members unfinished after the iteration bound");
            for (int rep = 0; rep < 2; ++rep) {
                if (has[SMALL_KIND_JACOBI]) HIP_TRY(launch_admm_small(g, s, nbatch, a));
                if (has[SMALL_KIND_COS]) HIP_TRY(launch_admm_cos(g, P->cos, s, nbatch, a, false));
                if (has[SMALL_KIND_COS_PCG]) HIP_TRY(launch_admm_cos(g, P->cos, s, nbatch, a, true));
            }
            HIP_TRY(hipMemcpyAsync(&left, d.rem + li, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return MVTV_OK;
}

// the per-(member, lambda) control blocks as rhos and stats; the call's return status
mvtv_status batch_stats(const mvtv_problem* P, const std::vector<SmallCtl>& log, size_t NL,
                        const std::vector<int32_t>& kind, double seconds, double* rhos_out, mvtv_admm_stats* stats) {
    mvtv_status worst = MVTV_OK;
    for (size_t i = 0; i < log.size(); ++i) {
        const SmallCtl& c = log[i];
        if (c.status == MVTV_PCG_NOT_CONVERGED) worst = MVTV_PCG_NOT_CONVERGED;
        else if (c.status == MVTV_MAXITER && worst == MVTV_OK) worst = MVTV_MAXITER;
        if (rhos_out) rhos_out[i] = c.rho;
        if (stats) {
            mvtv_admm_stats S{};
            S.iters = c.it;
            S.status = c.status;
            S.r_norm = c.primal;
            S.s_norm = c.dual;
            S.eps_pri = c.eps_p;
            S.eps_dual = c.eps_d;
            S.rho = c.rho;
            S.pcg_iters = c.pcg_iters;
            S.pcg_iters_max = c.pcg_max;
            S.pcg_unconverged = c.pcg_unconv;
            S.seconds = seconds;
            const int32_t k = P->batch_cos > 0 ? kind[i / NL] : int32_t(SMALL_KIND_JACOBI);
            S.theta_solver = k == SMALL_KIND_COS ? MVTV_SOLVER_SPECTRAL
                                                 : (k == SMALL_KIND_COS_PCG ? MVTV_SOLVER_PCG_SPECTRAL : MVTV_SOLVER_PCG);
            stats[i] = S;
        }
    }
    if (worst == MVTV_PCG_NOT_CONVERGED) fail(worst, "PCG hit pcg_max_iter");
    return worst;
}
}  // namespace

extern "C" {

// Many independent fits on the problem's mesh, each member's whole path in one workgroup (mvtv_small.hip,
// mvtv_small_cos.hip): the members' inputs go up, batch_loop runs them, the results come down.
mvtv_status mvtv_path_batch(mvtv_problem* P, const mvtv_admm_opts* opts, int32_t nbatch, const double* oty,
                            const double* wdiag, const double* lambdas, int32_t n_lambda, const double* theta_init,
                            const double* rho_init, double* thetas_out, double* u_out, double* rhos_out,
                            mvtv_admm_stats* stats) {
    if (!P || !opts || !oty || !lambdas || !theta_init || !rho_init) return fail(MVTV_BAD_ARG, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    const mvtv_admm_opts& o = *opts;
    MVTV_TRY(batch_check(P, o, nbatch, n_lambda));
    const size_t N = P->g.N, nbN = size_t(P->g.nb) * N, B = size_t(nbatch), NL = size_t(n_lambda);
    for (size_t i = 0; i < B * NL; ++i)
        if (!(lambdas[i] >= 0.0)) return fail(MVTV_BAD_ARG, "lambda must be >= 0");
    for (size_t b = 0; b < B; ++b)
        if (!(rho_init[b] > 0.0) || std::isinf(rho_init[b])) return fail(MVTV_BAD_ARG, "rho_init must be positive and finite");
    std::vector<int32_t> kind;
    std::vector<double> wstat;
    MVTV_TRY(batch_scan_w(wdiag, B, N, P->batch_cos, kind, wstat));
    bool has[3];
    MVTV_TRY(batch_kinds(P, o, kind, has));
    DeviceGuard dg(P->device);
    BatchDev d;
    BatchArena ar{P};
    batch_arena_add(ar, d, P, B, NL, wdiag != nullptr, thetas_out != nullptr);
    MVTV_TRY(ar.commit());
    hipStream_t s = P->stream;
    HIP_TRY(hipMemcpyAsync(d.oty, oty, B * N * sizeof(double), hipMemcpyHostToDevice, s));
    if (wdiag) HIP_TRY(hipMemcpyAsync(d.w, wdiag, B * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.lam, lambdas, B * NL * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.theta, theta_init, B * N * sizeof(double), hipMemcpyHostToDevice, s));
    BatchHostState hs;
    MVTV_TRY(batch_upload_state(P, d, B, NL, rho_init, kind, wstat, hs));
    MVTV_TRY(batch_loop(P, o, nbatch, n_lambda, d, has));
    std::vector<SmallCtl> log(B * NL);
    HIP_TRY(hipMemcpyAsync(log.data(), d.log, B * NL * sizeof(SmallCtl), hipMemcpyDeviceToHost, s));
    if (thetas_out) HIP_TRY(hipMemcpyAsync(thetas_out, d.thetas, B * NL * N * sizeof(double), hipMemcpyDeviceToHost, s));
    std::vector<double> z;
    if (u_out) {
        z.resize(B * nbN);
        HIP_TRY(hipMemcpyAsync(z.data(), d.z, B * nbN * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (u_out) {   // u = -c clamp(z, t_z) on the real edges, blocks in the problem's order, each a column-major reduced grid
        double* out = u_out;
        for (size_t b = 0; b < B; ++b) {
            const SmallCtl& c = log[b * NL + NL - 1];
            for (int k = 0; k < P->g.nb; ++k) {
                uint32_t rd[kMaxDims] = {1, 1, 1, 1};
                for (int j = 0; j < P->g.p; ++j) rd[j] = P->g.m[j] - ((P->sprime[k] >> j) & 1);
                const double* zk = z.data() + b * nbN + size_t(k) * N;
                for (uint32_t c3 = 0; c3 < rd[3]; ++c3)
                    for (uint32_t c2 = 0; c2 < rd[2]; ++c2)
                        for (uint32_t c1 = 0; c1 < rd[1]; ++c1)
                            for (uint32_t c0 = 0; c0 < rd[0]; ++c0) {
                                const size_t i = size_t(c0) * P->g.stride[0] + size_t(c1) * P->g.stride[1] +
                                                 size_t(c2) * P->g.stride[2] + size_t(c3) * P->g.stride[3];
                                const double cl = std::min(std::max(zk[i], -c.t_z), c.t_z);
                                *out++ = cl == 0.0 ? 0.0 : -c.c * cl;
                            }
            }
        }
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return batch_stats(P, log, NL, kind, seconds, rhos_out, stats);
}

mvtv_status mvtv_fitted(mvtv_problem* P, const int64_t* mesh_index, int64_t n, double* fitted) {
    if (!P || (n > 0 && (!mesh_index || !fitted))) return fail(MVTV_BAD_ARG, "null argument");
    if (n == 0) return MVTV_OK;
    DeviceGuard dg(P->device);
    int64_t* didx = nullptr;
    double* dout = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&didx), size_t(n) * sizeof(int64_t)));
    if (hipMalloc(reinterpret_cast<void**>(&dout), size_t(n) * sizeof(double)) != hipSuccess) {
        (void)hipFree(didx);
        return fail(MVTV_OUT_OF_MEMORY, "hipMalloc");
    }
    mvtv_status s = MVTV_OK;
    for (int64_t t = 0; t < n; ++t)
        if (mesh_index[t] < 0 || mesh_index[t] >= int64_t(P->g.N)) s = fail(MVTV_BAD_ARG, "mesh index out of range");
    if (s == MVTV_OK) {
        if (hipMemcpyAsync(didx, mesh_index, size_t(n) * sizeof(int64_t), hipMemcpyHostToDevice, P->stream) != hipSuccess ||
            launch_gather_index(P->stream, P->theta, didx, n, dout) != hipSuccess ||
            hipMemcpyAsync(fitted, dout, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, P->stream) != hipSuccess ||
            hipStreamSynchronize(P->stream) != hipSuccess)
            s = fail(MVTV_HIP_ERROR, "fitted: HIP failure");
    }
    (void)hipFree(didx);
    (void)hipFree(dout);
    return s;
}

}  // extern "C"

namespace {
// device scratch freed on scope exit (setup paths, not the iteration loop)
struct TmpDev {
    void* p = nullptr;
    ~TmpDev() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T* get() const { return static_cast<T*>(p); }
};

// axes (finite, ascending per dim) and data (finite) checked on the host, then axes and data copied over and the
// nearest node of every point computed into key (and idx when requested)
// the host checks of a scattered data set: not a slab rank, axes finite and ascending, data finite; *na = the axes'
// value count, span[j] = axis j's extent
mvtv_status check_axes_data(const mvtv_problem* P, const double* axes, const double* data, int64_t n, size_t* na_out,
                            double (&span)[MVTV_MAX_DIMS]) {
    if (P->slab) return fail(MVTV_BAD_ARG, "scattered data on a slab problem: set it up on the whole mesh");
    const int p = P->g.p;
    size_t na = 0;
    for (int j = 0; j < p; ++j) {
        const double* a = axes + na;
        span[j] = a[P->g.m[j] - 1] - a[0];
        for (uint32_t k = 0; k < P->g.m[j]; ++k)
            if (!std::isfinite(a[k]) || (k > 0 && !(a[k] > a[k - 1])))
                return fail(MVTV_BAD_ARG, "axes must be finite and strictly ascending per dimension");
        na += P->g.m[j];
    }
    for (int64_t i = 0; i < n * p; ++i)
        if (!std::isfinite(data[i])) return fail(MVTV_BAD_ARG, "NaN or infinite value in data");
    *na_out = na;
    return MVTV_OK;
}

mvtv_status nearest_on_device(mvtv_problem* P, const double* axes, const double* data, int64_t n, TmpDev& key,
                              TmpDev& idx, bool want_idx) {
    const int p = P->g.p;
    size_t na = 0;
    double span[MVTV_MAX_DIMS] = {0, 0, 0, 0};
    MVTV_TRY(check_axes_data(P, axes, data, n, &na, span));
    TmpDev daxes, ddata;
    HIP_TRY(hipMalloc(&daxes.p, na * sizeof(double)));
    HIP_TRY(hipMalloc(&ddata.p, size_t(std::max<int64_t>(n * p, 1)) * sizeof(double)));
    HIP_TRY(hipMalloc(&key.p, size_t(std::max<int64_t>(n, 1)) * sizeof(uint32_t)));
    if (want_idx) HIP_TRY(hipMalloc(&idx.p, size_t(std::max<int64_t>(n, 1)) * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(daxes.p, axes, na * sizeof(double), hipMemcpyHostToDevice, P->stream));
    if (n > 0)
        HIP_TRY(hipMemcpyAsync(ddata.p, data, size_t(n * p) * sizeof(double), hipMemcpyHostToDevice, P->stream));
    uint32_t m[MVTV_MAX_DIMS];
    for (int j = 0; j < p; ++j) m[j] = P->g.m[j];
    HIP_TRY(launch_nearest(P->stream, p, m, daxes.get<double>(), span, ddata.get<double>(), n, key.get<uint32_t>(),
                           want_idx ? idx.get<int64_t>() : nullptr));
    HIP_TRY(hipStreamSynchronize(P->stream));   // the temporaries above go out of scope
    return MVTV_OK;
}
}  // namespace

extern "C" {

mvtv_status mvtv_nearest(mvtv_problem* P, const double* axes, const double* data, int64_t n, int64_t* mesh_index_out) {
    if (!P || !axes || n < 0 || (n > 0 && (!data || !mesh_index_out))) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    TmpDev key, idx;
    MVTV_TRY(nearest_on_device(P, axes, data, n, key, idx, true));
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(mesh_index_out, idx.p, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
    }
    return MVTV_OK;
}

mvtv_status mvtv_problem_set_scattered(mvtv_problem* P, const double* axes, const double* data, int64_t n,
                                       const double* y, int64_t* mesh_index_out) {
    if (!P || !axes || n < 0 || (n > 0 && (!data || !y))) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    TmpDev key, idx, dy, runs;
    MVTV_TRY(nearest_on_device(P, axes, data, n, key, idx, mesh_index_out != nullptr));
    if (mesh_index_out && n > 0)
        HIP_TRY(hipMemcpyAsync(mesh_index_out, idx.p, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipMalloc(&dy.p, size_t(std::max<int64_t>(n, 1)) * sizeof(double)));
    HIP_TRY(hipMalloc(&runs.p, sizeof(unsigned long long)));
    if (n > 0) HIP_TRY(hipMemcpyAsync(dy.p, y, size_t(n) * sizeof(double), hipMemcpyHostToDevice, P->stream));
    if (!P->wdiag) MVTV_TRY(alloc(&P->wdiag, P->g.N));
    HIP_TRY(launch_scatter_sums(P->stream, key.get<uint32_t>(), dy.get<double>(), n, P->g.N, P->oty, P->wdiag,
                                runs.get<unsigned long long>()));
    unsigned long long hit = 0;
    HIP_TRY(hipMemcpy(&hit, runs.p, sizeof(hit), hipMemcpyDeviceToHost));
    // every node exactly one point <=> n == N and N nodes hit: W = I (the spectral solve applies)
    if (uint64_t(n) == uint64_t(P->g.N) && hit == uint64_t(P->g.N)) {
        P->wmode = W_IDENTITY;
        P->wmean = 1.0;
        P->wstd = 0.0;
    } else {
        P->wmode = W_DIAG;
        P->wmean = double(n) / double(P->g.N);
        std::vector<double> w(P->g.N);   // std(W) for the preconditioner choice (setup path)
        HIP_TRY(hipMemcpy(w.data(), P->wdiag, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToHost));
        double acc2 = 0.0;
        for (double v : w) acc2 += (v - P->wmean) * (v - P->wmean);
        P->wstd = std::sqrt(acc2 / double(P->g.N));
    }
    return MVTV_OK;
}

mvtv_status mvtv_predict(mvtv_problem* P, const double* axes, const double* data, int64_t n, double* fits) {
    if (!P || !axes || n < 0 || (n > 0 && (!data || !fits))) return fail(MVTV_BAD_ARG, "null argument");
    if (n == 0) return MVTV_OK;
    DeviceGuard dg(P->device);
    TmpDev key, idx, out;
    MVTV_TRY(nearest_on_device(P, axes, data, n, key, idx, true));
    HIP_TRY(hipMalloc(&out.p, size_t(n) * sizeof(double)));
    HIP_TRY(launch_gather_index(P->stream, P->theta, idx.get<int64_t>(), n, out.get<double>()));
    HIP_TRY(hipMemcpyAsync(fits, out.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    return MVTV_OK;
}

// mbs_impl's whole CV for a batch-admitted mesh (rcpp…/solvers.cpp:305-376 without the lambda selection): one upload
// of the data, every member set up and scored by the kernels of mvtv_cv.hip, the paths by mvtv_path_batch's loop
// (batch_loop), one download.
mvtv_status mvtv_cv_batch(mvtv_problem* P, const mvtv_admm_opts* opts, const double* axes, const double* data, int64_t n,
                          const double* y, const int32_t* fold, int32_t folds, const double* ref, const double* lambdas,
                          int32_t n_lambda, const double* theta0, double rho_init, double* mse_mat_out,
                          double* model_mses_out, double* thetas_out, double* fold_thetas_out, double* rhos_out,
                          int64_t* mesh_index_out, mvtv_admm_stats* stats) {
    if (!P || !opts || !axes || !data || !y || !lambdas || !mse_mat_out) return fail(MVTV_BAD_ARG, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    const mvtv_admm_opts& o = *opts;
    const int32_t nf = folds >= 2 ? folds : 0;   // fold members
    MVTV_TRY(batch_check(P, o, 1 + int64_t(nf), n_lambda));
    if (n < 1 || uint64_t(n) >= (uint64_t(1) << 32)) return fail(MVTV_BAD_ARG, "cv_batch: n must be in [1, 2^32)");
    if (nf > 0 && !fold) return fail(MVTV_BAD_ARG, "cv_batch: folds >= 2 needs the fold labels");
    if (int64_t(nf) > n) return fail(MVTV_BAD_ARG, "cv_batch: a fold has no test point");
    const size_t N = P->g.N, B = 1 + size_t(nf), NL = size_t(n_lambda), F = std::max<size_t>(nf, 1);
    if (B * NL > (size_t(1) << 30)) return fail(MVTV_BAD_ARG, "cv_batch: more than 2^30 (member, lambda) pairs");
    for (size_t i = 0; i < NL; ++i)
        if (!(lambdas[i] >= 0.0)) return fail(MVTV_BAD_ARG, "lambda must be >= 0");
    const double rho0 = std::isnan(rho_init) ? lambdas[0] / 5.0 : rho_init;   // rcpp…/solvers.cpp:209
    if (!(rho0 > 0.0) || std::isinf(rho0)) return fail(MVTV_BAD_ARG, "rho_init must be positive and finite");
    std::vector<int64_t> ntest(F, 0);
    for (int64_t i = 0; nf > 0 && i < n; ++i) {
        if (fold[i] < 0 || fold[i] >= nf) return fail(MVTV_BAD_ARG, "cv_batch: a fold label outside [0, folds)");
        ++ntest[size_t(fold[i])];
    }
    for (int32_t f = 0; f < nf; ++f) {
        if (ntest[size_t(f)] == 0) return fail(MVTV_BAD_ARG, "cv_batch: a fold has no test point");
        if (ntest[size_t(f)] == n) return fail(MVTV_BAD_ARG, "cv_batch: a member has no training point");
    }
    const int p = P->g.p;
    size_t na = 0;
    double span[MVTV_MAX_DIMS] = {0, 0, 0, 0};
    MVTV_TRY(check_axes_data(P, axes, data, n, &na, span));
    // every member's constant start: the caller's, or the mean of its y summed in data order
    std::vector<double> th0(B);
    for (size_t b = 0; b < B; ++b) {
        if (theta0) {
            th0[b] = theta0[b];
            continue;
        }
        double sum = 0.0;
        for (int64_t i = 0; i < n; ++i)
            if (b == 0 || fold[i] != int32_t(b) - 1) sum += y[i];
        th0[b] = sum / double(b == 0 ? n : n - ntest[b - 1]);
    }
    const std::vector<double> rho(B, rho0);
    std::vector<double> lam(B * NL);
    for (size_t b = 0; b < B; ++b) std::copy(lambdas, lambdas + NL, lam.begin() + b * NL);
    const int cosm = P->batch_cos;
    DeviceGuard dg(P->device);
    if (cosm > 0) MVTV_TRY(cos_plan_setup(P));
    size_t tmp_bytes = 0;
    HIP_TRY(cv_sort_temp_bytes(n, P->g.N, &tmp_bytes));
    BatchDev d;
    double *d_axes = nullptr, *d_data = nullptr, *d_y = nullptr, *d_ref = nullptr, *d_th0 = nullptr, *d_mse = nullptr,
           *d_mmse = nullptr;
    int32_t* d_fold = nullptr;
    uint32_t *d_key = nullptr, *d_pos = nullptr, *d_key2 = nullptr, *d_pos2 = nullptr;
    int64_t* d_idx = nullptr;
    char* d_tmp = nullptr;
    BatchArena ar{P};
    batch_arena_add(ar, d, P, B, NL, true, true);
    ar.add(&d_axes, na);
    ar.add(&d_data, size_t(n) * size_t(p));
    ar.add(&d_y, size_t(n));
    if (ref) ar.add(&d_ref, size_t(n));
    if (nf > 0) ar.add(&d_fold, size_t(n));
    ar.add(&d_th0, B);
    ar.add(&d_mse, NL * F);
    ar.add(&d_mmse, NL);
    ar.add(&d_key, size_t(n));
    ar.add(&d_pos, size_t(n));
    ar.add(&d_key2, size_t(n));
    ar.add(&d_pos2, size_t(n));
    ar.add(&d_idx, size_t(n));
    ar.add(&d_tmp, tmp_bytes);
    MVTV_TRY(ar.commit());
    hipStream_t s = P->stream;
    // inputs up, once
    HIP_TRY(hipMemcpyAsync(d_axes, axes, na * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_data, data, size_t(n) * size_t(p) * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_y, y, size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
    if (ref) HIP_TRY(hipMemcpyAsync(d_ref, ref, size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
    if (nf > 0) HIP_TRY(hipMemcpyAsync(d_fold, fold, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_th0, th0.data(), B * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.lam, lam.data(), B * NL * sizeof(double), hipMemcpyHostToDevice, s));
    // member setup: the nearest-node map once, one stable sort, every member's O^T y and W, theta_0
    uint32_t m[MVTV_MAX_DIMS];
    for (int j = 0; j < p; ++j) m[j] = P->g.m[j];
    HIP_TRY(launch_cv_fill(s, d_pos, n, d_th0, d.theta, P->g.N, int32_t(B)));
    HIP_TRY(launch_nearest(s, p, m, d_axes, span, d_data, n, d_key, d_idx));
    HIP_TRY(launch_cv_fold_sums(s, d_key, d_pos, d_key2, d_pos2, d_tmp, tmp_bytes, d_y, d_fold, n, P->g.N, int32_t(B),
                                d.oty, d.w));
    // the cosine modes' member data from the host scan of mvtv_path_batch over the W just built
    std::vector<int32_t> kind;
    std::vector<double> wstat, w_host;
    bool has[3];
    if (cosm > 0) {
        w_host.resize(B * N);
        HIP_TRY(hipMemcpyAsync(w_host.data(), d.w, B * N * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        MVTV_TRY(batch_scan_w(w_host.data(), B, N, cosm, kind, wstat));
    }
    MVTV_TRY(batch_kinds(P, o, kind, has));
    BatchHostState hs;
    MVTV_TRY(batch_upload_state(P, d, B, NL, rho.data(), kind, wstat, hs));
    MVTV_TRY(batch_loop(P, o, int32_t(B), n_lambda, d, has));
    HIP_TRY(launch_cv_mse(s, d.thetas, d_idx, d_y, ref ? d_ref : d_y, d_fold, n, P->g.N, n_lambda, int32_t(B), d_mse,
                          d_mmse));
    // one download
    std::vector<SmallCtl> log(B * NL);
    HIP_TRY(hipMemcpyAsync(log.data(), d.log, B * NL * sizeof(SmallCtl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mse_mat_out, d_mse, NL * F * sizeof(double), hipMemcpyDeviceToHost, s));
    if (model_mses_out) HIP_TRY(hipMemcpyAsync(model_mses_out, d_mmse, NL * sizeof(double), hipMemcpyDeviceToHost, s));
    if (thetas_out) HIP_TRY(hipMemcpyAsync(thetas_out, d.thetas, NL * N * sizeof(double), hipMemcpyDeviceToHost, s));
    if (fold_thetas_out && nf > 0)
        HIP_TRY(hipMemcpyAsync(fold_thetas_out, d.thetas + NL * N, size_t(nf) * NL * N * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    if (mesh_index_out) HIP_TRY(hipMemcpyAsync(mesh_index_out, d_idx, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return batch_stats(P, log, NL, kind, seconds, rhos_out, stats);
}

// ------------------------------------------------------------------------------ operators
mvtv_status mvtv_apply_D(mvtv_problem* P, const double* theta, double* d_out) {
    if (!P || !theta || !d_out) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    double *x = nullptr, *e = nullptr;
    MVTV_TRY(alloc(&x, P->g.N));
    mvtv_status s = alloc(&e, size_t(P->g.nb) * P->g.N);
    if (s == MVTV_OK) {
        if (hipMemcpyAsync(x, theta, size_t(P->g.N) * sizeof(double), hipMemcpyHostToDevice, P->stream) != hipSuccess ||
            launch_apply_D_padded(P->g, P->order, P->L(), x, e) != hipSuccess)
            s = fail(MVTV_HIP_ERROR, "apply_D");
        if (s == MVTV_OK) s = export_edges(P, e, d_out, U_EXPLICIT, 0.0, 1.0);
    }
    (void)hipFree(x);
    if (e) (void)hipFree(e);
    return s;
}

mvtv_status mvtv_apply_Dt(mvtv_problem* P, const double* v, double* g_out) {
    if (!P || !v || !g_out) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    double *gq = nullptr, *e = nullptr;
    MVTV_TRY(alloc(&gq, P->g.N));
    mvtv_status s = alloc(&e, size_t(P->g.nb) * P->g.N);
    if (s == MVTV_OK) s = import_edges(P, v, e);
    if (s == MVTV_OK) {
        if (launch_gather(P->g, P->order, U_EXPLICIT, P->L(), e, 0.0, nullptr, gq, nullptr, 1.0, P->partials) != hipSuccess ||
            hipMemcpyAsync(g_out, gq, size_t(P->g.N) * sizeof(double), hipMemcpyDeviceToHost, P->stream) != hipSuccess ||
            hipStreamSynchronize(P->stream) != hipSuccess)
            s = fail(MVTV_HIP_ERROR, "apply_Dt");
    }
    (void)hipFree(gq);
    if (e) (void)hipFree(e);
    return s;
}

mvtv_status mvtv_apply_A(mvtv_problem* P, double sigma, const double* x, double* q_out) {
    if (!P || !x || !q_out) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    double *dx = nullptr, *dq = nullptr;
    MVTV_TRY(alloc(&dx, P->g.N));
    mvtv_status s = alloc(&dq, P->g.N);
    if (s == MVTV_OK) {
        const size_t bytes = size_t(P->g.N) * sizeof(double);
        if (hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, P->stream) != hipSuccess ||
            launch_apply_A(P->g, P->L(), sigma, P->wmode, P->wdiag, dx, dq, nullptr, nullptr) != hipSuccess ||
            hipMemcpyAsync(q_out, dq, bytes, hipMemcpyDeviceToHost, P->stream) != hipSuccess ||
            hipStreamSynchronize(P->stream) != hipSuccess)
            s = fail(MVTV_HIP_ERROR, "apply_A");
    }
    (void)hipFree(dx);
    if (dq) (void)hipFree(dq);
    return s;
}

mvtv_status mvtv_solve(mvtv_problem* P, double sigma, const double* b, double* x_inout, double rtol, int32_t max_iter,
                       int32_t* iters, double* relres) {
    if (!P || !b || !x_inout) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    double *db = nullptr, *dx = nullptr;
    MVTV_TRY(alloc(&db, P->g.N));
    mvtv_status s = alloc(&dx, P->g.N);
    int it = 0;
    double rr = 0.0;
    if (s == MVTV_OK) {
        const size_t bytes = size_t(P->g.N) * sizeof(double);
        if (hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, P->stream) != hipSuccess ||
            hipMemcpyAsync(dx, x_inout, bytes, hipMemcpyHostToDevice, P->stream) != hipSuccess)
            s = fail(MVTV_HIP_ERROR, "solve upload");
        if (s == MVTV_OK)
            s = pcg_solve(P, sigma, db, db, 0.0, db, 0.0, dx, rtol > 0 ? rtol : 1e-10, max_iter > 0 ? max_iter : 20000,
                          &it, &rr);
        if (s == MVTV_OK && (hipMemcpyAsync(x_inout, dx, bytes, hipMemcpyDeviceToHost, P->stream) != hipSuccess ||
                             hipStreamSynchronize(P->stream) != hipSuccess))
            s = fail(MVTV_HIP_ERROR, "solve download");
    }
    if (iters) *iters = it;
    if (relres) *relres = rr;
    (void)hipFree(db);
    if (dx) (void)hipFree(dx);
    return s;
}

mvtv_status mvtv_lambda_max(mvtv_problem* P, double* out, int32_t* iters) {
    if (!P || !out) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    const Launch L = P->L();
    const size_t bytes = size_t(P->g.N) * sizeof(double);
    // scratch: x, d, r, p, t (the PCG buffers; the ADMM state theta / edges is untouched)
    if (!P->p2) MVTV_TRY(alloc(&P->p2, P->g.N));
    if (!P->thold) MVTV_TRY(alloc(&P->thold, P->g.N));
    double *x = P->thold, *d = P->r, *r = P->q, *p = P->p, *t = P->p2;
    auto dot = [&](double* v, double* res) -> mvtv_status {
        HIP_TRY(launch_cg_vec(P->g, L, 0, 0.0, v, nullptr, nullptr, nullptr, P->partials));
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 0, 0, P->red, P->st));
        HIP_TRY(hipMemcpyAsync(P->host_red, P->red, sizeof(double), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        *res = P->host_red[0];
        return MVTV_OK;
    };
    auto AtA = [&](const double* v, double* outv) -> mvtv_status {   // crossD * v (W = 0, sigma = 1)
        HIP_TRY(launch_apply_A(P->g, L, 1.0, W_NONE, nullptr, v, outv, nullptr, nullptr));
        return MVTV_OK;
    };
    // cg(ata, Oty) of rcpp…/utils.cpp:306-341, line by line
    HIP_TRY(hipMemsetAsync(x, 0, bytes, P->stream));
    HIP_TRY(hipMemcpyAsync(d, P->oty, bytes, hipMemcpyDeviceToDevice, P->stream));   // d = b - A x, x = 0
    MVTV_TRY(AtA(d, r));                                                             // r = A^T d
    HIP_TRY(hipMemcpyAsync(p, r, bytes, hipMemcpyDeviceToDevice, P->stream));
    double rr = 0.0;
    MVTV_TRY(dot(r, &rr));
    const double rsold0 = std::sqrt(rr);
    double rsold = std::pow(rsold0, 2), rsnew = rsold + 1.0;
    MVTV_TRY(AtA(p, t));
    int iter = 0;
    const int MAXIT = P->g.N < 2000 ? int(P->g.N) : 2000;
    while (std::sqrt(rsnew) >= 0.0001 * rsold0) {
        double tt = 0.0;
        MVTV_TRY(dot(t, &tt));
        const double alpha = rsold / std::pow(std::sqrt(tt), 2);
        HIP_TRY(launch_cg_vec(P->g, L, 1, alpha, x, d, p, t, nullptr));
        MVTV_TRY(AtA(d, r));
        MVTV_TRY(dot(r, &rr));
        rsnew = std::pow(std::sqrt(rr), 2);
        iter += 1;
        if (iter == MAXIT) break;
        HIP_TRY(launch_cg_vec(P->g, L, 2, rsnew / rsold, p, nullptr, r, nullptr, nullptr));   // p = r + beta p
        MVTV_TRY(AtA(p, t));
        rsold = rsnew;
    }
    // 5 * ||D x||_inf (lam_max_pinv, :351-355)
    HIP_TRY(launch_dmaxabs(P->g, P->order, L, x, P->partials));
    HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 1, 0, P->red, P->st));
    HIP_TRY(hipMemcpyAsync(P->host_red, P->red, sizeof(double), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    *out = 5.0 * P->host_red[0];
    if (iters) *iters = iter;
    return MVTV_OK;
}

mvtv_status mvtv_lambda_max_cpp(mvtv_problem* P, double* out, int32_t* iters) {
    if (!P || !out) return fail(MVTV_BAD_ARG, "null argument");
    DeviceGuard dg(P->device);
    const Launch L = P->L();
    const size_t n = P->g.N, bytes = n * sizeof(double);
    if (!P->p2) MVTV_TRY(alloc(&P->p2, n));
    if (!P->thold) MVTV_TRY(alloc(&P->thold, n));
    double *x = P->thold, *r = P->r, *p = P->p, *ap = P->p2;
    auto reduce1 = [&](double* res) -> mvtv_status {   // the one partial sum in P->partials
        HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 0, 0, P->red, P->st));
        HIP_TRY(hipMemcpyAsync(P->host_red, P->red, sizeof(double), hipMemcpyDeviceToHost, P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        *res = P->host_red[0];
        return MVTV_OK;
    };
    // cg(ata, Oty) of cpp-code/utils.cpp:354-386: x = mean(b), r = b - A x, p = r, absolute stop
    // ||r|| < 0.01, at most 500 iterations when N < 400 and 100 otherwise
    std::vector<double> hb(n);
    HIP_TRY(hipMemcpyAsync(hb.data(), P->oty, bytes, hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    double sum = 0.0;
    for (double v : hb) sum += v;
    HIP_TRY(launch_fill(P->stream, x, sum / double(n), n));
    HIP_TRY(launch_apply_A(P->g, L, 1.0, W_NONE, nullptr, x, ap, nullptr, nullptr));   // A x
    HIP_TRY(hipMemcpyAsync(r, P->oty, bytes, hipMemcpyDeviceToDevice, P->stream));
    HIP_TRY(launch_cg_vec(P->g, L, 3, 1.0, nullptr, r, nullptr, ap, nullptr));          // r = b - A x
    HIP_TRY(hipMemcpyAsync(p, r, bytes, hipMemcpyDeviceToDevice, P->stream));
    double rsold = 0.0;
    HIP_TRY(launch_cg_vec(P->g, L, 0, 0.0, r, nullptr, nullptr, nullptr, P->partials));
    MVTV_TRY(reduce1(&rsold));
    double rsnew = rsold + 1.0;
    const int MAXIT = n < 400 ? 500 : 100;
    int iter = 0;
    while (std::sqrt(rsnew) >= 0.01) {
        double pap = 0.0;   // Ap = A p, p.Ap
        HIP_TRY(launch_apply_A(P->g, L, 1.0, W_NONE, nullptr, p, ap, P->partials, nullptr));
        MVTV_TRY(reduce1(&pap));
        const double alpha = rsold / pap;
        HIP_TRY(launch_cg_vec(P->g, L, 1, alpha, x, r, p, ap, nullptr));                // x += a p, r -= a Ap
        HIP_TRY(launch_cg_vec(P->g, L, 0, 0.0, r, nullptr, nullptr, nullptr, P->partials));
        MVTV_TRY(reduce1(&rsnew));
        iter += 1;
        if (iter == MAXIT) break;
        HIP_TRY(launch_cg_vec(P->g, L, 2, rsnew / rsold, p, nullptr, r, nullptr, nullptr));   // p = r + beta p
        rsold = rsnew;
    }
    // lam_max_pinv (:399-404): max |D x|, no factor
    HIP_TRY(launch_dmaxabs(P->g, P->order, L, x, P->partials));
    HIP_TRY(launch_finalize(P->stream, P->partials, L.grid, 1, 1, 0, P->red, P->st));
    HIP_TRY(hipMemcpyAsync(P->host_red, P->red, sizeof(double), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    *out = P->host_red[0];
    if (iters) *iters = iter;
    return MVTV_OK;
}

mvtv_status mvtv_solve_spectral(mvtv_problem* P, double sigma, const double* b, double* x_out) {
    if (!P || !b || !x_out) return fail(MVTV_BAD_ARG, "null argument");
    if (!spectral_ok(P)) return fail(MVTV_BAD_ARG, "spectral theta-solve needs W = I and every m_j, j < p - 1, <= 4096 or a product of two 2-3-5-7-smooth factors <= 4096");
    DeviceGuard dg(P->device);
    double* dx = nullptr;
    MVTV_TRY(alloc(&dx, P->g.N));
    const size_t bytes = size_t(P->g.N) * sizeof(double);
    mvtv_status s = MVTV_OK;
    if (hipMemcpyAsync(dx, b, bytes, hipMemcpyHostToDevice, P->stream) != hipSuccess)
        s = fail(MVTV_HIP_ERROR, "solve upload");
    if (s == MVTV_OK) s = spectral_solve(P, sigma, dx, nullptr, 0.0, nullptr, 0.0, dx);
    if (s == MVTV_OK && (hipMemcpyAsync(x_out, dx, bytes, hipMemcpyDeviceToHost, P->stream) != hipSuccess ||
                         hipStreamSynchronize(P->stream) != hipSuccess))
        s = fail(MVTV_HIP_ERROR, "solve download");
    (void)hipFree(dx);
    return s;
}

mvtv_status mvtv_sync(mvtv_problem* P) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    return P->sync();
}

// ------------------------------------------------------------------------------ instrumentation
mvtv_status mvtv_timing_enable(mvtv_problem* P, int32_t on) {
    if (!P) return fail(MVTV_BAD_ARG, "null problem");
    DeviceGuard dg(P->device);
    MVTV_TRY(P->sync());
    P->timing = on != 0;
    for (int k = 0; k < MVTV_K_COUNT; ++k) {
        P->ms[k] = 0.0;
        P->launches[k] = 0;
    }
    P->fold_fix = 0;
    P->pcg_xmoves = 0;
    return MVTV_OK;
}

mvtv_status mvtv_timing_get(mvtv_problem* P, int32_t kid, double* total_ms, int64_t* launches, double* bytes) {
    if (!P || kid < 0 || kid >= MVTV_K_COUNT) return fail(MVTV_BAD_ARG, "kernel id");
    DeviceGuard dg(P->device);
    MVTV_TRY(P->sync());
    double N = double(P->g.N), E = double(P->E);
    const double w = P->wmode == W_DIAG ? 1.0 : 0.0;
    double own = 1.0;
    if (P->slab) {   // a slab rank's kernels work on its owned planes (ghost planes are read only as halos)
        own = double(P->ze - P->zb) / double(P->g.m[P->g.p - 1]);
        N *= own;
        E *= own;
    }
    // algorithmic bytes per launch (each array element read or written once)
    double b = 0.0;
    switch (kid) {
        case MVTV_K_EDGE_UPDATE: b = 8.0 * (N + 2.0 * E); break;        // theta in, z in/out
        case MVTV_K_GATHER:   // z in, g_uprev in, g_alpha/g_u out; 4-D two-pass: z in, 4 partial sums out
            b = P->g4 ? 8.0 * (E + 4.0 * N) : 8.0 * (E + 3.0 * N);
            break;
        case MVTV_K_GATHER4B: b = 8.0 * 7.0 * N; break;                // 4 partial sums, g_uprev in; g_alpha/g_u out
        case MVTV_K_PCG_INIT:   // classic: oty, ga, gb, x (+W) in, r, p out; fused 3-D: r out only
            b = 8.0 * (((P->g.p == 3 && P->fused3d) ? 5.0 : 6.0) + w) * N;
            break;
        case MVTV_K_PCG_APPLY: b = 8.0 * ((2.0 + w) * N); break;        // p (+W) in, q out
        case MVTV_K_PCG_UPDATE: b = 8.0 * ((6.0 + w) * N); break;       // x, r, p, q (+W) in, x, r out
        case MVTV_K_PCG_DIRECTION: b = 8.0 * ((3.0 + w) * N); break;    // r, p (+W) in, p out
        case MVTV_K_PCG_FUSED:   // r, p (+W) in, r, p out; + x in/out in the odd iterations (mean over the launches)
            b = 8.0 * N * (4.0 + w + (P->launches[kid] > 0 ? 2.0 * double(P->pcg_xmoves) / double(P->launches[kid]) : 0.0));
            break;
        case MVTV_K_DCT_FIRST: b = 8.0 * 4.0 * N; break;                 // oty, g_alpha, g_u in, x out
        case MVTV_K_DCT_FOLD:   // oty, s in, x out; + g_u in the launches after a rho change (mean over the launches)
            b = 8.0 * N * (3.0 + (P->launches[kid] > 0 ? double(P->fold_fix) / double(P->launches[kid]) : 0.0));
            break;
        case MVTV_K_DCT: b = 8.0 * 2.0 * N; break;                       // x in, x out
        case MVTV_K_ADMM_FUSED:   // theta, z, g_uprev in; z', g_alpha, g_u out (z without its twin blocks: twin_timed)
            b = 8.0 * (4.0 * N + 2.0 * (P->twin_timed ? E - twin_edges(P) * own : E));
            break;
        case MVTV_K_ADMM_FUSED4:   // theta, z in; z', 4 pass-A sums out (z without its twin blocks: twin_timed)
            b = 8.0 * (5.0 * N + 2.0 * (P->twin_timed ? E - twin_edges(P) * own : E));
            break;
        default: b = 0.0;
    }
    if (total_ms) *total_ms = P->ms[kid];
    if (launches) *launches = P->launches[kid];
    if (bytes) *bytes = b;
    return MVTV_OK;
}

const char* mvtv_kernel_name(int32_t kid) {
    static const char* names[MVTV_K_COUNT] = {"edge_update", "gather_Dt", "pcg_init", "pcg_apply_A",
                                               "pcg_update", "pcg_direction", "reduce", "other", "pcg_fused3d",
                                               "dct_first", "dct", "admm_fused", "gather4_b", "dct_first_fold",
                                               "admm_fused4"};
    return (kid >= 0 && kid < MVTV_K_COUNT) ? names[kid] : "?";
}

void mvtv_launch_log_enable(int32_t on) {
    // the ring's owner: freed here on disable, or at thread exit if the thread ends with the log on (g_launch_log
    // itself stays trivially destructible, so klaunch's flag test needs no thread-local init guard)
    static thread_local std::unique_ptr<LaunchRec[]> ring;
    LaunchLog& L = g_launch_log;
    L.on = false;
    L.count = 0;
    if (on && !ring) ring.reset(new LaunchRec[kLaunchLogCap]);
    if (!on) ring.reset();
    L.ring = ring.get();
    L.on = on != 0;
}

int64_t mvtv_launch_log_read(char* buf, int64_t cap) {
    const LaunchLog& L = g_launch_log;
    std::string out;
    if (L.ring) {
        const uint64_t first = L.count > kLaunchLogCap ? L.count - kLaunchLogCap : 0;
        if (first) out += "# " + std::to_string(first) + " earlier launches dropped\n";
        for (uint64_t i = first; i < L.count; ++i) {
            const LaunchRec& r = L.ring[i % kLaunchLogCap];
            out += kernel_display_name(r.fn);
            char dims[128];
            std::snprintf(dims, sizeof dims, "\t%u %u %u\t%u %u %u\n", r.grid[0], r.grid[1], r.grid[2], r.block[0],
                          r.block[1], r.block[2]);
            out += dims;
        }
    }
    if (buf && cap > 0) {
        const size_t n = std::min(out.size(), size_t(cap - 1));
        std::memcpy(buf, out.data(), n);
        buf[n] = '\0';
    }
    return int64_t(out.size());
}

}  // extern "C"
