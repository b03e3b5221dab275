// mvtv_spectral.hip — exact theta-solve by fast cosine transforms (W = I, power-of-two meshes).
//
// The reference solves (O^T O + rho D^T D) theta = b with SuperLU every ADMM iteration
// (rcpp-code/MultivarTV/src/solvers.cpp:113; cpp-code/solvers.cpp:116). On a mesh fit
// (mesh == data, O = I) that matrix is a sum of Kronecker products of 1-D Neumann Laplacians
// (SURVEY Appendix A):
//
//     A = I + sigma * sum_S cS[S] (x)_{j in S} L_j,      L_j = D1^T D1 (m_j x m_j)
//
// and every L_j is diagonalised by the DCT-II: L_j = C^T diag(lam_j) C with
// lam_j(k) = 4 sin^2(pi k / (2 m_j)). So A^-1 b = IDCT( DCT(b) / mu ), with
// mu(k) = 1 + sigma * sum_S cS[S] prod_{j in S} lam_j(k_j): a direct solve, exact to
// rounding, in 2p - 1 streaming passes over the mesh instead of K PCG iterations.
//
// One pass transforms every line of the mesh along one dimension d. A workgroup owns TQ
// lines (TQ consecutive line indices: for d > 0 they are TQ adjacent dim-0 cells, so every
// line position is a contiguous 8*TQ-byte row and loads are coalesced; for d = 0 each line
// is contiguous itself). Lines are paired as the real and imaginary parts of one complex
// sequence, so a length-m real DCT costs half a length-m complex FFT:
//
//   forward (DCT-II, Makhoul):  v[n] = x[2n], v[m-1-n] = x[2n+1];  Z = FFT(v_a + i v_b)
//                               A = (Z[k] + conj Z[m-k]) / 2, B = (Z[k] - conj Z[m-k]) / 2i
//                               X[k] = Re(e^{-i pi k/2m} A[k])   (same for B)
//   inverse (DCT-III):          V[k] = e^{i pi k/2m} (X[k] - i X[m-k]),  X[m] = 0
//                               v_a + i v_b = IFFT(V_a + i V_b), un-permute
//
// The FFT runs in LDS: radix-2^2 in-place stages, decimation in time on input loaded in
// bit-reversed order (forward), decimation in frequency leaving bit-reversed output (inverse),
// so both permutations fold into the global load/store index. The pass along the last
// dimension does forward, the divide by mu (and the 1/N of the inverse transforms) and the
// inverse in one launch. The first pass forms b = oty + ca*ga + cb*gb on load.
//
// HBM traffic per solve: 8 * (4N + 2N*(2p - 2)) bytes = 12N words at p = 3 (against 6N words
// per fused PCG iteration x ~44 iterations).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "mvtv_device.h"

namespace mvtv {

namespace spec {
constexpr int NT = 256;               // threads per workgroup
constexpr int LDS_WORDS = 8192;       // real doubles per workgroup tile (64 KB): TQ * m <= 8192
constexpr int PAD = 1;                // complex slots of padding per line (bank spread)
}  // namespace spec

struct SpecArgs {
    const double* in;        // input lines (FORMB: oty)
    const double* ga;        // FORMB: b = in + ca * ga + cb * gb
    const double* gb;
    double ca, cb;
    double* out;
    const double2* tw;       // FFT twiddles e^{-2 pi i k / m}, k < m/2
    const double2* twq;      // quarter-wave twiddles e^{-i pi k / 2m}, k < m
    const double* lam;       // MID: per-dim eigenvalue tables, lam + lam_off[j]
    uint32_t lam_off[kMaxDims];
    uint32_t m[kMaxDims];
    FastDiv fd[kMaxDims - 1];
    double cS[16];
    double sigma, w0, inv_n;
    uint32_t stride;         // element stride along the line (1 for d = 0)
    uint32_t nlines;         // N / m
    int32_t d, p, L, tq;     // line dimension, dims, log2 m, lines per workgroup
    int32_t ls;              // log2 stride
    uint32_t q_off;          // MID: global index of line 0
    const int32_t* skip;     // != nullptr and *skip: return at once (preconditioner of a converged PCG)
    const AdmmCtl* ctl;      // asynchronous ADMM loop: sigma, ca = rho, cb = rho c_prev from the device
    // mixed-radix lengths (k_dctg): the FFT's radices in stage order, division by the line stride
    int32_t nrad;
    int32_t rad[8];
    FastDiv fds;              // division by the line stride
    FastDiv fm;               // division by m
    FastDiv fper[8], fL[8];   // stage s: butterflies per line (m / rad[s]) and the span before it
    const uint32_t* perm;     // position of sample k in the digit-reversed Makhoul order (this dim)
    int32_t xcd;              // k_dct8: tiles dealt to the XCDs in contiguous runs (grid a multiple of 8)
    int32_t xrun;             // k_dctg / k_dctm / k_dctb8 / k_trigr: the same for any grid (xcd_run)
    PcgFuse pf;               // k_dct8 PC = 1 / 2: the PCG vector work of the preconditioner's d = 0 passes
    int32_t fold;             // FORMB from the folded s (k_dct8, ctl): b = in + fold_ka ga [+ fold_kb gb if ctl->fix]
    int32_t pair16;           // k_dct8 d = 0 forward / inverse: coefficients through LDS as 16-B pairs (dct_pair16)
    // Bluestein lengths (k_dctb8; L = log2 M then, tw = the length-M FFT twiddles): the chirp c[n] = e^{-i pi n^2/m}
    // and the transforms / M of the forward / inverse convolution kernels
    const double2* bchirp;
    const double2* bvf;
    const double2* bvi;
};

// Workgroup b of G runs on XCD b % 8. The tile it takes when the tiles are dealt to the XCDs in contiguous runs, for
// any G (XCD x takes G / 8 tiles, one more when x < G % 8): the tiles that share the 128-B lines of a strided row —
// a line pitch that is not a multiple of 128 B (500, 251, 100 points ...) — are then read through one L2 instead of
// two, where round-robin dealing put neighbouring tiles on different XCDs and each straddled line came from HBM twice
__device__ __forceinline__ uint32_t xcd_run(uint32_t b, uint32_t G) {
    const uint32_t x = b & 7u, i = b >> 3, q = G >> 3, r = G & 7u;
    return x * q + (x < r ? x : r) + i;
}

enum SpecMode { SPEC_FWD = 0, SPEC_INV = 1, SPEC_MID = 2 };

typedef double dvec2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ldnt2(const double* p) {
    const dvec2 v = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(p));
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ void stnt2(double* p, double2 v) {
    dvec2 w;
    w.x = v.x;
    w.y = v.y;
    __builtin_nontemporal_store(w, reinterpret_cast<dvec2*>(p));
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }
// multiply by -i (forward) or +i (inverse)
template <bool INV>
__device__ __forceinline__ double2 crot(double2 a) {
    return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

// Position of DCT input sample k in the bit-reversed Makhoul sequence.
__device__ __forceinline__ uint32_t perm_pos(uint32_t k, uint32_t m, int L) {
    const uint32_t n = (k & 1u) ? m - 1u - (k >> 1) : (k >> 1);
    return L ? (__brev(n) >> (32 - L)) : 0u;
}

// In-place radix-2^2 FFT over ncl complex lines of length m = 2^L at line pitch LP.
// DIT: bit-reversed in, natural out. DIF: natural in, bit-reversed out. INV conjugates twiddles.
template <bool DIF, bool INV>
__device__ __forceinline__ void fft_lines(double2* __restrict__ buf, const double2* __restrict__ tw, int ncl, int L,
                                          int LP) {
    const uint32_t m = 1u << L;
    auto twid = [&](uint32_t k) { return INV ? cconj(tw[k]) : tw[k]; };
    auto radix2 = [&]() {
        const int nb = ncl << (L - 1);
        for (int t = threadIdx.x; t < nb; t += spec::NT) {
            const int line = t >> (L - 1);
            const uint32_t j = uint32_t(t & ((1 << (L - 1)) - 1)) << 1;
            double2* x = buf + line * LP;
            const double2 a = x[j], b = x[j + 1];
            x[j] = cadd(a, b);
            x[j + 1] = csub(a, b);
        }
        __syncthreads();
    };
    if (L < 2) {
        if (L == 1) radix2();
        return;
    }
    const int nbf = ncl << (L - 2);   // radix-4 butterflies per stage
    if (!DIF) {
        uint32_t s = 1;
        if (L & 1) {
            radix2();
            s = 2;
        }
        for (; s < m; s <<= 2) {
            const uint32_t sh2 = m / (2 * s), sh4 = m / (4 * s);
            for (int t = threadIdx.x; t < nbf; t += spec::NT) {
                const int line = t >> (L - 2);
                const uint32_t bf = uint32_t(t & ((1 << (L - 2)) - 1));
                const uint32_t r = bf & (s - 1);
                const uint32_t j = (bf - r) * 4 + r;
                double2* x = buf + line * LP;
                const double2 w1 = twid(r * sh2), w2 = twid(r * sh4);
                const double2 a0 = x[j], a1 = cmul(x[j + s], w1), a2 = x[j + 2 * s], a3 = cmul(x[j + 3 * s], w1);
                const double2 b0 = cadd(a0, a1), b1 = csub(a0, a1), b2 = cadd(a2, a3), b3 = csub(a2, a3);
                const double2 t2 = cmul(w2, b2), t3 = crot<INV>(cmul(w2, b3));
                x[j] = cadd(b0, t2);
                x[j + 2 * s] = csub(b0, t2);
                x[j + s] = cadd(b1, t3);
                x[j + 3 * s] = csub(b1, t3);
            }
            __syncthreads();
        }
    } else {
        for (uint32_t s = m >> 2; s >= 1; s >>= 2) {
            const uint32_t sh2 = m / (2 * s), sh4 = m / (4 * s);
            for (int t = threadIdx.x; t < nbf; t += spec::NT) {
                const int line = t >> (L - 2);
                const uint32_t bf = uint32_t(t & ((1 << (L - 2)) - 1));
                const uint32_t r = bf & (s - 1);
                const uint32_t j = (bf - r) * 4 + r;
                double2* x = buf + line * LP;
                const double2 w4 = twid(r * sh4), w2 = twid(r * sh2);
                const double2 a0 = x[j], a1 = x[j + s], a2 = x[j + 2 * s], a3 = x[j + 3 * s];
                const double2 b0 = cadd(a0, a2), b2 = cmul(csub(a0, a2), w4);
                const double2 b1 = cadd(a1, a3), b3 = crot<INV>(cmul(csub(a1, a3), w4));
                x[j] = cadd(b0, b1);
                x[j + s] = cmul(csub(b0, b1), w2);
                x[j + 2 * s] = cadd(b2, b3);
                x[j + 3 * s] = cmul(csub(b2, b3), w2);
            }
            __syncthreads();
            if (s < 4) break;
        }
        if (L & 1) radix2();
    }
}

// Global element offset of (line ql of the tile starting at line q0, position k).
template <bool D0>
__device__ __forceinline__ uint32_t line_addr(const SpecArgs& a, uint32_t q0, uint32_t ql, uint32_t k) {
    if (D0) return ((q0 + ql) << a.L) + k;
    const uint32_t q = q0 + ql;                 // q0 .. q0+tq-1 lie in one stride block (tq | stride)
    return (q & (a.stride - 1)) + ((q >> a.ls) << (a.ls + a.L)) + (k << a.ls);
}

template <int MODE, bool D0, bool FORMB>
__global__ __launch_bounds__(spec::NT) void k_dct(const SpecArgs a) {
    double sigma = a.sigma, ca = a.ca, cb = a.cb;   // locals: see k_dct8
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
    }
    __shared__ double2 buf[spec::LDS_WORDS / 2 + 8 * spec::PAD];
    __shared__ double lc0[16], lc1[16];     // MID: per-line eigenvalue coefficients
    const int L = a.L;
    const uint32_t m = 1u << L;
    const int tq = a.tq, ncl = tq >> 1;
    const int LP = int(m) + spec::PAD;
    const uint32_t q0 = blockIdx.x * uint32_t(tq);
    const int log2tq = __ffs(tq) - 1;

    if (MODE == SPEC_MID && threadIdx.x < uint32_t(tq)) {
        // line q indexes dims 0..p-2 column-major (d = p - 1): split mu into c0 + c1 * lam_d(k)
        const uint32_t q = a.q_off + q0 + threadIdx.x;
        double lamv[kMaxDims] = {0, 0, 0, 0};
        uint32_t rest = (q - a.q_off) < a.nlines ? q : a.q_off;
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int j = 0; j < a.p; ++j) {
            if (j == a.d) continue;
            const uint32_t qq = (j < jlast) ? a.fd[j].div(rest) : 0u;
            const uint32_t c = rest - qq * a.m[j];
            lamv[j] = a.lam[a.lam_off[j] + c];
            rest = qq;
        }
        double c0 = a.w0, c1 = 0.0;
        const int dbit = 1 << a.d;
        for (int S = 1; S < (1 << a.p); ++S) {
            if (a.cS[S] == 0.0) continue;
            double prod = sigma * a.cS[S];
            for (int j = 0; j < a.p; ++j)
                if (j != a.d && ((S >> j) & 1)) prod *= lamv[j];
            if (S & dbit) c1 += prod;
            else c0 += prod;
        }
        lc0[threadIdx.x] = c0;
        lc1[threadIdx.x] = c1;
    }

    // ---- load (forward: bit-reversed Makhoul order; inverse: natural order) ----------------
    double* bw = reinterpret_cast<double*>(buf);
    const int total = tq << L;
    for (int e = threadIdx.x; e < total; e += spec::NT) {
        uint32_t ql, k;
        if (D0) {
            ql = uint32_t(e) >> L;
            k = uint32_t(e) & (m - 1);
        } else {
            ql = uint32_t(e) & uint32_t(tq - 1);
            k = uint32_t(e) >> log2tq;
        }
        double v = 0.0;
        if (q0 + ql < a.nlines) {
            const uint32_t gi = line_addr<D0>(a, q0, ql, k);
            v = __builtin_nontemporal_load(a.in + gi);
            if (FORMB) v += ca * __builtin_nontemporal_load(a.ga + gi) + cb * __builtin_nontemporal_load(a.gb + gi);
        }
        const uint32_t pos = (MODE == SPEC_INV) ? k : perm_pos(k, m, L);
        bw[2 * ((ql >> 1) * LP + pos) + (ql & 1)] = v;
    }
    __syncthreads();

    if (MODE != SPEC_INV) fft_lines<false, false>(buf, a.tw, ncl, L, LP);

    // ---- spectrum <-> DCT coefficients, paired (k, m-k) in registers ---------------------------
    {
        const uint32_t half = m >> 1;
        const int npairs = ncl << (L - 1);
        for (int t = threadIdx.x; t < npairs; t += spec::NT) {
            const int line = t >> (L - 1);
            const uint32_t k = uint32_t(t) & (half - 1);
            double2* x = buf + line * LP;
            // indices handled by this thread: k and m-k (k >= 1), or the self-pairs 0 and m/2
            const uint32_t ka = k, kb = k ? m - k : half;
            const bool self = (k == 0);
            double2 Xk, Xmk;   // (X_a, X_b) at ka and kb
            if (MODE != SPEC_INV) {
                const double2 Z1 = x[ka], Z2 = x[kb];
                const double2 q1 = a.twq[ka], q2 = a.twq[kb];
                if (self) {
                    // Z[0] and Z[m/2] pair with themselves: A = Re Z, B = Im Z
                    Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                    Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
                } else {
                    const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));   // (Z1 + conj Z2)/2
                    const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));  // (Z1 - conj Z2)/2i
                    // X[k] = Re(q1 A), X[m-k] = Re(q2 conj A)
                    Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                    Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
                }
            } else {
                Xk = x[ka];
                Xmk = x[kb];
            }
            if (MODE == SPEC_MID) {
                const double* lamd = a.lam + a.lam_off[a.d];
                const double la = lamd[ka], lb = lamd[kb];
                const int l0 = 2 * line, l1 = 2 * line + 1;
                Xk.x *= a.inv_n / (lc0[l0] + lc1[l0] * la);
                Xk.y *= a.inv_n / (lc0[l1] + lc1[l1] * la);
                Xmk.x *= a.inv_n / (lc0[l0] + lc1[l0] * lb);
                Xmk.y *= a.inv_n / (lc0[l1] + lc1[l1] * lb);
            }
            if (MODE == SPEC_FWD) {
                x[ka] = Xk;
                x[kb] = Xmk;
                continue;
            }
            // V[k] = conj(q[k]) (X[k] - i X[m-k]); Z = V_a + i V_b
            const double2 q1 = cconj(a.twq[ka]), q2 = cconj(a.twq[kb]);
            double2 Za, Zb;
            if (self) {
                // k = 0: X[m] = 0 -> V = X[0].  k = m/2: V = q (X - i X)
                Za = make_double2(Xk.x, Xk.y);   // V_a[0] = Xa[0], V_b[0] = Xb[0] -> Z = Xa + i Xb
                const double2 va = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                const double2 vb = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                Zb = make_double2(va.x - vb.y, va.y + vb.x);
                x[0] = Za;
                x[half] = Zb;
            } else {
                const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
                const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
                x[ka] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
                x[kb] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            }
        }
        __syncthreads();
    }

    if (MODE != SPEC_FWD) fft_lines<true, true>(buf, a.tw, ncl, L, LP);

    // ---- store (forward: natural order; inverse: un-permute from bit-reversed order) ------------
    for (int e = threadIdx.x; e < total; e += spec::NT) {
        uint32_t ql, k;
        if (D0) {
            ql = uint32_t(e) >> L;
            k = uint32_t(e) & (m - 1);
        } else {
            ql = uint32_t(e) & uint32_t(tq - 1);
            k = uint32_t(e) >> log2tq;
        }
        if (q0 + ql >= a.nlines) continue;
        const uint32_t pos = (MODE == SPEC_FWD) ? k : perm_pos(k, m, L);
        __builtin_nontemporal_store(bw[2 * ((ql >> 1) * LP + pos) + (ql & 1)], a.out + line_addr<D0>(a, q0, ql, k));
    }
}

// =============================================================================================
// Register-radix Stockham version (m >= 8): every thread holds 8 complex values of one complex
// line (two real lines) and runs radix-8 butterflies in registers (one radix-2/4 stage first
// when log2 m is not a multiple of 3); LDS only carries the exchange between stages. The first
// forward stage reads the Makhoul-permuted input straight from HBM and the last inverse stage
// stores the un-permuted output straight to HBM.
//
// Thread -> (complex line c, butterfly column j), j < m/8. For d > 0 lanes run over c first,
// so the two real lines of a complex line are one 16-B access and the 2*NCL lines of a tile
// make one contiguous row per mesh position; for d = 0 lanes run over j (lines are contiguous).
namespace spec8 {
template <int L>
struct Shape {
    static constexpr int M = 1 << L;
    static constexpr int TPL = M / 8;                                     // threads per complex line
    static constexpr int TQ = (8192 / M) < 16 ? (8192 / M) : 16;          // real lines per workgroup
    static constexpr int NCL = TQ / 2;                                    // complex lines per workgroup
    static constexpr int NT = NCL * TPL;
    // line pitch (complex slots): a multiple of 8 plus 8 mod 16, and slot = pidx(pos) ^ (c & 7), so
    // c-fastest lanes (d > 0) hit distinct banks for the 16-B reads (16-lane groups) and writes
    // (8-lane groups); j-fastest lanes (d = 0) are spread by pidx
    static constexpr int LP = (M + M / 8 + 15) / 16 * 16 + 8;
    static constexpr int R0 = (L % 3 == 0) ? 8 : (L % 3 == 1 ? 2 : 4);    // radix of the first stage
};
// kernel-level shape with an optional smaller tile (TQW real lines per workgroup)
template <int L, int TQW>
struct ShapeK : Shape<L> {
    static constexpr int TQ = TQW > 0 ? TQW : Shape<L>::TQ;
    static constexpr int NCL = TQ / 2;
    static constexpr int NT = NCL * Shape<L>::TPL;
};
__device__ __forceinline__ int pidx(int pos) { return pos + (pos >> 3); }   // one pad slot per 8
__device__ __forceinline__ int slot(int pos, int cx) { return pidx(pos) ^ cx; }
}  // namespace spec8

template <bool INV>
__device__ __forceinline__ void fft4r(double2& z0, double2& z1, double2& z2, double2& z3) {
    const double2 t0 = cadd(z0, z2), t1 = csub(z0, z2), t2 = cadd(z1, z3), t3 = crot<INV>(csub(z1, z3));
    z0 = cadd(t0, t2);
    z2 = csub(t0, t2);
    z1 = cadd(t1, t3);
    z3 = csub(t1, t3);
}

// natural-order radix-R DFT of z[0..R-1] in registers
template <int R, bool INV>
__device__ __forceinline__ void dft_r(double2* z) {
    if constexpr (R == 2) {
        const double2 a = z[0], b = z[1];
        z[0] = cadd(a, b);
        z[1] = csub(a, b);
    } else if constexpr (R == 4) {
        fft4r<INV>(z[0], z[1], z[2], z[3]);
    } else {
        double2 e0 = z[0], e1 = z[2], e2 = z[4], e3 = z[6];
        double2 o0 = z[1], o1 = z[3], o2 = z[5], o3 = z[7];
        fft4r<INV>(e0, e1, e2, e3);
        fft4r<INV>(o0, o1, o2, o3);
        constexpr double h = 0.70710678118654752440;
        // w8^k o_k, w8 = e^{-+ i pi/4}
        const double2 p1 = INV ? make_double2(h * (o1.x - o1.y), h * (o1.x + o1.y))
                               : make_double2(h * (o1.x + o1.y), h * (o1.y - o1.x));
        const double2 p2 = crot<INV>(o2);
        const double2 p3 = INV ? make_double2(-h * (o3.x + o3.y), h * (o3.x - o3.y))
                               : make_double2(h * (o3.y - o3.x), -h * (o3.x + o3.y));
        z[0] = cadd(e0, o0);
        z[4] = csub(e0, o0);
        z[1] = cadd(e1, p1);
        z[5] = csub(e1, p1);
        z[2] = cadd(e2, p2);
        z[6] = csub(e2, p2);
        z[3] = cadd(e3, p3);
        z[7] = csub(e3, p3);
    }
}

// One Stockham stage of radix R on this thread's 8/R butterflies b_s = j + s*TPL. Register
// z[s*R + r] holds input position b_s + r*M/R. Twiddles, then the DFT; output position of
// z[s*R + r] is (b_s / NS) * NS * R + b_s % NS + r * NS.
template <int L, int R, int NS, bool INV>
__device__ __forceinline__ void stage_compute(double2* z, int j, const double2* __restrict__ tw) {
    using S = spec8::Shape<L>;
#pragma unroll
    for (int s = 0; s < 8 / R; ++s) {
        if constexpr (NS > 1) {
            const int kk = (j + s * S::TPL) % NS;
            constexpr int step = S::M / (NS * R);
#pragma unroll
            for (int r = 1; r < R; ++r) {
                double2 w = tw[kk * r * step];
                if (INV) w = cconj(w);
                z[s * R + r] = cmul(z[s * R + r], w);
            }
        }
        dft_r<R, INV>(z + s * R);
    }
}
template <int L, int R>
__device__ __forceinline__ int stage_in_pos(int j, int i) {
    using S = spec8::Shape<L>;
    const int s = i / R, r = i % R;
    return j + S::TPL * (s + r * (8 / R));
}
template <int L, int R, int NS>
__device__ __forceinline__ int stage_out_pos(int j, int i) {
    using S = spec8::Shape<L>;
    const int s = i / R, r = i % R;
    const int b = j + s * S::TPL;
    return (b / NS) * NS * R + (b % NS) + r * NS;
}

// Barrier policies of the FFT exchanges: 0 __syncthreads, 1 LDS-only workgroup barrier (lds_barrier: global loads
// issued before the stages stay in flight), 2 the wave alone — for tiles where every complex line's threads are one
// wave's lanes (d = 0 passes with m / 8 <= 64 threads per line), whose exchange slots no other wave touches: a
// wave's LDS accesses complete in issue order, so only the compiler must not move them across the point
template <int BAR>
__device__ __forceinline__ void xbar() {
    if constexpr (BAR == 0) {
        __syncthreads();
    } else if constexpr (BAR == 1) {
        lds_barrier();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    }
}

// Stages after the first (the first is peeled: its input comes from HBM or the caller's LDS).
// STAGE counts radix-8 stages done after R0. Writes the outputs of stage NS_IN's butterflies
// to LDS, then (if more stages remain) reads the next stage's inputs. BAR: the barrier policy (xbar); true (1):
// LDS-only barriers (lds_barrier), so global loads issued before the stages stay in flight
template <int L, int R, int NS, bool INV, bool LAST_TO_REGS, int BAR = 0>
__device__ __forceinline__ void stages_from(double2* z, int j, double2* X, int cx, const double2* __restrict__ tw) {
    using S = spec8::Shape<L>;
    stage_compute<L, R, NS, INV>(z, j, tw);
    constexpr int NS_NEXT = NS * R;
    if constexpr (NS_NEXT == S::M && LAST_TO_REGS) {
        return;   // caller stores z (output positions stage_out_pos<L, R, NS>)
    } else {
        xbar<BAR>();   // everyone has read this stage's inputs
#pragma unroll
        for (int i = 0; i < 8; ++i) X[spec8::slot(stage_out_pos<L, R, NS>(j, i), cx)] = z[i];
        xbar<BAR>();
        if constexpr (NS_NEXT < S::M) {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = X[spec8::slot(stage_in_pos<L, 8>(j, i), cx)];
            stages_from<L, 8, NS_NEXT, INV, LAST_TO_REGS, BAR>(z, j, X, cx, tw);
        }
    }
}
// radix of the last stage and its NS (for the register-resident output positions)
template <int L>
struct LastStage {
    static constexpr int R = (L == 1 || L == 2) ? (1 << L) : 8;   // L >= 3 always ends with radix 8
    static constexpr int NS = (1 << L) / R;
};

// PC (PcgFuse, d = 0 passes of a preconditioner solve): 1 = first pass, r -= alpha q and x += alpha p on
// load with r and x written back, input sinv * r; 2 = last pass, out = sinv * transform, r.z and |r|^2 per
// workgroup
template <int L, int MODE, bool D0, bool FORMB, int TQW = 0, int PC = 0>
__global__ __launch_bounds__((spec8::ShapeK<L, TQW>::NT)) void k_dct8(const SpecArgs a) {
    using S = spec8::ShapeK<L, TQW>;
    static_assert(PC == 0 || (D0 && !FORMB && (PC == 1 ? MODE == SPEC_FWD : MODE == SPEC_INV)),
                  "PCG fusion: d = 0 forward (PC 1) / inverse (PC 2) passes only");
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    // scalars into locals: writing into the by-value argument struct would demote it to scratch
    double sigma = a.sigma, ca = a.ca, cb = a.cb;
    if (a.skip && *a.skip) return;
    const double alpha = PC == 1 ? a.pf.st->alpha : 0.0;
    double rz = 0.0, rr = 0.0;   // PC 2 reductions
    bool rd_gb = true;   // FORMB reads gb (the folded form only after a rho change)
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
        if (a.fold) {
            ca = a.ctl->fold_ka;
            cb = a.ctl->fold_kb;
            rd_gb = a.ctl->fix != 0;
        }
    }
    constexpr int M = S::M, TPL = S::TPL, NCL = S::NCL;
    // d = 0 with <= 64 threads per complex line: each line's exchanges stay inside one wave (no workgroup barrier;
    // MID keeps them: its line constants are shared)
    constexpr int BAR = (D0 && TPL <= 64 && 64 % TPL == 0 && MODE != SPEC_MID) ? 2 : 0;
    __shared__ double2 buf[NCL * S::LP];
    __shared__ double lc0[2 * NCL], lc1[2 * NCL];
    const int t = threadIdx.x;
    const int j = D0 ? (t % TPL) : (t / NCL);
    const int c = D0 ? (t / TPL) : (t % NCL);
    // xcd: workgroup b runs on XCD b % 8; dealing tiles in contiguous runs per XCD keeps the tiles that
    // share a 128-B row of a strided pass (d > 0, < 16 lines per tile) in one L2
    const uint32_t bx = a.xcd ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const uint32_t q0 = bx * uint32_t(a.tq);
    const int la = 2 * c, lb = 2 * c + 1;
    const bool va = la < a.tq && q0 + la < a.nlines;
    const bool vb = lb < a.tq && q0 + lb < a.nlines;
    double2* X = buf + c * S::LP;
    const int cx = c & 7;
    const double2* __restrict__ tw = a.tw;

    for (int l = t; MODE == SPEC_MID && l < a.tq; l += S::NT) {
        const uint32_t q = a.q_off + q0 + l;
        double lamv[kMaxDims] = {0, 0, 0, 0};
        uint32_t rest = (q - a.q_off) < a.nlines ? q : a.q_off;
        // line q enumerates the dims other than d, dim 0 fastest
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int jj = 0; jj < a.p; ++jj) {
            if (jj == a.d) continue;
            const uint32_t qq = (jj < jlast) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qq * a.m[jj])];
            rest = qq;
        }
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p; ++jj)
                if (jj != a.d && ((Sm >> jj) & 1)) prod *= lamv[jj];
            if ((Sm >> a.d) & 1) c1 += prod;
            else c0 += prod;
        }
        lc0[l] = c0;
        lc1[l] = c1;
    }

    // element k of real line ql (local) -> global offset
    auto gaddr = [&](int ql, uint32_t k) -> uint32_t {
        const uint32_t q = q0 + uint32_t(ql);
        if (D0) return (q << L) + k;
        return (q & (a.stride - 1)) + ((q >> a.ls) << (a.ls + L)) + (k << a.ls);
    };
    auto ld2 = [&](uint32_t k) -> double2 {   // (line la, line lb) at position k, b formed if FORMB
        double2 v = make_double2(0.0, 0.0);
        if (D0) {
            if (va) {
                const uint32_t g = gaddr(la, k);
                v.x = __builtin_nontemporal_load(a.in + g);
                if (FORMB && !rd_gb) v.x += ca * __builtin_nontemporal_load(a.ga + g);
                else if (FORMB) v.x += ca * __builtin_nontemporal_load(a.ga + g) + cb * __builtin_nontemporal_load(a.gb + g);
            }
            if (vb) {
                const uint32_t g = gaddr(lb, k);
                v.y = __builtin_nontemporal_load(a.in + g);
                if (FORMB && !rd_gb) v.y += ca * __builtin_nontemporal_load(a.ga + g);
                else if (FORMB) v.y += ca * __builtin_nontemporal_load(a.ga + g) + cb * __builtin_nontemporal_load(a.gb + g);
            }
        } else if (va) {   // d > 0: lines la, lb are adjacent words (vb == va)
            const uint32_t g = gaddr(la, k);
            v = ldnt2(a.in + g);
            if (FORMB && !rd_gb) {
                const double2 x1 = ldnt2(a.ga + g);
                v.x += ca * x1.x;
                v.y += ca * x1.y;
            } else if (FORMB) {
                const double2 x1 = ldnt2(a.ga + g);
                const double2 x2 = ldnt2(a.gb + g);
                v.x += ca * x1.x + cb * x2.x;
                v.y += ca * x1.y + cb * x2.y;
            }
        }
        return v;
    };
    auto st2 = [&](uint32_t k, double2 v) {
        if (D0) {
            if (va) __builtin_nontemporal_store(v.x, a.out + gaddr(la, k));
            if (vb) __builtin_nontemporal_store(v.y, a.out + gaddr(lb, k));
        } else if (va) {
            stnt2(a.out + gaddr(la, k), v);
        }
    };

    double2 z[8];
    if (MODE != SPEC_INV) {
        // ---- forward FFT of the Makhoul sequence z[n] = x[2n] | x[2(M-1-n)+1] -----------------
        constexpr int R0 = S::R0;
        if (D0) {
            // contiguous lines: 16-B loads of (x[2n], x[2n+1]) land at Makhoul positions n, M-1-n
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int n = j + s4 * TPL;
                double2 xa = make_double2(0.0, 0.0), xb = make_double2(0.0, 0.0);
                auto ld_in = [&](uint32_t g) -> double2 {
                    if constexpr (PC == 1) {   // the operations of k_pcgs_vec op 1
                        double2 rv = ldnt2(a.pf.r + g);
                        const double2 qv = ldnt2(a.pf.q + g);
                        double2 xv = ldnt2(a.pf.x + g);
                        const double2 pv = ldnt2(a.pf.p + g);
                        rv.x = fma(-alpha, qv.x, rv.x);
                        rv.y = fma(-alpha, qv.y, rv.y);
                        xv.x = fma(alpha, pv.x, xv.x);
                        xv.y = fma(alpha, pv.y, xv.y);
                        stnt2(a.pf.r + g, rv);
                        stnt2(a.pf.x + g, xv);
                        if (a.pf.sinv) {
                            const double2 sv = ldnt2(a.pf.sinv + g);
                            rv.x *= sv.x;
                            rv.y *= sv.y;
                        }
                        return rv;
                    } else {
                        double2 v = ldnt2(a.in + g);
                        if (FORMB && !rd_gb) {
                            const double2 g1 = ldnt2(a.ga + g);
                            v.x += ca * g1.x;
                            v.y += ca * g1.y;
                        } else if (FORMB) {
                            const double2 g1 = ldnt2(a.ga + g), g2 = ldnt2(a.gb + g);
                            v.x += ca * g1.x + cb * g2.x;
                            v.y += ca * g1.y + cb * g2.y;
                        }
                        return v;
                    }
                };
                if (va) xa = ld_in(gaddr(la, uint32_t(2 * n)));
                if (vb) xb = ld_in(gaddr(lb, uint32_t(2 * n)));
                X[spec8::slot(n, cx)] = make_double2(xa.x, xb.x);
                X[spec8::slot(M - 1 - n, cx)] = make_double2(xa.y, xb.y);
            }
            xbar<BAR>();
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = X[spec8::slot(stage_in_pos<L, R0>(j, i), cx)];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = stage_in_pos<L, R0>(j, i);
                const uint32_t k = n < M / 2 ? uint32_t(2 * n) : uint32_t(2 * (M - 1 - n) + 1);
                z[i] = ld2(k);
            }
        }
        stages_from<L, R0, 1, false, false, BAR>(z, j, X, cx, tw);   // natural-order spectrum in LDS
    }

    // ---- spectrum <-> DCT coefficients for the pairs (k, M-k); k = 0 also takes M/2 -------------
    // the inverse pass issues all 8 coefficient loads before the first LDS write (issued inside the loop,
    // each group waited for its loads before writing LDS: four HBM round trips per workgroup instead of one)
    // d = 0 with a.pair16: the coefficients of the two real lines cross LDS (the line's exchange slots as M + M doubles)
    // so that they arrive / leave as 16-B pairs (k, k + 1) of one line, as the other side of these passes does; read or
    // written directly they are 8-B accesses at positions k and M - k (round 6: the d = 0 forward pass 540 us for 2N
    // words against 383 for a strided one at 512^3)
    double* const Xd = reinterpret_cast<double*>(X);
    double2 pre[8];
    if constexpr (MODE == SPEC_INV) {
        if (D0 && a.pair16) {
            double2 qa[4], qb[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const uint32_t i2 = uint32_t(2 * (j + s4 * TPL));
                qa[s4] = va ? ldnt2(a.in + gaddr(la, i2)) : make_double2(0.0, 0.0);
                qb[s4] = vb ? ldnt2(a.in + gaddr(lb, i2)) : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int i2 = 2 * (j + s4 * TPL);
                *reinterpret_cast<double2*>(Xd + i2) = qa[s4];
                *reinterpret_cast<double2*>(Xd + M + i2) = qb[s4];
            }
            xbar<BAR>();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = j + s * TPL, kb = k ? M - k : M / 2;
                pre[2 * s] = make_double2(Xd[k], Xd[M + k]);
                pre[2 * s + 1] = make_double2(Xd[kb], Xd[M + kb]);
            }
            xbar<BAR>();   // every coefficient read before the IFFT input is written over them
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = j + s * TPL;
                pre[2 * s] = ld2(uint32_t(k));
                pre[2 * s + 1] = ld2(uint32_t(k ? M - k : M / 2));
            }
        }
    }
    double2 fco[8];   // d = 0 forward with a.pair16: the coefficient pairs, written after the loop
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = j + s * TPL;
        const int ka = k, kb = k ? M - k : M / 2;
        const bool self = k == 0;
        double2 Xk, Xmk;
        if (MODE != SPEC_INV) {
            const double2 Z1 = X[spec8::slot(ka, cx)], Z2 = X[spec8::slot(kb, cx)];
            const double2 q1 = a.twq[ka], q2 = a.twq[kb];
            if (self) {
                Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
            } else {
                const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
            }
        } else {
            Xk = pre[2 * s];
            Xmk = pre[2 * s + 1];
        }
        if (MODE == SPEC_FWD) {
            if (D0 && a.pair16) {
                fco[2 * s] = Xk;
                fco[2 * s + 1] = Xmk;
            } else {
                st2(uint32_t(ka), Xk);
                st2(uint32_t(kb), Xmk);
            }
            continue;
        }
        if (MODE == SPEC_MID) {
            const double* lamd = a.lam + a.lam_off[a.d];
            const double l1 = lamd[ka], l2 = lamd[kb];
            Xk.x *= a.inv_n / (lc0[la] + lc1[la] * l1);
            Xk.y *= a.inv_n / (lc0[lb] + lc1[lb] * l1);
            Xmk.x *= a.inv_n / (lc0[la] + lc1[la] * l2);
            Xmk.y *= a.inv_n / (lc0[lb] + lc1[lb] * l2);
        }
        const double2 q1 = cconj(a.twq[ka]), q2 = cconj(a.twq[kb]);
        if (self) {
            const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
            const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
            X[spec8::slot(0, cx)] = Xk;
            X[spec8::slot(M / 2, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
        } else {
            const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
            const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
            const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
            const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
            X[spec8::slot(ka, cx)] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
            X[spec8::slot(kb, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
        }
    }
    if (MODE == SPEC_FWD) {
        if (D0 && a.pair16) {
            xbar<BAR>();   // every spectrum read before the coefficients are written over it
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = j + s * TPL, kb = k ? M - k : M / 2;
                Xd[k] = fco[2 * s].x;
                Xd[M + k] = fco[2 * s].y;
                Xd[kb] = fco[2 * s + 1].x;
                Xd[M + kb] = fco[2 * s + 1].y;
            }
            xbar<BAR>();
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int i2 = 2 * (j + s4 * TPL);
                if (va) stnt2(a.out + gaddr(la, uint32_t(i2)), *reinterpret_cast<const double2*>(Xd + i2));
                if (vb) stnt2(a.out + gaddr(lb, uint32_t(i2)), *reinterpret_cast<const double2*>(Xd + M + i2));
            }
        }
        return;
    }
    xbar<BAR>();

    // ---- inverse FFT, natural in; the last stage's outputs go straight to HBM, un-permuted ------
    {
        constexpr int R0 = S::R0;
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = X[spec8::slot(stage_in_pos<L, R0>(j, i), cx)];
        if (D0) {
            // contiguous lines: the output goes through LDS so (x[2n], x[2n+1]) leave as one 16-B store
            stages_from<L, R0, 1, true, false, BAR>(z, j, X, cx, tw);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int n = j + s4 * TPL;
                const double2 v0 = X[spec8::slot(n, cx)], v1 = X[spec8::slot(M - 1 - n, cx)];
                auto st_out = [&](uint32_t g, double2 v) {
                    if constexpr (PC == 2) {   // the operations of k_pcgs_vec op 2
                        if (a.pf.sinv) {
                            const double2 sv = ldnt2(a.pf.sinv + g);
                            v.x *= sv.x;
                            v.y *= sv.y;
                        }
                        const double2 rv = ldnt2(a.pf.r + g);
                        rz = fma(rv.x, v.x, rz);
                        rr = fma(rv.x, rv.x, rr);
                        rz = fma(rv.y, v.y, rz);
                        rr = fma(rv.y, rv.y, rr);
                        stnt2(a.out + g, v);
                    } else {
                        stnt2(a.out + g, v);
                    }
                };
                if (va) st_out(gaddr(la, uint32_t(2 * n)), make_double2(v0.x, v1.x));
                if (vb) st_out(gaddr(lb, uint32_t(2 * n)), make_double2(v0.y, v1.y));
            }
            if constexpr (PC == 2) {
                double red[2] = {rz, rr};
                block_reduce_store<2, 0, S::NT>(red, a.pf.partials);
            }
        } else {
            stages_from<L, R0, 1, true, true>(z, j, X, cx, tw);
            using LS = LastStage<L>;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = stage_out_pos<L, LS::R, LS::NS>(j, i);
                const uint32_t k = n < M / 2 ? uint32_t(2 * n) : uint32_t(2 * (M - 1 - n) + 1);
                st2(k, z[i]);
            }
        }
    }
}

// =============================================================================================
// Two in-plane passes in one launch (m0 = m1 = 2^L, L <= 7): a workgroup owns one (dim 0, dim 1) plane,
// 128 KB at L = 7, and keeps it on chip between the two 1-D transforms, so the spectral solve of a 4-D
// 128^4 mesh makes 5 passes over HBM instead of 7 (3 instead of 5 at 128^3). NCL = M / 2 complex lines x
// TPL = M / 8 threads: the whole plane is one k_dct8 tile of M lines. Between the passes the coefficients go
// through a plane image in LDS (aliasing the FFT exchange buffer, barriers on both sides). Every barrier orders
// LDS only (lds_barrier): __syncthreads would also wait for the next plane's loads.
//   forward: dim-0 DCT of the rows (b formed on load as k_dct8's first pass), dim-1 DCT of the columns;
//   inverse: dim-1 inverse of the columns, dim-0 inverse of the rows.
template <int L, int MODE, bool FORMB>
__global__ __launch_bounds__((1 << L) / 2 * (1 << L) / 8) void k_plane8(const SpecArgs a, uint32_t nplanes) {
    using S = spec8::Shape<L>;
    constexpr int M = S::M, TPL = S::TPL, NCL = M / 2, R0 = S::R0;
    static_assert(L >= 4 && L <= 7, "the plane must fit the exchange buffer of one workgroup");
    static_assert(TPL <= 64 && 64 % TPL == 0, "a row pair's threads are lanes of one wave (xbar<2> on the rows)");
    // plane image pitch PP = M + M / 16 doubles (18 at M = 16): a wave's row accesses (8-B words, TPL = M / 8
    // lanes per row, 8 rows a wave at M = 64, 4 at 128) then start 16 PP bytes apart = M bytes mod 256, so the rows
    // of one wave instruction fall on different LDS banks; with pitch M every row started on bank 0 (rows 2 KB
    // apart at M = 128: 4-way conflicts on the transposes). Column accesses stay 16-B aligned (PP even).
    constexpr int PP = M + (M / 16 > 2 ? M / 16 : 2);
    static_assert(size_t(NCL) * S::LP * 16 >= size_t(M) * PP * 8, "plane image aliases the exchange buffer");
    static_assert(MODE == SPEC_FWD || !FORMB, "b is formed by the forward pass");
    double ca = a.ca, cb = a.cb;
    bool rd_gb = true;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
        if (a.fold) {
            ca = a.ctl->fold_ka;
            cb = a.ctl->fold_kb;
            rd_gb = a.ctl->fix != 0;
        }
    }
    __shared__ double2 buf[NCL * S::LP];
    double* const PI = reinterpret_cast<double*>(buf);   // plane image [row x1][column x0], pitch PP
    // rows mapping (dim-0 lines: lanes over j) and columns mapping (dim-1 lines: lanes over the line pair); the
    // loop below re-derives them from an opaque copy of the thread index each plane, so the many per-thread LDS
    // offsets are not hoisted out of it (kept live across the loop they spill)
    int t = threadIdx.x;
    int jr = t % TPL, cr = t / TPL, jc = t / NCL, cc = t % NCL;
    double2 z[8];
    // the workgroup walks planes blockIdx.x, + gridDim.x, ...; the next plane's loads are issued as soon as this
    // plane's have been moved to LDS, so they are in flight during both transforms
    double2 lv[8], lg1[8];   // forward: in, ga at (row 2cr + r, 2n) (gb, read only after a rho change or without the
                             // fold, is loaded when used); inverse: the coefficient pairs
    auto issue = [&](uint32_t e) {
        const uint32_t pb = e << (2 * L);
        if constexpr (MODE == SPEC_FWD) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const uint32_t g = pb + uint32_t(2 * cr + r) * M + uint32_t(2 * (jr + s4 * TPL));
                    lv[2 * s4 + r] = ldnt2(a.in + g);
                    if (FORMB) lg1[2 * s4 + r] = ldnt2(a.ga + g);
                }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = jc + s * TPL;
                lv[2 * s] = ldnt2(a.in + pb + uint32_t(k) * M + uint32_t(2 * cc));
                lv[2 * s + 1] = ldnt2(a.in + pb + uint32_t(k ? M - k : M / 2) * M + uint32_t(2 * cc));
            }
        }
    };
    uint32_t e = blockIdx.x;
    if (e < nplanes) issue(e);
    for (; e < nplanes; e += gridDim.x) {
        const uint32_t pb = e << (2 * L);
        const uint32_t en = e + gridDim.x;
        // the twiddle tables through opaque pointers: their loads stay in the loop (hoisted out of it, the
        // per-plane values would all stay live and spill)
        const double2* tw = a.tw;
        const double2* twq = a.twq;
        asm volatile("" : "+s"(tw), "+s"(twq));
        asm volatile("" : "+v"(t));
        jr = t % TPL;
        cr = t / TPL;
        jc = t / NCL;
        cc = t % NCL;
        double2* const Xr = buf + cr * S::LP;
        double2* const Xc = buf + cc * S::LP;
        const int cxr = cr & 7, cxc = cc & 7;
        // coefficients (k, M - k) -> the IFFT input of the Makhoul sequence, in X
        auto inv_spectrum = [&](double2* X, int cx, int k, double2 Xk, double2 Xmk) {
            const int ka = k, kb = k ? M - k : M / 2;
            const double2 q1 = cconj(twq[ka]), q2 = cconj(twq[kb]);
            if (k == 0) {
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                X[spec8::slot(0, cx)] = Xk;
                X[spec8::slot(M / 2, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            } else {
                const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
                const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
                X[spec8::slot(ka, cx)] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
                X[spec8::slot(kb, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            }
        };
        // the natural-order spectrum in X -> DCT-II coefficients (k, M - k) for k = j + s TPL
        auto fwd_coeff = [&](const double2* X, int cx, int k, double2& Xk, double2& Xmk) {
            const int ka = k, kb = k ? M - k : M / 2;
            const double2 Z1 = X[spec8::slot(ka, cx)], Z2 = X[spec8::slot(kb, cx)];
            const double2 q1 = twq[ka], q2 = twq[kb];
            if (k == 0) {
                Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
            } else {
                const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
            }
        };
        if constexpr (MODE == SPEC_FWD) {
            // ---- dim 0: rows 2cr, 2cr + 1 as one complex line ----------------------------------------------
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int n = jr + s4 * TPL;
                double2 xv[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    double2 v = lv[2 * s4 + r];
                    if (FORMB && !rd_gb) {
                        v.x += ca * lg1[2 * s4 + r].x;
                        v.y += ca * lg1[2 * s4 + r].y;
                    } else if (FORMB) {
                        const double2 g2 = ldnt2(a.gb + pb + uint32_t(2 * cr + r) * M + uint32_t(2 * n));
                        v.x += ca * lg1[2 * s4 + r].x + cb * g2.x;
                        v.y += ca * lg1[2 * s4 + r].y + cb * g2.y;
                    }
                    xv[r] = v;
                }
                Xr[spec8::slot(n, cxr)] = make_double2(xv[0].x, xv[1].x);
                Xr[spec8::slot(M - 1 - n, cxr)] = make_double2(xv[0].y, xv[1].y);
            }
            if (en < nplanes) issue(en);
            // a row pair's 16 threads are lanes of one wave and its exchange slots are that wave's alone: the row
            // transforms sync the wave only (xbar<2>); the plane image and the columns need the workgroup
            xbar<2>();
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = Xr[spec8::slot(stage_in_pos<L, R0>(jr, i), cxr)];
            stages_from<L, R0, 1, false, false, 2>(z, jr, Xr, cxr, tw);   // natural-order spectrum in X
#pragma unroll
            for (int s = 0; s < 4; ++s) fwd_coeff(Xr, cxr, jr + s * TPL, z[2 * s], z[2 * s + 1]);
            lds_barrier();   // every spectrum read before the plane image (same LDS) is written
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = jr + s * TPL, ka = k, kb = k ? M - k : M / 2;
                PI[(2 * cr) * PP + ka] = z[2 * s].x;
                PI[(2 * cr + 1) * PP + ka] = z[2 * s].y;
                PI[(2 * cr) * PP + kb] = z[2 * s + 1].x;
                PI[(2 * cr + 1) * PP + kb] = z[2 * s + 1].y;
            }
            lds_barrier();
            // ---- dim 1: columns 2cc, 2cc + 1 as one complex line -------------------------------------------
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = stage_in_pos<L, R0>(jc, i);
                const int k = n < M / 2 ? 2 * n : 2 * (M - 1 - n) + 1;
                z[i] = *reinterpret_cast<const double2*>(&PI[k * PP + 2 * cc]);
            }
            stages_from<L, R0, 1, false, false, true>(z, jc, Xc, cxc, tw);   // its first barrier ends the image reads
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = jc + s * TPL, ka = k, kb = k ? M - k : M / 2;
                double2 Xk, Xmk;
                fwd_coeff(Xc, cxc, k, Xk, Xmk);
                stnt2(a.out + pb + uint32_t(ka) * M + uint32_t(2 * cc), Xk);
                stnt2(a.out + pb + uint32_t(kb) * M + uint32_t(2 * cc), Xmk);
            }
            lds_barrier();   // every spectrum read before the next plane's rows are written
        } else {
            // ---- dim 1 inverse: columns 2cc, 2cc + 1 --------------------------------------------------------
#pragma unroll
            for (int s = 0; s < 4; ++s) inv_spectrum(Xc, cxc, jc + s * TPL, lv[2 * s], lv[2 * s + 1]);
            if (en < nplanes) issue(en);
            lds_barrier();
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = Xc[spec8::slot(stage_in_pos<L, R0>(jc, i), cxc)];
            stages_from<L, R0, 1, true, true, true>(z, jc, Xc, cxc, tw);   // outputs in registers
            lds_barrier();   // every exchange read before the plane image is written
            using LS = LastStage<L>;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = stage_out_pos<L, LS::R, LS::NS>(jc, i);
                const int k = n < M / 2 ? 2 * n : 2 * (M - 1 - n) + 1;
                *reinterpret_cast<double2*>(&PI[k * PP + 2 * cc]) = z[i];
            }
            lds_barrier();
            // ---- dim 0 inverse: rows 2cr, 2cr + 1 -----------------------------------------------------------
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = jr + s * TPL, kb = k ? M - k : M / 2;
                z[2 * s] = make_double2(PI[(2 * cr) * PP + k], PI[(2 * cr + 1) * PP + k]);
                z[2 * s + 1] = make_double2(PI[(2 * cr) * PP + kb], PI[(2 * cr + 1) * PP + kb]);
            }
            lds_barrier();   // every image read before the exchange buffer (same LDS) is written
#pragma unroll
            for (int s = 0; s < 4; ++s) inv_spectrum(Xr, cxr, jr + s * TPL, z[2 * s], z[2 * s + 1]);
            xbar<2>();   // the row transforms: one wave's slots (as forward)
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = Xr[spec8::slot(stage_in_pos<L, R0>(jr, i), cxr)];
            stages_from<L, R0, 1, true, false, 2>(z, jr, Xr, cxr, tw);   // output through X
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int n = jr + s4 * TPL;
                const double2 v0 = Xr[spec8::slot(n, cxr)], v1 = Xr[spec8::slot(M - 1 - n, cxr)];
                stnt2(a.out + pb + uint32_t(2 * cr) * M + uint32_t(2 * n), make_double2(v0.x, v1.x));
                stnt2(a.out + pb + uint32_t(2 * cr + 1) * M + uint32_t(2 * n), make_double2(v0.y, v1.y));
            }
            lds_barrier();   // every exchange read before the next plane's spectrum is written
        }
    }
}

// =============================================================================================
// Mixed-radix lengths: m = 2^a 3^b 5^c 7^d <= 4096 that is not a power of two (meshes such as
// 24 x 40, 100^3 or 1000^2). Same Makhoul pairing and pass structure as k_dct8, with the complex
// FFT of length m run in LDS as in-place Cooley-Tukey stages of radix 8, 4, 2, 3, 5, 7: decimation
// in time on input stored at digit-reversed positions (forward), decimation in frequency leaving
// digit-reversed output (inverse), so both permutations fold into the load / store index as the
// bit reversal does for k_dct. Line addresses take a general stride (FastDiv).
namespace dctg {
constexpr int NT = 512;   // threads per workgroup: 16 lines of <= 512 points (two workgroups per CU)
// cos / sin (2 pi k / R), k < R
__device__ __constant__ const double c3[3] = {1.0, -0.5, -0.5};
__device__ __constant__ const double s3[3] = {0.0, 0.86602540378443864676, -0.86602540378443864676};
__device__ __constant__ const double c5[5] = {1.0, 0.30901699437494742410, -0.80901699437494742410,
                                             -0.80901699437494742410, 0.30901699437494742410};
__device__ __constant__ const double s5[5] = {0.0, 0.95105651629515357212, 0.58778525229247312917,
                                             -0.58778525229247312917, -0.95105651629515357212};
__device__ __constant__ const double c7[7] = {1.0, 0.62348980185873353053, -0.22252093395631440429,
                                             -0.90096886790241912624, -0.90096886790241912624,
                                             -0.22252093395631440429, 0.62348980185873353053};
__device__ __constant__ const double s7[7] = {0.0, 0.78183148246802980871, 0.97492791218182360702,
                                             0.43388373911755812048, -0.43388373911755812048,
                                             -0.97492791218182360702, -0.78183148246802980871};
}  // namespace dctg

// natural-order DFT of z[0..R-1] for R in {3, 5, 7}
template <int R, bool INV>
__device__ __forceinline__ void dft_odd(double2* z) {
    const double* C = R == 3 ? dctg::c3 : (R == 5 ? dctg::c5 : dctg::c7);
    const double* Sn = R == 3 ? dctg::s3 : (R == 5 ? dctg::s5 : dctg::s7);
    double2 y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double2 acc = z[0];
#pragma unroll
        for (int q = 1; q < R; ++q) {
            const int k = (q * r) % R;
            const double c = C[k], s = INV ? Sn[k] : -Sn[k];   // e^{-+ i 2 pi k / R}
            acc.x += z[q].x * c - z[q].y * s;
            acc.y += z[q].x * s + z[q].y * c;
        }
        y[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) z[r] = y[r];
}

template <int R, bool INV>
__device__ __forceinline__ void dft_any(double2* z) {
    if constexpr (R == 2 || R == 4 || R == 8) dft_r<R, INV>(z);
    else dft_odd<R, INV>(z);
}

// One in-place stage over ncl lines of pitch LP: butterflies (block b of L1 = L R, column j < L) on
// elements b L1 + j + r L. DIT: twiddle w^{r j m / L1} then DFT; DIF: DFT then twiddle.
template <int R, bool DIF, bool INV>
__device__ __forceinline__ void mr_stage(double2* __restrict__ buf, const double2* __restrict__ tw, int ncl, int m,
                                         int LP, int L, const FastDiv& fper, const FastDiv& fL) {
    const int L1 = L * R, per = m / R, nb = ncl * per, tstep = m / L1;
    for (int t = threadIdx.x; t < nb; t += dctg::NT) {
        const int line = int(fper.div(uint32_t(t))), bi = t - line * per;
        const int b = int(fL.div(uint32_t(bi))), j = bi - b * L;
        double2* x = buf + line * LP + b * L1 + j;
        double2 z[R];
#pragma unroll
        for (int r = 0; r < R; ++r) z[r] = x[r * L];
        if (!DIF) {
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const double2 w = tw[r * j * tstep];   // r j m / L1 < m
                z[r] = cmul(z[r], INV ? cconj(w) : w);
            }
        }
        dft_any<R, INV>(z);
        if (DIF) {
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const double2 w = tw[r * j * tstep];
                z[r] = cmul(z[r], INV ? cconj(w) : w);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) x[r * L] = z[r];
    }
    __syncthreads();
}

// (PL: SpecArgs, or a split pass's SubFft: nrad, rad, fper, fL of the length-m plan)
template <bool DIF, bool INV, typename PL>
__device__ __forceinline__ void mr_fft(double2* buf, const double2* tw, int ncl, int m, int LP, const PL& a) {
    auto stage = [&](int s, int L) {
        switch (a.rad[s]) {
            case 2: mr_stage<2, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
            case 3: mr_stage<3, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
            case 4: mr_stage<4, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
            case 5: mr_stage<5, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
            case 7: mr_stage<7, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
            default: mr_stage<8, DIF, INV>(buf, tw, ncl, m, LP, L, a.fper[s], a.fL[s]); break;
        }
    };
    if (!DIF) {
        for (int s = 0, L = 1; s < a.nrad; ++s) {
            stage(s, L);
            L *= a.rad[s];
        }
    } else {
        for (int s = a.nrad - 1, L1 = m; s >= 0; --s) {
            const int L = L1 / a.rad[s];
            stage(s, L);
            L1 = L;
        }
    }
}

template <int MODE, bool D0, bool FORMB>
__global__ __launch_bounds__(dctg::NT) __attribute__((amdgpu_waves_per_eu(4))) void k_dctg(const SpecArgs a) {
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    double sigma = a.sigma, ca = a.ca, cb = a.cb;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
    }
    extern __shared__ double2 buf[];   // tq / 2 lines of m + PAD complex slots (launch-time size)
    __shared__ double lc0[16], lc1[16];
    const int m = int(a.m[a.d]);
    const int tq = a.tq, ncl = tq >> 1;
    const int LP = m + spec::PAD;
    const uint32_t q0 = (a.xrun ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x) * uint32_t(tq);

    if (MODE == SPEC_MID && threadIdx.x < uint32_t(tq)) {
        const uint32_t q = a.q_off + q0 + threadIdx.x;
        double lamv[kMaxDims] = {0, 0, 0, 0};
        uint32_t rest = (q - a.q_off) < a.nlines ? q : a.q_off;
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int j = 0; j < a.p; ++j) {
            if (j == a.d) continue;
            const uint32_t qq = (j < jlast) ? a.fd[j].div(rest) : 0u;
            lamv[j] = a.lam[a.lam_off[j] + (rest - qq * a.m[j])];
            rest = qq;
        }
        double c0 = a.w0, c1 = 0.0;
        for (int S = 1; S < (1 << a.p); ++S) {
            if (a.cS[S] == 0.0) continue;
            double prod = sigma * a.cS[S];
            for (int j = 0; j < a.p; ++j)
                if (j != a.d && ((S >> j) & 1)) prod *= lamv[j];
            if ((S >> a.d) & 1) c1 += prod;
            else c0 += prod;
        }
        lc0[threadIdx.x] = c0;
        lc1[threadIdx.x] = c1;
    }

    // global offset of (local line ql, position k): line q = (block q / stride, offset q % stride)
    auto gaddr = [&](uint32_t ql, uint32_t k) -> uint32_t {
        const uint32_t q = q0 + ql;
        if (D0) return q * uint32_t(m) + k;
        const uint32_t hi = a.fds.div(q);
        return (q - hi * a.stride) + hi * a.stride * uint32_t(m) + k * a.stride;
    };
    const int ltq = __ffs(tq) - 1;   // tq is a power of two

    double* bw = reinterpret_cast<double*>(buf);
    const int total = tq * m;
    for (int e = threadIdx.x; e < total; e += dctg::NT) {
        const int ql = D0 ? int(a.fm.div(uint32_t(e))) : (e & (tq - 1));
        const int k = D0 ? e - ql * m : (e >> ltq);
        double v = 0.0;
        if (q0 + uint32_t(ql) < a.nlines) {
            const uint32_t gi = gaddr(uint32_t(ql), uint32_t(k));
            v = __builtin_nontemporal_load(a.in + gi);
            if (FORMB) v += ca * __builtin_nontemporal_load(a.ga + gi) + cb * __builtin_nontemporal_load(a.gb + gi);
        }
        const int pos = MODE == SPEC_INV ? k : int(a.perm[k]);
        bw[2 * ((ql >> 1) * LP + pos) + (ql & 1)] = v;
    }
    __syncthreads();

    const double2* tw = a.tw;
    if (MODE != SPEC_INV) mr_fft<false, false>(buf, tw, ncl, m, LP, a);

    // spectrum <-> DCT coefficients over the pairs (k, m-k); k = 0 pairs with itself, and so does
    // k = m/2 for even m (handled with k = 0)
    {
        const int half = m >> 1, npl = (m & 1) ? half + 1 : half;
        const int npairs = ncl * npl;
        for (int t = threadIdx.x; t < npairs; t += dctg::NT) {
            const int line = t / npl, k = t - line * npl;
            double2* x = buf + line * LP;
            const bool self = k == 0;
            const bool mid = self && !(m & 1);   // also the self pair m/2
            const int ka = k, kb = self ? half : m - k;
            double2 Xk, Xmk = make_double2(0.0, 0.0);
            if (MODE != SPEC_INV) {
                const double2 Z1 = x[ka], q1 = a.twq[ka];
                if (self) {
                    Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                    if (mid) {
                        const double2 Z2 = x[kb], q2 = a.twq[kb];
                        Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
                    }
                } else {
                    const double2 Z2 = x[kb], q2 = a.twq[kb];
                    const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                    const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                    Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                    Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
                }
            } else {
                Xk = x[ka];
                if (!self || mid) Xmk = x[kb];
            }
            if (MODE == SPEC_MID) {
                const double* lamd = a.lam + a.lam_off[a.d];
                const int l0 = 2 * line, l1 = 2 * line + 1;
                const double la = lamd[ka];
                Xk.x *= a.inv_n / (lc0[l0] + lc1[l0] * la);
                Xk.y *= a.inv_n / (lc0[l1] + lc1[l1] * la);
                if (!self || mid) {
                    const double lb = lamd[kb];
                    Xmk.x *= a.inv_n / (lc0[l0] + lc1[l0] * lb);
                    Xmk.y *= a.inv_n / (lc0[l1] + lc1[l1] * lb);
                }
            }
            if (MODE == SPEC_FWD) {
                x[ka] = Xk;
                if (!self || mid) x[kb] = Xmk;
                continue;
            }
            const double2 q2 = cconj(a.twq[kb]);
            if (self) {
                x[0] = Xk;   // X[m] = 0: V[0] = X[0]
                if (mid) {
                    const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                    const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                    x[half] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
                }
            } else {
                const double2 q1 = cconj(a.twq[ka]);
                const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
                const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
                x[ka] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
                x[kb] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            }
        }
        __syncthreads();
    }

    if (MODE != SPEC_FWD) mr_fft<true, true>(buf, tw, ncl, m, LP, a);

    for (int e = threadIdx.x; e < total; e += dctg::NT) {
        const int ql = D0 ? int(a.fm.div(uint32_t(e))) : (e & (tq - 1));
        const int k = D0 ? e - ql * m : (e >> ltq);
        if (q0 + uint32_t(ql) >= a.nlines) continue;
        const int pos = MODE == SPEC_FWD ? k : int(a.perm[k]);
        __builtin_nontemporal_store(bw[2 * ((ql >> 1) * LP + pos) + (ql & 1)], a.out + gaddr(uint32_t(ql), uint32_t(k)));
    }
}

// ---------------------------------------------------------------------------------------------
// k_dctm: register-resident mixed-radix passes for the lengths of the BASELINE-adjacent meshes (500 = 4 5^3,
// 1000 = 2 4 5^3): k_dct8's Stockham scheme with a compile-time radix plan. A thread holds V complex values
// of one complex line (two real lines, Makhoul pairing) and runs its V / R radix-R butterflies of each stage in
// registers; LDS carries the exchanges between stages (k_dctg: one in-place LDS stage per radix with FastDiv
// index math and a permutation-table load per element). FWD and INV passes (the last dimension takes k_trigr or
// k_dctg's MID pass); TQ = 16 real lines per workgroup, lanes over the lines for a strided pass (16-B accesses
// of a line pair, 128-B rows when the tile does not straddle a stride boundary), over j for d = 0.
namespace dctm {
constexpr int NCL = 8;   // complex lines per workgroup (default tile)
// radix plan and values per thread (every radix divides V): 500 = 2 2 5^3 with V = 10 (400 threads, two
// workgroups per CU), 1000 = 2 4 5^3 with V = 20 (400 threads)
template <int M> struct Plan;
template <> struct Plan<500> {
    static constexpr int n = 5, V = 10;
    static constexpr int r[5] = {2, 2, 5, 5, 5};
};
template <> struct Plan<1000> {
    static constexpr int n = 5, V = 20;
    static constexpr int r[5] = {2, 4, 5, 5, 5};
};
template <int M> struct Shape {
    static constexpr int V = Plan<M>::V;      // complex values per thread
    static constexpr int T = M / V;           // threads per complex line
    static constexpr int NT = NCL * T;
    static constexpr int LP = M + 4;          // line pitch (complex slots)
};
}  // namespace dctm

// stage S (span NS) of the thread's butterflies b_s = j + s T; z[s R + r] holds position b_s + r M / R
template <int M, int S, int NS, bool INV>
__device__ __forceinline__ void dctm_stages(double2* z, int j, double2* X, const double2* __restrict__ tw) {
    using P = dctm::Plan<M>;
    constexpr int V = P::V, R = P::r[S], T = M / V, NB = V / R;
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        if constexpr (NS > 1) {
            const int kk = (j + s * T) % NS;
            constexpr int step = M / (NS * R);
#pragma unroll
            for (int r = 1; r < R; ++r) {
                double2 w = tw[kk * r * step];
                if (INV) w = cconj(w);
                z[s * R + r] = cmul(z[s * R + r], w);
            }
        }
        dft_any<R, INV>(z + s * R);
    }
    if constexpr (S + 1 < P::n) {
        constexpr int R2 = P::r[S + 1];
        __syncthreads();   // every thread has read this stage's inputs
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int b = j + s * T;
#pragma unroll
            for (int r = 0; r < R; ++r) X[(b / NS) * NS * R + b % NS + r * NS] = z[s * R + r];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < V / R2; ++s)
#pragma unroll
            for (int r = 0; r < R2; ++r) z[s * R2 + r] = X[j + s * T + r * (M / R2)];
        dctm_stages<M, S + 1, NS * R, INV>(z, j, X, tw);
    }
}
// output position of z[i] after the last stage
template <int M>
__device__ __forceinline__ int dctm_out_pos(int j, int i) {
    using P = dctm::Plan<M>;
    constexpr int R = P::r[P::n - 1], NS = M / R, T = M / P::V;
    const int s = i / R, r = i % R, b = j + s * T;
    return (b / NS) * NS * R + b % NS + r * NS;
}
// input position of z[i] of the first stage
template <int M>
__device__ __forceinline__ int dctm_in_pos(int j, int i) {
    using P = dctm::Plan<M>;
    constexpr int R = P::r[0], T = M / P::V;
    return j + (i / R) * T + (i % R) * (M / R);
}

// NCLW complex lines (2 NCLW real lines) per workgroup: 4 (64-B rows; half the LDS of the 8-line tile that round 5
// measured against it: more workgroups a CU) or 1 (few lines)
template <int M, int MODE, bool D0, bool FORMB, int NCLW = dctm::NCL>
__global__ __launch_bounds__(NCLW * dctm::Shape<M>::T) void k_dctm(const SpecArgs a) {
    using S = dctm::Shape<M>;
    constexpr int T = S::T, NCL = NCLW, V = S::V, TQ = 2 * NCLW;
    static_assert(MODE == SPEC_FWD || MODE == SPEC_INV, "FWD / INV passes");
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    double ca = a.ca, cb = a.cb;
    bool rd_gb = true;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
        if (a.fold) {
            ca = a.ctl->fold_ka;
            cb = a.ctl->fold_kb;
            rd_gb = a.ctl->fix != 0;
        }
    }
    __shared__ double2 buf[NCL * S::LP];
    const int t = threadIdx.x;
    const int j = D0 ? (t % T) : (t / NCL);
    const int c = D0 ? (t / T) : (t % NCL);
    const uint32_t q0 = (a.xrun ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x) * uint32_t(TQ);
    const int la = 2 * c;
    const bool va = q0 + uint32_t(la) < a.nlines;   // lines come in pairs: nlines is even (launcher)
    double2* X = buf + c * S::LP;
    const double2* __restrict__ tw = a.tw;
    // global offset of (real line la of this thread's pair, position k); line la + 1 is the next word
    const uint32_t q = q0 + uint32_t(la);
    uint32_t lbase;
    if (D0) {
        lbase = q * uint32_t(M);
    } else {
        const uint32_t hi = a.fds.div(q);
        lbase = (q - hi * a.stride) + hi * a.stride * uint32_t(M);
    }
    auto gidx = [&](uint32_t k) -> uint32_t { return D0 ? lbase + k : lbase + k * a.stride; };
    auto ld_pair2 = [&](uint32_t g) -> double2 {   // b (or the input) at global offsets g, g + 1
        double2 v = ldnt2(a.in + g);
        if (FORMB && !rd_gb) {
            const double2 g1 = ldnt2(a.ga + g);
            v.x += ca * g1.x;
            v.y += ca * g1.y;
        } else if (FORMB) {
            const double2 g1 = ldnt2(a.ga + g), g2 = ldnt2(a.gb + g);
            v.x += ca * g1.x + cb * g2.x;
            v.y += ca * g1.y + cb * g2.y;
        }
        return v;
    };
    auto ld_pair = [&](uint32_t k) -> double2 {   // (line la, line la + 1) at position k, strided pass
        const uint32_t g = gidx(k);
        double2 v = ldnt2(a.in + g);
        if (FORMB && !rd_gb) {
            const double2 g1 = ldnt2(a.ga + g);
            v.x += ca * g1.x;
            v.y += ca * g1.y;
        } else if (FORMB) {
            const double2 g1 = ldnt2(a.ga + g), g2 = ldnt2(a.gb + g);
            v.x += ca * g1.x + cb * g2.x;
            v.y += ca * g1.y + cb * g2.y;
        }
        return v;
    };
    double2 z[V];
    if constexpr (MODE == SPEC_FWD) {
        // ---- Makhoul input v[n] = x[2n], v[M-1-n] = x[2n+1] into the first stage --------------------------
        if (D0) {
            // contiguous lines: 16-B loads of (x[2n], x[2n+1]) of each real line land at positions n, M-1-n
#pragma unroll
            for (int s = 0; s < M / 2 / T; ++s) {
                const int n = j + s * T;
                double2 xa = make_double2(0.0, 0.0), xb = make_double2(0.0, 0.0);
                if (va) {   // (x[2n], x[2n+1]) of lines la and la + 1: 16-B loads (M even: aligned)
                    xa = ld_pair2(lbase + uint32_t(2 * n));
                    xb = ld_pair2(lbase + uint32_t(M) + uint32_t(2 * n));
                }
                X[n] = make_double2(xa.x, xb.x);
                X[M - 1 - n] = make_double2(xa.y, xb.y);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < V; ++i) z[i] = X[dctm_in_pos<M>(j, i)];
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int n = dctm_in_pos<M>(j, i);
                const uint32_t k = n < M / 2 ? uint32_t(2 * n) : uint32_t(2 * (M - 1 - n) + 1);
                z[i] = va ? ld_pair(k) : make_double2(0.0, 0.0);
            }
        }
        dctm_stages<M, 0, 1, false>(z, j, X, tw);
        __syncthreads();   // every thread has read the last exchange
#pragma unroll
        for (int i = 0; i < V; ++i) X[dctm_out_pos<M>(j, i)] = z[i];   // natural-order spectrum
        __syncthreads();
        // ---- spectrum -> DCT-II coefficients (k, M - k); k = 0 and M / 2 pair with themselves --------------
#pragma unroll
        for (int s = 0; s < (M / 2 + T) / T; ++s) {
            const int k = j + s * T;
            if (k > M / 2) continue;
            const int ka = k, kb = k ? M - k : M / 2;
            const double2 Z1 = X[ka], Z2 = X[kb];
            const double2 q1 = a.twq[ka], q2 = a.twq[kb];
            double2 Xk, Xmk;
            if (k == 0) {
                Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
            } else {
                const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
            }
            if (!va || k == M / 2) continue;   // k = M/2 is written by k = 0 (its pair)
            if (D0) {
                __builtin_nontemporal_store(Xk.x, a.out + gidx(uint32_t(ka)));
                __builtin_nontemporal_store(Xk.y, a.out + gidx(uint32_t(ka)) + uint32_t(M));
                __builtin_nontemporal_store(Xmk.x, a.out + gidx(uint32_t(kb)));
                __builtin_nontemporal_store(Xmk.y, a.out + gidx(uint32_t(kb)) + uint32_t(M));
            } else {
                stnt2(a.out + gidx(uint32_t(ka)), Xk);
                stnt2(a.out + gidx(uint32_t(kb)), Xmk);
            }
        }
    } else {
        // ---- DCT-III: coefficient pairs (k, M - k) -> the Makhoul spectrum in X -----------------------------
#pragma unroll
        for (int s = 0; s < (M / 2 + T) / T; ++s) {
            const int k = j + s * T;
            if (k >= M / 2) continue;   // k = 0 also writes slot M / 2
            const int ka = k, kb = k ? M - k : M / 2;
            double2 Xk = make_double2(0.0, 0.0), Xmk = make_double2(0.0, 0.0);
            if (va) {
                if (D0) {
                    Xk = make_double2(__builtin_nontemporal_load(a.in + gidx(uint32_t(ka))),
                                      __builtin_nontemporal_load(a.in + gidx(uint32_t(ka)) + uint32_t(M)));
                    Xmk = make_double2(__builtin_nontemporal_load(a.in + gidx(uint32_t(kb))),
                                       __builtin_nontemporal_load(a.in + gidx(uint32_t(kb)) + uint32_t(M)));
                } else {
                    Xk = ldnt2(a.in + gidx(uint32_t(ka)));
                    Xmk = ldnt2(a.in + gidx(uint32_t(kb)));
                }
            }
            const double2 q1 = cconj(a.twq[ka]), q2 = cconj(a.twq[kb]);
            if (k == 0) {
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                X[0] = Xk;
                X[M / 2] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            } else {
                const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
                const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
                X[ka] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
                X[kb] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < V; ++i) z[i] = X[dctm_in_pos<M>(j, i)];
        dctm_stages<M, 0, 1, true>(z, j, X, tw);
        // ---- un-permute v[n] -> x[2n] (n < M/2), x[2(M-1-n)+1] -------------------------------------------
        if (D0) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < V; ++i) X[dctm_out_pos<M>(j, i)] = z[i];
            __syncthreads();
#pragma unroll
            for (int s = 0; s < M / 2 / T; ++s) {
                const int n = j + s * T;
                const double2 v0 = X[n], v1 = X[M - 1 - n];
                if (va) {
                    stnt2(a.out + lbase + uint32_t(2 * n), make_double2(v0.x, v1.x));
                    stnt2(a.out + lbase + uint32_t(M) + uint32_t(2 * n), make_double2(v0.y, v1.y));
                }
            }
        } else if (va) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int n = dctm_out_pos<M>(j, i);
                const uint32_t k = n < M / 2 ? uint32_t(2 * n) : uint32_t(2 * (M - 1 - n) + 1);
                stnt2(a.out + gidx(k), z[i]);
            }
        }
    }
}

// few lines (2-D meshes): halve a tile of tq lines, down to lo, while the grid has < 512 workgroups
static int few_lines_tq(uint32_t nlines, int tq, int lo) {
    while (tq > lo && (nlines + uint32_t(tq) - 1) / uint32_t(tq) < 512u) tq /= 2;
    return tq;
}

// k_dctm serves FWD / INV passes of m = 500 / 1000 lines; false: the caller takes k_dctg
static bool launch_dctm(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    const uint32_t m = a.m[a.d];
    // the first pass (b formed on load): k_dctm at 500 (V = 10: 0.89 against k_dctg's 1.09 ms at 500^3), k_dctg at
    // 1000 (V = 20: 31 against 29 us at 1000^2; profiles/r03/v19_dctm)
    if ((m != 500 && m != 1000) || mode == SPEC_MID || (formb && m != 500) || (a.nlines & 1u) ||
        probe_env("MVTV_DCTM_OFF"))
        return false;
    if (!d0 && (a.stride & 1u)) return false;   // line pairs must be adjacent words
    // 8-line tiles (500: 32 KB of LDS, up to five workgroups a CU against two with 16 lines; 1000: two against one):
    // 500^3 137.5 / 138.3 -> 141.6 / 142.4 ADMM it/s on one box, the first pass 0.93 -> 0.86 ms
    // (profiles/r05/v11_dctm_ncl4); few lines (1000 x 1000: 125 such tiles) one line pair per workgroup
    static const bool few_off = probe_flag("MVTV_FEW_LINES_OFF");
    const int ncl = few_off ? 4 : few_lines_tq(a.nlines, 8, 2) / 2;
    // (b is formed on load along dim 0 only: launch_dct_pass)
#define MVTV_DCTM(MM, NC)                                                                                       \
    do {                                                                                                        \
        const dim3 grid((a.nlines + uint32_t(2 * NC) - 1) / uint32_t(2 * NC));                                 \
        const dim3 block(NC * dctm::Shape<MM>::T);                                                              \
        if (mode == SPEC_INV) {                                                                                 \
            if (d0) klaunch(k_dctm<MM, SPEC_INV, true, false, NC>, grid, block, 0, s, a);                       \
            else klaunch(k_dctm<MM, SPEC_INV, false, false, NC>, grid, block, 0, s, a);                         \
        } else if (d0) {                                                                                        \
            if (formb) klaunch(k_dctm<MM, SPEC_FWD, true, true, NC>, grid, block, 0, s, a);                     \
            else klaunch(k_dctm<MM, SPEC_FWD, true, false, NC>, grid, block, 0, s, a);                          \
        } else {                                                                                                \
            klaunch(k_dctm<MM, SPEC_FWD, false, false, NC>, grid, block, 0, s, a);                              \
        }                                                                                                       \
    } while (0)
    if (m == 500) {
        if (ncl == 4) MVTV_DCTM(500, 4);
        else MVTV_DCTM(500, 1);
    } else {
        if (ncl == 4) MVTV_DCTM(1000, 4);
        else MVTV_DCTM(1000, 1);
    }
#undef MVTV_DCTM
    return true;
}

static void launch_dctg(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    const dim3 grid((a.nlines + uint32_t(a.tq) - 1) / uint32_t(a.tq)), block(dctg::NT);
    const size_t smem = size_t(a.tq / 2) * (a.m[a.d] + spec::PAD) * sizeof(double2);
    // (m = 4096 over a general stride: one complex line of 4097 slots is just above 64 KB)
#define MVTV_DCTG(MODE, D0, FB)                                                                               \
    do {                                                                                                       \
        if (smem > 65536)                                                                                      \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dctg<MODE, D0, FB>),                    \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(smem));                  \
        klaunch(k_dctg<MODE, D0, FB>, grid, block, uint32_t(smem), s, a);                                      \
    } while (0)
    if (mode == SPEC_FWD) {
        if (d0) {
            if (formb) MVTV_DCTG(SPEC_FWD, true, true);
            else MVTV_DCTG(SPEC_FWD, true, false);
        } else {
            MVTV_DCTG(SPEC_FWD, false, false);
        }
    } else if (mode == SPEC_INV) {
        if (d0) MVTV_DCTG(SPEC_INV, true, false);
        else MVTV_DCTG(SPEC_INV, false, false);
    } else {
        if (d0) {
            if (formb) MVTV_DCTG(SPEC_MID, true, true);
            else MVTV_DCTG(SPEC_MID, true, false);
        } else {
            MVTV_DCTG(SPEC_MID, false, false);
        }
    }
#undef MVTV_DCTG
}

// radices of m = 2^a 3^b 5^c 7^d in stage order (8s first); false if m has another prime factor
bool dct_radix_plan(uint32_t m, int* rad, int* nrad) {
    int n = 0;
    for (const uint32_t r : {8u, 4u, 2u, 3u, 5u, 7u})
        while (m % r == 0 && m > 1) {
            if (n == 8) return false;
            rad[n++] = int(r);
            m /= r;
        }
    *nrad = n;
    return m == 1;
}

// =============================================================================================
// Any other length m <= 4096 (a prime factor >= 11: 31, 37, 79, 1009 ... the released R API's default mesh
// m = floor(sqrt(n)) per dimension, rcpp-code/MultivarTV/R/MultivarTV.R:44-48, lands on such lengths). The
// length-m complex DFT of the Makhoul pairing by Bluestein's chirp-z identity nk = (n^2 + k^2 - (k - n)^2) / 2:
//
//   Y[k] = c[k] sum_n (y[n] c[n]) b[k - n],   c[n] = e^{s i pi n^2 / m},  b[j] = conj c[j]   (s = -1 / +1)
//
// a linear convolution, evaluated as a circular one of length M = 2^ceil(log2(2m - 1)): the chirped input goes
// through a forward FFT, the product with the transform of b (a per-dimension table, 1/M folded in) through the
// inverse FFT. The Makhoul pairing (k, m - k), the MID divide and b formed on load are k_dctg's. Per line pair: two
// length-M FFTs per transform (four in a MID pass); fp64 round-off grows as log M, like the planned FFTs'.
//
// k_dctb8 runs the length-M FFTs with k_dct8's register-resident radix-8 Stockham stages (stages_from): a thread
// holds 8 complex values of one complex line (two real lines), LDS carries only the exchanges between stages, both
// FFTs of a convolution leave natural order. (The first form, k_dctb, ran them with k_dct's radix-2^2 LDS FFT: every
// stage a round trip through LDS, ~20x the HBM bytes in LDS traffic and ~0.9 TB/s at 251^3. It was removed; it last
// existed in commit ae72d5c.)
template <int L, int MODE, bool D0, bool FORMB, int TQW>
__global__ __launch_bounds__((spec8::ShapeK<L, TQW>::NT)) void k_dctb8(const SpecArgs a) {
    using S = spec8::ShapeK<L, TQW>;
    constexpr int M = S::M, TPL = S::TPL, NCL = S::NCL, R0 = S::R0;
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    double sigma = a.sigma, ca = a.ca, cb = a.cb;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
    }
    __shared__ double2 buf[NCL * S::LP];
    __shared__ double lc0[2 * NCL], lc1[2 * NCL];
    const int m = int(a.m[a.d]);
    const int t = threadIdx.x;
    const int j = D0 ? (t % TPL) : (t / NCL);
    const int c = D0 ? (t / TPL) : (t % NCL);
    const uint32_t q0 = (a.xrun ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x) * uint32_t(TQW);
    const int la = 2 * c, lb = 2 * c + 1;
    const bool va = q0 + uint32_t(la) < a.nlines, vb = q0 + uint32_t(lb) < a.nlines;
    double2* const X = buf + c * S::LP;
    const int cx = c & 7;
    const double2* __restrict__ tw = a.tw;       // length-M twiddles
    const double2* __restrict__ chirp = a.bchirp;

    for (int l = t; MODE == SPEC_MID && l < TQW; l += S::NT) {   // c0 + c1 lam_d(k) per line (k_dct8)
        const uint32_t q = a.q_off + q0 + l;
        double lamv[kMaxDims] = {0, 0, 0, 0};
        uint32_t rest = (q - a.q_off) < a.nlines ? q : a.q_off;
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int jj = 0; jj < a.p; ++jj) {
            if (jj == a.d) continue;
            const uint32_t qq = (jj < jlast) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qq * a.m[jj])];
            rest = qq;
        }
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p; ++jj)
                if (jj != a.d && ((Sm >> jj) & 1)) prod *= lamv[jj];
            if ((Sm >> a.d) & 1) c1 += prod;
            else c0 += prod;
        }
        lc0[l] = c0;
        lc1[l] = c1;
    }

    auto gaddr = [&](int ql, uint32_t k) -> uint32_t {
        const uint32_t q = q0 + uint32_t(ql);
        if (D0) return q * uint32_t(m) + k;
        const uint32_t hi = a.fds.div(q);
        return (q - hi * a.stride) + hi * a.stride * uint32_t(m) + k * a.stride;
    };
    auto ld1 = [&](int ql, uint32_t k) -> double {
        const uint32_t gi = gaddr(ql, k);
        double v = __builtin_nontemporal_load(a.in + gi);
        if (FORMB) v += ca * __builtin_nontemporal_load(a.ga + gi) + cb * __builtin_nontemporal_load(a.gb + gi);
        return v;
    };
    auto ld2 = [&](uint32_t k) {
        return make_double2(va ? ld1(la, k) : 0.0, vb ? ld1(lb, k) : 0.0);
    };
    auto st2 = [&](uint32_t k, double2 v) {
        if (va) __builtin_nontemporal_store(v.x, a.out + gaddr(la, k));
        if (vb) __builtin_nontemporal_store(v.y, a.out + gaddr(lb, k));
    };
    // circular convolution with b (bhat = its transform / M) of u (u_at(n), n < M): natural order in X
    auto convolve = [&](auto&& u_at, const double2* __restrict__ bhat) {
        double2 z[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = u_at(stage_in_pos<L, R0>(j, i));
        stages_from<L, R0, 1, false, false>(z, j, X, cx, tw);   // DFT, natural order in X
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = stage_in_pos<L, R0>(j, i);
            z[i] = cmul(X[spec8::slot(n, cx)], bhat[n]);
        }
        stages_from<L, R0, 1, true, false>(z, j, X, cx, tw);    // inverse DFT, natural order in X
    };
    const int half = m >> 1, npl = (m & 1) ? half + 1 : half;
    // the inverse transform's input: V[k] conj c[k] at k < m (pairs (k, m - k)), zeros at [m, M)
    auto put_v = [&](int k, double2 Xk, double2 Xmk) {
        const bool self = k == 0, mid = self && !(m & 1);
        const int ka = k, kb = self ? half : m - k;
        const double2 q2 = cconj(a.twq[kb]);
        if (self) {
            X[spec8::slot(0, cx)] = cmul(Xk, cconj(chirp[0]));
            if (mid) {
                const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                X[spec8::slot(kb, cx)] = cmul(make_double2(va2.x - vb2.y, va2.y + vb2.x), cconj(chirp[kb]));
            }
        } else {
            const double2 q1 = cconj(a.twq[ka]);
            const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
            const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
            const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
            const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
            X[spec8::slot(ka, cx)] = cmul(make_double2(va1.x - vb1.y, va1.y + vb1.x), cconj(chirp[ka]));
            X[spec8::slot(kb, cx)] = cmul(make_double2(va2.x - vb2.y, va2.y + vb2.x), cconj(chirp[kb]));
        }
    };
    auto zero_pad = [&]() {
        for (int n = m + j; n < M; n += TPL) X[spec8::slot(n, cx)] = make_double2(0.0, 0.0);
    };

    if (MODE != SPEC_INV) {
        // forward: u[n] = y[n] c[n], y the Makhoul sequence of the two lines (sample k(n))
        convolve(
            [&](int n) {
                if (n >= m) return make_double2(0.0, 0.0);
                const int k = 2 * n < m ? 2 * n : 2 * (m - 1 - n) + 1;
                return cmul(ld2(uint32_t(k)), chirp[n]);
            },
            a.bvf);
        for (int k = j; k < npl; k += TPL) {   // Z[k] = c[k] conv[k] -> DCT-II coefficients of the pair (k, m - k)
            const bool self = k == 0, mid = self && !(m & 1);
            const int ka = k, kb = self ? half : m - k;
            const double2 Z1 = cmul(X[spec8::slot(ka, cx)], chirp[ka]), q1 = a.twq[ka];
            double2 Xk, Xmk = make_double2(0.0, 0.0);
            if (self) {
                Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                if (mid) {
                    const double2 Z2 = cmul(X[spec8::slot(kb, cx)], chirp[kb]), q2 = a.twq[kb];
                    Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
                }
            } else {
                const double2 Z2 = cmul(X[spec8::slot(kb, cx)], chirp[kb]), q2 = a.twq[kb];
                const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
            }
            if (MODE == SPEC_FWD) {
                st2(uint32_t(ka), Xk);
                if (!self || mid) st2(uint32_t(kb), Xmk);
                continue;
            }
            const double* lamd = a.lam + a.lam_off[a.d];
            const double l1 = lamd[ka];
            Xk.x *= a.inv_n / (lc0[la] + lc1[la] * l1);
            Xk.y *= a.inv_n / (lc0[lb] + lc1[lb] * l1);
            if (!self || mid) {
                const double l2 = lamd[kb];
                Xmk.x *= a.inv_n / (lc0[la] + lc1[la] * l2);
                Xmk.y *= a.inv_n / (lc0[lb] + lc1[lb] * l2);
            }
            put_v(k, Xk, Xmk);
        }
        if (MODE == SPEC_FWD) return;
    } else {
        for (int k = j; k < npl; k += TPL) {   // coefficients (k, m - k) from HBM
            const bool self = k == 0, mid = self && !(m & 1);
            const double2 Xk = ld2(uint32_t(k));
            const double2 Xmk = (!self || mid) ? ld2(uint32_t(self ? half : m - k)) : make_double2(0.0, 0.0);
            put_v(k, Xk, Xmk);
        }
    }
    zero_pad();
    __syncthreads();
    convolve([&](int n) { return X[spec8::slot(n, cx)]; }, a.bvi);
    for (int k = j; k < m; k += TPL) {   // sample k = conj c[n] conv[n], n its Makhoul position
        const int n = (k & 1) ? m - 1 - (k >> 1) : (k >> 1);
        st2(uint32_t(k), cmul(X[spec8::slot(n, cx)], cconj(chirp[n])));
    }
}

// k_dctb8's tile: k_dct8's default real lines per workgroup (16, fewer for M > 512), at least one wave of threads
template <int L>
constexpr int dctb8_tq() {
    constexpr int TQ = spec8::Shape<L>::TQ, TPL = spec8::Shape<L>::TPL;
    return TQ < 2 ? 2 : ((TQ / 2) * TPL >= 64 ? TQ : 2 * (64 / TPL));
}

template <int L, int TQW>
static void launch_dctb8_t(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    const dim3 grid((a.nlines + uint32_t(TQW) - 1) / uint32_t(TQW)), block(spec8::ShapeK<L, TQW>::NT);
#define MVTV_DCTB8(MODE, D0, FB) klaunch(k_dctb8<L, MODE, D0, FB, TQW>, grid, block, 0, s, a)
    if (mode == SPEC_FWD) {
        if (d0) {
            if (formb) MVTV_DCTB8(SPEC_FWD, true, true);
            else MVTV_DCTB8(SPEC_FWD, true, false);
        } else {
            MVTV_DCTB8(SPEC_FWD, false, false);
        }
    } else if (mode == SPEC_INV) {
        if (d0) MVTV_DCTB8(SPEC_INV, true, false);
        else MVTV_DCTB8(SPEC_INV, false, false);
    } else {
        if (d0) {
            if (formb) MVTV_DCTB8(SPEC_MID, true, true);
            else MVTV_DCTB8(SPEC_MID, true, false);
        } else {
            MVTV_DCTB8(SPEC_MID, false, false);
        }
    }
#undef MVTV_DCTB8
}

// few lines (a 2-D mesh: 251 lines of 251): one line pair per workgroup where that is >= one wave of threads
// (M >= 512), the default tile is >= 8 lines (M <= 1024) and leaves < 512 workgroups: 251^2 12851 / 12874 -> 16902 /
// 16751 ADMM it/s; at M = 2048 (1009^2: 253 workgroups of 4 lines) one pair was slower, 8356 -> 8061
// (profiles/r05/v14_few_lines_bluestein; probe builds: MVTV_FEW_LINES_OFF=1)
template <int L>
static void launch_dctb8_l(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    constexpr int TQW = dctb8_tq<L>();
    static const bool few_off = probe_flag("MVTV_FEW_LINES_OFF");
    if constexpr (L >= 9 && L <= 10 && TQW > 2) {
        if (!few_off && (a.nlines + uint32_t(TQW) - 1) / uint32_t(TQW) < 512u)
            return launch_dctb8_t<L, 2>(a, s, mode, d0, formb);
    }
    launch_dctb8_t<L, TQW>(a, s, mode, d0, formb);
}

static hipError_t launch_dctb(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    switch (a.L) {   // M = 2^L: 11 <= m <= 4096 gives L = 5 .. 13
        case 5: launch_dctb8_l<5>(a, s, mode, d0, formb); return hipGetLastError();
        case 6: launch_dctb8_l<6>(a, s, mode, d0, formb); return hipGetLastError();
        case 7: launch_dctb8_l<7>(a, s, mode, d0, formb); return hipGetLastError();
        case 8: launch_dctb8_l<8>(a, s, mode, d0, formb); return hipGetLastError();
        case 9: launch_dctb8_l<9>(a, s, mode, d0, formb); return hipGetLastError();
        case 10: launch_dctb8_l<10>(a, s, mode, d0, formb); return hipGetLastError();
        case 11: launch_dctb8_l<11>(a, s, mode, d0, formb); return hipGetLastError();
        case 12: launch_dctb8_l<12>(a, s, mode, d0, formb); return hipGetLastError();
        case 13: launch_dctb8_l<13>(a, s, mode, d0, formb); return hipGetLastError();
        default: return hipErrorInvalidValue;
    }
}

// =============================================================================================
// Last dimension by a tridiagonal solve instead of DCT / divide / inverse DCT.
//
// After the forward transforms along dims 0..p-2, line q of the last dimension d carries the 1-D
// operator c0(q) I + c1(q) T, T = D1^T D1 = tridiag(-1, [1, 2, ..., 2, 1], -1) (the Neumann
// Laplacian the DCT along d would diagonalise: mu = c0 + c1 lam_d(k)). Solving it directly costs
// ~6 flops per element against two length-m FFTs, a divide and the DCT pre/post twiddles, with the
// same 2N words of HBM traffic; the pass stops being VALU/latency bound.
//
// The line is cut into segments of SEG consecutive rows, one thread each; the Neumann ends are the mirror
// conditions x[-1] = x[0], x[m] = x[m-1]. The result is the exact solve (the system is strictly diagonally
// dominant: c0 > 0, c1 >= 0), scaled by inv_n * m_d (the normalisation of the transforms along the other dims).
// (The first form, k_tri, was a partitioned Thomas elimination with the segments' neighbours kept symbolic and a
// 2 x NSEG interface system per line; the factorised form below replaced it in round 6, DESIGN.md section 4.1. It
// was removed and last existed in commit ae72d5c.)
namespace tri {
constexpr int TQ = 16;    // lines per workgroup: one 128-B row per position (d > 0)
}  // namespace tri

// ---------------------------------------------------------------------------------------------
// k_trir: the line solves by the factorised operator (round 6). c0 I + c1 T is, away from the ends,
// -c1 x[i-1] + (c0 + 2 c1) x[i] - c1 x[i+1] = kappa (1 - r S+)(1 - r S-) with r the root in (0, 1) of
// c1 r^2 - (c0 + 2 c1) r + c1 = 0; its Green's function is r^|k| / D with D = sqrt(c0 (c0 + 4 c1)). The
// Neumann ends are the mirror conditions, so the line's solve is the bi-infinite one on the even extension of
// the data: x_i = (F_i + B_i - f_i) / D with the two first-order recursions
//     F_i = f_i + r F_{i-1} (forward),      B_i = f_i + r B_{i+1} (backward),
// closed by the mirror: F_{-1} = B_0 and B_m = F_{m-1} (a 2 x 2 system with determinant 1 - r^2m).
// Segment-parallel: a thread runs both recursions over its SEG rows from zero (two independent chains),
// one thread per line combines the segments' sums into every segment's carries (F into its first row, B into
// its last) and closes the mirror, and every thread reruns the recursions with its carries. No divide per row,
// no per-row line constants (the Thomas form kept four [SEG][TQ] tables in ~97 KB of LDS, so one workgroup fit a CU,
// and eliminated the interface on one wave with a divide per step); LDS here is 2 sums per segment and five
// constants per line. r = 2 c1 / (c0 + 2 c1 + D) and 1 - r = (c0 + D) / (c0 + 2 c1 + D) are cancellation-free;
// 1 - r^k by t_2k = t_k (2 - t_k). Against a long-double Thomas solve (numpy transcription): 1e-15 at
// c1 / c0 = 1e2, 3e-14 at 1e7 relative (an LU solve of the same system: 2e-11 at 1e7).
namespace trir {
template <int L, int SEG, int TQL>
struct Shape {
    static constexpr int M = 1 << L;
    static constexpr int NSEG = M / SEG;
    static constexpr int NT = TQL * NSEG;
};
}  // namespace trir

template <int L, int SEG, int TQL>
__global__ __launch_bounds__((trir::Shape<L, SEG, TQL>::NT), (SEG <= 16 ? 8 : 4)) void k_trir(const SpecArgs a) {
    using S = trir::Shape<L, SEG, TQL>;
    constexpr int TQ = TQL, NSEG = S::NSEG;
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double s_f[NSEG][TQ], s_b[NSEG][TQ];   // segment sums from zero, then the segments' carries
    __shared__ double s_r[TQ], s_sd[TQ];               // r, scale / D per line
    const int t = threadIdx.x, c = t % TQ, sj = t / TQ;
    const uint32_t bx = a.xcd ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const uint32_t q0 = bx * uint32_t(TQ);
    const uint32_t q = q0 + uint32_t(c);
    const bool valid = q < a.nlines;
    const uint32_t base = (q & (a.stride - 1)) + ((q >> a.ls) << (a.ls + L)) + (uint32_t(sj * SEG) << a.ls);

    double lamv[kMaxDims] = {0, 0, 0, 0};
    if (t < TQ) {
        const uint32_t ql = a.q_off + (valid ? q : q0);
        uint32_t rest = ql;
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int jj = 0; jj < a.p; ++jj) {
            if (jj == a.d) continue;
            const uint32_t qq = (jj < jlast) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qq * a.m[jj])];
            rest = qq;
        }
    }
    double g[SEG];
#pragma unroll
    for (int i = 0; i < SEG; ++i) g[i] = valid ? __builtin_nontemporal_load(a.in + base + (uint32_t(i) << a.ls)) : 0.0;

    double rm = 0.0, idet = 1.0, rseg = 0.0;   // t < TQ: r^m, 1 / (1 - r^2m), r^SEG
    if (t < TQ) {
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p; ++jj)
                if (jj != a.d && ((Sm >> jj) & 1)) prod *= lamv[jj];
            if ((Sm >> a.d) & 1) c1 += prod;
            else c0 += prod;
        }
        const double D = sqrt(c0 * (c0 + 4.0 * c1));
        const double den = 1.0 / (c0 + 2.0 * c1 + D);
        const double r = 2.0 * c1 * den;
        double pk = r, tk = (c0 + D) * den;   // r^k, 1 - r^k at k = 1
#pragma unroll
        for (int k = 1; k < SEG; k <<= 1) {
            pk *= pk;
            tk *= 2.0 - tk;
        }
        rseg = pk;
#pragma unroll
        for (int k = SEG; k < S::M; k <<= 1) {
            pk *= pk;
            tk *= 2.0 - tk;
        }
        rm = pk;
        idet = 1.0 / (tk * (2.0 - tk));   // 1 / (1 - r^2m)
        s_r[c] = r;
        s_sd[c] = a.inv_n * double(S::M) / D;
    }
    __syncthreads();

    const double r = s_r[c];
    {
        // both recursions over this segment from zero: two independent chains
        double fl = 0.0, bl = 0.0;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            fl = fma(r, fl, g[i]);
            bl = fma(r, bl, g[SEG - 1 - i]);
        }
        s_f[sj][c] = fl;
        s_b[sj][c] = bl;
    }
    __syncthreads();

    if (t < TQ) {
        // carries: F into segment j's first row = sum_{k<j} r^{SEG(j-1-k)} fl_k + r^{SEG j} F_{-1}, B likewise from
        // the right; F_{-1} = B_0 and B_m = F_{m-1} close the mirror
        double acc = 0.0, bcc = 0.0;
#pragma unroll 8
        for (int k = 0; k < NSEG; ++k) {
            const double fk = s_f[k][c], bk = s_b[NSEG - 1 - k][c];
            s_f[k][c] = acc;
            s_b[NSEG - 1 - k][c] = bcc;
            acc = fma(acc, rseg, fk);
            bcc = fma(bcc, rseg, bk);
        }
        const double fm1 = (bcc + rm * acc) * idet, bm = (acc + rm * bcc) * idet;
        double pw = 1.0;
#pragma unroll 8
        for (int k = 0; k < NSEG; ++k) {
            s_f[k][c] = fma(pw, fm1, s_f[k][c]);
            s_b[NSEG - 1 - k][c] = fma(pw, bm, s_b[NSEG - 1 - k][c]);
            pw *= rseg;
        }
    }
    __syncthreads();

    if (!valid) return;
    const double sd = s_sd[c], bin = s_b[sj][c];
    double fv = s_f[sj][c];
    // g <- B (backward with the carry), then x_i = (B_i + r F_{i-1}) / D, F_i = B_i + r (F_{i-1} - B_{i+1})
    {
        double bv = bin;
#pragma unroll
        for (int i = SEG - 1; i >= 0; --i) {
            bv = fma(r, bv, g[i]);
            g[i] = bv;
        }
    }
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        const double gn = i + 1 < SEG ? g[i + 1] : bin;
        __builtin_nontemporal_store(sd * fma(r, fv, g[i]), a.out + base + (uint32_t(i) << a.ls));
        fv = fma(r, fv - gn, g[i]);
    }
}

// The general lines: the same solve for any line length m = (NSEG - 1) * s + sr (segment length s <= SMAX chosen at
// launch, NSEG <= NS, the last segment sr <= s rows; m may have no divisor in the segment range, e.g. a prime length)
// and any line stride (FastDiv addressing): the last-dimension pass of the mixed-radix and prime-length meshes. Rows
// past a segment's length in the fixed-size register arrays are predicated off. TQ lines per workgroup: 16 (128-B
// rows, any block of <= 64 segments) or, where the block fits 1024 threads, 32 / 64 (256- / 512-B rows) with the
// segment arrays sized to the block (the slab solve's tiles)
namespace trig {
constexpr int SMAX = 32, NSMAX = 64, TQ = 16;
}

// (r^k, 1 - r^k) pairs: products and powers keep 1 - r^k free of cancellation (1 - r^(a+b) = t_a + r^a t_b)
struct PowT {
    double p, t;
};
__device__ __forceinline__ PowT powt_mul(PowT a, PowT b) { return {a.p * b.p, fma(a.p, b.t, a.t)}; }
__device__ __forceinline__ PowT powt_pow(PowT x, uint32_t n) {
    PowT y{1.0, 0.0};
    while (n) {
        if (n & 1u) y = powt_mul(y, x);
        x = powt_mul(x, x);
        n >>= 1;
    }
    return y;
}

// k_trigr: k_trir's factorised solve for the general lines (any length m = (nseg - 1) sl + sr, any stride; a shorter
// last segment sr <= sl). Segment j's carries go through r^len_j; the mirror closure through r^m.
template <int SMAX, int TQ, int NS>
__global__ __launch_bounds__(1024) void k_trigr(const SpecArgs a, int sl, int nseg, int sr) {
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double s_f[NS][TQ], s_b[NS][TQ];
    __shared__ double s_r[TQ], s_sd[TQ];
    const int t = threadIdx.x, c = t % TQ, sj = t / TQ;
    const int ln = sj == nseg - 1 ? sr : sl;   // this thread's segment length
    const uint32_t m = a.m[a.d];
    const uint32_t q0 = (a.xrun ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x) * uint32_t(TQ);
    const uint32_t q = q0 + uint32_t(c);
    const bool valid = q < a.nlines;
    const uint32_t qq = valid ? q : q0;
    const uint32_t hi = a.fds.div(qq);
    const uint32_t base = (qq - hi * a.stride) + hi * a.stride * m + uint32_t(sj * sl) * a.stride;

    double lamv[kMaxDims] = {0, 0, 0, 0};
    if (t < TQ) {
        uint32_t rest = a.q_off + qq;
        const int jlast = a.d == a.p - 1 ? a.p - 2 : a.p - 1;
        for (int jj = 0; jj < a.p; ++jj) {
            if (jj == a.d) continue;
            const uint32_t qd = (jj < jlast) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
            rest = qd;
        }
    }
    double g[SMAX];
    {
        const double* pin = a.in + base;
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            g[i] = (valid && i < ln) ? __builtin_nontemporal_load(pin) : 0.0;
            pin += a.stride;
        }
    }

    double rsl = 0.0, rsr = 0.0, rm = 0.0, idet = 1.0;   // t < TQ: r^sl, r^sr, r^m, 1 / (1 - r^2m)
    if (t < TQ) {
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p; ++jj)
                if (jj != a.d && ((Sm >> jj) & 1)) prod *= lamv[jj];
            if ((Sm >> a.d) & 1) c1 += prod;
            else c0 += prod;
        }
        const double D = sqrt(c0 * (c0 + 4.0 * c1));
        const double den = 1.0 / (c0 + 2.0 * c1 + D);
        const PowT r1{2.0 * c1 * den, (c0 + D) * den};
        const PowT ps = powt_pow(r1, uint32_t(sl)), pr = powt_pow(r1, uint32_t(sr));
        const PowT pm = powt_mul(powt_pow(ps, uint32_t(nseg - 1)), pr);
        rsl = ps.p;
        rsr = pr.p;
        rm = pm.p;
        idet = 1.0 / powt_mul(pm, pm).t;
        s_r[c] = r1.p;
        s_sd[c] = a.inv_n * double(m) / D;
    }
    __syncthreads();

    const double r = s_r[c];
    {
        double fl = 0.0, bl = 0.0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            if (i < ln) fl = fma(r, fl, g[i]);
            bl = fma(r, bl, g[SMAX - 1 - i]);   // rows past ln are 0: bl stays 0 until row ln - 1
        }
        s_f[sj][c] = fl;
        s_b[sj][c] = bl;
    }
    __syncthreads();

    if (t < TQ) {
        double acc = 0.0, bcc = 0.0;
        for (int k = 0; k < nseg; ++k) {
            const int kb = nseg - 1 - k;
            const double fk = s_f[k][c], bk = s_b[kb][c];
            s_f[k][c] = acc;
            s_b[kb][c] = bcc;
            acc = fma(acc, k == nseg - 1 ? rsr : rsl, fk);
            bcc = fma(bcc, k == 0 ? rsr : rsl, bk);
        }
        const double fm1 = (bcc + rm * acc) * idet, bm = (acc + rm * bcc) * idet;
        double pf = 1.0, pb = 1.0;
        for (int k = 0; k < nseg; ++k) {
            const int kb = nseg - 1 - k;
            s_f[k][c] = fma(pf, fm1, s_f[k][c]);
            s_b[kb][c] = fma(pb, bm, s_b[kb][c]);
            pf *= rsl;
            pb *= k == 0 ? rsr : rsl;
        }
    }
    __syncthreads();

    if (!valid) return;
    const double sd = s_sd[c], bin = s_b[sj][c];
    double fv = s_f[sj][c];
    {
        double bv = bin;
#pragma unroll
        for (int i = SMAX - 1; i >= 0; --i)
            if (i < ln) {
                bv = fma(r, bv, g[i]);
                g[i] = bv;
            }
    }
    double* pout = a.out + base;
#pragma unroll
    for (int i = 0; i < SMAX; ++i)
        if (i < ln) {
            const double gn = i + 1 < ln ? g[i + 1] : bin;
            __builtin_nontemporal_store(sd * fma(r, fv, g[i]), pout);
            pout += a.stride;
            fv = fma(r, fv - gn, g[i]);
        }
}

// =============================================================================================
// The last dimension of a slab-decomposed mesh (mvtv_slab.cpp): the same tridiagonal line solves, with
// every line cut at the rank boundaries, solved by substructuring instead of transposing the mesh.
//
// Rank r holds rows [zb_r, ze_r) of every line (its owned planes). Its local block of the line's
// operator, with the neighbours x[zb_r - 1] = L and x[ze_r] = R as unknowns (a mirror at the mesh's own
// ends), has the solution x = G + L H + R K (G: the data with L = R = 0; H, K: the responses to L = 1 and
// R = 1). Phase 1 computes, per line, what the rank's block contributes to the interface without writing the mesh;
// the interface system that couples the ranks' (first, last) rows of a line is solved where the line's chunk lives
// (one thread per line, O(G)); phase 3 solves the local block again with the now known neighbours and writes x.
// The ranks exchange a few numbers per line instead of the 2 x (owned planes) numbers per line of two transposes:
// at 512^3 over 8 ranks 15 MB (the Thomas form's 6 + 2 numbers; the factorised form below sends 2 + 2) instead of
// 235 MB per rank per iteration. Within a rank the block is cut into nseg segments of sl rows, one thread each.
// (The Thomas form, k_tris / k_tris_iface, was removed; it last existed in commit ae72d5c.)
namespace tris {
constexpr int NSMAX = 64, TQ = 16;
}

// The slab line solves by the factorised operator (round 6; k_trir's recursions F_i = f_i + r F_{i-1},
// B_i = f_i + r B_{i+1}, x = (F + B - f) / D). A rank's block of a line enters the global recursions only through
// two numbers: F at its last row and B at its first row, each from zero carries (phase 1). The chunk owner combines
// the ranks' pairs with the multipliers r^n_r of the block lengths and closes the mirror (k_trisr_iface): every
// block's carries, F into its first row and B into its last. Phase 3 reruns the block's recursions from them. Two
// numbers per line cross the ranks each way (6 + 2 with the Thomas responses), and no step divides per row.
// TQ lines per workgroup (16: 128-B rows; 64: 512-B rows, one full run per wave load), NS >= nseg segments (the LDS
// of the segment sums is sized by it)
template <int PHASE, int SMAX, int TQ = tris::TQ, int NS = tris::NSMAX>
__global__ __launch_bounds__(1024) void k_trisr(const SpecArgs a, int sl, int nseg, double* __restrict__ x,
                                                double* __restrict__ coef, const double* __restrict__ lr,
                                                uint32_t chunk, int, int, double scale) {
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double s_f[NS][TQ], s_b[NS][TQ];
    __shared__ double s_r[TQ], s_sd[TQ];
    const int t = threadIdx.x, c = t % TQ, sj = t / TQ;
    const uint32_t q0 = blockIdx.x * uint32_t(TQ);
    const uint32_t q = q0 + uint32_t(c);
    const bool valid = q < a.nlines;
    const uint32_t qq = valid ? q : q0;
    const size_t base = size_t(qq) + size_t(sj * sl) * a.stride;   // lines are contiguous: stride = plane

    double lamv[kMaxDims] = {0, 0, 0, 0};
    if (t < TQ) {
        uint32_t rest = qq;
        for (int jj = 0; jj < a.p - 1; ++jj) {
            const uint32_t qd = (jj < a.p - 2) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
            rest = qd;
        }
    }
    double g[SMAX];
#pragma unroll
    for (int i = 0; i < SMAX; ++i)
        g[i] = (valid && i < sl) ? __builtin_nontemporal_load(x + base + size_t(i) * a.stride) : 0.0;
    double fin = 0.0, bout = 0.0, rsl = 0.0;   // t < TQ, phase 3: the block's carries; r^sl
    if (t < TQ) {
        if (PHASE == 3) {
            const uint32_t s = qq / chunk, l = qq - s * chunk;
            fin = lr[(size_t(s) * 2) * chunk + l];
            bout = lr[(size_t(s) * 2 + 1) * chunk + l];
        }
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p - 1; ++jj)
                if ((Sm >> jj) & 1) prod *= lamv[jj];
            if ((Sm >> (a.p - 1)) & 1) c1 += prod;
            else c0 += prod;
        }
        const double D = sqrt(c0 * (c0 + 4.0 * c1));
        const double den = 1.0 / (c0 + 2.0 * c1 + D);
        const PowT r1{2.0 * c1 * den, (c0 + D) * den};
        rsl = powt_pow(r1, uint32_t(sl)).p;
        s_r[c] = r1.p;
        s_sd[c] = scale / D;
    }
    __syncthreads();

    const double r = s_r[c];
    {
        double fl = 0.0, bl = 0.0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            if (i < sl) fl = fma(r, fl, g[i]);
            bl = fma(r, bl, g[SMAX - 1 - i]);   // rows past sl are 0
        }
        s_f[sj][c] = fl;
        s_b[sj][c] = bl;
    }
    __syncthreads();

    if (t < TQ) {
        // phase 1: the block's F at its last row and B at its first row from zero carries; phase 3: every
        // segment's carries from the block's
        double acc = PHASE == 3 ? fin : 0.0, bcc = PHASE == 3 ? bout : 0.0;
        for (int k = 0; k < nseg; ++k) {
            const int kb = nseg - 1 - k;
            const double fk = s_f[k][c], bk = s_b[kb][c];
            if (PHASE == 3) {
                s_f[k][c] = acc;
                s_b[kb][c] = bcc;
            }
            acc = fma(acc, rsl, fk);
            bcc = fma(bcc, rsl, bk);
        }
        if (PHASE == 1 && valid) {   // [chunk s][2][line in chunk]: F_last, B_first
            const uint32_t s = q / chunk, l = q - s * chunk;
            coef[(size_t(s) * 2) * chunk + l] = acc;
            coef[(size_t(s) * 2 + 1) * chunk + l] = bcc;
        }
    }
    if constexpr (PHASE == 3) {
        __syncthreads();
        if (!valid) return;
        const double sd = s_sd[c], bin = s_b[sj][c];
        double fv = s_f[sj][c];
        {
            double bv = bin;
#pragma unroll
            for (int i = SMAX - 1; i >= 0; --i)
                if (i < sl) {
                    bv = fma(r, bv, g[i]);
                    g[i] = bv;
                }
        }
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if (i < sl) {
                const double gn = i + 1 < sl ? g[i + 1] : bin;
                __builtin_nontemporal_store(sd * fma(r, fv, g[i]), x + base + size_t(i) * a.stride);
                fv = fma(r, fv - gn, g[i]);
            }
    }
}

// the chunk owner's lines (global line q = rank * chunk + l): from every rank's (F_last, B_first) [r][2][chunk] the
// carries of every rank's block, (F into its first row, B into its last) [r][2][chunk], with the mirror closure at the
// mesh's ends. Rank k's block: planes [floor(mg k / G), floor(mg (k + 1) / G)).
__global__ __launch_bounds__(256) void k_trisr_iface(const SpecArgs a, const double* __restrict__ co,
                                                     double* __restrict__ lr, uint32_t chunk, int G, int rank,
                                                     uint32_t mg) {
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= chunk) return;
    const size_t C = chunk;
    double lamv[kMaxDims] = {0, 0, 0, 0};
    uint32_t rest = uint32_t(rank) * chunk + l;
    for (int jj = 0; jj < a.p - 1; ++jj) {
        const uint32_t qd = (jj < a.p - 2) ? a.fd[jj].div(rest) : 0u;
        lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
        rest = qd;
    }
    double c0 = a.w0, c1 = 0.0;
    for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
        if (a.cS[Sm] == 0.0) continue;
        double prod = sigma * a.cS[Sm];
        for (int jj = 0; jj < a.p - 1; ++jj)
            if ((Sm >> jj) & 1) prod *= lamv[jj];
        if ((Sm >> (a.p - 1)) & 1) c1 += prod;
        else c0 += prod;
    }
    const double D = sqrt(c0 * (c0 + 4.0 * c1));
    const double den = 1.0 / (c0 + 2.0 * c1 + D);
    const PowT r1{2.0 * c1 * den, (c0 + D) * den};
    // the multipliers r^n_k of the blocks: n_k = floor(mg (k + 1) / G) - floor(mg k / G) takes two values at most
    const uint32_t nlo = mg / uint32_t(G);
    const PowT plo = powt_pow(r1, nlo);
    const double rlo = plo.p, rhi = plo.p * r1.p;
    auto rblk = [&](int k) {
        const uint32_t n = uint32_t(uint64_t(mg) * uint64_t(k + 1) / uint64_t(G) - uint64_t(mg) * uint64_t(k) / uint64_t(G));
        return n == nlo ? rlo : rhi;
    };
    // forward: F into block k's first row from the blocks before it (zero at the mesh's start)
    double acc = 0.0;
    for (int k = 0; k < G; ++k) {
        lr[(size_t(k) * 2) * C + l] = acc;
        acc = fma(acc, rblk(k), co[(size_t(k) * 2) * C + l]);
    }
    double bcc = 0.0;
    for (int k = G - 1; k >= 0; --k) {
        lr[(size_t(k) * 2 + 1) * C + l] = bcc;
        bcc = fma(bcc, rblk(k), co[(size_t(k) * 2 + 1) * C + l]);
    }
    const PowT pm = powt_pow(r1, mg);
    const double idet = 1.0 / powt_mul(pm, pm).t;
    const double fm1 = (bcc + pm.p * acc) * idet, bm = (acc + pm.p * bcc) * idet;
    double pf = 1.0, pb = 1.0;
    for (int k = 0; k < G; ++k) {
        const int kb = G - 1 - k;
        lr[(size_t(k) * 2) * C + l] = fma(pf, fm1, lr[(size_t(k) * 2) * C + l]);
        lr[(size_t(kb) * 2 + 1) * C + l] = fma(pb, bm, lr[(size_t(kb) * 2 + 1) * C + l]);
        pf *= rblk(k);
        pb *= rblk(kb);
    }
}

// ---------------------------------------------------------------------------------------------
// The last dimension of any length on one GPU: the same substructuring with the blocks of one line as the "ranks".
// The line's m rows split into nblk blocks [floor(m k / nblk), floor(m (k + 1) / nblk)) (k_trisr_iface's rule: two
// block lengths at most). Phase 1 runs every block's recursions from zero carries and leaves (F at its last row, B at
// its first) in coef [block][2][line]; the interface turns them into every block's carries lr [block][2][line] and
// closes the mirror; phase 3 reruns the block from its carries and writes the solve. Phase 1 only reads: 3N words and
// 2 nblk nlines doubles each way per solve, against the 2N of a line that fits one workgroup.
//
// k_trib (p >= 2): k_trigr's tile (TQ adjacent lines x NS segments of sl <= SMAX rows) on a (line tile x block) grid,
// tile fastest. A block of n rows has n / sl whole segments, one of n % sl rows and empty ones after it (the longer
// block length sizes the workgroup); a segment's multiplier is r^rows, 1 for an empty one. d = p - 1: the line stride
// is the plane, nlines of them, any count and any stride.
//
// Multipliers. A long line at a large sigma has r close to 1 in every line that matters (p = 1: c1 / c0 = sigma w^2 in
// the one line there is), and the recursions' gain 1 / (1 - r) turns the half-ulp that rounding r to a double loses
// into a relative 1e-16 / (1 - r) of the whole solve (4e-14 at c1 / c0 = 2e5: a systematic error of the constant
// component, above the forward-error bound of the tests). So every multiplier here is a pair h + l: h = 1 - t rounded
// and l = (1 - h) - t, exact where h >= 1/2, from the cancellation-free t = 1 - r^n; t_n comes from t alone
// (t_{a+b} = t_a + t_b - t_a t_b: a few eps relative for any n), never from powers of the rounded r.
namespace trib {
constexpr int SMAX = 32;
}

// tpow, Mul2 and its helpers: mvtv_device.h (shared with mvtv_small_cos.hip)

template <int PHASE, int SMAX, int TQ, int NS>
__global__ __launch_bounds__((TQ * NS)) void k_trib(const SpecArgs a, int sl, uint32_t nblk, uint32_t ntile,
                                                    double* __restrict__ coef, const double* __restrict__ lr) {
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double s_f[NS][TQ], s_b[NS][TQ];
    __shared__ double s_rh[TQ], s_rl[TQ], s_sd[TQ];
    const int t = threadIdx.x, c = t % TQ, sj = t / TQ;
    const int nseg = int(blockDim.x) / TQ;
    const uint32_t kb = blockIdx.x / ntile, tile = blockIdx.x - kb * ntile;
    const uint32_t m = a.m[a.d];
    const uint32_t lo = uint32_t(uint64_t(m) * kb / nblk), hi = uint32_t(uint64_t(m) * (kb + 1) / nblk);
    const int n = int(hi - lo);
    const int ln = min(max(n - sj * sl, 0), sl);   // this thread's segment length
    const uint32_t q0 = tile * uint32_t(TQ);
    const uint32_t q = q0 + uint32_t(c);
    const bool valid = q < a.nlines;
    const uint32_t qq = valid ? q : q0;
    const size_t base = size_t(qq) + (size_t(lo) + size_t(sj * sl)) * a.stride;

    double lamv[kMaxDims] = {0, 0, 0, 0};
    if (t < TQ) {
        uint32_t rest = a.q_off + qq;
        for (int jj = 0; jj < a.p - 1; ++jj) {
            const uint32_t qd = (jj < a.p - 2) ? a.fd[jj].div(rest) : 0u;
            lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
            rest = qd;
        }
    }
    double g[SMAX];
    {
        const double* pin = a.in + base;
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            g[i] = (valid && i < ln) ? __builtin_nontemporal_load(pin) : 0.0;
            pin += a.stride;
        }
    }
    const int nfull = n / sl, rem = n - nfull * sl;   // whole segments, the rows of the one after them
    Mul2 rsl{0.0, 0.0}, rrem{1.0, 0.0};               // t < TQ: r^sl, r^rem
    if (t < TQ) {
        double c0 = a.w0, c1 = 0.0;
        for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
            if (a.cS[Sm] == 0.0) continue;
            double prod = sigma * a.cS[Sm];
            for (int jj = 0; jj < a.p - 1; ++jj)
                if ((Sm >> jj) & 1) prod *= lamv[jj];
            if ((Sm >> (a.p - 1)) & 1) c1 += prod;
            else c0 += prod;
        }
        const double D = sqrt(c0 * (c0 + 4.0 * c1));
        const double den = 1.0 / (c0 + 2.0 * c1 + D);
        const double t1 = (c0 + D) * den;   // 1 - r
        rsl = mul2_from_t(tpow(t1, uint32_t(sl)));
        rrem = mul2_from_t(tpow(t1, uint32_t(rem)));
        const Mul2 r1 = mul2_from_t(t1);
        s_rh[c] = r1.h;
        s_rl[c] = r1.l;
        s_sd[c] = a.inv_n * double(m) / D;
    }
    __syncthreads();

    const Mul2 r{s_rh[c], s_rl[c]};
    {
        double fl = 0.0, bl = 0.0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            if (i < ln) fl = mul2_mac(r, fl, g[i]);
            bl = mul2_mac(r, bl, g[SMAX - 1 - i]);   // rows past ln are 0
        }
        s_f[sj][c] = fl;
        s_b[sj][c] = bl;
    }
    __syncthreads();

    if (t < TQ) {
        // phase 1: the block's F at its last row and B at its first row from zero carries; phase 3: every
        // segment's carries from the block's
        double acc = 0.0, bcc = 0.0;
        if (PHASE == 3) {
            acc = lr[(size_t(kb) * 2) * a.nlines + qq];
            bcc = lr[(size_t(kb) * 2 + 1) * a.nlines + qq];
        }
        auto mult = [&](int k) { return k < nfull ? rsl : (k == nfull ? rrem : Mul2{1.0, 0.0}); };
        for (int k = 0; k < nseg; ++k) {
            const int kr = nseg - 1 - k;
            const double fk = s_f[k][c], bk = s_b[kr][c];
            if (PHASE == 3) {
                s_f[k][c] = acc;
                s_b[kr][c] = bcc;
            }
            acc = mul2_mac(mult(k), acc, fk);
            bcc = mul2_mac(mult(kr), bcc, bk);
        }
        if (PHASE == 1 && valid) {
            coef[(size_t(kb) * 2) * a.nlines + q] = acc;
            coef[(size_t(kb) * 2 + 1) * a.nlines + q] = bcc;
        }
    }
    if constexpr (PHASE == 3) {
        __syncthreads();
        if (!valid) return;
        const double sd = s_sd[c], bin = s_b[sj][c];
        double fv = s_f[sj][c];
        {
            double bv = bin;
#pragma unroll
            for (int i = SMAX - 1; i >= 0; --i)
                if (i < ln) {
                    bv = mul2_mac(r, bv, g[i]);
                    g[i] = bv;
                }
        }
        double* pout = a.out + base;
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if (i < ln) {
                const double gn = i + 1 < ln ? g[i + 1] : bin;
                __builtin_nontemporal_store(sd * mul2_mac(r, fv, g[i]), pout);
                pout += a.stride;
                fv = mul2_mac(r, fv - gn, g[i]);
            }
    }
}

// k_trib's interface: one thread per line walks the nblk blocks twice (k_trisr_iface's steps with the multipliers as
// pairs): the line's totals from zero carries, the mirror closure, then every block's carries in order.
__global__ __launch_bounds__(256) void k_trib_iface(const SpecArgs a, const double* __restrict__ co,
                                                    double* __restrict__ lr, uint32_t nblk) {
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.nlines) return;
    const size_t C = a.nlines;
    double lamv[kMaxDims] = {0, 0, 0, 0};
    uint32_t rest = a.q_off + l;
    for (int jj = 0; jj < a.p - 1; ++jj) {
        const uint32_t qd = (jj < a.p - 2) ? a.fd[jj].div(rest) : 0u;
        lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
        rest = qd;
    }
    double c0 = a.w0, c1 = 0.0;
    for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
        if (a.cS[Sm] == 0.0) continue;
        double prod = sigma * a.cS[Sm];
        for (int jj = 0; jj < a.p - 1; ++jj)
            if ((Sm >> jj) & 1) prod *= lamv[jj];
        if ((Sm >> (a.p - 1)) & 1) c1 += prod;
        else c0 += prod;
    }
    const double D = sqrt(c0 * (c0 + 4.0 * c1));
    const double t1 = (c0 + D) / (c0 + 2.0 * c1 + D);
    const uint32_t m = a.m[a.d], nlo = m / nblk;
    const double tlo = tpow(t1, nlo);
    const Mul2 mlo = mul2_from_t(tlo), mhi = mul2_from_t(fma(-tlo, t1, tlo + t1));
    auto rblk = [&](uint32_t k) {
        const uint32_t nk = uint32_t(uint64_t(m) * (k + 1) / nblk - uint64_t(m) * k / nblk);
        return nk == nlo ? mlo : mhi;
    };
    double acc = 0.0, bcc = 0.0;
    for (uint32_t k = 0; k < nblk; ++k) acc = mul2_mac(rblk(k), acc, co[(size_t(k) * 2) * C + l]);
    for (uint32_t k = nblk; k > 0; --k) bcc = mul2_mac(rblk(k - 1), bcc, co[(size_t(k - 1) * 2 + 1) * C + l]);
    const double tm = tpow(t1, m), pm = 1.0 - tm, idet = 1.0 / (tm * (2.0 - tm));   // r^m, 1 / (1 - r^2m)
    double f = (bcc + pm * acc) * idet, b = (acc + pm * bcc) * idet;                // F_{-1} = B_0, B_m = F_{m-1}
    for (uint32_t k = 0; k < nblk; ++k) {
        lr[(size_t(k) * 2) * C + l] = f;
        f = mul2_mac(rblk(k), f, co[(size_t(k) * 2) * C + l]);
    }
    for (uint32_t k = nblk; k > 0; --k) {
        lr[(size_t(k - 1) * 2 + 1) * C + l] = b;
        b = mul2_mac(rblk(k - 1), b, co[(size_t(k - 1) * 2 + 1) * C + l]);
    }
}

// Exclusive weighted scan over the workgroup's threads in order (REV: from the last thread down). Every thread holds
// v, the sum of its rows from a zero carry, and p, the multiplier r^rows of its span; (ev, ep) is what the threads
// before it make of a zero carry and their multiplier, tv the whole workgroup's sum. Wave shuffles, then the NW waves'
// pairs through LDS (s_v, s_h, s_l: NW doubles each). Every thread of the NW * 64 calls it.
template <int NW, bool REV>
__device__ __forceinline__ void wg_scan_pair(double v, Mul2 p, double* s_v, double* s_h, double* s_l, double& ev,
                                             Mul2& ep, double& tv) {
    const int lane = int(threadIdx.x) & 63, w = int(threadIdx.x) >> 6;
    auto from = [&](double x, int off) { return REV ? __shfl_down(x, off) : __shfl_up(x, off); };
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double lv = from(v, off);
        const Mul2 lp{from(p.h, off), from(p.l, off)};
        if (REV ? lane + off < 64 : lane >= off) {
            v = mul2_mac(p, lv, v);
            p = mul2_mul(p, lp);
        }
    }
    if (lane == (REV ? 0 : 63)) {
        s_v[w] = v;
        s_h[w] = p.h;
        s_l[w] = p.l;
    }
    double xv = from(v, 1);
    Mul2 xp{from(p.h, 1), from(p.l, 1)};
    if (lane == (REV ? 63 : 0)) {
        xv = 0.0;
        xp = Mul2{1.0, 0.0};
    }
    __syncthreads();
    double wv = 0.0;
    Mul2 wp{1.0, 0.0}, tp{1.0, 0.0};
    tv = 0.0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int kk = REV ? NW - 1 - k : k;
        if (kk == w) {
            wv = tv;
            wp = tp;
        }
        const Mul2 pk{s_h[kk], s_l[kk]};
        tv = mul2_mac(pk, tv, s_v[kk]);
        tp = mul2_mul(tp, pk);
    }
    ev = mul2_mac(xp, wv, xv);
    ep = mul2_mul(wp, xp);
    __syncthreads();
}

// k_tri1 (p = 1): one contiguous line, one constant r. A workgroup owns a block of <= NT * R rows; they move between
// memory and LDS as coalesced 16-B accesses (the block's first and last rows, which may sit in a pair's other half,
// and a line's odd last row singly), and thread t takes its R consecutive rows from LDS (pitch R + 1: the threads' rows
// on different banks). The threads' pairs combine by the weighted scan with multiplier r^rows. FORMB (the ADMM loop's
// only pass): phase 1 forms b = in + ca ga + cb gb on load and writes it to out, phase 3 reads it there: 6N words per
// solve, against the 7N of forming it twice.
namespace tri1 {
constexpr int NT = 256, R = 16, BL = NT * R;   // threads, rows per thread, rows per block at most
constexpr int NP = BL / 2 / NT + 1;            // 16-B pairs per thread over a block and its two edge pairs
}

template <int PHASE, bool FORMB>
__global__ __launch_bounds__(tri1::NT) void k_tri1(const SpecArgs a, uint32_t nblk, double* __restrict__ coef,
                                                   const double* __restrict__ lr) {
    using namespace tri1;
    double sigma = a.sigma, ca = a.ca, cb = a.cb;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
        ca = a.ctl->rho;
        cb = a.ctl->rho * a.ctl->c_prev;
    }
    __shared__ double s_x[BL + NT];   // row i of the block at i + i / R
    __shared__ double s_v[NT / 64], s_h[NT / 64], s_l[NT / 64];
    const int t = threadIdx.x;
    const uint32_t m = a.m[0], kb = blockIdx.x;
    const uint32_t lo = uint32_t(uint64_t(m) * kb / nblk), hi = uint32_t(uint64_t(m) * (kb + 1) / nblk);
    const int n = int(hi - lo);
    const double* src = (FORMB && PHASE == 3) ? a.out : a.in;
    const uint32_t e0 = (lo & ~1u) + 2u * uint32_t(t);   // this thread's first pair (16-B aligned)

    // line constants (p = 1: c0 = w0, c1 = sigma cS[{0}])
    const double c0 = a.w0, c1 = sigma * a.cS[1];
    const double D = sqrt(c0 * (c0 + 4.0 * c1));
    const double den = 1.0 / (c0 + 2.0 * c1 + D);
    const double t1 = (c0 + D) * den, sd = a.inv_n * double(m) / D;   // 1 - r
    const Mul2 r = mul2_from_t(t1);

#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t e = e0 + uint32_t(2 * NT * j);
        if (e >= hi) continue;
        const bool in0 = e >= lo, in1 = e + 1u < hi;   // in1 implies e + 1 < m
        double2 v;
        if (in1) {
            v = ldnt2(src + e);
            if (FORMB && PHASE == 1) {
                const double2 va = ldnt2(a.ga + e), vb = ldnt2(a.gb + e);
                v.x += ca * va.x + cb * vb.x;
                v.y += ca * va.y + cb * vb.y;
            }
        } else {
            v.x = __builtin_nontemporal_load(src + e);
            if (FORMB && PHASE == 1)
                v.x += ca * __builtin_nontemporal_load(a.ga + e) + cb * __builtin_nontemporal_load(a.gb + e);
            v.y = 0.0;
        }
        if (FORMB && PHASE == 1) {
            if (in0 && in1) stnt2(a.out + e, v);
            else if (in0) __builtin_nontemporal_store(v.x, a.out + e);
            else __builtin_nontemporal_store(v.y, a.out + e + 1);
        }
        const int i0 = int(e) - int(lo);
        if (in0) s_x[i0 + i0 / R] = v.x;
        if (in1) s_x[i0 + 1 + (i0 + 1) / R] = v.y;
    }
    __syncthreads();

    const int rows = min(max(n - t * R, 0), R);
    double g[R];
#pragma unroll
    for (int i = 0; i < R; ++i) g[i] = i < rows ? s_x[t * (R + 1) + i] : 0.0;
    double fl = 0.0, bl = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (i < rows) fl = mul2_mac(r, fl, g[i]);
        bl = mul2_mac(r, bl, g[R - 1 - i]);   // rows past `rows` are 0
    }
    const Mul2 pr = mul2_from_t(tpow(t1, uint32_t(rows)));   // r^rows

    double fev, ftv, bev, btv;
    Mul2 fep, bep;
    wg_scan_pair<NT / 64, false>(fl, pr, s_v, s_h, s_l, fev, fep, ftv);
    wg_scan_pair<NT / 64, true>(bl, pr, s_v, s_h, s_l, bev, bep, btv);
    if (PHASE == 1) {
        if (t == 0) {
            coef[size_t(kb) * 2] = ftv;
            coef[size_t(kb) * 2 + 1] = btv;
        }
        return;
    }
    const double bin = mul2_mac(bep, lr[size_t(kb) * 2 + 1], bev);
    double fv = mul2_mac(fep, lr[size_t(kb) * 2], fev);
    {
        double bv = bin;
#pragma unroll
        for (int i = R - 1; i >= 0; --i)
            if (i < rows) {
                bv = mul2_mac(r, bv, g[i]);
                g[i] = bv;
            }
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (i < rows) {
            const double gn = i + 1 < rows ? g[i + 1] : bin;
            s_x[t * (R + 1) + i] = sd * mul2_mac(r, fv, g[i]);
            fv = mul2_mac(r, fv - gn, g[i]);
        }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t e = e0 + uint32_t(2 * NT * j);
        if (e >= hi) continue;
        const bool in0 = e >= lo, in1 = e + 1u < hi;
        const int i0 = int(e) - int(lo);
        double2 v;
        v.x = in0 ? s_x[i0 + i0 / R] : 0.0;
        v.y = in1 ? s_x[i0 + 1 + (i0 + 1) / R] : 0.0;
        if (in0 && in1) stnt2(a.out + e, v);
        else if (in0) __builtin_nontemporal_store(v.x, a.out + e);
        else __builtin_nontemporal_store(v.y, a.out + e + 1);
    }
}

// The interface of one line's nblk blocks in one workgroup of NW waves (line blockIdx.x): thread t walks a run of
// consecutive blocks serially, the runs' pairs combine by the workgroup scan (multipliers r^rows of the runs), the
// mirror closes on the line's totals, and every thread walks its run again from its carries. co, lr: [block][2][line].
// p = 1: the one line on 16 waves (a 2^27-point line has 32768 blocks: runs of 32); p >= 2 with too few lines to
// fill the chip a thread each (k_trib_iface): one wave a line.
template <int NW>
__global__ __launch_bounds__((NW * 64)) void k_blk_iface(const SpecArgs a, const double* __restrict__ co,
                                                         double* __restrict__ lr, uint32_t nblk) {
    constexpr int NTI = NW * 64;
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double s_v[NW], s_h[NW], s_l[NW];
    const uint32_t m = a.m[a.d], t = threadIdx.x, l = blockIdx.x;
    const size_t C = a.nlines;
    double lamv[kMaxDims] = {0, 0, 0, 0};
    uint32_t rest = a.q_off + l;
    for (int jj = 0; jj < a.p - 1; ++jj) {
        const uint32_t qd = (jj < a.p - 2) ? a.fd[jj].div(rest) : 0u;
        lamv[jj] = a.lam[a.lam_off[jj] + (rest - qd * a.m[jj])];
        rest = qd;
    }
    double c0 = a.w0, c1 = 0.0;
    for (int Sm = 1; Sm < (1 << a.p); ++Sm) {
        if (a.cS[Sm] == 0.0) continue;
        double prod = sigma * a.cS[Sm];
        for (int jj = 0; jj < a.p - 1; ++jj)
            if ((Sm >> jj) & 1) prod *= lamv[jj];
        if ((Sm >> (a.p - 1)) & 1) c1 += prod;
        else c0 += prod;
    }
    const double D = sqrt(c0 * (c0 + 4.0 * c1));
    const double t1 = (c0 + D) / (c0 + 2.0 * c1 + D);   // 1 - r
    const uint32_t nlo = m / nblk;
    const double tlo = tpow(t1, nlo);
    const Mul2 mlo = mul2_from_t(tlo), mhi = mul2_from_t(fma(-tlo, t1, tlo + t1));
    auto rblk = [&](uint32_t k) {
        const uint32_t nk = uint32_t(uint64_t(m) * (k + 1) / nblk - uint64_t(m) * k / nblk);
        return nk == nlo ? mlo : mhi;
    };
    const uint32_t per = (nblk + uint32_t(NTI) - 1) / uint32_t(NTI);
    const uint32_t k0 = min(t * per, nblk), k1 = min(k0 + per, nblk);
    double acc = 0.0, bcc = 0.0;
    Mul2 pp{1.0, 0.0};
    for (uint32_t k = k0; k < k1; ++k) {
        const Mul2 rk = rblk(k);
        acc = mul2_mac(rk, acc, co[(size_t(k) * 2) * C + l]);
        pp = mul2_mul(pp, rk);
    }
    for (uint32_t k = k1; k > k0; --k) bcc = mul2_mac(rblk(k - 1), bcc, co[(size_t(k - 1) * 2 + 1) * C + l]);
    double fev, ftv, bev, btv;
    Mul2 fep, bep;
    wg_scan_pair<NTI / 64, false>(acc, pp, s_v, s_h, s_l, fev, fep, ftv);
    wg_scan_pair<NTI / 64, true>(bcc, pp, s_v, s_h, s_l, bev, bep, btv);
    // F_{-1} = B_0 and B_m = F_{m-1}: ftv, btv are F_{m-1} and B_0 from zero carries
    const double tm = tpow(t1, m), pm = 1.0 - tm, idet = 1.0 / (tm * (2.0 - tm));   // r^m, 1 / (1 - r^2m)
    const double fm1 = (btv + pm * ftv) * idet, bm = (ftv + pm * btv) * idet;
    double f = mul2_mac(fep, fm1, fev), b = mul2_mac(bep, bm, bev);
    for (uint32_t k = k0; k < k1; ++k) {
        lr[(size_t(k) * 2) * C + l] = f;
        f = mul2_mac(rblk(k), f, co[(size_t(k) * 2) * C + l]);
    }
    for (uint32_t k = k1; k > k0; --k) {
        lr[(size_t(k - 1) * 2 + 1) * C + l] = b;
        b = mul2_mac(rblk(k - 1), b, co[(size_t(k - 1) * 2 + 1) * C + l]);
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep: the dim-1 transforms of a 3-D solve fused into the dim-2 line solve as two marching sweeps (round 7).
// The factorised line solve is two first-order recursions with one constant r per (k0, k1) line, so a workgroup that
// owns a k_dct8 strided tile (16 adjacent k0 x all m1 = 2^L points of dim 1) and marches the planes of dim 2 keeps its
// 16 coefficients per thread, (k1, M - k1) pairs x 2 adjacent k0, in the same registers from plane to plane:
//   down (UP = false), i = hi - 1 ... lo: dim-1 forward DCT of the plane's tile (k_dct8's strided forward pass), then
//       B <- f + r B from B = 0 and Fs <- Fs + p f, p <- p r from p = 1; B is stored in the pass's coefficient layout,
//       and (Fs, B) at the chunk's end go to coef as k_trisr<1> writes them: F at the chunk's last row and B at its
//       first row, each from a zero carry;
//   (k_trisr_iface over the C chunks as "ranks": the true F entering every chunk's first row, B entering its last)
//   up (UP = true), i = lo ... hi - 1: with the stored B_i and B_{i+1} (0 past the chunk's top) f_i = B_i - r B_{i+1}
//       (k_trisr<3>'s recovery: the carry's terms cancel in it), x_i = (scale / D) (B_i + r^(hi-i) Bin + r F),
//       F <- r F + f_i from F = Fin, then k_dct8's strided inverse pass on x_i.
// The planes of dim 2 split into C chunks [floor(m2 k / C), floor(m2 (k + 1) / C)) (k_trisr_iface's block rule);
// workgroup b owns tile b % (m0 / 16) of chunk b / (m0 / 16). In place: a chunk reads and writes its own planes only,
// plane i + 1 is read before it is written. The three launches are ordered by the stream alone.
// r^(hi-i) Bin by a two-level exponent (uniform over the workgroup): with hi - i = 8 a + b, b < 8, Bin's registers
// hold Q = r^(8 a) Bin and a plane forms r^b Q with <= 2 squarings and <= 3 products; where a drops (b = 0 -> 7) Bin
// is loaded again from lr into the same registers, issued at the end of the b = 0 step, and raised by (r^8)^a at
// the start of the next (binary powering, once per 8 planes). No division by r (r = 0 at sigma = 0), and a factor
// that underflows belongs to a term below the result's rounding. r^2, r^4 and r^8 are loop-invariant: their inputs
// pass through an opaque copy so that they are recomputed, not kept in 48 more registers.
// Registers: B, Fs, p (down) or r, F, Bin (up) and two planes' values, 16 doubles each; r (down) or scale / D (up) and
// the twiddles sit in LDS beside the exchange buffer, so the loop holds no invariant loads the compiler could hoist
// into registers (224 / 254 VGPRs, no scratch, 153 KB of LDS). One 512-thread workgroup per CU (L = 9). Barriers in
// the plane loop order LDS only, so the next plane's loads, issued before this plane's stages, stay in flight. The
// down sweep keeps p as a running product: powering it per plane cost 577 against 449 us.
template <int L, bool UP>
__global__ __launch_bounds__((spec8::Shape<L>::NT)) void k_sweep(const SpecArgs a, double* __restrict__ car,
                                                                  uint32_t m2, int C) {
    using S = spec8::Shape<L>;
    constexpr int M = S::M, TPL = S::TPL, NCL = S::NCL, NT = S::NT, R0 = S::R0;
    static_assert(S::TQ == 16 && L >= 6, "k_sweep: 16-line tiles (m1 <= 512)");
    double sigma = a.sigma;
    if (a.skip && *a.skip) return;
    if (a.ctl) {
        if (a.ctl->done) return;
        sigma = a.ctl->sigma;
    }
    __shared__ double2 buf[NCL * S::LP];          // FFT exchange (k_dct8's slot layout)
    __shared__ double2 s_tw[M], s_twq[M];         // radix-8 stages index tw up to 7 M / 8
    __shared__ double s_lc[16 * NT];              // this thread's 16 line constants [e][t]: r (down), scale / D (up)
    const int t = threadIdx.x;
    const int j0 = t / NCL, c0 = t % NCL;
    const uint32_t m0 = a.m[0];
    const uint32_t ntile = m0 / 16u;
    const uint32_t tile = blockIdx.x % ntile, ck = blockIdx.x / ntile;
    const uint32_t lo = uint32_t(uint64_t(m2) * ck / uint32_t(C)), hi = uint32_t(uint64_t(m2) * (ck + 1u) / uint32_t(C));
    const size_t ps = size_t(m0) * M;             // plane
    const size_t nl = ps;                         // lines

    for (int i = t; i < M; i += NT) {
        s_twq[i] = a.twq[i];
        s_tw[i] = a.tw[i];
    }

    // line constants of the coefficients e = 4 s + {0, 1}: (ka, k0 | k0 + 1), {2, 3}: (kb, k0 | k0 + 1), as k_trisr
    // builds them
    double r[UP ? 16 : 1];
    {
        const uint32_t k0 = tile * 16u + uint32_t(2 * c0);
        const double l0[2] = {a.lam[a.lam_off[0] + k0], a.lam[a.lam_off[0] + k0 + 1u]};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = j0 + s * TPL;
            const int kk[2] = {k, k ? M - k : M / 2};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double l1 = a.lam[a.lam_off[1] + uint32_t(kk[h])];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    double c0v = a.w0, c1v = 0.0;
                    for (int Sm = 1; Sm < 8; ++Sm) {
                        if (a.cS[Sm] == 0.0) continue;
                        double prod = sigma * a.cS[Sm];
                        if (Sm & 1) prod *= l0[e];
                        if (Sm & 2) prod *= l1;
                        if (Sm & 4) c1v += prod;
                        else c0v += prod;
                    }
                    const double D = sqrt(c0v * (c0v + 4.0 * c1v));
                    const double den = 1.0 / (c0v + 2.0 * c1v + D);
                    if constexpr (UP) {
                        r[4 * s + 2 * h + e] = 2.0 * c1v * den;
                        s_lc[(4 * s + 2 * h + e) * NT + t] = a.inv_n * double(m2) / D;
                    } else {
                        s_lc[(4 * s + 2 * h + e) * NT + t] = 2.0 * c1v * den;
                    }
                }
            }
        }
    }
    // [chunk][2][line]: the pair (k0, k0 + 1) of coefficient (s, h)
    auto carp = [&](int which, int s, int h) -> double* {
        const int k = j0 + s * TPL;
        const uint32_t k1 = uint32_t(h == 0 ? k : (k ? M - k : M / 2));
        return car + (size_t(ck) * 2 + size_t(which)) * nl + size_t(k1) * m0 + (tile * 16u + uint32_t(2 * c0));
    };
    // y r^n by binary powering (n is uniform over the workgroup)
    auto rpow = [](double rp, uint32_t n, double y) -> double {
        for (; n; n >>= 1) {
            if (n & 1u) y *= rp;
            rp *= rp;
        }
        return y;
    };
    __syncthreads();   // the tables

    // The plane loops take the thread's coordinates through an opaque copy per iteration: the indices derived from
    // them (8 LDS slots per exchange, 8 global offsets) are then recomputed per plane, a few integer operations,
    // where the compiler would otherwise keep them all in registers over the loop, next to the 16-element state
#define MVTV_SWEEP_COORDS                                            \
    int j = j0, c = c0;                                              \
    asm volatile("" : "+v"(j), "+v"(c));                             \
    double2* const X = buf + c * S::LP;                              \
    const int cx = c & 7;                                            \
    const uint32_t k0 = tile * 16u + uint32_t(2 * c)

    if constexpr (!UP) {
        double B[16], Fs[16], pw[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) B[e] = 0.0, Fs[e] = 0.0, pw[e] = 1.0;
        double2 zn[8];
        auto issue = [&](uint32_t i, int j, uint32_t k0) {
            const double* p = a.in + size_t(i) * ps + k0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int n = stage_in_pos<L, R0>(j, q);
                const uint32_t k = n < M / 2 ? uint32_t(2 * n) : uint32_t(2 * (M - 1 - n) + 1);
                zn[q] = ldnt2(p + k * m0);
            }
        };
        issue(hi - 1u, j0, tile * 16u + uint32_t(2 * c0));
        for (uint32_t i = hi; i-- > lo;) {
            MVTV_SWEEP_COORDS;
            double2 z[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) z[q] = zn[q];
            if (i > lo) issue(i - 1u, j, k0);
            stages_from<L, R0, 1, false, false, 1>(z, j, X, cx, s_tw);   // natural-order spectrum in LDS
            double* const o = a.out + size_t(i) * ps + k0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = j + s * TPL;
                const int ka = k, kb = k ? M - k : M / 2;
                const double2 Z1 = X[spec8::slot(ka, cx)], Z2 = X[spec8::slot(kb, cx)];
                const double2 q1 = s_twq[ka], q2 = s_twq[kb];
                double2 Xk, Xmk;
                if (k == 0) {
                    Xk = make_double2(q1.x * Z1.x, q1.x * Z1.y);
                    Xmk = make_double2(q2.x * Z2.x, q2.x * Z2.y);
                } else {
                    const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                    const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                    Xk = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                    Xmk = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
                }
                const double f[4] = {Xk.x, Xk.y, Xmk.x, Xmk.y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = 4 * s + e;
                    const double rx = s_lc[x * NT + t];
                    B[x] = fma(rx, B[x], f[e]);
                    Fs[x] = fma(pw[x], f[e], Fs[x]);   // r^(hi-1-i) f_i
                    pw[x] *= rx;
                }
                stnt2(o + uint32_t(ka) * m0, make_double2(B[4 * s], B[4 * s + 1]));
                stnt2(o + uint32_t(kb) * m0, make_double2(B[4 * s + 2], B[4 * s + 3]));
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int x = 4 * s + 2 * h;
                stnt2(carp(0, s, h), make_double2(Fs[x], Fs[x + 1]));
                stnt2(carp(1, s, h), make_double2(B[x], B[x + 1]));
            }
    } else {
        double F[16], Bin[16], cur[16], nxt[16];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int x = 4 * s + 2 * h;
                const double2 fv = ldnt2(carp(0, s, h)), bv = ldnt2(carp(1, s, h));
                F[x] = fv.x;
                F[x + 1] = fv.y;
                Bin[x] = bv.x;
                Bin[x + 1] = bv.y;
            }
        auto issue = [&](uint32_t i, double* v, int j, uint32_t k0) {   // plane i's stored B; zero past the chunk's top
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = j + s * TPL;
                const int ka = k, kb = k ? M - k : M / 2;
                double2 va = make_double2(0.0, 0.0), vb = va;
                if (i < hi) {
                    const double* p = a.in + size_t(i) * ps + k0;
                    va = ldnt2(p + uint32_t(ka) * m0);
                    vb = ldnt2(p + uint32_t(kb) * m0);
                }
                v[4 * s] = va.x;
                v[4 * s + 1] = va.y;
                v[4 * s + 2] = vb.x;
                v[4 * s + 3] = vb.y;
            }
        };
        issue(lo, cur, j0, tile * 16u + uint32_t(2 * c0));
        issue(lo + 1u, nxt, j0, tile * 16u + uint32_t(2 * c0));
        // Bin's registers hold Q = r^(8 a) Bin while hi - i = 8 a + b, b < 8
        auto requant = [&](uint32_t a8) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                double r8 = r[e];
                asm volatile("" : "+v"(r8));   // r^8 is loop-invariant: recomputed here, not 16 more registers
                r8 *= r8;
                r8 *= r8;
                r8 *= r8;
                Bin[e] = rpow(r8, a8, Bin[e]);
            }
        };
        requant((hi - lo) >> 3);
        for (uint32_t i = lo; i < hi; ++i) {
            MVTV_SWEEP_COORDS;
            const uint32_t n = hi - i, b = n & 7u;
            if (b == 7u && i > lo) requant(n >> 3);   // Bin reloaded at the end of the last step
            xbar<1>();   // the last stage of plane i - 1 has read its inputs
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                double xv[4];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    // r^b Q of the pair (k0, k0 + 1), b uniform: <= 2 squarings and <= 3 products each
                    const int e0 = 4 * s + 2 * h;
                    double rp[2] = {r[e0], r[e0 + 1]}, y[2] = {Bin[e0], Bin[e0 + 1]};
                    asm volatile("" : "+v"(rp[0]), "+v"(rp[1]));   // r^2, r^4 are loop-invariant: not kept in registers
                    if (b & 1u) y[0] *= rp[0], y[1] *= rp[1];
                    if (b > 1u) {
                        rp[0] *= rp[0], rp[1] *= rp[1];
                        if (b & 2u) y[0] *= rp[0], y[1] *= rp[1];
                        if (b > 3u) {
                            rp[0] *= rp[0], rp[1] *= rp[1];
                            y[0] *= rp[0], y[1] *= rp[1];
                        }
                    }
#pragma unroll
                    for (int e2 = 0; e2 < 2; ++e2) {
                        const int e = e0 + e2;
                        const double f = fma(-r[e], nxt[e], cur[e]);
                        xv[2 * h + e2] = s_lc[e * NT + t] * (cur[e] + y[e2] + r[e] * F[e]);
                        F[e] = fma(r[e], F[e], f);
                        cur[e] = nxt[e];
                    }
                }
                const int k = j + s * TPL;
                const int ka = k, kb = k ? M - k : M / 2;
                const double2 Xk = make_double2(xv[0], xv[1]), Xmk = make_double2(xv[2], xv[3]);
                const double2 q1 = cconj(s_twq[ka]), q2 = cconj(s_twq[kb]);
                if (k == 0) {
                    const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xmk.x));
                    const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xmk.y));
                    X[spec8::slot(0, cx)] = Xk;
                    X[spec8::slot(M / 2, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
                } else {
                    const double2 va1 = cmul(q1, make_double2(Xk.x, -Xmk.x));
                    const double2 vb1 = cmul(q1, make_double2(Xk.y, -Xmk.y));
                    const double2 va2 = cmul(q2, make_double2(Xmk.x, -Xk.x));
                    const double2 vb2 = cmul(q2, make_double2(Xmk.y, -Xk.y));
                    X[spec8::slot(ka, cx)] = make_double2(va1.x - vb1.y, va1.y + vb1.x);
                    X[spec8::slot(kb, cx)] = make_double2(va2.x - vb2.y, va2.y + vb2.x);
                }
            }
            if (b == 0u) {   // the next 8 planes' Q starts from Bin again: into its own registers, a step ahead
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = j + s * TPL;
                    const double* const p = car + (size_t(ck) * 2 + 1) * nl + k0;
                    const double2 va = ldnt2(p + uint32_t(k) * m0), vb = ldnt2(p + uint32_t(k ? M - k : M / 2) * m0);
                    Bin[4 * s] = va.x;
                    Bin[4 * s + 1] = va.y;
                    Bin[4 * s + 2] = vb.x;
                    Bin[4 * s + 3] = vb.y;
                }
            }
            issue(i + 2u, nxt, j, k0);   // in flight over the stages and the stores of plane i (plane i + 2: not written yet)
            xbar<1>();
            double2 z[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) z[q] = X[spec8::slot(stage_in_pos<L, R0>(j, q), cx)];
            stages_from<L, R0, 1, true, true, 1>(z, j, X, cx, s_tw);
            using LS = LastStage<L>;
            double* const o = a.out + size_t(i) * ps + k0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int nn = stage_out_pos<L, LS::R, LS::NS>(j, q);
                const uint32_t k = nn < M / 2 ? uint32_t(2 * nn) : uint32_t(2 * (M - 1 - nn) + 1);
                stnt2(o + k * m0, z[q]);
            }
        }
    }
#undef MVTV_SWEEP_COORDS
}

static void tris_seg(uint32_t n, int* sl, int* nseg) {
    // >= 4 segments when the block allows it, segments of <= 16 rows (32 past 1024 rows), <= 64 segments
    uint32_t s = std::max<uint32_t>(1u, std::min<uint32_t>(n > 1024u ? 32u : 16u, n / 4u));
    while (s > 1 && n % s) --s;
    *sl = int(s);
    *nseg = int(n / s);
}

bool tri_slab_ok(uint32_t n) {
    int sl = 0, nseg = 0;
    tris_seg(n, &sl, &nseg);
    return n >= 1 && sl <= 32 && nseg <= tris::NSMAX;
}

hipError_t launch_tri_slab(const SpecPlan& sp, const Geom& og, hipStream_t s, int phase, double* x, double* coef,
                           const double* lr, uint32_t chunk, int lo_ext, int hi_ext, double scale,
                           const AdmmCtl* ctl, double sigma, double w0, const int32_t* skip) {
    const int p = og.p, d = p - 1;
    SpecArgs a{};
    a.ctl = ctl;
    a.skip = skip;
    a.sigma = sigma;
    a.w0 = w0;
    a.lam = sp.lam;
    for (int j = 0; j < kMaxDims; ++j) {
        a.lam_off[j] = sp.lam_off[j];
        a.m[j] = og.m[j];
    }
    for (int j = 0; j < kMaxDims - 1; ++j) a.fd[j] = og.fd[j];
    for (int S = 0; S < 16; ++S) a.cS[S] = og.cS[S];
    a.d = d;
    a.p = p;
    a.stride = og.stride[d];
    a.nlines = og.stride[d];
    const uint32_t n = og.m[d];
    int sl = 0, nseg = 0;
    tris_seg(n, &sl, &nseg);
    if (!tri_slab_ok(n) || chunk == 0 || a.nlines % chunk != 0)
        return hipErrorInvalidValue;
    if (phase != 1 && phase != 3) return hipErrorInvalidValue;
    // 64-line tiles with the segment arrays sized to the block (<= 16 segments: <= 1024 threads) where the lines
    // fill >= 128 such workgroups; otherwise 16-line tiles sized for any block (<= 64 segments)
    static const bool wide_off = probe_env("MVTV_TRIS_NARROW") != nullptr;
    auto go = [&](auto kern, uint32_t tq) {
        klaunch(kern, dim3((a.nlines + tq - 1) / tq), dim3(tq * uint32_t(nseg)), 0, s, a, sl, nseg, x, coef, lr, chunk,
                lo_ext, hi_ext, scale);
        return hipGetLastError();
    };
    if (!wide_off && nseg <= 16 && a.nlines >= 64u * 128u) {
        // segments of <= 16 rows keep the row registers at 16 (blocks up to 256 planes here); <= 4 rows (blocks of
        // <= 16 planes: a 4-D rank at G = 8) size the line constants for 4
        const int ns = nseg <= 4 ? 4 : (nseg <= 8 ? 8 : 16);
        if (sl <= 4 && ns == 4) {
            if (phase == 1) return go(k_trisr<1, 4, 64, 4>, 64u);
            return go(k_trisr<3, 4, 64, 4>, 64u);
        }
        if (sl <= 16) {
            if (phase == 1) {
                if (ns == 4) return go(k_trisr<1, 16, 64, 4>, 64u);
                if (ns == 8) return go(k_trisr<1, 16, 64, 8>, 64u);
                return go(k_trisr<1, 16, 64, 16>, 64u);
            }
            if (ns == 4) return go(k_trisr<3, 16, 64, 4>, 64u);
            if (ns == 8) return go(k_trisr<3, 16, 64, 8>, 64u);
            return go(k_trisr<3, 16, 64, 16>, 64u);
        }
    }
    const uint32_t tq = uint32_t(tris::TQ);
    if (phase == 1 && sl <= 16) return go(k_trisr<1, 16>, tq);
    if (phase == 1) return go(k_trisr<1, 32>, tq);
    if (sl <= 16) return go(k_trisr<3, 16>, tq);
    return go(k_trisr<3, 32>, tq);
}

hipError_t launch_tri_iface(const SpecPlan& sp, const Geom& og, hipStream_t s, double* coef_in, double* lr_out,
                            uint32_t chunk, int G, int rank, uint32_t mg, const AdmmCtl* ctl, double sigma, double w0,
                            const int32_t* skip) {
    if (G < 1 || chunk == 0) return hipErrorInvalidValue;
    SpecArgs a{};
    a.ctl = ctl;
    a.skip = skip;
    a.sigma = sigma;
    a.w0 = w0;
    a.lam = sp.lam;
    for (int j = 0; j < kMaxDims; ++j) {
        a.lam_off[j] = sp.lam_off[j];
        a.m[j] = og.m[j];
    }
    for (int j = 0; j < kMaxDims - 1; ++j) a.fd[j] = og.fd[j];
    for (int S = 0; S < 16; ++S) a.cS[S] = og.cS[S];
    a.p = og.p;
    a.d = og.p - 1;
    klaunch(k_trisr_iface, dim3((chunk + 255) / 256), dim3(256), 0, s, a, coef_in, lr_out, chunk, G, rank, mg);
    return hipGetLastError();
}

// segment length for k_trigr: the smallest divisor of m in [16, 32], else the largest in [4, 16),
// with at most 64 segments; else (no such divisor: a prime length, 2 x a prime ...; probe builds keep the
// Bluestein MID pass with MVTV_TRIG_EXACT=1) 16 rows (32 past 1024 points; m / 4 rounded up below 64 points) with a
// shorter last segment; 0 when there is none (m < 8, m > 2048)
static int trig_seg(uint32_t m) {
    static const int force = [] {   // probe builds: MVTV_TRIG_SL=s forces the segment length (a shorter last one
        const char* e = probe_env("MVTV_TRIG_SL");   // when s does not divide m)
        return e ? std::atoi(e) : 0;
    }();
    if (force >= 4 && force <= trig::SMAX && m / uint32_t(force) >= 2 &&
        (m + uint32_t(force) - 1) / uint32_t(force) <= uint32_t(trig::NSMAX))
        return force;
    for (uint32_t sl = 16; sl <= uint32_t(trig::SMAX); ++sl)
        if (m % sl == 0 && m / sl <= uint32_t(trig::NSMAX) && m / sl >= 2) return int(sl);
    for (uint32_t sl = 15; sl >= 4; --sl)
        if (m % sl == 0 && m / sl <= uint32_t(trig::NSMAX) && m / sl >= 2) return int(sl);
    static const bool exact = probe_flag("MVTV_TRIG_EXACT");
    if (exact || m < 8 || m > 2048) return 0;
    if (m < 64) return int((m + 3) / 4);
    return m > 1024 ? 32 : 16;
}

// k_trigr's tile: 64 / 32 lines (512- / 256-B rows) with the segment arrays sized to the block where it fits 1024
// threads and the lines fill >= 256 such workgroups, else 16 lines for any block (round 4's form; probe builds:
// MVTV_TRIG_NARROW=1). sr < sl: a shorter last segment
static void launch_trig(const SpecArgs& a, hipStream_t s, int sl, int nseg, int sr) {
    static const bool narrow = probe_flag("MVTV_TRIG_NARROW");
    auto go = [&](auto kern, uint32_t tq) {
        klaunch(kern, dim3((a.nlines + tq - 1) / tq), dim3(tq * uint32_t(nseg)), 0, s, a, sl, nseg, sr);
    };
#define MVTV_TRIG(SM, TQ, NS)                                                                                   \
    do {                                                                                                        \
        go(k_trigr<SM, TQ, NS>, uint32_t(TQ));                                                                  \
        return;                                                                                                 \
    } while (0)
    if (!narrow) {
        if (nseg <= 16 && a.nlines / 64u >= 256u) {
            if (sl <= 16) {
                if (nseg <= 8) MVTV_TRIG(16, 64, 8);
                MVTV_TRIG(16, 64, 16);
            }
            if (nseg <= 8) MVTV_TRIG(32, 64, 8);
            MVTV_TRIG(32, 64, 16);
        }
        if (nseg <= 32 && a.nlines / 32u >= 256u) {
            if (sl <= 16) MVTV_TRIG(16, 32, 32);
            MVTV_TRIG(32, 32, 32);
        }
        // few lines (the last dimension of a 2-D mesh: 1009 lines): 8- / 4-line tiles, >= 128 / 256 workgroups
        if (a.nlines / uint32_t(trig::TQ) < 256u) {
            const int tq = few_lines_tq(a.nlines, trig::TQ, 4);
            if (tq == 4) MVTV_TRIG(trig::SMAX, 4, trig::NSMAX);
            if (tq == 8) MVTV_TRIG(trig::SMAX, 8, trig::NSMAX);
        }
    }
    MVTV_TRIG(trig::SMAX, trig::TQ, trig::NSMAX);
#undef MVTV_TRIG
}

// The line solve serves the last-dimension pass when the lines are long enough for >= 4 segments and short enough
// for <= 64 (16 rows per segment up to 1024 points, 32 at 2048), the stride holds the tile's lines, and
// either 16-line tiles fill the chip (>= 256 workgroups: 3-D and 4-D meshes) or, for the few 2048-point
// lines of a 2-D mesh, 8-line tiles in XCD runs (2048^2: 4844 -> 5145 ADMM it/s on one box; at 1024^2 the
// FFT pass stays faster: 9866 against 9381 with 8-line and 9050 with 4-line tiles, profiles/r02/v19_tri2d). Round 6, with
// the factorised line solve (k_trir): 1024- and 512-point lines take it too, on 4-line tiles (one box, two reps each,
// profiles/r06/v8_tri2d: 1024^2 12928 / 12925 -> 14312 / 14249 ADMM it/s, 512^2 18185 / 18166 -> 20543 / 20357; 8-line
// tiles 14173 / 20397; 2048^2 keeps 8-line tiles: 6279 / 6226, 4-line 5319).
// Probe builds: MVTV_DCT_TRI2D=0 keeps the FFT pass on 2-D meshes (the other tiles of that A/B, 8 lines at 512 / 1024
// and 4 at 2048, were removed; they last existed in commit ae72d5c).
static int tri_tiles(const SpecArgs& a, int mode, bool formb) {
    if (mode != SPEC_MID || a.d == 0 || formb) return 0;
    const char* e = probe_env("MVTV_DCT_TRI");
    if (e && std::atoi(e) == 0) return 0;
    if (a.L < 6 || a.L > 11 || a.stride < 4u) return 0;
    if (a.L <= 10 && a.stride >= uint32_t(tri::TQ) && a.nlines / uint32_t(tri::TQ) >= 256u) return tri::TQ;
    static const bool t2d_off = [] {
        const char* v = probe_env("MVTV_DCT_TRI2D");
        return v && std::atoi(v) == 0;
    }();
    const int t2d = t2d_off ? 0 : (a.L == 11 ? 8 : (a.L >= 9 ? 4 : 0));
    if (t2d == 0) return 0;
    if (uint32_t(t2d) > a.stride || (a.nlines / uint32_t(t2d)) % 8u != 0u) return 0;
    return t2d;
}

// The line solves of tri_tiles. tq = 16, the last-dimension pass of 3-D / 4-D meshes. Tiles, where the lines fill
// >= 256 workgroups of 64: 64 lines (512-B rows per wave load) of 32-row segments up to 256-point lines (256 / 512
// threads), 32 lines of 16-row segments (1024 threads, 64 VGPRs: two workgroups a CU) at 512, 32 lines of 32-row
// segments at 1024; 16 lines of 16-row segments otherwise. Against the Thomas form (round 6, one box, kernel trace,
// profiles/r06/v1_trir): 512^3 441 -> 392 us, 256^3 73 -> 49 us, 128^4 948 -> 797 us. tq = 4 / 8, the few lines of a
// 2-D mesh: narrow tiles in XCD runs (grid a multiple of 8), 2048-point lines in 64 segments of 32 rows, else 16-row
// segments.
static hipError_t launch_tri(SpecArgs& a, hipStream_t s, int tq) {
    // (the line stride is a power of two >= the tile here, and nlines a multiple of it: whole tiles)
#define MVTV_TRIR(LL, SEG, TQL)                                                                                 \
    do {                                                                                                        \
        a.tq = TQL;                                                                                             \
        klaunch(k_trir<LL, SEG, TQL>, dim3((a.nlines + uint32_t(TQL) - 1) / uint32_t(TQL)),                     \
                dim3(trir::Shape<LL, SEG, TQL>::NT), 0, s, a);                                                  \
        return hipGetLastError();                                                                               \
    } while (0)
    if (tq == tri::TQ) {
        a.xcd = 0;
        if (a.nlines / 64u >= 256u && a.stride >= 64u) {
            switch (a.L) {
                case 6: MVTV_TRIR(6, 32, 64);
                case 7: MVTV_TRIR(7, 32, 64);
                case 8: MVTV_TRIR(8, 32, 64);
                case 9: MVTV_TRIR(9, 16, 32);
                case 10: MVTV_TRIR(10, 32, 32);
            }
            return hipErrorInvalidValue;
        }
        switch (a.L) {
            case 6: MVTV_TRIR(6, 16, 16);
            case 7: MVTV_TRIR(7, 16, 16);
            case 8: MVTV_TRIR(8, 16, 16);
            case 9: MVTV_TRIR(9, 16, 16);
            case 10: MVTV_TRIR(10, 16, 16);
        }
        return hipErrorInvalidValue;
    }
    a.xcd = 1;
    if (tq == 4 && a.L == 9) MVTV_TRIR(9, 16, 4);
    if (tq == 4 && a.L == 10) MVTV_TRIR(10, 16, 4);
    if (tq == 8 && a.L == 11) MVTV_TRIR(11, 32, 8);
#undef MVTV_TRIR
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------ launcher
// One k_dct8 pass with TQW real lines per workgroup (NT = TQW / 2 * m / 8 threads).
// (tq < TQW: narrow meshes whose stride is below the tile; the extra lanes idle)
template <int L, int TQW>
static void launch_dct8_tile(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb, int tq = TQW) {
    a.tq = tq;
    const uint32_t grid = (a.nlines + uint32_t(tq) - 1) / uint32_t(tq);
    a.xcd = a.xcd && (grid & 7u) == 0u;
    const dim3 block(spec8::ShapeK<L, TQW>::NT);
    if constexpr (L >= 6 && spec8::ShapeK<L, TQW>::NT >= 64) {
        if (a.pf.mode) {   // PCG-fused d = 0 passes (dct_pcg_fusable)
            if (a.pf.mode == 2 && 2 * size_t(grid) > a.pf.cap) {   // the rows would overrun the partials
                *a.pf.nparts = -1;
                return;
            }
            if (a.pf.nparts) *a.pf.nparts = int(grid);
            if (a.pf.mode == 1) klaunch(k_dct8<L, SPEC_FWD, true, false, TQW, 1>, dim3(grid), block, 0, s, a);
            else klaunch(k_dct8<L, SPEC_INV, true, false, TQW, 2>, dim3(grid), block, 0, s, a);
            return;
        }
    }
#define MVTV_DCT8(MODE, D0, FB) klaunch(k_dct8<L, MODE, D0, FB, TQW>, dim3(grid), block, 0, s, a)
    if (mode == SPEC_FWD) {
        if (d0) {
            if (formb) MVTV_DCT8(SPEC_FWD, true, true);
            else MVTV_DCT8(SPEC_FWD, true, false);
        } else {
            MVTV_DCT8(SPEC_FWD, false, false);
        }
    } else if (mode == SPEC_INV) {
        if (d0) MVTV_DCT8(SPEC_INV, true, false);
        else MVTV_DCT8(SPEC_INV, false, false);
    } else {
        if (d0) {
            if (formb) MVTV_DCT8(SPEC_MID, true, true);
            else MVTV_DCT8(SPEC_MID, true, false);
        } else {
            MVTV_DCT8(SPEC_MID, false, false);
        }
    }
#undef MVTV_DCT8
}

// tile sizes a pass may take: a power of two in [max(2, 1024 / m), 16 * 2^(L <= 9 ? 1 : 0)], with
// NT = TQW / 2 * m / 8 in [64, 1024] and <= ~150 KB of LDS
template <int L>
constexpr bool tile_ok(int tq) {
    constexpr int M = 1 << L;
    return tq >= 2 && (tq / 2) * (M / 8) >= 64 && (tq / 2) * (M / 8) <= 1024 &&
           (tq / 2) * spec8::Shape<L>::LP * 16 <= 152 * 1024;
}
template <int L, int TQW>
static bool try_tile(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb, int want) {
    if constexpr (tile_ok<L>(TQW)) {
        if (want == TQW) {
            launch_dct8_tile<L, TQW>(a, s, mode, d0, formb);
            return true;
        }
    }
    return false;
}

// Tile choice. Default: 16 lines (128-B rows for d > 0) up to 512 points per line, then 8 / 4 / 2 for
// 1024 / 2048 / 4096 (LDS); strided passes of 1024 - 4096-point lines twice that (one ~148-KB workgroup
// per CU: 2048^2 strided passes 49 -> 28 us, 3670 -> 4320 ADMM it/s). Meshes with few lines (2-D) would
// leave CUs idle with those tiles: a d = 0 pass under 1024 workgroups takes the smallest tile (>= one wave),
// a strided pass under 128 wide workgroups takes 4 lines (32-B rows) with the tiles dealt to the XCDs in
// contiguous runs, so the 4 tiles of a 128-B row share one L2. 1024^2: 8355 -> 9650 ADMM it/s (d = 0
// passes 17.5 -> 14.8 us, strided 18.7 -> 11.8 us); 2048^2: 4797 -> 4862 (profiles/r02/v17_dct_tiles).
// Probe builds: MVTV_DCT_T0 / _T1 set the d = 0 / d > 0 tile, MVTV_DCT_XCD=0/1 the XCD runs.
template <int L>
static void launch_dct8(SpecArgs& a, hipStream_t s, int mode, bool d0, bool formb) {
    using S = spec8::Shape<L>;
    constexpr int TMIN = tile_ok<L>(2) ? 2 : (tile_ok<L>(4) ? 4 : (tile_ok<L>(8) ? 8 : 16));
    int want = S::TQ;
    bool xcd_def = false;
    if (d0) {
        if (a.nlines / uint32_t(S::TQ) < 1024u) want = std::min(TMIN, S::TQ);
    } else {
        // strided passes: tiles in XCD runs (512^3: the dim-1 passes' bucket 0.436 -> 0.405 ms, 174.7 / 174.6 ->
        // 178.3 / 178.3 ADMM it/s on one box, profiles/r05/v16_dct8_xcd; the d = 0 passes stay round-robin there)
        xcd_def = true;
        if (L >= 10 && L <= 12 && 2 * S::TQ <= int(a.stride)) {
            want = 2 * S::TQ;
            if (a.nlines / uint32_t(want) < 128u && tile_ok<L>(4) && int(a.stride) >= 4) want = 4;
        }
    }
    // (probe builds read these per launch, so a probe can vary them within one process)
    const char* e0 = probe_env("MVTV_DCT_T0");
    const char* e1 = probe_env("MVTV_DCT_T1");
    const char* ex = probe_env("MVTV_DCT_XCD");
    const int t0 = e0 ? std::atoi(e0) : 0, t1 = e1 ? std::atoi(e1) : 0, xcd_env = ex ? std::atoi(ex) : -1;
    if (d0 && t0 > 0) want = t0;
    if (!d0 && t1 > 0) want = t1;
    if (!d0) want = std::min<int>(want, int(a.stride));
    a.xcd = xcd_env >= 0 ? xcd_env : (xcd_def ? 1 : 0);
    if (try_tile<L, 2>(a, s, mode, d0, formb, want) || try_tile<L, 4>(a, s, mode, d0, formb, want) ||
        try_tile<L, 8>(a, s, mode, d0, formb, want) || try_tile<L, 16>(a, s, mode, d0, formb, want) ||
        try_tile<L, 32>(a, s, mode, d0, formb, want))
        return;
    a.xcd = 0;
    launch_dct8_tile<L, S::TQ>(a, s, mode, d0, formb, std::min(want, S::TQ));   // the default tile
}

// the fused in-plane passes (k_plane8): m0 = m1 = 2^L, 16 <= m <= 128, dims 0 and 1 transformed first
bool plane_pass_ok(const Geom& g) {
    if (g.p < 3 || g.m[0] != g.m[1] || probe_env("MVTV_PLANE_OFF") || probe_env("MVTV_DCT_LDS")) return false;
    // and enough planes to fill the chip: 128^3's 128 planes (one workgroup each) ran 1 % slower than the two
    // passes, 128^4's 16384 3.5 % faster per ADMM iteration (profiles/r03/v15_plane)
    const uint32_t m = g.m[0];
    return m >= 16 && m <= 128 && (m & (m - 1)) == 0 && g.N / (uint64_t(m) * m) >= 1024;
}

// mode SPEC_FWD (dims 0 then 1; b formed on load when ga != nullptr, from the folded s when fold) or SPEC_INV
// (dims 1 then 0), in place over every (dim 0, dim 1) plane of g
hipError_t launch_plane_pass(const SpecPlan& sp, const Geom& g, hipStream_t s, int mode, const double* in,
                             const double* ga, double ca, const double* gb, double cb, double* out,
                             const AdmmCtl* ctl, const int32_t* skip, bool fold) {
    if (!plane_pass_ok(g) || (mode != SPEC_FWD && mode != SPEC_INV) || (mode == SPEC_INV && ga) ||
        (fold && (!ga || !gb || !ctl)))
        return hipErrorInvalidValue;
    SpecArgs a{};
    a.ctl = ctl;
    a.skip = skip;
    a.in = in;
    a.ga = ga;
    a.gb = gb ? gb : ga;
    a.ca = ca;
    a.cb = gb ? cb : 0.0;
    a.out = out;
    a.tw = reinterpret_cast<const double2*>(sp.tw + sp.tw_off[0]);    // m0 = m1: one table serves both dims
    a.twq = reinterpret_cast<const double2*>(sp.twq + sp.twq_off[0]);
    a.fold = fold ? 1 : 0;
    const uint32_t m = g.m[0];
    const uint32_t nplanes = g.N / (m * m);
    // persistent over the planes: one workgroup per CU (the plane's 152 KB of LDS) at m = 128, so the next
    // plane's loads overlap the transforms; smaller planes keep one workgroup per plane
    static thread_local int dev = -1, cus = 256;
    int dv = 0;
    if (hipGetDevice(&dv) == hipSuccess && dv != dev) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dv) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        dev = dv;
    }
    const dim3 grid(m == 128 ? std::min<uint32_t>(nplanes, uint32_t(cus)) : nplanes);
    const bool formb = ga != nullptr;
#define MVTV_PLANE(LL)                                                                                          \
    do {                                                                                                        \
        const dim3 block((1u << LL) / 2 * (1u << LL) / 8);                                                      \
        if (mode == SPEC_INV) klaunch(k_plane8<LL, SPEC_INV, false>, grid, block, 0, s, a, nplanes);            \
        else if (formb) klaunch(k_plane8<LL, SPEC_FWD, true>, grid, block, 0, s, a, nplanes);                   \
        else klaunch(k_plane8<LL, SPEC_FWD, false>, grid, block, 0, s, a, nplanes);                             \
    } while (0)
    switch (m) {
        case 16: MVTV_PLANE(4); break;
        case 32: MVTV_PLANE(5); break;
        case 64: MVTV_PLANE(6); break;
        case 128: MVTV_PLANE(7); break;
        default: return hipErrorInvalidValue;
    }
#undef MVTV_PLANE
    return hipGetLastError();
}

// The marching line sweeps (k_sweep): shapes with an instantiation
// (m0 = m1: every 3-D mesh of the reference orders; the sweeps have not run on m0 != 512, which only a nominal
// order admits, so such a mesh keeps the per-dimension passes: DESIGN §8)
bool line_sweep_shape_ok(const Geom& g) {
    return g.p == 3 && g.m[1] == 512u && g.m[0] == g.m[1] && g.m[0] % 16u == 0u && g.m[2] >= 2u;
}

// Chunk count of the sweeps: the grid runs in rounds of the resident workgroups (occupancy x CUs), and a round lasts
// as long as its longest chunk, plus the chunk's share of fixed work in plane steps: the line constants and the
// pipeline's fill (~1) and the carries (8 words per line and chunk over the two sweeps and the interface, against the
// 4 a plane step moves: 2). The up sweep's reload of Bin, 1 word per line every 8 planes, grows with the planes and
// not with the chunks (the chunk's first Q comes from the carry it loads anyway). Ties take the fewer chunks. 0: no
// grid of >= one workgroup per CU with chunks of >= 8 planes (the auto gate). 512^3: 32 tiles x 8 chunks of 64 planes,
// one round of one workgroup a CU.
int line_sweep_chunks(const Geom& g, bool gate) {
    if (!line_sweep_shape_ok(g)) return 0;
    static thread_local int dev = -1, slots = 256, cus = 256;
    int dv = 0;
    if (hipGetDevice(&dv) == hipSuccess && dv != dev) {
        hipDeviceProp_t prop;
        int per_cu = 1;
        cus = 256;
        if (hipGetDeviceProperties(&prop, dv) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep<9, true>, spec8::Shape<9>::NT, 0) != hipSuccess ||
            per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        slots = per_cu * cus;
        dev = dv;
    }
    const uint32_t ntile = g.m[0] / 16u, m2 = g.m[2];
    int best = 0;
    uint64_t best_cost = ~uint64_t(0);
    for (uint32_t C = 1; C <= std::min<uint32_t>(m2, uint32_t(kLineSweepMaxChunks)); ++C) {
        if (gate && (ntile * C < uint32_t(cus) || m2 / C < 8u)) continue;
        const uint64_t rounds = (uint64_t(ntile) * C + uint32_t(slots) - 1) / uint32_t(slots);
        const uint64_t cost = rounds * ((m2 + C - 1) / C + 3u);
        if (cost < best_cost) best_cost = cost, best = int(C);
    }
    return best;
}

// phase 0: the down sweep (x holds the dim-0 coefficients; writes B and the chunks' pairs to coef), 1: the interface
// (coef -> lr), 2: the up sweep (reads lr; x = the solve's dim-0 coefficients). coef, lr: 2 C m0 m1 doubles each.
hipError_t launch_line_sweep(const SpecPlan& sp, const Geom& g, hipStream_t s, int phase, double* x, double* coef,
                             double* lr, int C, double sigma, double w0, const AdmmCtl* ctl, const int32_t* skip) {
    if (!line_sweep_shape_ok(g) || C < 1 || uint32_t(C) > g.m[2] || !x || !coef || !lr) return hipErrorInvalidValue;
    const uint32_t nl = g.m[0] * g.m[1];
    if (phase < 0 || phase > 2) return hipErrorInvalidValue;
    SpecArgs a{};
    a.ctl = ctl;
    a.skip = skip;
    a.in = x;
    a.out = x;
    a.tw = reinterpret_cast<const double2*>(sp.tw + sp.tw_off[1]);
    a.twq = reinterpret_cast<const double2*>(sp.twq + sp.twq_off[1]);
    a.lam = sp.lam;
    for (int j = 0; j < kMaxDims; ++j) {
        a.lam_off[j] = sp.lam_off[j];
        a.m[j] = g.m[j];
    }
    for (int S = 0; S < 16; ++S) a.cS[S] = g.cS[S];
    a.sigma = sigma;
    a.w0 = w0;
    a.inv_n = 1.0 / double(g.N);
    a.d = 2;
    a.p = 3;
    for (int j = 0; j < kMaxDims - 1; ++j) a.fd[j] = g.fd[j];
    if (phase == 1) {   // the chunks as k_trisr_iface's ranks: every line owned here (rank 0 of chunk m0 m1)
        klaunch(k_trisr_iface, dim3((nl + 255u) / 256u), dim3(256), 0, s, a, coef, lr, nl, C, 0, g.m[2]);
        return hipGetLastError();
    }
    const dim3 grid(g.m[0] / 16u * uint32_t(C)), block(spec8::Shape<9>::NT);
    if (phase == 0) klaunch(k_sweep<9, false>, grid, block, 0, s, a, coef, g.m[2], C);
    else klaunch(k_sweep<9, true>, grid, block, 0, s, a, lr, g.m[2], C);
    return hipGetLastError();
}

// The blocked last-dimension solve's shape (k_trib, k_tri1). p = 1: blocks of <= 4096 rows (256 threads x 16 rows).
// p >= 2, workgroups of <= 512 threads (phase 3 holds a segment's 32 rows and the carries in registers: 1024 threads
// leave 128 VGPRs and spill): 64-line tiles (512-B rows per wave load; <= 8 segments: blocks of <= 256 rows) where such
// a grid has >= 256 workgroups, else 16-line tiles (<= 32 segments: <= 1024 rows), 4-line tiles for the < 16 lines of a
// narrow 2-D mesh (<= 64 segments: <= 2048 rows); a grid short of 512 workgroups takes more blocks, down to 128 rows
// each. blocks >= 2 forces the count.
bool line_blocks_plan(const Geom& g, int blocks, LineBlocks* lb) {
    const uint32_t m = g.m[g.p - 1], nlines = g.N / m;
    *lb = LineBlocks{};
    if (blocks < 0 || blocks == 1 || uint32_t(blocks) > m) return false;
    auto cdiv = [](uint32_t x, uint32_t y) { return (x + y - 1) / y; };
    if (g.p == 1) {
        const uint32_t nb = blocks ? uint32_t(blocks) : cdiv(m, uint32_t(tri1::BL));
        if (cdiv(m, nb) > uint32_t(tri1::BL)) return false;
        lb->nblk = int(std::max(nb, 1u));
        return true;
    }
    const uint32_t sm = uint32_t(trib::SMAX);
    const uint32_t narrow = nlines >= 16u ? 16u : 4u, nmax = (nlines >= 16u ? 32u : 64u) * sm;   // the fallback tile
    uint32_t tq, nb;
    if (blocks) {
        nb = uint32_t(blocks);
        const uint32_t nhi = cdiv(m, nb);
        tq = (nlines >= 64u && nhi <= 8u * sm && uint64_t(nlines / 64u) * nb >= 256u) ? 64u : narrow;
        if (tq != 64u && nhi > nmax) return false;
    } else {
        nb = cdiv(m, 8u * sm);
        if (nlines >= 64u && uint64_t(nlines / 64u) * nb >= 256u) {
            tq = 64u;
        } else {
            tq = narrow;
            nb = std::max(cdiv(m, nmax), std::min(cdiv(m, 128u), cdiv(512u, cdiv(nlines, tq))));
        }
    }
    const uint32_t nhi = cdiv(m, nb);
    lb->nblk = int(nb);
    lb->tq = int(tq);
    lb->sl = int(std::min(sm, nhi));
    lb->nseg = int(cdiv(nhi, uint32_t(lb->sl)));
    return true;
}

// one launch per phase on s: phase 1 (pairs from zero carries), the interface, phase 3 (the solve into a.out). A timed
// pass (g_timed) spans the three launches: the start event on the first, the stop event on the last.
static hipError_t launch_line_blocks(const SpecPlan& sp, const SpecArgs& a, hipStream_t s, bool formb) {
    const LineBlocks& lb = sp.lb;
    const uint32_t nblk = uint32_t(lb.nblk);
    if (!sp.lb_coef || !sp.lb_lr || nblk < 1 || nblk > a.m[a.d]) return hipErrorInvalidValue;
    const TimedLaunch tl = g_timed;
    g_timed = TimedLaunch{};
    auto go = [&](auto kern, dim3 grid, dim3 block, int phase, auto... args) {
        if (g_launch_log.on) launch_log_push(reinterpret_cast<const void*>(kern), grid, block);
        hipEvent_t e0 = phase == 1 ? tl.start : nullptr, e1 = phase == 3 ? tl.stop : nullptr;
        if (e0 || e1) hipExtLaunchKernelGGL(kern, grid, block, 0, s, e0, e1, 0u, args...);
        else hipLaunchKernelGGL(kern, grid, block, 0, s, args...);
    };
    if (a.p == 1) {
        // 16-B accesses: every array on a 16-B boundary
        uintptr_t al = reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out);
        if (formb) al |= reinterpret_cast<uintptr_t>(a.ga) | reinterpret_cast<uintptr_t>(a.gb);
        if (al & 15u) return hipErrorInvalidValue;
        const dim3 grid(nblk), block(tri1::NT);
        if (formb) go(k_tri1<1, true>, grid, block, 1, a, nblk, sp.lb_coef, sp.lb_lr);
        else go(k_tri1<1, false>, grid, block, 1, a, nblk, sp.lb_coef, sp.lb_lr);
        go(k_blk_iface<16>, dim3(1), dim3(1024), 2, a, sp.lb_coef, sp.lb_lr, nblk);
        if (formb) go(k_tri1<3, true>, grid, block, 3, a, nblk, sp.lb_coef, sp.lb_lr);
        else go(k_tri1<3, false>, grid, block, 3, a, nblk, sp.lb_coef, sp.lb_lr);
        return hipGetLastError();
    }
    if (formb || a.d != a.p - 1) return hipErrorInvalidValue;
    const uint32_t tq = uint32_t(lb.tq), ntile = (a.nlines + tq - 1) / tq;
    if (uint64_t(ntile) * nblk > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid(ntile * nblk), block(tq * uint32_t(lb.nseg));
    constexpr int SM = trib::SMAX;
    if (tq == 64) go(k_trib<1, SM, 64, 8>, grid, block, 1, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    else if (tq == 16) go(k_trib<1, SM, 16, 32>, grid, block, 1, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    else go(k_trib<1, SM, 4, 64>, grid, block, 1, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    // a thread a line where the lines fill the chip, else a wave a line
    if (a.nlines >= 8192u) go(k_trib_iface, dim3((a.nlines + 255u) / 256u), dim3(256), 2, a, sp.lb_coef, sp.lb_lr, nblk);
    else go(k_blk_iface<1>, dim3(a.nlines), dim3(64), 2, a, sp.lb_coef, sp.lb_lr, nblk);
    if (tq == 64) go(k_trib<3, SM, 64, 8>, grid, block, 3, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    else if (tq == 16) go(k_trib<3, SM, 16, 32>, grid, block, 3, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    else go(k_trib<3, SM, 4, 64>, grid, block, 3, a, lb.sl, nblk, ntile, sp.lb_coef, sp.lb_lr);
    return hipGetLastError();
}

// =============================================================================================
// A leading dimension longer than one workgroup's LDS (m > 4096), or any m = a b under mvtv_problem_dct_split: the
// length-m complex FFT of the Makhoul pairing in two passes (the "four-step" factorisation). A line is an a x b matrix,
// sample n = n1 b + n2, frequency k = k1 + a k2:
//
//   Z[k1 + a k2] = sum_n2 W_b^{n2 k2} ( W_m^{n2 k1} sum_n1 W_a^{n1 k1} v[n1 b + n2] )
//
// k_dsc (columns): length-a FFTs over n1 of a tile of columns n2 (the Makhoul order and b = in + ca ga + cb gb folded
// into the load), times W_m^{n2 k1}, into the scratch as packed complex line pairs [pair][k1][n2]. k_dsr (rows):
// length-b FFTs over n2 of rows k1 and a - k1 together, since Z[m - k] lives at (a - k1, b - 1 - k2) (row 0:
// (0, b - k2)); Z[k], Z[m - k] -> the two lines' cosine coefficients as in k_dctg, stored at position b k1 + k2: the
// frequencies stay in that order, the dimension's lam table is stored in it, and the inverse (k_dsr<INV> then
// k_dsc<INV>) reads it back. Both run k_dctg's in-LDS stages (mr_fft, 512 threads).
//
// Twiddles. W_m^j, j < m and the quarter-wave e^{-i pi k/2m}, k < m are both powers of w = e^{-2 pi i/4m}: w^J =
// T1[J >> 12] T2[J & 4095] with every entry a long-double value split into hi + lo doubles, the product formed with
// its rounding errors carried, so a twiddle is as good as one rounded table entry at 32 B (4096 + m / 1024) of table
// instead of 32 B m.
namespace dsp {
constexpr int SLOTS = spec::LDS_WORDS / 2 + 8 * spec::PAD;   // complex slots of a workgroup (64 KB and the pads)
constexpr int GMAX = 64;                                     // row pairs per workgroup of the row pass
}  // namespace dsp

struct SubFft {
    int32_t nrad;
    int32_t rad[8];
    FastDiv fper[8], fL[8];
};

struct SplitArgs {
    const double* in;
    const double* ga;
    const double* gb;
    double ca, cb;
    double* out;
    double2* scr;
    const double2 *twa, *twb;
    const double2 *t1, *t2;
    const uint32_t *reva, *revb;
    uint32_t m, a, b, stride, nlines, nclt;   // nclt: complex lines (line pairs)
    uint32_t C, nct;                          // k_dsc: columns per workgroup, column tiles per line tile
    uint32_t G, npr;                          // k_dsr: row pairs per workgroup, row pairs per line (a / 2 + 1)
    int32_t tq;                               // k_dsc: real lines per workgroup
    FastDiv fds, fC, fa, fb, fG, fnpr, fnclt, fnct;
    const int32_t* skip;
    const AdmmCtl* ctl;
    SubFft pa, pb;
};

// w^J = T1[J >> 12] * T2[J & 4095], entries (re, im) hi then (re, im) lo
__device__ __forceinline__ double2 dd_tw(const double2* __restrict__ t1, const double2* __restrict__ t2, uint32_t J) {
#pragma clang fp contract(off)
    const double2 uh = t1[2 * (J >> 12)], ul = t1[2 * (J >> 12) + 1];
    const double2 vh = t2[2 * (J & 4095u)], vl = t2[2 * (J & 4095u) + 1];
    auto two = [](double x, double y, double& e) {   // x + y = s + e
        const double s = x + y, bb = s - x;
        e = (x - (s - bb)) + (y - bb);
        return s;
    };
    const double p1 = uh.x * vh.x, e1 = fma(uh.x, vh.x, -p1);
    const double p2 = uh.y * vh.y, e2 = fma(uh.y, vh.y, -p2);
    const double p3 = uh.x * vh.y, e3 = fma(uh.x, vh.y, -p3);
    const double p4 = uh.y * vh.x, e4 = fma(uh.y, vh.x, -p4);
    double er, ei;
    const double re = two(p1, -p2, er), im = two(p3, p4, ei);
    const double lr = er + (e1 - e2) + ((uh.x * vl.x + ul.x * vh.x) - (uh.y * vl.y + ul.y * vh.y));
    const double li = ei + (e3 + e4) + ((uh.x * vl.y + ul.x * vh.y) + (uh.y * vl.x + ul.y * vh.x));
    return make_double2(re + lr, im + li);
}

template <bool D0>
__device__ __forceinline__ uint32_t dsp_addr(const SplitArgs& s, uint32_t q, uint32_t pos) {
    if (D0) return q * s.m + pos;
    const uint32_t hi = s.fds.div(q);
    return (q - hi * s.stride) + hi * s.stride * s.m + pos * s.stride;
}

template <bool INV, bool D0, bool FORMB>
__global__ __launch_bounds__(dctg::NT) void k_dsc(const SplitArgs s) {
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    double ca = s.ca, cb = s.cb;
    if (s.skip && *s.skip) return;
    if (s.ctl) {
        if (s.ctl->done) return;
        ca = s.ctl->rho;
        cb = s.ctl->rho * s.ctl->c_prev;
    }
    extern __shared__ double2 buf[];   // (tq / 2) * C lines of a + PAD complex slots
    const uint32_t a = s.a, b = s.b, m = s.m, C = s.C, tq = uint32_t(s.tq), ncl = tq >> 1;
    const int LP = int(a) + spec::PAD;
    const uint32_t lt = s.fnct.div(blockIdx.x), ct = blockIdx.x - lt * s.nct;
    const uint32_t q0 = lt * tq, c0 = ct * C;
    const uint32_t Ca = min(C, b - c0);   // this tile's columns
    const int ltq = __ffs(int(tq)) - 1;
    double* bw = reinterpret_cast<double*>(buf);
    // real element e -> (line ql, column cc, row n1): lanes over the columns for d = 0, over the lines for d > 0
    auto real_el = [&](uint32_t e, uint32_t& ql, uint32_t& cc, uint32_t& n1) {
        if (D0) {
            const uint32_t r = s.fC.div(e);
            cc = e - r * C;
            ql = s.fa.div(r);
            n1 = r - ql * a;
        } else {
            ql = e & (tq - 1u);
            const uint32_t r = e >> ltq;
            n1 = s.fC.div(r);
            cc = r - n1 * C;
        }
    };
    // complex element e -> (complex line cl, column cc, row k1), lanes over the columns
    auto cplx_el = [&](uint32_t e, uint32_t& cl, uint32_t& cc, uint32_t& k1) {
        const uint32_t r = s.fC.div(e);
        cc = e - r * C;
        cl = s.fa.div(r);
        k1 = r - cl * a;
    };
    const uint32_t nreal = tq * C * a, ncplx = ncl * C * a;

    if (!INV) {
        for (uint32_t e = threadIdx.x; e < nreal; e += dctg::NT) {
            uint32_t ql, cc, n1;
            real_el(e, ql, cc, n1);
            double v = 0.0;
            if (cc < Ca && q0 + ql < s.nlines) {
                const uint32_t n = n1 * b + c0 + cc;
                const uint32_t k = 2u * n < m ? 2u * n : 2u * (m - 1u - n) + 1u;   // v[n] = x[2n], v[m-1-n] = x[2n+1]
                const uint32_t gi = dsp_addr<D0>(s, q0 + ql, k);
                v = s.in[gi];
                if (FORMB) v += ca * s.ga[gi] + cb * s.gb[gi];
            }
            bw[2 * (((ql >> 1) * C + cc) * LP + s.reva[n1]) + (ql & 1u)] = v;
        }
    } else {
        for (uint32_t e = threadIdx.x; e < ncplx; e += dctg::NT) {
            uint32_t cl, cc, k1;
            cplx_el(e, cl, cc, k1);
            const uint32_t c = (q0 >> 1) + cl;
            double2 v = make_double2(0.0, 0.0);
            if (cc < Ca && c < s.nclt)
                v = cmul(s.scr[(c * a + k1) * b + c0 + cc], cconj(dd_tw(s.t1, s.t2, 4u * (c0 + cc) * k1)));
            buf[(cl * C + cc) * LP + k1] = v;
        }
    }
    __syncthreads();
    if (!INV) mr_fft<false, false>(buf, s.twa, int(ncl * C), int(a), LP, s.pa);
    else mr_fft<true, true>(buf, s.twa, int(ncl * C), int(a), LP, s.pa);
    if (!INV) {
        for (uint32_t e = threadIdx.x; e < ncplx; e += dctg::NT) {
            uint32_t cl, cc, k1;
            cplx_el(e, cl, cc, k1);
            const uint32_t c = (q0 >> 1) + cl;
            if (cc >= Ca || c >= s.nclt) continue;
            s.scr[(c * a + k1) * b + c0 + cc] =
                cmul(buf[(cl * C + cc) * LP + k1], dd_tw(s.t1, s.t2, 4u * (c0 + cc) * k1));
        }
    } else {
        for (uint32_t e = threadIdx.x; e < nreal; e += dctg::NT) {
            uint32_t ql, cc, n1;
            real_el(e, ql, cc, n1);
            if (cc >= Ca || q0 + ql >= s.nlines) continue;
            const uint32_t n = n1 * b + c0 + cc;
            const uint32_t k = 2u * n < m ? 2u * n : 2u * (m - 1u - n) + 1u;
            s.out[dsp_addr<D0>(s, q0 + ql, k)] = bw[2 * (((ql >> 1) * C + cc) * LP + s.reva[n1]) + (ql & 1u)];
        }
    }
}

template <bool INV, bool D0>
__global__ __launch_bounds__(dctg::NT) void k_dsr(const SplitArgs s) {
    if (s.skip && *s.skip) return;
    if (s.ctl && s.ctl->done) return;
    extern __shared__ double2 buf[];   // 2 G lines (rows k1 and a - k1 of G row pairs) of b + PAD complex slots
    const uint32_t a = s.a, b = s.b, G = s.G;
    const int LP = int(b) + spec::PAD;
    const uint32_t u0 = blockIdx.x * G, nU = s.nclt * s.npr;
    // row pair g of this workgroup -> (complex line c, pair pr): pairs of a line adjacent for d = 0, lines adjacent
    // for d > 0; false past the last one
    auto unit = [&](uint32_t g, uint32_t& c, uint32_t& pr) {
        const uint32_t u = u0 + g;
        if (D0) {
            c = s.fnpr.div(u);
            pr = u - c * s.npr;
        } else {
            pr = s.fnclt.div(u);
            c = u - pr * s.nclt;
        }
        return u < nU;
    };
    // LDS line fl = 2 g + which -> its row of the a x b matrix; false: no such line (past the end, or the pairs 0 and
    // a / 2, which are one row)
    auto line_row = [&](uint32_t fl, uint32_t& c, uint32_t& row) {
        uint32_t pr;
        const bool ok = unit(fl >> 1, c, pr);
        row = (fl & 1u) ? a - pr : pr;
        return ok && (!(fl & 1u) || (pr > 0u && 2u * pr != a));
    };
    // element e of the lines' global side -> (LDS line, position k2): lanes over k2 for d = 0, over the pairs for d > 0
    auto glob_el = [&](uint32_t e, uint32_t& fl, uint32_t& k2) {
        if (D0) {
            fl = s.fb.div(e);
            k2 = e - fl * b;
        } else {
            const uint32_t r = s.fG.div(e), g = e - r * G, w = s.fb.div(r);
            k2 = r - w * b;
            fl = 2u * g + w;
        }
    };
    const uint32_t nel = 2u * G * b;

    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t fl, k2, c, row;
        double2 v = make_double2(0.0, 0.0);
        if (!INV) {
            fl = s.fb.div(e);
            k2 = e - fl * b;
            if (line_row(fl, c, row)) v = s.scr[(c * a + row) * b + k2];
            buf[fl * LP + s.revb[k2]] = v;
        } else {
            glob_el(e, fl, k2);
            if (line_row(fl, c, row)) {
                v.x = s.in[dsp_addr<D0>(s, 2u * c, row * b + k2)];
                if (2u * c + 1u < s.nlines) v.y = s.in[dsp_addr<D0>(s, 2u * c + 1u, row * b + k2)];
            }
            buf[fl * LP + k2] = v;
        }
    }
    __syncthreads();
    if (!INV) mr_fft<false, false>(buf, s.twb, int(2u * G), int(b), LP, s.pb);

    // spectrum <-> cosine coefficients over the pairs (k, m - k), k = pr + a k2: the partner sits at (a - pr, b - 1 - k2),
    // in the same row for the pairs 0 ((0, b - k2)) and a / 2; k = 0 and k = m / 2 pair with themselves
    for (uint32_t t = threadIdx.x; t < G * b; t += dctg::NT) {
        const uint32_t g = s.fb.div(t), k2 = t - g * b;
        uint32_t c, pr;
        if (!unit(g, c, pr)) continue;
        const bool one_row = pr == 0u || 2u * pr == a;
        const uint32_t k2p = pr == 0u ? (k2 ? b - k2 : 0u) : b - 1u - k2;
        if (one_row && k2 > k2p) continue;
        const bool self = one_row && k2 == k2p;
        double2* xa = buf + (2u * g) * LP + k2;
        double2* xb = buf + (2u * g + (one_row ? 0u : 1u)) * LP + k2p;
        const uint32_t k = pr + a * k2;
        const double2 q1 = dd_tw(s.t1, s.t2, k);            // e^{-i pi k / 2m}
        const double2 q2 = make_double2(-q1.y, -q1.x);      // e^{-i pi (m - k) / 2m} = -i conj q1
        if (!INV) {
            const double2 Z1 = *xa;
            if (self) {
                *xa = make_double2(q1.x * Z1.x, q1.x * Z1.y);
            } else {
                const double2 Z2 = *xb;
                const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
                const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
                *xa = make_double2(q1.x * Ap.x - q1.y * Ap.y, q1.x * Bp.x - q1.y * Bp.y);
                *xb = make_double2(q2.x * Ap.x + q2.y * Ap.y, q2.x * Bp.x + q2.y * Bp.y);
            }
        } else {
            // V[k] = conj(q[k]) (X[k] - i X[m-k]), X[m] = 0; Z = V_a + i V_b
            const double2 Xk = *xa;
            const double2 Xmk = self ? (k == 0u ? make_double2(0.0, 0.0) : Xk) : *xb;
            const double2 q1c = cconj(q1), q2c = cconj(q2);
            const double2 va1 = cmul(q1c, make_double2(Xk.x, -Xmk.x));
            const double2 vb1 = cmul(q1c, make_double2(Xk.y, -Xmk.y));
            *xa = make_double2(va1.x - vb1.y, va1.y + vb1.x);
            if (!self) {
                const double2 va2 = cmul(q2c, make_double2(Xmk.x, -Xk.x));
                const double2 vb2 = cmul(q2c, make_double2(Xmk.y, -Xk.y));
                *xb = make_double2(va2.x - vb2.y, va2.y + vb2.x);
            }
        }
    }
    __syncthreads();
    if (INV) mr_fft<true, true>(buf, s.twb, int(2u * G), int(b), LP, s.pb);

    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t fl, k2, c, row;
        if (!INV) {
            glob_el(e, fl, k2);
            if (!line_row(fl, c, row)) continue;
            const double2 v = buf[fl * LP + k2];
            s.out[dsp_addr<D0>(s, 2u * c, row * b + k2)] = v.x;
            if (2u * c + 1u < s.nlines) s.out[dsp_addr<D0>(s, 2u * c + 1u, row * b + k2)] = v.y;
        } else {
            fl = s.fb.div(e);
            k2 = e - fl * b;
            if (line_row(fl, c, row)) s.scr[(c * a + row) * b + k2] = buf[fl * LP + s.revb[k2]];
        }
    }
}

uint32_t dct_split_auto(uint32_t m) {
    int rad[8], nrad = 0;
    uint32_t best = 0;
    for (uint32_t a = 2; uint64_t(a) * a <= m; ++a)
        if (m % a == 0 && m / a <= kSplitMax && dct_radix_plan(a, rad, &nrad) && dct_radix_plan(m / a, rad, &nrad))
            best = a;
    return best;
}

static bool sub_fft_plan(uint32_t n, SubFft* f) {
    if (!dct_radix_plan(n, f->rad, &f->nrad)) return false;
    for (int st = 0, L = 1; st < f->nrad; ++st) {
        f->fper[st] = FastDiv(n / uint32_t(f->rad[st]));
        f->fL[st] = FastDiv(uint32_t(L));
        L *= f->rad[st];
    }
    return true;
}

// the two launches of a split pass on s: forward k_dsc then k_dsr, inverse k_dsr<INV> then k_dsc<INV>. A timed pass
// (g_timed) spans both: the start event on the first, the stop event on the second.
static hipError_t launch_dct_split(const SpecPlan& sp, const Geom& g, hipStream_t st, int mode, int d, const double* in,
                                   const double* ga, double ca, const double* gb, double cb, double* out,
                                   const AdmmCtl* ctl, const int32_t* skip) {
    const DctSplit& ds = sp.split[d];
    const uint32_t m = g.m[d], a = ds.a, b = ds.b;
    if (mode == SPEC_MID || d >= g.p - 1 || a < 2 || b < 2 || uint64_t(a) * b != m || a > kSplitMax || b > kSplitMax ||
        !sp.stw || !sp.srev || !sp.sscr)
        return hipErrorInvalidValue;
    SplitArgs s{};
    s.in = in;
    s.ga = ga;
    s.gb = gb;
    s.ca = ca;
    s.cb = cb;
    s.out = out;
    s.scr = reinterpret_cast<double2*>(sp.sscr);
    s.twa = reinterpret_cast<const double2*>(sp.stw + ds.twa);
    s.twb = reinterpret_cast<const double2*>(sp.stw + ds.twb);
    s.t1 = reinterpret_cast<const double2*>(sp.stw + ds.t1);
    s.t2 = reinterpret_cast<const double2*>(sp.stw + ds.t2);
    s.reva = sp.srev + ds.reva;
    s.revb = sp.srev + ds.revb;
    s.m = m;
    s.a = a;
    s.b = b;
    s.stride = g.stride[d];
    s.nlines = g.N / m;
    s.nclt = (s.nlines + 1u) / 2u;
    if (2 * size_t(s.nclt) * m > sp.sscr_cap) return hipErrorInvalidValue;
    s.skip = skip;
    s.ctl = ctl;
    if (!sub_fft_plan(a, &s.pa) || !sub_fft_plan(b, &s.pb)) return hipErrorInvalidValue;
    const bool d0 = d == 0, formb = ga != nullptr, inv = mode == SPEC_INV;
    if (formb && (inv || !gb)) return hipErrorInvalidValue;
    // columns: 2 lines (d = 0) or <= 16 adjacent ones (128-B rows) by as many columns as the LDS holds, in even tiles
    static const int slots_env = [] {   // probe builds: MVTV_DSP_SLOTS sizes both passes' tiles (complex LDS slots)
        const char* e = probe_env("MVTV_DSP_SLOTS");
        return e ? std::atoi(e) : 0;
    }();
    const uint32_t slots = slots_env > 0 ? uint32_t(slots_env) : uint32_t(dsp::SLOTS);
    uint32_t tq = d0 ? 2u : 16u;
    while (tq > 2u && (tq / 2u) * (a + 1u) > uint32_t(dsp::SLOTS)) tq /= 2u;
    const uint32_t cmax = std::min(b, std::max(1u, slots / ((tq / 2u) * (a + 1u))));
    s.tq = int(tq);
    s.nct = (b + cmax - 1u) / cmax;
    s.C = (b + s.nct - 1u) / s.nct;
    // rows: as many row pairs as the LDS holds, <= GMAX
    s.npr = a / 2u + 1u;
    s.G = std::min<uint32_t>(uint32_t(dsp::GMAX), std::max(1u, slots / (2u * (b + 1u))));
    s.fds = FastDiv(s.stride);
    s.fC = FastDiv(s.C);
    s.fa = FastDiv(a);
    s.fb = FastDiv(b);
    s.fG = FastDiv(s.G);
    s.fnpr = FastDiv(s.npr);
    s.fnclt = FastDiv(s.nclt);
    s.fnct = FastDiv(s.nct);
    const uint64_t gc = uint64_t((s.nlines + tq - 1u) / tq) * s.nct, gr = (uint64_t(s.nclt) * s.npr + s.G - 1u) / s.G;
    if (gc > 0x7fffffffull || gr > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 gridc{uint32_t(gc)}, gridr{uint32_t(gr)}, block(dctg::NT);
    const size_t smc = size_t(tq / 2u) * s.C * (a + 1u) * sizeof(double2), smr = size_t(2u * s.G) * (b + 1u) * sizeof(double2);
    const TimedLaunch tl = g_timed;
    g_timed = TimedLaunch{};
    auto go = [&](auto kern, dim3 grid, size_t smem, bool first) {
        if (smem > 65536)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      int(smem));
        if (g_launch_log.on) launch_log_push(reinterpret_cast<const void*>(kern), grid, block);
        hipEvent_t e0 = first ? tl.start : nullptr, e1 = first ? nullptr : tl.stop;
        if (e0 || e1) hipExtLaunchKernelGGL(kern, grid, block, uint32_t(smem), st, e0, e1, 0u, s);
        else hipLaunchKernelGGL(kern, grid, block, uint32_t(smem), st, s);
    };
    if (!inv) {
        if (d0) {
            if (formb) go(k_dsc<false, true, true>, gridc, smc, true);
            else go(k_dsc<false, true, false>, gridc, smc, true);
            go(k_dsr<false, true>, gridr, smr, false);
        } else {   // (b is formed on load along dim 0 only: launch_dct_pass)
            go(k_dsc<false, false, false>, gridc, smc, true);
            go(k_dsr<false, false>, gridr, smr, false);
        }
    } else if (d0) {
        go(k_dsr<true, true>, gridr, smr, true);
        go(k_dsc<true, true, false>, gridc, smc, false);
    } else {
        go(k_dsr<true, false>, gridr, smr, true);
        go(k_dsc<true, false, false>, gridc, smc, false);
    }
    return hipGetLastError();
}

// =============================================================================================
// A leading dimension under mvtv_problem_dct_chirp (any m, so also m > 4096 with a prime factor >= 11): the length-m
// complex DFT of the Makhoul pairing by Bluestein's identity n k = (n^2 + k^2 - (k - n)^2) / 2,
//
//   Z[k] = c[k] sum_n (v[n] c[n]) conj c[k - n],   c[n] = e^{-i pi n^2 / m},
//
// a circular convolution of length M = a b >= 2m - 1 taken as a two-pass FFT (sample n = n1 b + n2, frequency
// k1 + a k2 of the length-M transform, as in the split passes above). Three launches, one round trip of the scratch
// [pair][k1][n2] between each:
//
//   k_chc (columns in):  load (the Makhoul order and b = in + ca ga + cb gb folded in), times c[n], zero for n >= m,
//                        length-a FFTs over n1, times W_M^{n2 k1}
//   k_chr (rows):        per row k1 the length-b FFT, times the filter spectrum H at (k1, k2) (stored in that order, so
//                        no transposition exists), the inverse length-b FFT, times conj W_M^{n2 k1}, in place
//   k_cho (columns out): inverse length-a FFTs, n < m kept, times c[n]; Z[k] and Z[m - k] -> the two lines' cosine
//                        coefficients at their natural position k
//
// Z[m - k] of k = n1 b + n2 sits in column (m - n2) mod b whatever n1, so a column tile is a set of orbits of that
// involution (chirp_orbit) and a workgroup of k_cho holds both partners: no fourth pass, no complex spectrum written
// out. All three kernels tile by orbits, so one index rule serves them. The inverse cosine transform is the same
// three launches: the inverse DFT is conj(DFT(conj V)), V[k] = conj q[k] (X[k] - i X[m - k]) gathered on k_chc's load,
// the real lines stored by k_cho in the Makhoul order; the filter h[j] = conj c[|j|] is symmetric, so one H serves both.
// The frequencies come out in natural order: the dimension's lam table is the natural one.
struct ChirpArgs {
    const double* in;
    const double* ga;
    const double* gb;
    double ca, cb;
    double* out;
    double2* scr;
    const double2 *twa, *twb;   // the factor FFTs' twiddles
    const double2 *t1, *t2;     // W_M^J = T1[J >> 12] T2[J & 4095], hi + lo entries (dd_tw)
    const double2 *chirp, *qw;  // c[n], n < m; e^{-i pi k / 2m}, k < m
    const double2* H;           // FFT_M(h) / M at position b k1 + k2 for frequency k1 + a k2
    const uint32_t *reva, *revb;
    uint32_t m, a, b, stride, nlines, nclt;
    uint32_t r, nlo, norb;      // m mod b; orbits (t, r - t), t < nlo = r / 2 + 1; then (r + 1 + t - nlo, b - 1 - (t - nlo))
    uint32_t Ch, nct;           // orbits per workgroup (2 Ch column slots), column tiles per line tile
    uint32_t G;                 // k_chr: rows per workgroup
    int32_t tq;                 // real lines per workgroup of the column passes
    FastDiv fds, fC, fa, fb;
    FastDiv fnct;
    const int32_t* skip;
    const AdmmCtl* ctl;
    SubFft pa, pb;
};

// column of slot cc of the tile starting at orbit t0: the orbits' first columns in slots [0, Ch), their partners in
// [Ch, 2 Ch); false for a slot past the last orbit or the second slot of a fixed point
__device__ __forceinline__ bool chirp_col(const ChirpArgs& s, uint32_t t0, uint32_t cc, uint32_t& col) {
    const bool second = cc >= s.Ch;
    const uint32_t t = t0 + (second ? cc - s.Ch : cc);
    if (t >= s.norb) return false;
    uint32_t u, up;
    if (t < s.nlo) {
        u = t;
        up = s.r - t;
    } else {
        u = s.r + 1u + (t - s.nlo);
        up = s.b - 1u - (t - s.nlo);
    }
    col = second ? up : u;
    return !second || up != u;
}

template <bool D0>
__device__ __forceinline__ uint32_t chirp_addr(const ChirpArgs& s, uint32_t q, uint32_t pos) {
    if (D0) return q * s.m + pos;
    const uint32_t hi = s.fds.div(q);
    return (q - hi * s.stride) + hi * s.stride * s.m + pos * s.stride;
}

// element e of a column tile -> (complex line cl, slot cc, row): the scratch side has the lanes over the columns; the
// global side too for d = 0, over the adjacent lines for d > 0
template <bool LINES>
__device__ __forceinline__ void chirp_el(const ChirpArgs& s, uint32_t e, uint32_t ncl, uint32_t& cl, uint32_t& cc,
                                         uint32_t& row) {
    const uint32_t C = 2u * s.Ch;
    if (!LINES) {
        const uint32_t r = s.fC.div(e);
        cc = e - r * C;
        cl = s.fa.div(r);
        row = r - cl * s.a;
    } else {
        cl = e & (ncl - 1u);   // ncl a power of two
        const uint32_t r = e >> (__ffs(int(ncl)) - 1);
        row = s.fC.div(r);
        cc = r - row * C;
    }
}

template <bool INV, bool D0, bool FORMB>
__global__ __launch_bounds__(dctg::NT) void k_chc(const ChirpArgs s) {
    static_assert(D0 || !FORMB, "b is formed on load along dim 0 only");
    double ca = s.ca, cb = s.cb;
    if (s.skip && *s.skip) return;
    if (s.ctl) {
        if (s.ctl->done) return;
        ca = s.ctl->rho;
        cb = s.ctl->rho * s.ctl->c_prev;
    }
    extern __shared__ double2 buf[];   // (tq / 2) * 2 Ch lines of a + PAD complex slots
    const uint32_t a = s.a, b = s.b, m = s.m, C = 2u * s.Ch, ncl = uint32_t(s.tq) >> 1;
    const int LP = int(a) + spec::PAD;
    const uint32_t lt = s.fnct.div(blockIdx.x), ct = blockIdx.x - lt * s.nct;
    const uint32_t c0 = lt * ncl, t0 = ct * s.Ch;
    const uint32_t nel = ncl * C * a;

    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t cl, cc, n1, col = 0;
        chirp_el<!D0>(s, e, ncl, cl, cc, n1);
        const bool live = chirp_col(s, t0, cc, col);
        const uint32_t c = c0 + cl, n = n1 * b + col;
        double2 v = make_double2(0.0, 0.0);
        if (live && c < s.nclt && n < m) {   // (rows n1 >= ceil(m / b) are zero padding: nothing to load)
            const bool two = 2u * c + 1u < s.nlines;
            if (!INV) {
                const uint32_t k = 2u * n < m ? 2u * n : 2u * (m - 1u - n) + 1u;   // v[n] = x[2n], v[m-1-n] = x[2n+1]
                const uint32_t g0 = chirp_addr<D0>(s, 2u * c, k);
                v.x = s.in[g0];
                if (FORMB) v.x += ca * s.ga[g0] + cb * s.gb[g0];
                if (two) {
                    const uint32_t g1 = chirp_addr<D0>(s, 2u * c + 1u, k);
                    v.y = s.in[g1];
                    if (FORMB) v.y += ca * s.ga[g1] + cb * s.gb[g1];
                }
            } else {
                // V[k] = conj(q[k]) (X[k] - i X[m-k]), X[m] = 0; Z = V_a + i V_b; the DFT below takes conj Z
                const uint32_t kp = n ? m - n : 0u;
                double2 Xk, Xm = make_double2(0.0, 0.0);
                Xk.x = s.in[chirp_addr<D0>(s, 2u * c, n)];
                Xk.y = two ? s.in[chirp_addr<D0>(s, 2u * c + 1u, n)] : 0.0;
                if (n) {
                    Xm.x = s.in[chirp_addr<D0>(s, 2u * c, kp)];
                    Xm.y = two ? s.in[chirp_addr<D0>(s, 2u * c + 1u, kp)] : 0.0;
                }
                const double2 qc = cconj(s.qw[n]);
                const double2 va = cmul(qc, make_double2(Xk.x, -Xm.x));
                const double2 vb = cmul(qc, make_double2(Xk.y, -Xm.y));
                v = make_double2(va.x - vb.y, -(va.y + vb.x));
            }
            v = cmul(v, s.chirp[n]);
        }
        buf[(cl * C + cc) * LP + s.reva[n1]] = v;
    }
    __syncthreads();
    mr_fft<false, false>(buf, s.twa, int(ncl * C), int(a), LP, s.pa);
    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t cl, cc, k1, col = 0;
        chirp_el<false>(s, e, ncl, cl, cc, k1);
        const uint32_t c = c0 + cl;
        if (!chirp_col(s, t0, cc, col) || c >= s.nclt) continue;
        s.scr[(size_t(c) * a + k1) * b + col] = cmul(buf[(cl * C + cc) * LP + k1], dd_tw(s.t1, s.t2, col * k1));
    }
}

// rows of the scratch, all lines' alike (no global side): u = c a + k1
__global__ __launch_bounds__(dctg::NT) void k_chr(const ChirpArgs s) {
    if (s.skip && *s.skip) return;
    if (s.ctl && s.ctl->done) return;
    extern __shared__ double2 buf[];   // G lines of b + PAD complex slots
    const uint32_t a = s.a, b = s.b, G = s.G;
    const int LP = int(b) + spec::PAD;
    const size_t u0 = size_t(blockIdx.x) * G, nU = size_t(s.nclt) * a;
    const uint32_t nel = G * b;
    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        const uint32_t g = s.fb.div(e), n2 = e - g * b;
        buf[g * LP + s.revb[n2]] = u0 + g < nU ? s.scr[(u0 + g) * b + n2] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    mr_fft<false, false>(buf, s.twb, int(G), int(b), LP, s.pb);
    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        const uint32_t g = s.fb.div(e), k2 = e - g * b;
        if (u0 + g >= nU) continue;
        const uint32_t u = uint32_t(u0 + g), k1 = u - s.fa.div(u) * a;
        buf[g * LP + k2] = cmul(buf[g * LP + k2], s.H[k1 * b + k2]);
    }
    __syncthreads();
    mr_fft<true, true>(buf, s.twb, int(G), int(b), LP, s.pb);
    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        const uint32_t g = s.fb.div(e), n2 = e - g * b;
        if (u0 + g >= nU) continue;
        const uint32_t u = uint32_t(u0 + g), k1 = u - s.fa.div(u) * a;
        s.scr[(u0 + g) * b + n2] = cmul(buf[g * LP + s.revb[n2]], cconj(dd_tw(s.t1, s.t2, n2 * k1)));
    }
}

template <bool INV, bool D0>
__global__ __launch_bounds__(dctg::NT) void k_cho(const ChirpArgs s) {
    if (s.skip && *s.skip) return;
    if (s.ctl && s.ctl->done) return;
    extern __shared__ double2 buf[];   // (tq / 2) * 2 Ch lines of a + PAD complex slots
    const uint32_t a = s.a, b = s.b, m = s.m, C = 2u * s.Ch, ncl = uint32_t(s.tq) >> 1;
    const int LP = int(a) + spec::PAD;
    const uint32_t lt = s.fnct.div(blockIdx.x), ct = blockIdx.x - lt * s.nct;
    const uint32_t c0 = lt * ncl, t0 = ct * s.Ch;
    const uint32_t nel = ncl * C * a;

    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t cl, cc, k1, col = 0;
        chirp_el<false>(s, e, ncl, cl, cc, k1);
        const uint32_t c = c0 + cl;
        double2 v = make_double2(0.0, 0.0);
        if (chirp_col(s, t0, cc, col) && c < s.nclt) v = s.scr[(size_t(c) * a + k1) * b + col];
        buf[(cl * C + cc) * LP + k1] = v;
    }
    __syncthreads();
    mr_fft<true, true>(buf, s.twa, int(ncl * C), int(a), LP, s.pa);   // sample n1 at reva[n1]
    for (uint32_t e = threadIdx.x; e < nel; e += dctg::NT) {
        uint32_t cl, cc, n1, col = 0;
        chirp_el<!D0>(s, e, ncl, cl, cc, n1);
        const uint32_t c = c0 + cl;
        if (!chirp_col(s, t0, cc, col) || c >= s.nclt) continue;
        const uint32_t n = n1 * b + col;
        if (n >= m) continue;
        const bool two = 2u * c + 1u < s.nlines;
        const double2 Z1 = cmul(buf[(cl * C + cc) * LP + s.reva[n1]], s.chirp[n]);
        if (INV) {   // the real lines, conj of the DFT of conj V, back in the Makhoul order
            const uint32_t k = 2u * n < m ? 2u * n : 2u * (m - 1u - n) + 1u;
            s.out[chirp_addr<D0>(s, 2u * c, k)] = Z1.x;
            if (two) s.out[chirp_addr<D0>(s, 2u * c + 1u, k)] = -Z1.y;
            continue;
        }
        // Z[m - k]: column (m - n2) mod b, the partner slot of this orbit (the slot itself at a fixed point), row
        // (m - k) / b; k = 0 pairs with itself
        double2 Z2 = Z1;
        if (n) {
            const uint32_t kp = m - n, n1p = s.fb.div(kp), colp = kp - n1p * b;
            const uint32_t ccp = colp == col ? cc : (cc >= s.Ch ? cc - s.Ch : cc + s.Ch);
            Z2 = cmul(buf[(cl * C + ccp) * LP + s.reva[n1p]], s.chirp[kp]);
        }
        const double2 q1 = s.qw[n];
        const double2 Ap = make_double2(0.5 * (Z1.x + Z2.x), 0.5 * (Z1.y - Z2.y));
        const double2 Bp = make_double2(0.5 * (Z1.y + Z2.y), -0.5 * (Z1.x - Z2.x));
        s.out[chirp_addr<D0>(s, 2u * c, n)] = q1.x * Ap.x - q1.y * Ap.y;
        if (two) s.out[chirp_addr<D0>(s, 2u * c + 1u, n)] = q1.x * Bp.x - q1.y * Bp.y;
    }
}

// the library's convolution length for m: the smallest 2-3-5-7-smooth M >= 2m - 1 with a factorisation a b, both
// <= kSplitMax; a the largest such divisor <= sqrt(M). false: none (m > (4096^2 + 1) / 2)
bool dct_chirp_auto(uint32_t m, uint32_t* a, uint32_t* b) {
    const uint64_t lim = uint64_t(kSplitMax) * kSplitMax;
    for (uint64_t M = std::max<uint64_t>(4, 2 * uint64_t(m) - 1); M <= lim; ++M) {
        uint64_t r = M;
        for (uint64_t q : {2, 3, 5, 7})
            while (r % q == 0) r /= q;
        if (r != 1) continue;
        uint64_t best = 0;
        for (uint64_t d = 2; d * d <= M; ++d)
            if (M % d == 0 && M / d <= kSplitMax) best = d;
        if (best) {
            *a = uint32_t(best);
            *b = uint32_t(M / best);
            return true;
        }
    }
    return false;
}

// the three launches of a chirp pass (both directions: k_chc, k_chr, k_cho). A timed pass (g_timed) spans them: the
// start event on the first, the stop event on the last.
static hipError_t launch_dct_chirp(const SpecPlan& sp, const Geom& g, hipStream_t st, int mode, int d, const double* in,
                                   const double* ga, double ca, const double* gb, double cb, double* out,
                                   const AdmmCtl* ctl, const int32_t* skip) {
    const DctChirp& dc = sp.chirp[d];
    const uint32_t m = g.m[d], a = dc.a, b = dc.b;
    if (mode == SPEC_MID || d >= g.p - 1 || a < 2 || b < 2 || uint64_t(a) * b + 1 < 2 * uint64_t(m) ||
        a > kSplitMax || b > kSplitMax || !sp.stw || !sp.srev || !sp.sscr)
        return hipErrorInvalidValue;
    ChirpArgs s{};
    s.in = in;
    s.ga = ga;
    s.gb = gb;
    s.ca = ca;
    s.cb = cb;
    s.out = out;
    s.scr = reinterpret_cast<double2*>(sp.sscr);
    s.twa = reinterpret_cast<const double2*>(sp.stw + dc.twa);
    s.twb = reinterpret_cast<const double2*>(sp.stw + dc.twb);
    s.t1 = reinterpret_cast<const double2*>(sp.stw + dc.t1);
    s.t2 = reinterpret_cast<const double2*>(sp.stw + dc.t2);
    s.chirp = reinterpret_cast<const double2*>(sp.stw + dc.chirp);
    s.qw = reinterpret_cast<const double2*>(sp.stw + dc.qw);
    s.H = reinterpret_cast<const double2*>(sp.stw + dc.H);
    s.reva = sp.srev + dc.reva;
    s.revb = sp.srev + dc.revb;
    s.m = m;
    s.a = a;
    s.b = b;
    s.stride = g.stride[d];
    s.nlines = g.N / m;
    s.nclt = (s.nlines + 1u) / 2u;
    if (2 * size_t(s.nclt) * a * b > sp.sscr_cap) return hipErrorInvalidValue;
    s.skip = skip;
    s.ctl = ctl;
    if (!sub_fft_plan(a, &s.pa) || !sub_fft_plan(b, &s.pb)) return hipErrorInvalidValue;
    const bool d0 = d == 0, formb = ga != nullptr, inv = mode == SPEC_INV;
    if (formb && (inv || !gb)) return hipErrorInvalidValue;
    s.r = m % b;
    s.nlo = s.r / 2u + 1u;
    s.norb = s.nlo + (s.r + b) / 2u - s.r;
    // columns: one line pair (d = 0) or <= 8 adjacent ones (128-B rows) by as many orbits (two columns each) as the
    // LDS holds, in even tiles; one orbit of a = 4096 is 131 KB
    const uint32_t slots = uint32_t(dsp::SLOTS);
    uint32_t tq = d0 ? 2u : 16u;
    while (tq > 2u && (tq / 2u) * 2u * (a + 1u) > slots) tq /= 2u;
    const uint32_t hmax = std::min(s.norb, std::max(1u, slots / ((tq / 2u) * 2u * (a + 1u))));
    s.tq = int(tq);
    s.nct = (s.norb + hmax - 1u) / hmax;
    s.Ch = (s.norb + s.nct - 1u) / s.nct;
    s.G = std::min<uint32_t>(2u * uint32_t(dsp::GMAX), std::max(1u, slots / (b + 1u)));
    s.fds = FastDiv(s.stride);
    s.fC = FastDiv(2u * s.Ch);
    s.fa = FastDiv(a);
    s.fb = FastDiv(b);
    s.fnct = FastDiv(s.nct);
    const uint64_t gc = uint64_t((s.nclt + tq / 2u - 1u) / (tq / 2u)) * s.nct;
    const uint64_t gr = (uint64_t(s.nclt) * a + s.G - 1u) / s.G;
    if (gc > 0x7fffffffull || gr > 0x7fffffffull || uint64_t(s.nclt) * a > 0xffffffffull)
        return hipErrorInvalidValue;
    const dim3 gridc{uint32_t(gc)}, gridr{uint32_t(gr)}, block(dctg::NT);
    const size_t smc = size_t(tq / 2u) * 2u * s.Ch * (a + 1u) * sizeof(double2), smr = size_t(s.G) * (b + 1u) * sizeof(double2);
    const TimedLaunch tl = g_timed;
    g_timed = TimedLaunch{};
    auto go = [&](auto kern, dim3 grid, size_t smem, int which) {
        if (smem > 65536)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      int(smem));
        if (g_launch_log.on) launch_log_push(reinterpret_cast<const void*>(kern), grid, block);
        hipEvent_t e0 = which == 0 ? tl.start : nullptr, e1 = which == 2 ? tl.stop : nullptr;
        if (e0 || e1) hipExtLaunchKernelGGL(kern, grid, block, uint32_t(smem), st, e0, e1, 0u, s);
        else hipLaunchKernelGGL(kern, grid, block, uint32_t(smem), st, s);
    };
    if (!inv) {
        if (d0) {
            if (formb) go(k_chc<false, true, true>, gridc, smc, 0);
            else go(k_chc<false, true, false>, gridc, smc, 0);
        } else {   // (b is formed on load along dim 0 only: launch_dct_pass)
            go(k_chc<false, false, false>, gridc, smc, 0);
        }
        go(k_chr, gridr, smr, 1);
        if (d0) go(k_cho<false, true>, gridc, smc, 2);
        else go(k_cho<false, false>, gridc, smc, 2);
    } else {
        if (d0) go(k_chc<true, true, false>, gridc, smc, 0);
        else go(k_chc<true, false, false>, gridc, smc, 0);
        go(k_chr, gridr, smr, 1);
        if (d0) go(k_cho<true, true>, gridc, smc, 2);
        else go(k_cho<true, false>, gridc, smc, 2);
    }
    return hipGetLastError();
}

bool dct_pcg_fusable(const Geom& g, size_t partial_words) {
    const uint32_t m = g.m[0];
    if (g.p < 2 || m < 64 || m > 4096 || (m & (m - 1)) != 0 || probe_env("MVTV_DCT_LDS") || probe_env("MVTV_PCGS_NINE"))
        return false;
    // partial rows of the last pass: one per tile of launch_dct8's d = 0 choice (16 lines up to m = 512,
    // 8192 / m beyond; the smallest one-wave tile, >= 1024 / m lines, when that leaves < 1024 tiles)
    const size_t nlines = g.N / m, tq = std::min<size_t>(16, 8192 / m);
    const size_t tmin = std::max<size_t>(2, 1024 / m);
    const size_t rows = nlines / tq >= 1024 ? (nlines + tq - 1) / tq : (nlines + tmin - 1) / tmin;
    return 2 * rows <= partial_words;
}

hipError_t launch_dct_pass(const SpecPlan& sp, const Geom& g, hipStream_t s, int mode, int d, const double* in,
                           const double* ga, double ca, const double* gb, double cb, double* out, double sigma,
                           double w0, const AdmmCtl* ctl, uint32_t q_off, double inv_n, const int32_t* skip,
                           const PcgFuse* pf, bool fold) {
    if (ga != nullptr && d != 0) return hipErrorInvalidValue;   // b is formed on load along dim 0 only
    SpecArgs a{};
    a.ctl = ctl;
    a.skip = skip;
    a.q_off = q_off;
    a.in = in;
    a.ga = ga;
    a.gb = gb;
    a.ca = ca;
    a.cb = cb;
    a.out = out;
    a.tw = reinterpret_cast<const double2*>(sp.tw + sp.tw_off[d]);
    a.twq = reinterpret_cast<const double2*>(sp.twq + sp.twq_off[d]);
    a.lam = sp.lam;
    for (int j = 0; j < kMaxDims; ++j) {
        a.lam_off[j] = sp.lam_off[j];
        a.m[j] = g.m[j];
    }
    for (int j = 0; j < kMaxDims - 1; ++j) a.fd[j] = g.fd[j];
    for (int S = 0; S < 16; ++S) a.cS[S] = g.cS[S];
    a.sigma = sigma;
    a.w0 = w0;
    a.inv_n = inv_n > 0.0 ? inv_n : 1.0 / double(g.N);   // 1 / (all mesh points): the inverse transforms' scale
    a.stride = g.stride[d];
    a.ls = 0;
    while ((1u << a.ls) < a.stride) ++a.ls;
    const uint32_t m = g.m[d];
    a.nlines = g.N / m;
    a.d = d;
    a.p = g.p;
    a.L = 0;
    while ((1u << a.L) < m) ++a.L;
    const bool formb = ga != nullptr;
    a.fold = fold ? 1 : 0;   // b from the folded s: k_dct8 (power-of-two m >= 8), asynchronous loop only
    static const bool pair16 = [] {   // probe builds: MVTV_DCT_P16=0 keeps the d = 0 passes' 8-B coefficient accesses
        const char* e = probe_env("MVTV_DCT_P16");
        return !(e && std::atoi(e) == 0);
    }();
    a.pair16 = pair16 ? 1 : 0;
    // the line solve along the last dimension in blocks: any length (mvtv_problem_line_blocks forces it at any m)
    if (sp.lb.nblk > 0 && mode == SPEC_MID && d == g.p - 1 && !fold && !(pf && pf->mode))
        return launch_line_blocks(sp, a, s, formb);
    // a leading dimension in two passes: m > 4096 (the library's factorisation) or forced (mvtv_problem_dct_split)
    if (d < g.p - 1 && sp.split[d].a > 0) {
        if (fold || (pf && pf->mode)) return hipErrorInvalidValue;
        return launch_dct_split(sp, g, s, mode, d, in, ga, ca, gb, cb, out, ctl, skip);
    }
    // a leading dimension by Bluestein's identity over a two-pass convolution (mvtv_problem_dct_chirp): any m
    if (d < g.p - 1 && sp.chirp[d].a > 0) {
        if (fold || (pf && pf->mode)) return hipErrorInvalidValue;
        return launch_dct_chirp(sp, g, s, mode, d, in, ga, ca, gb, cb, out, ctl, skip);
    }
    if (m > 4096) return hipErrorInvalidValue;
    if (a.fold && (!formb || !gb || !ctl || (1u << a.L) != m || (1u << a.ls) != a.stride || a.L < 3 ||
                   probe_env("MVTV_DCT_LDS") || mode == SPEC_MID))
        return hipErrorInvalidValue;
    if (pf && pf->mode) {   // PCG-fused d = 0 pass (dct_pcg_fusable meshes): k_dct8 only
        if (d != 0 || formb || (1u << a.L) != m || a.L < 6 || mode != (pf->mode == 1 ? SPEC_FWD : SPEC_INV) ||
            (pf->mode == 2 && !pf->nparts))
            return hipErrorInvalidValue;
        a.pf = *pf;
    }
    if ((1u << a.L) != m || (1u << a.ls) != a.stride) {   // mixed radix, or a power of two over a general stride
        const bool planned = dct_radix_plan(m, a.rad, &a.nrad);
        if (!planned && sp.blu_M[d] == 0) return hipErrorInvalidValue;
        a.fds = FastDiv(a.stride);
        a.fm = FastDiv(m);
        if (planned) {
            for (int st = 0, L = 1; st < a.nrad; ++st) {
                a.fper[st] = FastDiv(m / uint32_t(a.rad[st]));
                a.fL[st] = FastDiv(uint32_t(L));
                L *= a.rad[st];
            }
            a.perm = sp.perm + sp.perm_off[d];
        }
        static const bool few_off = probe_flag("MVTV_FEW_LINES_OFF");
        // strided passes: tiles in XCD runs (probe builds: MVTV_XRUN_OFF=1 deals them round-robin)
        static const bool xrun_off = probe_flag("MVTV_XRUN_OFF");
        a.xrun = (d > 0 && !xrun_off) ? 1 : 0;
        // the line solve along the last dimension also for the few lines of a 2-D mesh, on 4-line tiles where that
        // makes >= 250 workgroups (a Bluestein MID pass is four FFTs of twice the length per line pair): 2039^2 2070 ->
        // 3310 ADMM it/s, 1009^2 8431 -> 9086, 1000^2 10682 -> 11017; 500^2 (125 such tiles) 16059 -> 15855 keeps the
        // MID pass (profiles/r05/v15_trig_2d; probe builds: MVTV_TRIG_FEW_OFF=1)
        static const bool trig_few_off = probe_flag("MVTV_TRIG_FEW_OFF");
        const bool trig_lines = a.nlines / uint32_t(trig::TQ) >= 256u || (!trig_few_off && a.nlines >= 1000u);
        if (mode == SPEC_MID && d > 0 && !formb && trig_lines && !probe_env("MVTV_DCT_TRI0")) {
            int sl = trig_seg(m);
            // more than 16 segments keep k_trigr on 32-line tiles; where 64-line tiles fill the chip, <= 32-row
            // segments with a shorter last one bring it to 16 (500: 25 x 20 -> 15 x 32 + 20 rows, 0.69 -> 0.48 ms
            // at 500^3, profiles/r05/v13_trig_sl32; probe builds: MVTV_TRIG_SL forces, MVTV_TRIG_NARROW keeps)
            static const bool sl_forced = probe_env("MVTV_TRIG_SL") != nullptr;
            if (sl > 0 && !sl_forced && (m + uint32_t(sl) - 1) / uint32_t(sl) > 16u && a.nlines / 64u >= 256u &&
                (m + 15u) / 16u <= uint32_t(trig::SMAX))
                sl = int((m + 15u) / 16u);
            if (sl > 0) {
                const int nseg = int((m + uint32_t(sl) - 1) / uint32_t(sl));
                launch_trig(a, s, sl, nseg, int(m) - (nseg - 1) * sl);
                return hipGetLastError();
            }
        }
        if (!planned) {   // Bluestein (k_dctb8): L = log2 M, the length-M twiddles
            const double2* t = reinterpret_cast<const double2*>(sp.blu + sp.blu_off[d]);
            a.L = 0;
            while ((1u << a.L) < sp.blu_M[d]) ++a.L;
            a.bchirp = t;
            a.bvf = t + m;
            a.bvi = t + m + sp.blu_M[d];
            a.tw = t + m + 2 * sp.blu_M[d];
            return launch_dctb(a, s, mode, d == 0, formb);
        }
        if (launch_dctm(a, s, mode, d == 0, formb)) return hipGetLastError();
        // <= 16 lines (128-B rows for d > 0) in <= 64 KB of LDS; few lines (a 2-D mesh: 1000 lines of 1000) take
        // smaller tiles until the grid has >= 512 workgroups (two a CU) or the tile two lines (probe builds:
        // MVTV_FEW_LINES_OFF=1 keeps the LDS-sized tile)
        int tq = 16;
        while (tq > 2 && (tq / 2) * int(m + spec::PAD) > spec::LDS_WORDS / 2 + 8 * spec::PAD) tq /= 2;
        if (!few_off) tq = few_lines_tq(a.nlines, tq, 2);
        a.tq = tq;
        launch_dctg(a, s, mode, d == 0, formb);
        return hipGetLastError();
    }
    if (const int tq = tri_tiles(a, mode, formb)) return launch_tri(a, s, tq);
    if (a.L >= 3 && !probe_env("MVTV_DCT_LDS")) {
        switch (a.L) {
            case 3: launch_dct8<3>(a, s, mode, d == 0, formb); break;
            case 4: launch_dct8<4>(a, s, mode, d == 0, formb); break;
            case 5: launch_dct8<5>(a, s, mode, d == 0, formb); break;
            case 6: launch_dct8<6>(a, s, mode, d == 0, formb); break;
            case 7: launch_dct8<7>(a, s, mode, d == 0, formb); break;
            case 8: launch_dct8<8>(a, s, mode, d == 0, formb); break;
            case 9: launch_dct8<9>(a, s, mode, d == 0, formb); break;
            case 10: launch_dct8<10>(a, s, mode, d == 0, formb); break;
            case 11: launch_dct8<11>(a, s, mode, d == 0, formb); break;
            case 12: launch_dct8<12>(a, s, mode, d == 0, formb); break;
        }
        if (pf && pf->mode == 2 && *pf->nparts < 0) return hipErrorInvalidValue;
        return hipGetLastError();
    }
    int tq = std::max(2, std::min(16, int(spec::LDS_WORDS / m)));
    if (d > 0) tq = std::min<int>(tq, int(g.stride[d]));
    if (tq < 2) return hipErrorInvalidValue;
    a.tq = tq;
    const dim3 grid((a.nlines + uint32_t(tq) - 1) / uint32_t(tq)), block(spec::NT);
#define MVTV_DCT_LAUNCH(MODE, D0, FB) klaunch(k_dct<MODE, D0, FB>, grid, block, 0, s, a)
    if (mode == SPEC_FWD) {
        if (d == 0) {
            if (formb) MVTV_DCT_LAUNCH(SPEC_FWD, true, true);
            else MVTV_DCT_LAUNCH(SPEC_FWD, true, false);
        } else {
            MVTV_DCT_LAUNCH(SPEC_FWD, false, false);
        }
    } else if (mode == SPEC_INV) {
        if (d == 0) MVTV_DCT_LAUNCH(SPEC_INV, true, false);
        else MVTV_DCT_LAUNCH(SPEC_INV, false, false);
    } else {
        if (d == 0) {   // p = 1: the only pass
            if (formb) MVTV_DCT_LAUNCH(SPEC_MID, true, true);
            else MVTV_DCT_LAUNCH(SPEC_MID, true, false);
        } else {
            MVTV_DCT_LAUNCH(SPEC_MID, false, false);
        }
    }
#undef MVTV_DCT_LAUNCH
    return hipGetLastError();
}

}  // namespace mvtv
