// C-SVC fits of the reference's `-bc SVM` branch: GridSearchCV(SVC(kernel, probability=True, max_iter, tol), {'C': 1/alphas})
// (set_model / fit_model, modeling.py:1025-1029, :1050-1056, :1086-1090).  scikit-learn's SVC is libsvm; at the reference's
// default --max_iter 1000 a fit on a non-separable design stops at the cap, and what GridSearchCV then scores is the 1000th
// iterate of libsvm's solver, not the optimum.  So this is libsvm's Solver::Solve WITHOUT shrinking restated step for step:
//   min 1/2 a'Qa - e'a,  0 <= a_i <= C,  y'a = 0,  Q_ij = y_i y_j K_ij,  class 0 is +1, no class weights
//   * solver index order = the fit's training samples, class 0 first, then class 1, input order kept within a class;
//     alpha = 0, G = -1
//   * working set by WSS2 (Fan, Chen, Lin 2005): i = arg max of -y_t G_t over I_up, the LAST maximal index; j = arg min of
//     -(Gmax + y_j G_j)^2 / max(QD_i + QD_j - 2 y_i y_j Q_ij, 1e-12) over I_low with a positive numerator, the LAST
//     minimal index; stop when Gmax + Gmax2 < tol (not counted as an iteration) or after max_iter iterations
//   * the two-variable update with libsvm's clipping, then G_k += Q_ik d_alpha_i + Q_jk d_alpha_j in that operation order,
//     f64 throughout, no FMA fusion (the translation unit is compiled -ffp-contract=off)
//   * Q entries are float (libsvm's Qfloat): K evaluated in double, times y_i y_j, rounded; QD is double
//   * rho: mean of y_i G_i over the free variables, else the midpoint of the bounds (calculate_rho)
// Two kernels: svc_gram_kernel builds the sample x sample dot products once per call (popcounts of bit-packed rows for a
// 0/1 design, which are exact in float; f64 dot products otherwise); svc_smo_kernel runs one workgroup of four waves per
// fit with alpha, G, QD, the index list, the current row Q_i and the labels in LDS (33 B per training sample, 135 KB at
// 4096 samples).  psk_svc_decision (svc_decision_kernel, further down) evaluates a fitted model on new rows in the order of
// the loop that ends svc_smo_kernel, without a sample x sample matrix.
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_host.h"

namespace {

constexpr int SVC_THREADS = 256;
constexpr int SVC_MAX_N = 4096;
constexpr int SVC_TILE = 16;
constexpr double SVC_TAU = 1e-12;
constexpr int SVC_RED_BYTES = 28 * 8 + 12 * 4;   // 28 doubles and 12 ints of reduction slots: 272 B, a multiple of 16

// ---- Gram matrix -------------------------------------------------------------------------------------------------------
// D[i][j] = popc(r_i & r_j) over the W u64 words of the bit-packed rows: a 16 x 16 tile per workgroup, the rows of the
// tile staged in LDS 16 words at a time.
__global__ __launch_bounds__(SVC_TILE * SVC_TILE) void svc_gram_bits_kernel(const uint64_t *__restrict__ bits, int n, int W,
                                                                            float *__restrict__ D)
{
    __shared__ uint64_t ra[SVC_TILE][SVC_TILE + 1], rb[SVC_TILE][SVC_TILE + 1];
    const int tx = threadIdx.x & (SVC_TILE - 1), ty = threadIdx.x / SVC_TILE;
    const int i0 = blockIdx.y * SVC_TILE, j0 = blockIdx.x * SVC_TILE;
    uint32_t s = 0;
    for (int w0 = 0; w0 < W; w0 += SVC_TILE) {
        const int w = w0 + tx;
        ra[ty][tx] = (i0 + ty < n && w < W) ? bits[(size_t)(i0 + ty) * W + w] : 0;
        rb[ty][tx] = (j0 + ty < n && w < W) ? bits[(size_t)(j0 + ty) * W + w] : 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SVC_TILE; q++) s += (uint32_t)__popcll(ra[ty][q] & rb[tx][q]);
        __syncthreads();
    }
    if (i0 + ty < n && j0 + tx < n) D[(size_t)(i0 + ty) * n + j0 + tx] = (float)s;
}

// D[i][j] = sum_k x_ik x_jk in f64, k ascending (libsvm's dot() order), for designs that are not 0/1.
__global__ __launch_bounds__(SVC_TILE * SVC_TILE) void svc_gram_dense_kernel(const float *__restrict__ X, int n, int p,
                                                                             double *__restrict__ D)
{
    __shared__ float ra[SVC_TILE][SVC_TILE + 1], rb[SVC_TILE][SVC_TILE + 1];
    const int tx = threadIdx.x & (SVC_TILE - 1), ty = threadIdx.x / SVC_TILE;
    const int i0 = blockIdx.y * SVC_TILE, j0 = blockIdx.x * SVC_TILE;
    double s = 0.0;
    for (int k0 = 0; k0 < p; k0 += SVC_TILE) {
        const int k = k0 + tx;
        ra[ty][tx] = (i0 + ty < n && k < p) ? X[(size_t)(i0 + ty) * p + k] : 0.0f;
        rb[ty][tx] = (j0 + ty < n && k < p) ? X[(size_t)(j0 + ty) * p + k] : 0.0f;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SVC_TILE; q++) s += (double)ra[ty][q] * (double)rb[tx][q];
        __syncthreads();
    }
    if (i0 + ty < n && j0 + tx < n) D[(size_t)(i0 + ty) * n + j0 + tx] = s;
}

template <typename T> __global__ void svc_diag_kernel(const T *__restrict__ D, int n, double *__restrict__ diag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) diag[i] = (double)D[(size_t)i * n + i];
}

// ---- SMO ---------------------------------------------------------------------------------------------------------------
// (value, index) maximum with the LAST index winning among equal values: a total order, so the result does not depend on
// the order in which lanes and waves are combined.
__device__ __forceinline__ bool svc_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i > bi); }

__device__ __forceinline__ void svc_wave_argmax(double &v, int &i)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double ov = psk_shfl_xor_f64(v, d);
        const int oi = __shfl_xor(i, d, 64);
        if (svc_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

__device__ __forceinline__ double svc_wave_max(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, psk_shfl_xor_f64(v, d));
    return v;
}

// K(a, b) in double from the dot product d_ab and the squared norms (rbf: libsvm's exp(-gamma (|a|^2 + |b|^2 - 2 a.b)))
template <int KERN> __device__ __forceinline__ double svc_kval(double dab, double sa, double sb, double gamma)
{
    if (KERN == 0) return dab;
    return exp(-gamma * (sa + sb - 2 * dab));
}

template <typename T, int KERN>
__global__ __launch_bounds__(SVC_THREADS) void svc_smo_kernel(
    const T *__restrict__ D, const double *__restrict__ diag, const int32_t *__restrict__ y01, const int32_t *__restrict__ fold,
    int n, int l_cap, const double *__restrict__ fit_C, const double *__restrict__ fit_gamma,
    const int32_t *__restrict__ fit_fold, double tol, int max_iter, double *__restrict__ dual, double *__restrict__ rho_out,
    double *__restrict__ dec, int32_t *__restrict__ iters)
{
    // all LDS in the dynamic region, every carve a multiple of 16 bytes (l_cap is a multiple of 8): the reductions' slots
    // first (SVC_RED_BYTES), then the per-sample arrays
    extern __shared__ __attribute__((aligned(16))) double svc_lds[];
    double *r1v = svc_lds, *r1g = r1v + 4, *r2v = r1g + 4;
    double(*rr)[4] = reinterpret_cast<double(*)[4]>(r2v + 4);
    int *r1i = reinterpret_cast<int *>(svc_lds + 28), *r2i = r1i + 4;
    uint32_t *scan_lds = reinterpret_cast<uint32_t *>(r2i + 4);
    double *alpha = svc_lds + SVC_RED_BYTES / 8, *G = alpha + l_cap, *SQ = G + l_cap;   // SQ: x_k . x_k (QD of the linear kernel)
    int32_t *idx = reinterpret_cast<int32_t *>(SQ + l_cap);
    float *Qi = reinterpret_cast<float *>(idx + l_cap);
    int8_t *ys = reinterpret_cast<int8_t *>(Qi + l_cap);

    const int fit = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double C = fit_C[fit], gamma = KERN ? fit_gamma[fit] : 0.0;
    const int tf = fit_fold[fit];

    // index list: training samples of class 0 in input order, then those of class 1 (svm_group_classes)
    int l = 0;
    for (int cls = 0; cls < 2; cls++)
        for (int s0 = 0; s0 < n; s0 += SVC_THREADS) {
            const int s = s0 + tid;
            const uint32_t take = (s < n && fold[s] != tf && (y01[s] != 0) == (cls != 0)) ? 1u : 0u;
            uint32_t total;
            const uint32_t off = psk_block_excl_scan_u32<SVC_THREADS>(take, &total, scan_lds);
            if (take) {
                const int k = l + (int)off;
                idx[k] = s;
                ys[k] = cls ? -1 : 1;
                alpha[k] = 0.0;
                G[k] = -1.0;
                SQ[k] = diag[s];
            }
            l += (int)total;
        }
    __syncthreads();

    int iter = 0;
    while (max_iter == -1 || iter < max_iter) {
        // i and Gmax over I_up; Gmax2 over I_low (it does not depend on i)
        double bv = -INFINITY, g2 = -INFINITY;
        int bi = -1;
        for (int k = tid; k < l; k += SVC_THREADS) {
            const double a = alpha[k], g = G[k];
            if (ys[k] > 0) {
                if (a < C && -g >= bv) { bv = -g; bi = k; }
                if (a > 0.0) g2 = fmax(g2, g);
            } else {
                if (a > 0.0 && g >= bv) { bv = g; bi = k; }
                if (a < C) g2 = fmax(g2, -g);
            }
        }
        svc_wave_argmax(bv, bi);
        g2 = svc_wave_max(g2);
        if (lane == 0) { r1v[wave] = bv; r1i[wave] = bi; r1g[wave] = g2; }
        __syncthreads();
        double Gmax = r1v[0], Gmax2 = r1g[0];
        int i = r1i[0];
#pragma unroll
        for (int w = 1; w < 4; w++) {
            if (svc_better(r1v[w], r1i[w], Gmax, i)) { Gmax = r1v[w]; i = r1i[w]; }
            Gmax2 = fmax(Gmax2, r1g[w]);
        }
        if (i < 0 || Gmax + Gmax2 < tol) break;

        // row i of Q, kept in LDS for the update; j over I_low
        const int yi = ys[i], si = idx[i];
        const double sqi = SQ[i], QDi = KERN ? 1.0 : sqi;
        const T *Di = D + (size_t)si * n;
        bv = -INFINITY;
        bi = -1;
        for (int k = tid; k < l; k += SVC_THREADS) {
            const int yk = ys[k];
            const double sqk = SQ[k], QDk = KERN ? 1.0 : sqk;
            const float q = (float)((double)(yi * yk) * svc_kval<KERN>((double)Di[idx[k]], sqi, sqk, gamma));
            Qi[k] = q;
            const double a = alpha[k], g = G[k];
            double gd, qc;
            bool in_low;
            if (yk > 0) {
                in_low = a > 0.0;
                gd = Gmax + g;
                qc = QDi + QDk - 2.0 * yi * (double)q;
            } else {
                in_low = a < C;
                gd = Gmax - g;
                qc = QDi + QDk + 2.0 * yi * (double)q;
            }
            if (in_low && gd > 0.0) {
                const double o = (gd * gd) / (qc > 0.0 ? qc : SVC_TAU);   // -obj_diff: its maximum is obj_diff's minimum
                if (o >= bv) { bv = o; bi = k; }
            }
        }
        svc_wave_argmax(bv, bi);
        if (lane == 0) { r2v[wave] = bv; r2i[wave] = bi; }
        __syncthreads();
        double ov = r2v[0];
        int j = r2i[0];
#pragma unroll
        for (int w = 1; w < 4; w++)
            if (svc_better(r2v[w], r2i[w], ov, j)) { ov = r2v[w]; j = r2i[w]; }
        if (j < 0) break;
        iter++;

        // the two-variable update, by every thread for itself from the same LDS words
        const int yj = ys[j], sj = idx[j];
        const double sqj = SQ[j], QDj = KERN ? 1.0 : sqj;
        const double oai = alpha[i], oaj = alpha[j], Gi = G[i], Gj = G[j], Qij = (double)Qi[j];
        double ai = oai, aj = oaj;
        if (yi != yj) {
            double qc = QDi + QDj + 2 * Qij;
            if (qc <= 0.0) qc = SVC_TAU;
            const double delta = (-Gi - Gj) / qc, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) { aj = 0.0; ai = diff; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = -diff; }
            }
            if (diff > 0.0) {   // C_i - C_j = 0: no class weights
                if (ai > C) { ai = C; aj = C - diff; }
            } else {
                if (aj > C) { aj = C; ai = C + diff; }
            }
        } else {
            double qc = QDi + QDj - 2 * Qij;
            if (qc <= 0.0) qc = SVC_TAU;
            const double delta = (Gi - Gj) / qc, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) {
                if (ai > C) { ai = C; aj = sum - C; }
            } else {
                if (aj < 0.0) { aj = 0.0; ai = sum; }
            }
            if (sum > C) {
                if (aj > C) { aj = C; ai = sum - C; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = sum; }
            }
        }
        const double dai = ai - oai, daj = aj - oaj;
        __syncthreads();   // every thread has read alpha and G of i and j
        const T *Dj = D + (size_t)sj * n;
        for (int k = tid; k < l; k += SVC_THREADS) {
            const double sqk = SQ[k];
            const float qj = (float)((double)(yj * ys[k]) * svc_kval<KERN>((double)Dj[idx[k]], sqj, sqk, gamma));
            G[k] += (double)Qi[k] * dai + (double)qj * daj;
        }
        if (tid == (i & (SVC_THREADS - 1))) alpha[i] = ai;
        if (tid == (j & (SVC_THREADS - 1))) alpha[j] = aj;
        // the next pass reads only the thread's own k; the reductions' barriers order everything else
    }
    __syncthreads();

    // rho (calculate_rho)
    double nfree = 0.0, sfree = 0.0, ub = INFINITY, lb = -INFINITY;
    for (int k = tid; k < l; k += SVC_THREADS) {
        const double a = alpha[k], yG = (double)ys[k] * G[k];
        if (a >= C) {
            if (ys[k] < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
        } else if (a <= 0.0) {
            if (ys[k] > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG);
        } else {
            nfree += 1.0;
            sfree += yG;
        }
    }
    nfree = psk_wave_sum_f64_dpp(nfree);
    sfree = psk_wave_sum_f64_dpp(sfree);
    ub = -svc_wave_max(-ub);
    lb = svc_wave_max(lb);
    if (lane == 0) { rr[0][wave] = nfree; rr[1][wave] = sfree; rr[2][wave] = ub; rr[3][wave] = lb; }
    __syncthreads();
    nfree = (rr[0][0] + rr[0][1]) + (rr[0][2] + rr[0][3]);
    sfree = (rr[1][0] + rr[1][1]) + (rr[1][2] + rr[1][3]);
    ub = fmin(fmin(rr[2][0], rr[2][1]), fmin(rr[2][2], rr[2][3]));
    lb = fmax(fmax(rr[3][0], rr[3][1]), fmax(rr[3][2], rr[3][3]));
    const double rho = nfree > 0.0 ? sfree / nfree : (ub + lb) / 2;

    for (int k = tid; k < l; k += SVC_THREADS) dual[(size_t)fit * n + idx[k]] = (double)ys[k] * alpha[k];
    if (tid == 0) { rho_out[fit] = rho; iters[fit] = iter; }
    // decision values of every sample, support vectors in solver order (svm_predict_values)
    for (int s = tid; s < n; s += SVC_THREADS) {
        const double sqs = KERN ? diag[s] : 0.0;
        double sum = 0.0;
        for (int k = 0; k < l; k++) {
            const double a = alpha[k];
            if (a != 0.0)
                sum += ((double)ys[k] * a) * svc_kval<KERN>((double)D[(size_t)idx[k] * n + s], SQ[k], sqs, gamma);
        }
        dec[(size_t)fit * n + s] = sum - rho;
    }
}

// what every SMO launch reads and writes, beside its kernel matrix
struct SvcArrs {
    FitArr<double> diag, C, gamma, dual, rho, dec;
    FitArr<int32_t> y, fold, fit_fold, iters;
};

template <typename T>
int svc_launch_smo(psk_ctx *ctx, const T *D, const SvcArrs &b, int n, int n_fits, int kernel, double tol, int max_iter)
{
    const int l_cap = (n + 7) & ~7;
    const size_t lds = SVC_RED_BYTES + (size_t)l_cap * (3 * 8 + 4 + 4 + 1);
    auto kern = kernel == 0 ? svc_smo_kernel<T, 0> : svc_smo_kernel<T, 1>;
    if (lds > 64 * 1024)
        PSK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<n_fits, SVC_THREADS, lds, ctx->stream>>>(D, b.diag, b.y, b.fold, n, l_cap, b.C, b.gamma, b.fit_fold, tol, max_iter, b.dual,
                                                    b.rho, b.dec, b.iters);
    PSK_HIP(ctx, hipGetLastError());
    return PSK_OK;
}

// ---- decision values of new rows ---------------------------------------------------------------------------------------
// psk_svc_decision: dec[i] = (sum_j coef[j] K(SV_j, X_i)) - rho in the order of the loop that ends svc_smo_kernel.  A
// workgroup owns DEC_ROWS rows and walks the support vectors in tiles of DEC_TILE; within a tile it walks the columns in
// chunks staged in LDS (DEC_WORDS packed words, or DEC_COLS floats), every thread keeping the dot products of one row with
// DEC_PER of the tile's support vectors.  The rounded products coef[j] * K then go to LDS, and ONE lane per row adds them
// in j order: the sum of a row is serial and stays in that lane's register from the first support vector to the last.
constexpr int DEC_THREADS = 256;
constexpr int DEC_ROWS = 32;
constexpr int DEC_TILE = 64;
constexpr int DEC_GROUPS = DEC_THREADS / DEC_ROWS;   // thread t: row t % DEC_ROWS, support vectors t / DEC_ROWS + DEC_GROUPS q
constexpr int DEC_PER = DEC_TILE / DEC_GROUPS;
constexpr int DEC_WORDS = 16;                        // u64 words of a row per staged chunk
constexpr int DEC_COLS = 32;                         // floats of a row per staged chunk

// row norms: popcount of the packed row, or the f64 sum of squares with the columns ascending (the diagonal of the fit's
// Gram matrix, computed the same way)
__global__ void svc_norm_bits_kernel(const uint64_t *__restrict__ bits, int rows, int W, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows) return;
    uint32_t s = 0;
    for (int w = 0; w < W; w++) s += (uint32_t)__popcll(bits[i * W + w]);
    out[i] = (double)s;
}

__global__ void svc_norm_dense_kernel(const float *__restrict__ X, int rows, int p, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows) return;
    double s = 0.0;
    for (int k = 0; k < p; k++) {
        const double v = (double)X[i * p + k];
        s += v * v;
    }
    out[i] = s;
}

// T = uint64_t: rows of W packed words, the dot product a popcount; T = float: rows of W floats, the dot product in f64 with
// the columns ascending.  CH = the chunk of a row staged at a time.
template <typename T, int CH, int KERN>
__global__ __launch_bounds__(DEC_THREADS) void svc_decision_kernel(const T *__restrict__ X, int m, int W, const T *__restrict__ SV,
                                                                    int n_sv, const double *__restrict__ xnorm,
                                                                    const double *__restrict__ svnorm, const double *__restrict__ coef,
                                                                    double rho, double gamma, double *__restrict__ dec)
{
    using Acc = typename std::conditional<std::is_same<T, uint64_t>::value, uint32_t, double>::type;
    __shared__ T xs[DEC_ROWS][CH + 1], ss[DEC_TILE][CH + 1];
    __shared__ double prod[DEC_ROWS][DEC_TILE + 1];
    const int tid = threadIdx.x, r = tid % DEC_ROWS, g = tid / DEC_ROWS;
    const size_t row0 = (size_t)blockIdx.x * DEC_ROWS;
    const bool row_ok = row0 + r < (size_t)m;
    const double sb = (KERN && row_ok) ? xnorm[row0 + r] : 0.0;
    double sum = 0.0;   // (threads below DEC_ROWS: the decision value of row tid)
    for (int j0 = 0; j0 < n_sv; j0 += DEC_TILE) {
        const int tile = min(DEC_TILE, n_sv - j0);
        Acc d[DEC_PER];
#pragma unroll
        for (int q = 0; q < DEC_PER; q++) d[q] = 0;
        for (int w0 = 0; w0 < W; w0 += CH) {
            const int wn = min(CH, W - w0);
            for (int e = tid; e < DEC_ROWS * CH; e += DEC_THREADS) {
                const int er = e / CH, ew = e % CH;
                xs[er][ew] = (row0 + er < (size_t)m && ew < wn) ? X[(row0 + er) * W + w0 + ew] : T(0);
            }
            for (int e = tid; e < DEC_TILE * CH; e += DEC_THREADS) {
                const int ej = e / CH, ew = e % CH;
                ss[ej][ew] = (ej < tile && ew < wn) ? SV[(size_t)(j0 + ej) * W + w0 + ew] : T(0);
            }
            __syncthreads();
            for (int w = 0; w < wn; w++) {
                const T xv = xs[r][w];
#pragma unroll
                for (int q = 0; q < DEC_PER; q++) {
                    if constexpr (std::is_same<T, uint64_t>::value) d[q] += (uint32_t)__popcll(xv & ss[g + DEC_GROUPS * q][w]);
                    else d[q] += (double)ss[g + DEC_GROUPS * q][w] * (double)xv;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < DEC_PER; q++) {
            const int jl = g + DEC_GROUPS * q;
            if (jl < tile && row_ok) {
                const int j = j0 + jl;
                prod[r][jl] = coef[j] * svc_kval<KERN>((double)d[q], KERN ? svnorm[j] : 0.0, sb, gamma);
            }
        }
        __syncthreads();
        if (tid < DEC_ROWS && row_ok)
            for (int jl = 0; jl < tile; jl++) sum += prod[tid][jl];
        __syncthreads();
    }
    if (tid < DEC_ROWS && row_ok) dec[row0 + tid] = sum - rho;
}

template <typename T> bool svc_all_finite(const T *v, size_t count)
{
    return std::all_of(v, v + count, [](T x) { return std::isfinite(x); });
}

// one pass over a design: every entry finite (x - x is 0 only then); *binary &= every entry 0 or 1.  No early exit: the
// loop has no branch on the data.
bool svc_scan_design(const float *v, size_t count, bool *binary)
{
    unsigned bad = 0, other = 0;
    for (size_t i = 0; i < count; i++) {
        const float x = v[i];
        bad |= !(x - x == 0.0f);
        other |= (x != 0.0f) & (x != 1.0f);
    }
    *binary = *binary && !other;
    return !bad;
}

// rows[count][p] of 0/1 floats -> [count][W] words, column j at bit j & 63 of word j >> 6 (the packing of psk_svc_fit),
// a word at a time
std::vector<uint64_t> svc_pack_rows(const float *X, size_t count, int p, int W)
{
    std::vector<uint64_t> bits(count * W);
    for (size_t i = 0; i < count; i++)
        for (int w = 0; w < W; w++) {
            const float *x = X + i * p + (size_t)w * 64;
            const int nb = std::min(64, p - w * 64);
            uint64_t word = 0;
            for (int b = 0; b < nb; b++) word |= (uint64_t)(x[b] != 0.0f) << b;
            bits[i * W + w] = word;
        }
    return bits;
}

template <typename T, int CH>
int svc_launch_decision(psk_ctx *ctx, const T *X, int m, int W, const T *SV, int n_sv, const double *coef, double rho, int kernel,
                        double gamma, double *dec)
{
    FitArr<double> xnorm, svnorm;
    if (kernel == 1) {
        PSK_HIP(ctx, xnorm.alloc(m));
        PSK_HIP(ctx, svnorm.alloc(n_sv));
        if constexpr (std::is_same<T, uint64_t>::value) {
            svc_norm_bits_kernel<<<div_up(m, 256), 256, 0, ctx->stream>>>(X, m, W, xnorm);
            svc_norm_bits_kernel<<<div_up(n_sv, 256), 256, 0, ctx->stream>>>(SV, n_sv, W, svnorm);
        } else {
            svc_norm_dense_kernel<<<div_up(m, 256), 256, 0, ctx->stream>>>(X, m, W, xnorm);
            svc_norm_dense_kernel<<<div_up(n_sv, 256), 256, 0, ctx->stream>>>(SV, n_sv, W, svnorm);
        }
        PSK_HIP(ctx, hipGetLastError());
    }
    auto kern = kernel == 0 ? svc_decision_kernel<T, CH, 0> : svc_decision_kernel<T, CH, 1>;
    kern<<<div_up(m, DEC_ROWS), DEC_THREADS, 0, ctx->stream>>>(X, m, W, SV, n_sv, xnorm, svnorm, coef, rho, gamma, dec);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the norms are freed on return)
    return PSK_OK;
}

}  // namespace

extern "C" int psk_svc_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                           const double *fit_C, const double *fit_gamma, const int32_t *fit_fold, int n_fits, int kernel,
                           double tol, int max_iter, double *dual_out, double *rho_out, double *dec_out, int32_t *iters_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !fold || !fit_C || !fit_fold || !dual_out || !rho_out || !dec_out)
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (n < 2 || p < 1 || n_fits < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d", n, p, n_fits);
    if (kernel != 0 && kernel != 1) return psk_fail(ctx, PSK_EINVAL, "kernel must be 0 (linear) or 1 (rbf), got %d", kernel);
    if (kernel == 1 && !fit_gamma) return psk_fail(ctx, PSK_EINVAL, "the rbf kernel needs fit_gamma");
    if (!(tol > 0.0) || (max_iter < 1 && max_iter != -1))
        return psk_fail(ctx, PSK_EINVAL, "tol must be > 0 and max_iter >= 1 or -1 (no limit)");
    if (n > SVC_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "psk_svc_fit holds the sample x sample kernel matrix on the device: at most %d samples, got %d",
                        SVC_MAX_N, n);
    for (int f = 0; f < n_fits; f++) {
        if (!(fit_C[f] > 0.0)) return psk_fail(ctx, PSK_EINVAL, "fit %d: C must be > 0", f);
        if (kernel == 1 && !(fit_gamma[f] >= 0.0)) return psk_fail(ctx, PSK_EINVAL, "fit %d: gamma must be >= 0", f);
        int c0 = 0, c1 = 0;
        for (int i = 0; i < n; i++)
            if (fold[i] != fit_fold[f]) { if (y01[i]) c1++; else c0++; }
        if (!c0 || !c1) return psk_fail(ctx, PSK_EINVAL, "fit %d trains on one class only (%d of class 0, %d of class 1)", f, c0, c1);
    }
    const bool binary = design_is_binary(X, (size_t)n * p);

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    SvcArrs b;
    FitArr<uint64_t> xbits;
    FitArr<float> x, Df;   // the kernel matrix of a 0/1 design holds counts: exact in f32
    FitArr<double> Dd;
    const dim3 tiles(div_up(n, SVC_TILE), div_up(n, SVC_TILE));
    PSK_HIP(ctx, b.diag.alloc(n));
    if (binary) {
        const int W = (p + 63) / 64;
        std::vector<uint64_t> bits((size_t)n * W, 0);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < p; j++)
                if (X[(size_t)i * p + j] != 0.0f) bits[(size_t)i * W + (j >> 6)] |= 1ull << (j & 63);
        PSK_HIP(ctx, xbits.upload(bits, ctx->stream));
        PSK_HIP(ctx, Df.alloc((size_t)n * n));
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `bits` leaves scope
        svc_gram_bits_kernel<<<tiles, SVC_TILE * SVC_TILE, 0, ctx->stream>>>(xbits, n, W, Df);
        svc_diag_kernel<float><<<div_up(n, 256), 256, 0, ctx->stream>>>(Df, n, b.diag);
    } else {
        PSK_HIP(ctx, x.upload(X, (size_t)n * p, ctx->stream));
        PSK_HIP(ctx, Dd.alloc((size_t)n * n));
        svc_gram_dense_kernel<<<tiles, SVC_TILE * SVC_TILE, 0, ctx->stream>>>(x, n, p, Dd);
        svc_diag_kernel<double><<<div_up(n, 256), 256, 0, ctx->stream>>>(Dd, n, b.diag);
    }
    PSK_HIP(ctx, hipGetLastError());

    std::vector<double> gam(n_fits, 0.0);
    if (kernel == 1) memcpy(gam.data(), fit_gamma, (size_t)n_fits * 8);
    PSK_HIP(ctx, b.y.upload(y01, n, ctx->stream));
    PSK_HIP(ctx, b.fold.upload(fold, n, ctx->stream));
    PSK_HIP(ctx, b.C.upload(fit_C, n_fits, ctx->stream));
    PSK_HIP(ctx, b.gamma.upload(gam, ctx->stream));
    PSK_HIP(ctx, b.fit_fold.upload(fit_fold, n_fits, ctx->stream));
    PSK_HIP(ctx, b.dual.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, b.rho.alloc(n_fits));
    PSK_HIP(ctx, b.dec.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, b.iters.alloc(n_fits));
    PSK_HIP(ctx, b.dual.zero(ctx->stream));   // samples a fit did not train on
    if (binary) PSK_TRY(svc_launch_smo<float>(ctx, Df, b, n, n_fits, kernel, tol, max_iter));
    else PSK_TRY(svc_launch_smo<double>(ctx, Dd, b, n, n_fits, kernel, tol, max_iter));
    PSK_HIP(ctx, b.dual.download(dual_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, b.rho.download(rho_out, n_fits, ctx->stream));
    PSK_HIP(ctx, b.dec.download(dec_out, (size_t)n_fits * n, ctx->stream));
    if (iters_out) PSK_HIP(ctx, b.iters.download(iters_out, n_fits, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (`gam` must outlive its copy)
    return PSK_OK;
}

extern "C" int psk_svc_decision(psk_ctx *ctx, const float *X, int m, int p, const float *SV, int n_sv, const double *coef, double rho,
                                int kernel, double gamma, double *dec_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !SV || !coef || !dec_out) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (m < 1 || p < 1 || n_sv < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape m=%d p=%d n_sv=%d", m, p, n_sv);
    if (kernel != 0 && kernel != 1) return psk_fail(ctx, PSK_EINVAL, "kernel must be 0 (linear) or 1 (rbf), got %d", kernel);
    if (!std::isfinite(gamma) || gamma < 0.0) return psk_fail(ctx, PSK_EINVAL, "gamma must be finite and >= 0, got %g", gamma);
    if (!std::isfinite(rho) || !svc_all_finite(coef, (size_t)n_sv)) return psk_fail(ctx, PSK_EINVAL, "coef and rho must be finite");
    bool binary = true;
    const bool x_ok = svc_scan_design(X, (size_t)m * p, &binary), sv_ok = svc_scan_design(SV, (size_t)n_sv * p, &binary);
    if (!x_ok || !sv_ok) return psk_fail(ctx, PSK_EINVAL, "X and SV must be finite");

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    FitArr<double> d_coef, d_dec;
    PSK_HIP(ctx, d_coef.upload(coef, n_sv, ctx->stream));
    PSK_HIP(ctx, d_dec.alloc(m));
    if (binary) {
        const int W = (p + 63) / 64;
        const std::vector<uint64_t> xb = svc_pack_rows(X, m, p, W), sb = svc_pack_rows(SV, n_sv, p, W);
        FitArr<uint64_t> d_x, d_sv;
        PSK_HIP(ctx, d_x.upload(xb, ctx->stream));
        PSK_HIP(ctx, d_sv.upload(sb, ctx->stream));
        PSK_TRY((svc_launch_decision<uint64_t, DEC_WORDS>(ctx, d_x, m, W, d_sv, n_sv, d_coef, rho, kernel, gamma, d_dec)));
    } else {
        FitArr<float> d_x, d_sv;
        PSK_HIP(ctx, d_x.upload(X, (size_t)m * p, ctx->stream));
        PSK_HIP(ctx, d_sv.upload(SV, (size_t)n_sv * p, ctx->stream));
        PSK_TRY((svc_launch_decision<float, DEC_COLS>(ctx, d_x, m, p, d_sv, n_sv, d_coef, rho, kernel, gamma, d_dec)));
    }
    PSK_HIP(ctx, d_dec.download(dec_out, m, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}
