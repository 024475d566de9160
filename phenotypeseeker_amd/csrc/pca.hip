// Principal components of the selected k-mers: the reference's `--pca` branch (modeling.py:1147-1206, prediction.py:131-163)
// runs StandardScaler().fit/transform and PCA().fit/transform on the k-mer columns.  The reference itself cannot finish that
// branch -- PCA_analysis calls self.t_test (:1184), which does not exist --, so the yardstick is scikit-learn 1.7.2's
// StandardScaler() and PCA() with their defaults.  Everything is f64; -ffp-contract=off holds here too.
//   * psk_pca_fit: column moments; the standardised design Z; the Gram matrix G = Z Z' (n x n, f64 MFMA, split over the
//     columns into partial tiles that are added in a fixed order); a one-sided Jacobi (Hestenes) eigen-solver on G (below); the leading components S^-1 U' Z (f64 MFMA); the sign rule; the scores U S.
//   * psk_pca_transform: scores[i][c] = sum_j ((X[i][j] - center[j]) / scale[j]) * components[c][j], in a stated order
//     (include/psk.h, f11; model_pca.py and tests/pca_restated.py restate it).  This product is NOT on the matrix unit: its
//     contract is a result that NumPy reproduces bit for bit, which an order of separate multiplications and additions gives
//     and a fused multiply-add chain does not.
// The eigen-solver: W = G and V = I as rows; a rotation of the rows (a, b) makes w_a . w_b = 0 and is applied to V as well; when
// all rows of W are orthogonal, w_r = lambda_r v_r.  The n (n - 1) / 2 pairs of a sweep come in m - 1 rounds of m / 2 disjoint
// pairs (m = n rounded up to even; the circle method).  While W and V fit the LDS of one workgroup (n <= PCA_LDS_N) the whole
// solver is one launch of one workgroup, a wave per pair and a barrier of the workgroup per round; beyond that a round is one
// launch with a workgroup per pair, and a round boundary is a kernel boundary.  Rotations are counted with an integer atomic; a
// sweep without one ends the solver; PCA_MAX_SWEEPS caps it.  Every floating-point sum has a fixed order (which of the two
// forms runs is a function of n alone), so two calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_host.h"

namespace {

constexpr int PCA_MAX_N = 4096;
constexpr int PCA_THREADS = 256;
constexpr int PCA_WAVES = PCA_THREADS / 64;
constexpr int PCA_NPT = PCA_MAX_N / PCA_THREADS;   // elements of a row per thread of a rotation
constexpr int PCA_MAX_SWEEPS = 60;
constexpr int PCA_LDS_N = 96;                      // W and V of 2 x 96 x 96 doubles: 144 of the 160 KiB of a workgroup's LDS
constexpr int PCA_LDS_THREADS = 1024;
constexpr int PCA_TILE = 16;                       // v_mfma_f64_16x16x4_f64
constexpr int PCA_CB = 8;                          // components per wave of the transform
constexpr int PCA_MAX_GRID_YZ = 65535;

typedef double pca_f64x4 __attribute__((ext_vector_type(4)));

inline int pad16(int v) { return (v + PCA_TILE - 1) / PCA_TILE * PCA_TILE; }

// mean[j] = (sum_i X[i][j]) / n and var[j] = (sum_i (X[i][j] - mean[j])^2) / n, both sums over i ascending; a thread owns a
// column, so a wave reads 256 contiguous bytes of a row.  A non-finite entry raises *bad.
__global__ __launch_bounds__(PCA_THREADS) void pca_moments_kernel(const float *__restrict__ X, int n, int p, double *__restrict__ mean,
                                                                  double *__restrict__ var, int *__restrict__ bad)
{
    const int j = blockIdx.x * PCA_THREADS + threadIdx.x;
    if (j >= p) return;
    double s = 0.0;
    bool finite = true;
    for (int i = 0; i < n; i++) {
        const float v = X[(size_t)i * p + j];
        finite = finite && isfinite(v);
        s += (double)v;
    }
    if (!finite) atomicOr(bad, 1);
    const double mu = s / (double)n;
    double q = 0.0;
    for (int i = 0; i < n; i++) {
        const double d = (double)X[(size_t)i * p + j] - mu;
        q += d * d;
    }
    mean[j] = mu;
    var[j] = q / (double)n;
}

// Z[n_pad][p_pad] = (X - mean) / scale, zero in the padding (so the matrix products need no bounds)
__global__ __launch_bounds__(PCA_THREADS) void pca_standardise_kernel(const float *__restrict__ X, int n, int p, int p_pad,
                                                                      const double *__restrict__ mean, const double *__restrict__ scale,
                                                                      double *__restrict__ Z)
{
    const int j = blockIdx.x * PCA_THREADS + threadIdx.x, i = blockIdx.y;
    if (j >= p_pad) return;
    Z[(size_t)i * p_pad + j] = (i < n && j < p) ? ((double)X[(size_t)i * p + j] - mean[j]) / scale[j] : 0.0;
}

// One wave: the 16 x 16 tile (ti, tk), tk <= ti, of Z Z' over the column blocks [s chunk, (s + 1) chunk) of 16 columns.
// v_mfma_f64_16x16x4_f64: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and receives
// D[row = (l >> 4) + 4 reg][col = l & 15].  A lane reads four consecutive columns of its row (32 bytes) and feeds them to four
// instructions: within one instruction the four k of the four lane groups are the columns 4 q + e, the same for A and B.
__global__ __launch_bounds__(64) void pca_gram_kernel(const double *__restrict__ Z, int n_pad, int p_pad, int kblocks, int chunk,
                                                      double *__restrict__ P)
{
    const int ti = blockIdx.x, tk = blockIdx.y, s = blockIdx.z;
    if (tk > ti) return;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const double *a = Z + (size_t)(ti * PCA_TILE + r) * p_pad + 4 * q;
    const double *b = Z + (size_t)(tk * PCA_TILE + r) * p_pad + 4 * q;
    pca_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    const int kb1 = min(kblocks, (s + 1) * chunk);
    for (int kb = s * chunk; kb < kb1; kb++) {
        const double *pa = a + (size_t)kb * PCA_TILE, *pb = b + (size_t)kb * PCA_TILE;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2], a3 = pa[3];
        const double b0 = pb[0], b1 = pb[1], b2 = pb[2], b3 = pb[3];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b3, acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++)
        P[((size_t)s * n_pad + ti * PCA_TILE + q + 4 * reg) * n_pad + tk * PCA_TILE + r] = acc[reg];
}

// W[i][k] = sum over the splits s ascending of P[s][max(i, k)][min(i, k)]: the Gram matrix, exactly symmetric; V = I
__global__ __launch_bounds__(PCA_THREADS) void pca_gram_sum_kernel(const double *__restrict__ P, int n, int n_pad, int splits,
                                                                   double *__restrict__ W, double *__restrict__ V)
{
    const int k = blockIdx.x * PCA_THREADS + threadIdx.x, i = blockIdx.y;
    if (k >= n) return;
    const int hi = max(i, k), lo = min(i, k);
    double g = 0.0;
    for (int s = 0; s < splits; s++) g += P[((size_t)s * n_pad + hi) * n_pad + lo];
    W[(size_t)i * n + k] = g;
    V[(size_t)i * n + k] = i == k ? 1.0 : 0.0;
}

// The pair of round `round` that workgroup (or wave) k takes; false when one of its players does not exist (n odd).
__device__ __forceinline__ bool pca_pair(int k, int round, int n, int m, int &ra, int &rb)
{
    if (k == 0) {
        ra = round;
        rb = m - 1;
    } else {
        ra = (round + k) % (m - 1);
        rb = (round - k + (m - 1)) % (m - 1);
    }
    if (ra >= n || rb >= n) return false;
    if (ra > rb) {
        const int t = ra;
        ra = rb;
        rb = t;
    }
    return true;
}

// Sums of three values over the workgroup, the same in every thread: per wave the butterfly xor 32 .. 1, then the four wave
// sums in ascending order.  lds: 3 x PCA_WAVES doubles.
__device__ __forceinline__ void pca_block_sum3(double &a, double &b, double &c, double *lds)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        a += psk_shfl_xor_f64(a, s);
        b += psk_shfl_xor_f64(b, s);
        c += psk_shfl_xor_f64(c, s);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds[wave] = a;
        lds[PCA_WAVES + wave] = b;
        lds[2 * PCA_WAVES + wave] = c;
    }
    __syncthreads();
    a = b = c = 0.0;
#pragma unroll
    for (int w = 0; w < PCA_WAVES; w++) {
        a += lds[w];
        b += lds[PCA_WAVES + w];
        c += lds[2 * PCA_WAVES + w];
    }
    __syncthreads();
}

// Round `round` of a sweep: workgroup k takes the pair k of the circle method over m players (m even, player m - 1 fixed);
// a player >= n does not exist (n odd).  Thread t holds the elements t, t + 256, ... of both rows.  The pair is left alone when
// it is orthogonal to `tol` relative to the two norms, or when one of the rows is below `null_norm2` (squared): such a row lies
// in the numerical null space of G, below the rank floor of psk_pca_fit, and its component is written as zeros.
__global__ __launch_bounds__(PCA_THREADS) void pca_round_kernel(double *__restrict__ W, double *__restrict__ V, int n, int m, int round,
                                                                double tol, double null_norm2, int *__restrict__ rotations)
{
    __shared__ double lds[3 * PCA_WAVES];
    int ra, rb;
    if (!pca_pair(blockIdx.x, round, n, m, ra, rb)) return;   // (uniform over the workgroup)
    double *wa = W + (size_t)ra * n, *wb = W + (size_t)rb * n;
    double xa[PCA_NPT], xb[PCA_NPT];
    double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
    for (int e = 0; e < PCA_NPT; e++) {
        const int i = threadIdx.x + e * PCA_THREADS;
        xa[e] = i < n ? wa[i] : 0.0;
        xb[e] = i < n ? wb[i] : 0.0;
        a += xa[e] * xa[e];
        b += xb[e] * xb[e];
        c += xa[e] * xb[e];
    }
    pca_block_sum3(a, b, c, lds);
    if (a <= null_norm2 || b <= null_norm2 || !(fabs(c) > tol * (sqrt(a) * sqrt(b)))) return;   // (uniform)
    const double zeta = (b - a) / (2.0 * c);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
    for (int e = 0; e < PCA_NPT; e++) {
        const int i = threadIdx.x + e * PCA_THREADS;
        if (i < n) {
            wa[i] = cs * xa[e] - sn * xb[e];
            wb[i] = sn * xa[e] + cs * xb[e];
        }
    }
    double *va = V + (size_t)ra * n, *vb = V + (size_t)rb * n;
    for (int i = threadIdx.x; i < n; i += PCA_THREADS) {
        const double ya = va[i], yb = vb[i];
        va[i] = cs * ya - sn * yb;
        vb[i] = sn * ya + cs * yb;
    }
    if (threadIdx.x == 0) atomicAdd(rotations, 1);
}

// The whole solver in one workgroup for n <= PCA_LDS_N: W and V live in LDS (n x n doubles each), wave w takes the pairs w,
// w + 16, ... of a round, lane l the elements l, l + 64 of the two rows; the three sums are the lanes' partial sums under the
// butterfly xor 32 .. 1.  The pairs of a round share no row, so the waves need no order within a round; __syncthreads() ends
// it.  out[0] = sweeps taken, out[1] = rotations of the last sweep (0: converged; else the cap was reached).
__global__ __launch_bounds__(PCA_LDS_THREADS) void pca_jacobi_lds_kernel(double *__restrict__ Wg, double *__restrict__ Vg, int n, int m,
                                                                         double tol, double null_norm2, int max_sweeps,
                                                                         int32_t *__restrict__ out)
{
    extern __shared__ double pca_lds[];
    __shared__ int rot;
    double *W = pca_lds, *V = pca_lds + n * n;
    for (int e = threadIdx.x; e < n * n; e += PCA_LDS_THREADS) {
        W[e] = Wg[e];
        V[e] = Vg[e];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sweeps = 0, last = 0;
    __syncthreads();
    while (sweeps < max_sweeps) {
        if (threadIdx.x == 0) rot = 0;
        __syncthreads();
        for (int round = 0; round < m - 1; round++) {
            for (int k = wave; k < m / 2; k += PCA_LDS_THREADS / 64) {
                int ra, rb;
                if (!pca_pair(k, round, n, m, ra, rb)) continue;   // (uniform over the wave, as everything below)
                double *wa = W + ra * n, *wb = W + rb * n, *va = V + ra * n, *vb = V + rb * n;
                double a = 0.0, b = 0.0, c = 0.0;
                for (int i = lane; i < n; i += 64) {
                    a += wa[i] * wa[i];
                    b += wb[i] * wb[i];
                    c += wa[i] * wb[i];
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    a += psk_shfl_xor_f64(a, s);
                    b += psk_shfl_xor_f64(b, s);
                    c += psk_shfl_xor_f64(c, s);
                }
                if (a <= null_norm2 || b <= null_norm2 || !(fabs(c) > tol * (sqrt(a) * sqrt(b)))) continue;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int i = lane; i < n; i += 64) {
                    const double xa = wa[i], xb = wb[i], ya = va[i], yb = vb[i];
                    wa[i] = cs * xa - sn * xb;
                    wb[i] = sn * xa + cs * xb;
                    va[i] = cs * ya - sn * yb;
                    vb[i] = sn * ya + cs * yb;
                }
                if (lane == 0) atomicAdd(&rot, 1);
            }
            __syncthreads();
        }
        last = rot;          // (after the barrier of the last round: the same in every thread)
        sweeps++;
        __syncthreads();     // every thread has read the count before thread 0 clears it
        if (last == 0) break;
    }
    for (int e = threadIdx.x; e < n * n; e += PCA_LDS_THREADS) {
        Wg[e] = W[e];
        Vg[e] = V[e];
    }
    if (threadIdx.x == 0) {
        out[0] = sweeps;
        out[1] = last;
    }
}

// lambda[r] = v_r . w_r (the Rayleigh quotient of a unit vector: w_r = G v_r), a workgroup per row
__global__ __launch_bounds__(PCA_THREADS) void pca_lambda_kernel(const double *__restrict__ W, const double *__restrict__ V, int n,
                                                                 double *__restrict__ lambda)
{
    __shared__ double lds[3 * PCA_WAVES];
    const int r = blockIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += PCA_THREADS) a += V[(size_t)r * n + i] * W[(size_t)r * n + i];
    pca_block_sum3(a, b, c, lds);
    if (threadIdx.x == 0) lambda[r] = a;
}

// U'[nc_pad][n_pad]: row c = the eigenvector order[c], zero in the padding
__global__ __launch_bounds__(PCA_THREADS) void pca_gather_kernel(const double *__restrict__ V, const int32_t *__restrict__ order, int n,
                                                                 int n_comp, int n_pad, double *__restrict__ UT)
{
    const int i = blockIdx.x * PCA_THREADS + threadIdx.x, c = blockIdx.y;
    if (i >= n_pad) return;
    UT[(size_t)c * n_pad + i] = (c < n_comp && i < n) ? V[(size_t)order[c] * n + i] : 0.0;
}

// One wave: the 16 x 16 tile (components tc, columns tj) of U' Z, divided by the singular value; a component below the rank
// floor (sv = 0) is written as zeros.  Operand layout as in pca_gram_kernel; here B[k][j] = Z[k][j] is read along a row of Z.
__global__ __launch_bounds__(64) void pca_components_kernel(const double *__restrict__ UT, const double *__restrict__ Z, int n_pad,
                                                            int p_pad, const double *__restrict__ sv, int n_comp, int p,
                                                            double *__restrict__ comp)
{
    const int tj = blockIdx.x, tc = blockIdx.y, lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const double *a = UT + (size_t)(tc * PCA_TILE + r) * n_pad + 4 * q;
    const double *b = Z + (size_t)(4 * q) * p_pad + tj * PCA_TILE + r;
    pca_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < n_pad / PCA_TILE; kb++) {
        const double *pa = a + (size_t)kb * PCA_TILE, *pb = b + (size_t)kb * PCA_TILE * p_pad;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2], a3 = pa[3];
        const double b0 = pb[0], b1 = pb[p_pad], b2 = pb[2 * (size_t)p_pad], b3 = pb[3 * (size_t)p_pad];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b3, acc, 0, 0, 0);
    }
    const int j = tj * PCA_TILE + r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int c = tc * PCA_TILE + q + 4 * reg;
        if (c < n_comp && j < p) comp[(size_t)c * p + j] = sv[c] > 0.0 ? acc[reg] / sv[c] : 0.0;
    }
}

// The sign rule, a workgroup per component: the entry of largest magnitude of the row becomes positive, the lowest column
// among equal magnitudes deciding; sign[c] = -1 when the row was negated.
__global__ __launch_bounds__(PCA_THREADS) void pca_sign_kernel(double *__restrict__ comp, int p, double *__restrict__ sign)
{
    __shared__ double best_v[PCA_THREADS];
    __shared__ int best_j[PCA_THREADS];
    double *row = comp + (size_t)blockIdx.x * p;
    double bv = -1.0;
    int bj = 0;
    for (int j = threadIdx.x; j < p; j += PCA_THREADS) {   // (ascending: a later equal magnitude does not replace)
        const double v = fabs(row[j]);
        if (v > bv) {
            bv = v;
            bj = j;
        }
    }
    best_v[threadIdx.x] = bv;
    best_j[threadIdx.x] = bj;
    __syncthreads();
    for (int s = PCA_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = best_v[threadIdx.x + s];
            const int oj = best_j[threadIdx.x + s];
            if (ov > best_v[threadIdx.x] || (ov == best_v[threadIdx.x] && oj < best_j[threadIdx.x])) {
                best_v[threadIdx.x] = ov;
                best_j[threadIdx.x] = oj;
            }
        }
        __syncthreads();
    }
    const bool flip = row[best_j[0]] < 0.0;
    __syncthreads();   // (every thread has read the deciding entry before it changes)
    if (flip)
        for (int j = threadIdx.x; j < p; j += PCA_THREADS) row[j] = -row[j];
    if (threadIdx.x == 0) sign[blockIdx.x] = flip ? -1.0 : 1.0;
}

// scores[i][c] = sign[c] * (U'[c][i] * sv[c])
__global__ __launch_bounds__(PCA_THREADS) void pca_scores_kernel(const double *__restrict__ UT, int n_pad, const double *__restrict__ sv,
                                                                 const double *__restrict__ sign, int n, int n_comp,
                                                                 double *__restrict__ scores)
{
    const int c = blockIdx.x * PCA_THREADS + threadIdx.x, i = blockIdx.y;
    if (c >= n_comp) return;
    scores[(size_t)i * n_comp + c] = sign[c] * (UT[(size_t)c * n_pad + i] * sv[c]);
}

// One wave: row i under the components c0 .. c0 + PCA_CB - 1, in the order stated in include/psk.h: lane l starts from +0.0
// and adds z_j * components[c][j] for j = l, l + 64, ... ascending (a product, then a sum: no fused operation), then the
// butterfly.  z_j = (X[i][j] - center[j]) / scale[j] is formed once per column for the PCA_CB components.
__global__ __launch_bounds__(64) void pca_transform_kernel(const float *__restrict__ X, int p, const double *__restrict__ center,
                                                           const double *__restrict__ scale, const double *__restrict__ comp, int k,
                                                           double *__restrict__ scores)
{
    const size_t i = blockIdx.x;
    const int c0 = blockIdx.y * PCA_CB, lane = threadIdx.x;
    double acc[PCA_CB];
#pragma unroll
    for (int e = 0; e < PCA_CB; e++) acc[e] = 0.0;
    for (int j = lane; j < p; j += 64) {
        const double z = ((double)X[i * p + j] - center[j]) / scale[j];
#pragma unroll
        for (int e = 0; e < PCA_CB; e++)
            if (c0 + e < k) acc[e] += z * comp[(size_t)(c0 + e) * p + j];
    }
#pragma unroll
    for (int e = 0; e < PCA_CB; e++) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) acc[e] += psk_shfl_xor_f64(acc[e], s);
        if (lane == e && c0 + e < k) scores[i * k + c0 + e] = acc[e];   // (every lane holds the same sum)
    }
}

}  // namespace

extern "C" int psk_pca_fit(psk_ctx *ctx, const float *X, int n, int p, int n_comp, double *mean_out, double *var_out, double *scale_out,
                           double *lambda_out, double *scores_out, double *components_out, int32_t *sweeps_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !mean_out || !var_out || !scale_out || !lambda_out || !scores_out || !components_out)
        return psk_fail(ctx, PSK_EINVAL, "psk_pca_fit: null buffer");
    if (n < 2) return psk_fail(ctx, PSK_EINVAL, "psk_pca_fit: n must be at least 2 samples, got n=%d", n);
    if (n > PCA_MAX_N) return psk_fail(ctx, PSK_ERANGE, "psk_pca_fit: n must be at most %d samples, got n=%d", PCA_MAX_N, n);
    if (p < 1) return psk_fail(ctx, PSK_EINVAL, "psk_pca_fit: p must be at least 1 column, got p=%d", p);
    const int rank_max = std::min(n, p);
    if (n_comp < 1 || n_comp > rank_max)
        return psk_fail(ctx, PSK_EINVAL, "psk_pca_fit: n_comp must be 1..min(n, p) = %d, got n_comp=%d", rank_max, n_comp);

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n_pad = pad16(n), p_pad = pad16(p), nc_pad = pad16(n_comp);
    FitArr<float> d_X;
    FitArr<double> d_mean, d_var, d_scale, Z;
    FitArr<int32_t> d_flag;
    PSK_HIP(ctx, d_X.upload(X, (size_t)n * p, st));
    PSK_HIP(ctx, d_mean.alloc(p));
    PSK_HIP(ctx, d_var.alloc(p));
    PSK_HIP(ctx, d_flag.alloc(1));
    PSK_HIP(ctx, d_flag.zero(st));
    pca_moments_kernel<<<div_up(p, PCA_THREADS), PCA_THREADS, 0, st>>>(d_X, n, p, d_mean, d_var, d_flag);
    PSK_HIP(ctx, hipGetLastError());
    int32_t bad = 0;
    PSK_HIP(ctx, d_mean.download(mean_out, p, st));
    PSK_HIP(ctx, d_var.download(var_out, p, st));
    PSK_HIP(ctx, d_flag.download(&bad, 1, st));
    PSK_HIP(ctx, hipStreamSynchronize(st));
    if (bad) return psk_fail(ctx, PSK_EINVAL, "psk_pca_fit: X has an entry that is not finite");
    // the square root is the host's (correctly rounded, as numpy's); a constant column divides by 1 (StandardScaler)
    int64_t varying = 0;
    for (int j = 0; j < p; j++) {
        scale_out[j] = var_out[j] == 0.0 ? 1.0 : std::sqrt(var_out[j]);
        varying += var_out[j] != 0.0;
    }
    PSK_HIP(ctx, d_scale.upload(scale_out, p, st));
    PSK_HIP(ctx, Z.alloc((size_t)n_pad * p_pad));
    pca_standardise_kernel<<<dim3(div_up(p_pad, PCA_THREADS), n_pad), PCA_THREADS, 0, st>>>(d_X, n, p, p_pad, d_mean, d_scale, Z);
    PSK_HIP(ctx, hipGetLastError());

    // the Gram matrix: as many splits of the column blocks as give about 1,024 waves, a function of (n, p) alone
    const int T = n_pad / PCA_TILE, kblocks = p_pad / PCA_TILE;
    const int tiles = T * (T + 1) / 2;
    int splits = std::max(1, std::min(std::min(kblocks, PCA_MAX_GRID_YZ), 1024 / tiles));
    const int chunk = (kblocks + splits - 1) / splits;
    splits = (kblocks + chunk - 1) / chunk;
    FitArr<double> P, W, V, d_lambda;
    FitArr<int32_t> d_rot;
    PSK_HIP(ctx, P.alloc((size_t)splits * n_pad * n_pad));
    PSK_HIP(ctx, W.alloc((size_t)n * n));
    PSK_HIP(ctx, V.alloc((size_t)n * n));
    PSK_HIP(ctx, d_lambda.alloc(n));
    PSK_HIP(ctx, d_rot.alloc(1));
    pca_gram_kernel<<<dim3(T, T, splits), 64, 0, st>>>(Z, n_pad, p_pad, kblocks, chunk, P);
    PSK_HIP(ctx, hipGetLastError());
    pca_gram_sum_kernel<<<dim3(div_up(n, PCA_THREADS), n), PCA_THREADS, 0, st>>>(P, n, n_pad, splits, W, V);
    PSK_HIP(ctx, hipGetLastError());

    // trace(G) = sum of the squared entries of Z = n per varying column; a row of W whose norm is below 2^-52 trace(G) <=
    // n 2^-52 lambda_1 lies under the rank floor
    const double trace = (double)n * (double)varying;
    const double null_norm = std::ldexp(trace, -52), tol = std::sqrt((double)n) * std::ldexp(1.0, -52);
    const int m = (n + 1) & ~1;
    int sweeps = 0;
    int32_t rotations = 0;
    if (n <= PCA_LDS_N) {
        const size_t lds = 2 * (size_t)n * n * sizeof(double);
        static PerDeviceOnce attr_set;
        if (attr_set.first(ctx->device))
            PSK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(pca_jacobi_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(2 * (size_t)PCA_LDS_N * PCA_LDS_N * sizeof(double))));
        FitArr<int32_t> d_out;
        int32_t out[2] = {0, 0};
        PSK_HIP(ctx, d_out.alloc(2));
        pca_jacobi_lds_kernel<<<1, PCA_LDS_THREADS, lds, st>>>(W, V, n, m, tol, null_norm * null_norm, PCA_MAX_SWEEPS, d_out);
        PSK_HIP(ctx, hipGetLastError());
        PSK_HIP(ctx, d_out.download(out, 2, st));
        PSK_HIP(ctx, hipStreamSynchronize(st));
        sweeps = out[0];
        rotations = out[1];
    } else {
        do {
            PSK_HIP(ctx, d_rot.zero(st));
            for (int round = 0; round < m - 1; round++)
                pca_round_kernel<<<m / 2, PCA_THREADS, 0, st>>>(W, V, n, m, round, tol, null_norm * null_norm, d_rot);
            PSK_HIP(ctx, hipGetLastError());
            PSK_HIP(ctx, d_rot.download(&rotations, 1, st));
            PSK_HIP(ctx, hipStreamSynchronize(st));
            sweeps++;
        } while (rotations != 0 && sweeps < PCA_MAX_SWEEPS);
    }
    if (rotations != 0)
        return psk_fail(ctx, PSK_ESTATE, "psk_pca_fit: the Jacobi eigen-solver has not converged after %d sweeps (n=%d p=%d)",
                        PCA_MAX_SWEEPS, n, p);
    if (sweeps_out) *sweeps_out = sweeps;
    pca_lambda_kernel<<<n, PCA_THREADS, 0, st>>>(W, V, n, d_lambda);
    PSK_HIP(ctx, hipGetLastError());
    std::vector<double> lam(n);
    PSK_HIP(ctx, d_lambda.download(lam.data(), n, st));
    PSK_HIP(ctx, hipStreamSynchronize(st));

    // descending, the lower row first among equals; clamped at 0; the rank floor of numpy.linalg.matrix_rank
    std::vector<int32_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return lam[x] > lam[y]; });
    const double lam1 = std::max(lam[order[0]], 0.0);
    const double floor_ = (double)std::max(n, p) * std::ldexp(1.0, -52) * lam1;
    for (int c = 0; c < rank_max; c++) lambda_out[c] = std::max(lam[order[c]], 0.0);
    std::vector<double> sv(nc_pad, 0.0);
    for (int c = 0; c < n_comp; c++) sv[c] = lambda_out[c] > floor_ ? std::sqrt(lambda_out[c]) : 0.0;

    FitArr<int32_t> d_order;
    FitArr<double> UT, d_sv, d_sign, d_comp, d_scores;
    PSK_HIP(ctx, d_order.upload(order.data(), n, st));
    PSK_HIP(ctx, d_sv.upload(sv, st));
    PSK_HIP(ctx, UT.alloc((size_t)nc_pad * n_pad));
    PSK_HIP(ctx, d_sign.alloc(n_comp));
    PSK_HIP(ctx, d_comp.alloc((size_t)n_comp * p));
    PSK_HIP(ctx, d_scores.alloc((size_t)n * n_comp));
    pca_gather_kernel<<<dim3(div_up(n_pad, PCA_THREADS), nc_pad), PCA_THREADS, 0, st>>>(V, d_order, n, n_comp, n_pad, UT);
    PSK_HIP(ctx, hipGetLastError());
    pca_components_kernel<<<dim3(p_pad / PCA_TILE, nc_pad / PCA_TILE), 64, 0, st>>>(UT, Z, n_pad, p_pad, d_sv, n_comp, p, d_comp);
    PSK_HIP(ctx, hipGetLastError());
    pca_sign_kernel<<<n_comp, PCA_THREADS, 0, st>>>(d_comp, p, d_sign);
    PSK_HIP(ctx, hipGetLastError());
    pca_scores_kernel<<<dim3(div_up(n_comp, PCA_THREADS), n), PCA_THREADS, 0, st>>>(UT, n_pad, d_sv, d_sign, n, n_comp, d_scores);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, d_comp.download(components_out, (size_t)n_comp * p, st));
    PSK_HIP(ctx, d_scores.download(scores_out, (size_t)n * n_comp, st));
    PSK_HIP(ctx, hipStreamSynchronize(st));
    return PSK_OK;
}

extern "C" int psk_pca_transform(psk_ctx *ctx, const float *X, int m, int p, const double *center, const double *scale,
                                 const double *components, int k, double *scores_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !center || !scale || !components || !scores_out) return psk_fail(ctx, PSK_EINVAL, "psk_pca_transform: null buffer");
    if (m < 1 || p < 1 || k < 1) return psk_fail(ctx, PSK_EINVAL, "psk_pca_transform: bad problem shape m=%d p=%d k=%d", m, p, k);
    if (div_up(k, PCA_CB) > (unsigned)PCA_MAX_GRID_YZ)
        return psk_fail(ctx, PSK_ERANGE, "psk_pca_transform: at most %d components per call, got k=%d", PCA_MAX_GRID_YZ * PCA_CB, k);

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    FitArr<float> d_X;
    FitArr<double> d_center, d_scale, d_comp, d_scores;
    PSK_HIP(ctx, d_X.upload(X, (size_t)m * p, ctx->stream));
    PSK_HIP(ctx, d_center.upload(center, p, ctx->stream));
    PSK_HIP(ctx, d_scale.upload(scale, p, ctx->stream));
    PSK_HIP(ctx, d_comp.upload(components, (size_t)k * p, ctx->stream));
    PSK_HIP(ctx, d_scores.alloc((size_t)m * k));
    pca_transform_kernel<<<dim3(m, div_up(k, PCA_CB)), 64, 0, ctx->stream>>>(d_X, p, d_center, d_scale, d_comp, k, d_scores);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, d_scores.download(scores_out, (size_t)m * k, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}
