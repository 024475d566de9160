// Bernoulli naive-Bayes fits of the reference's `-bc NB` branch: set_model makes BernoulliNB() (modeling.py:1034-1035).  The
// reference itself cannot finish that branch -- get_best_model (:1075-1103) has no NB case, best_model stays None (:623) and
// fit_model (:1216) fails on None.fit --, so the yardstick is scikit-learn 1.7.2's BernoulliNB() with its default parameters,
// fitted directly, no search.  The design is 0/1, so the whole estimator is counting:
//   * psk_nb_fit: per fit and column the training samples of class 0 and of class 1 that carry the k-mer (feature_count_), and
//     the training samples of each class (class_count_): popcounts of  bits[w][j] & train[w] & (~ymask[w] | ymask[w])  added
//     over the words w.  Integers: exact, and no order to state.  The logarithms that turn the counts into feature_log_prob_
//     and class_log_prior_ are taken on the HOST in scikit-learn's own expressions (model_nb.py), where they are bit-equal to
//     scikit-learn's attributes; there is no log in this unit.
//   * psk_nb_jll: the joint log-likelihood of every sample under every model,
//         jll[m][i][c] = ((sum over the columns j that sample i carries of delta[m][c][j]) + class_log_prior[m][c]) + neg_sum[m][c]
//     in f64.  x is 0 or 1, so the dot product is a sum of selected delta values with no multiplication.  THE ORDER OF THAT SUM
//     IS FIXED (model_nb.py and tests/nb_restated.py restate it): lane l of a wave starts from +0.0 and adds the columns l,
//     l + 64, l + 128, ... it finds set, ascending; the 64 lane sums are then combined by the butterfly
//     a_l = a_l + a_(l xor m) for m = 32, 16, 8, 4, 2, 1 (both partners of a pair add the same two numbers, so every lane ends
//     with the same value).  The sum of a sample reads nothing but that sample's bits and the model's delta: it depends neither
//     on the launch shape, nor on the number of models, nor on the samples that share its word.
// Three kernels besides tree_pack_kernel (solver_tree_common.h: the float design as W x p bit words, word-major, W =
// ceil(n / 64), and the label mask): nb_train_kernel makes every fit's training mask, nb_count_kernel counts with one column
// per thread, nb_jll_kernel gives a workgroup one word (64 samples) of one model, 16 samples per wave.
#include <hip/hip_runtime.h>

#include <vector>

#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_host.h"
#include "solver_tree_common.h"

namespace {

constexpr int NB_THREADS = 256;
constexpr int NB_WAVES = NB_THREADS / 64;
constexpr int NB_ROWS = 64 / NB_WAVES;   // samples of a word per wave: 2 x 16 f64 accumulators per lane
// the y dimension of a grid: the words of tree_pack_kernel and nb_train_kernel, the fits, the models
constexpr int NB_MAX_GRID_Y = 65535;
constexpr int NB_MAX_N = NB_MAX_GRID_Y * 64;

// train[fit][w]: bit k = sample 64 w + k exists and is not in the fit's held-out fold (a wave per word)
__global__ __launch_bounds__(64) void nb_train_kernel(const int32_t *__restrict__ fold, const int32_t *__restrict__ fit_fold, int n, int W,
                                                      uint64_t *__restrict__ train)
{
    const int w = blockIdx.x, fit = blockIdx.y, s = w * 64 + (int)threadIdx.x;
    const uint64_t t = __ballot(s < n && fold[min(s, n - 1)] != fit_fold[fit]);
    if (threadIdx.x == 0) train[(size_t)fit * W + w] = t;
}

// feature_count[fit][c][j] and class_count[fit][c].  A thread owns a column: the 64 loads of a wave are one word of 64
// consecutive columns, 512 contiguous bytes.  ymask has no bit past n and neither has train, so ~ymask needs no tail mask.
__global__ __launch_bounds__(NB_THREADS) void nb_count_kernel(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ymask,
                                                              const uint64_t *__restrict__ train, int p, int W,
                                                              int32_t *__restrict__ feature_count, int32_t *__restrict__ class_count)
{
    const int j = blockIdx.x * NB_THREADS + threadIdx.x, fit = blockIdx.y;
    const uint64_t *T = train + (size_t)fit * W;
    if (j < p) {
        int c0 = 0, c1 = 0;
        for (int w = 0; w < W; w++) {
            const uint64_t t = T[w];
            if (!t) continue;   // (uniform: the mask words are the fit's)
            const uint64_t v = bits[tree_bit_at(j, w, p)] & t, y = ymask[w];
            c0 += __popcll(v & ~y);
            c1 += __popcll(v & y);
        }
        feature_count[((size_t)fit * 2 + 0) * p + j] = c0;
        feature_count[((size_t)fit * 2 + 1) * p + j] = c1;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {   // the first wave of the fit's first workgroup: the class counts
        int c0 = 0, c1 = 0;
        for (int w = threadIdx.x; w < W; w += 64) {
            const uint64_t t = T[w], y = ymask[w];
            c0 += __popcll(t & ~y);
            c1 += __popcll(t & y);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            c0 += __shfl_xor(c0, s, 64);
            c1 += __shfl_xor(c1, s, 64);
        }
        if (threadIdx.x == 0) {
            class_count[(size_t)fit * 2 + 0] = c0;
            class_count[(size_t)fit * 2 + 1] = c1;
        }
    }
}

// Workgroup (w, m): the 64 samples of word w under model m; wave v takes the samples 64 w + 16 v .. + 15 and walks the columns
// once for all of them: lane l reads word w of the columns l, l + 64, ... (512 contiguous bytes per wave and step) and both
// delta values of the column, and adds them to the accumulators of the samples whose bit is set.  Per sample that is the
// order stated at the top of this file.
__global__ __launch_bounds__(NB_THREADS) void nb_jll_kernel(const uint64_t *__restrict__ bits, int n, int p,
                                                            const double *__restrict__ delta, const double *__restrict__ class_log_prior,
                                                            const double *__restrict__ neg_sum, double *__restrict__ jll)
{
    const int w = blockIdx.x, m = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = wave * NB_ROWS, s0 = w * 64 + k0;
    if (s0 >= n) return;   // (uniform: a wave without a sample; the kernel has no barrier)
    const double *d0 = delta + (size_t)m * 2 * p, *d1 = d0 + p;
    double a0[NB_ROWS], a1[NB_ROWS];
#pragma unroll
    for (int r = 0; r < NB_ROWS; r++) a0[r] = a1[r] = 0.0;
    for (int j = lane; j < p; j += 64) {
        const uint64_t v = bits[tree_bit_at(j, w, p)] >> k0;
        const double e0 = d0[j], e1 = d1[j];
#pragma unroll
        for (int r = 0; r < NB_ROWS; r++)
            if ((v >> r) & 1ull) { a0[r] += e0; a1[r] += e1; }
    }
    const double prior0 = class_log_prior[(size_t)m * 2], prior1 = class_log_prior[(size_t)m * 2 + 1];
    const double neg0 = neg_sum[(size_t)m * 2], neg1 = neg_sum[(size_t)m * 2 + 1];
#pragma unroll
    for (int r = 0; r < NB_ROWS; r++) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            a0[r] += psk_shfl_xor_f64(a0[r], s);
            a1[r] += psk_shfl_xor_f64(a1[r], s);
        }
        if (lane == r && s0 + r < n) {   // (lane r writes sample r: every lane holds the same sum)
            double *out = jll + ((size_t)m * n + s0 + r) * 2;
            out[0] = (a0[r] + prior0) + neg0;
            out[1] = (a1[r] + prior1) + neg1;
        }
    }
}

int nb_check_shape(psk_ctx *ctx, const char *who, int n, int p, int count, const char *what)
{
    if (n < 1 || p < 1 || count < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d %s=%d", n, p, what, count);
    if (n > NB_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s packs a word of 64 samples per grid row: at most %d samples, got %d", who, NB_MAX_N, n);
    if (count > NB_MAX_GRID_Y) return psk_fail(ctx, PSK_ERANGE, "%s: at most %d %s per call, got %d", who, NB_MAX_GRID_Y, what, count);
    return PSK_OK;
}

}  // namespace

extern "C" int psk_nb_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold, const int32_t *fit_fold,
                          int n_fits, int32_t *feature_count_out, int32_t *class_count_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !fold || !fit_fold || !feature_count_out || !class_count_out) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (const int rc = nb_check_shape(ctx, "psk_nb_fit", n, p, n_fits, "fits")) return rc;
    for (int f = 0; f < n_fits; f++) {
        bool has0 = false, has1 = false;
        for (int i = 0; i < n && !(has0 && has1); i++)
            if (fold[i] != fit_fold[f]) (y01[i] ? has1 : has0) = true;
        if (!(has0 && has1)) return psk_fail(ctx, PSK_EINVAL, "psk_nb_fit: the training samples of fit %d are of one class", f);
    }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    FitArr<uint64_t> bits, ymask, train;
    FitArr<int32_t> d_fold, d_fit_fold, fc, cc;
    if (const int rc = tree_pack_design(ctx, "psk_nb_fit", X, y01, n, p, bits, ymask)) return rc;
    PSK_HIP(ctx, d_fold.upload(fold, n, ctx->stream));
    PSK_HIP(ctx, d_fit_fold.upload(fit_fold, n_fits, ctx->stream));
    PSK_HIP(ctx, train.alloc((size_t)n_fits * W));
    PSK_HIP(ctx, fc.alloc((size_t)n_fits * 2 * p));
    PSK_HIP(ctx, cc.alloc((size_t)n_fits * 2));
    nb_train_kernel<<<dim3(W, n_fits), 64, 0, ctx->stream>>>(d_fold, d_fit_fold, n, W, train);
    PSK_HIP(ctx, hipGetLastError());
    nb_count_kernel<<<dim3(div_up(p, NB_THREADS), n_fits), NB_THREADS, 0, ctx->stream>>>(bits, ymask, train, p, W, fc, cc);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, fc.download(feature_count_out, (size_t)n_fits * 2 * p, ctx->stream));
    PSK_HIP(ctx, cc.download(class_count_out, (size_t)n_fits * 2, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

extern "C" int psk_nb_jll(psk_ctx *ctx, const float *X, int n, int p, const double *delta, int n_models, const double *class_log_prior,
                          const double *neg_sum, double *jll_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !delta || !class_log_prior || !neg_sum || !jll_out) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (const int rc = nb_check_shape(ctx, "psk_nb_jll", n, p, n_models, "models")) return rc;

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    FitArr<uint64_t> bits, ymask;
    FitArr<double> d_delta, d_prior, d_neg, d_jll;
    const std::vector<int32_t> no_labels((size_t)n, 0);   // (the packing kernel takes labels; nothing reads their mask here)
    if (const int rc = tree_pack_design(ctx, "psk_nb_jll", X, no_labels.data(), n, p, bits, ymask)) return rc;
    PSK_HIP(ctx, d_delta.upload(delta, (size_t)n_models * 2 * p, ctx->stream));
    PSK_HIP(ctx, d_prior.upload(class_log_prior, (size_t)n_models * 2, ctx->stream));
    PSK_HIP(ctx, d_neg.upload(neg_sum, (size_t)n_models * 2, ctx->stream));
    PSK_HIP(ctx, d_jll.alloc((size_t)n_models * n * 2));
    nb_jll_kernel<<<dim3(W, n_models), NB_THREADS, 0, ctx->stream>>>(bits, n, p, d_delta, d_prior, d_neg, d_jll);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, d_jll.download(jll_out, (size_t)n_models * n * 2, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}
