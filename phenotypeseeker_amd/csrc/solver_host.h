// Host side of the solver entry points (solver.hip, solver_l2.hip, solver_svc.hip, solver_tree.hip, solver_forest.hip,
// solver_nb.hip): an owned, typed device
// array; the argument check and the input / result block of the four linear-model fits; the host packings of the design.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "psk_internal.h"

namespace {

// One hipMalloc of `count` elements of T, freed with the object.  Converts to T * (and so to const T *): a launch site
// passes the array itself and the compiler checks the element type.
template <class T> class FitArr {
    T *ptr_ = nullptr;
    size_t count_ = 0;

  public:
    FitArr() = default;
    FitArr(const FitArr &) = delete;
    FitArr &operator=(const FitArr &) = delete;
    ~FitArr() { if (ptr_) (void)hipFree(ptr_); }
    operator T *() const { return ptr_; }
    hipError_t alloc(size_t count)
    {
        if (ptr_) return hipErrorInvalidValue;   // one allocation per array
        count_ = count;
        return hipMalloc(&ptr_, count ? count * sizeof(T) : 8);
    }
    hipError_t upload(const T *src, size_t count, hipStream_t stream)
    {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemcpyAsync(ptr_, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    hipError_t upload(const std::vector<T> &src, hipStream_t stream) { return upload(src.data(), src.size(), stream); }
    hipError_t download(T *dst, size_t count, hipStream_t s) const { return hipMemcpyAsync(dst, ptr_, count * sizeof(T), hipMemcpyDeviceToHost, s); }
    hipError_t zero(hipStream_t stream) { return hipMemsetAsync(ptr_, 0, count_ * sizeof(T), stream); }
};

// the arguments that psk_logreg_l1_fit, psk_lasso_fit, psk_ridge_fit and psk_logreg_l2_fit share
struct FitArgs {
    const float *X;
    int n, p;
    const int32_t *fold;
    const double *fit_param;
    const int32_t *fit_fold;
    int n_fits;
    double *coef_out, *icpt_out;
    int32_t *iters_out;
};

inline int check_fit_args(psk_ctx *ctx, const FitArgs &a, const void *y)
{
    if (!ctx) return PSK_EINVAL;
    if (!a.X || !y || !a.fold || !a.fit_param || !a.fit_fold || !a.coef_out || !a.icpt_out)
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (a.n < 2 || a.p < 1 || a.n_fits < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d", a.n, a.p, a.n_fits);
    return PSK_OK;
}

// the device side of FitArgs: fold of every sample, parameter and held-out fold of every fit (in); coefficients, intercept
// and iteration count of every fit (out)
struct FitIO {
    FitArr<int32_t> fold, fit_fold, iters;
    FitArr<double> fit_param, coef, icpt;

    // copies the inputs in and allocates the outputs; `folds` = false leaves both fold arrays out (a form that reads neither)
    int upload(psk_ctx *ctx, const FitArgs &a, bool folds = true)
    {
        if (folds) PSK_HIP(ctx, fold.upload(a.fold, a.n, ctx->stream));
        if (folds) PSK_HIP(ctx, fit_fold.upload(a.fit_fold, a.n_fits, ctx->stream));
        PSK_HIP(ctx, fit_param.upload(a.fit_param, a.n_fits, ctx->stream));
        PSK_HIP(ctx, coef.alloc((size_t)a.n_fits * a.p));
        PSK_HIP(ctx, icpt.alloc(a.n_fits));
        PSK_HIP(ctx, iters.alloc(a.n_fits));
        return PSK_OK;
    }
    // after the launch; returns with the stream idle, so host vectors that were uploaded may go out of scope after it
    int download(psk_ctx *ctx, const FitArgs &a) const
    {
        PSK_HIP(ctx, hipGetLastError());
        PSK_HIP(ctx, coef.download(a.coef_out, (size_t)a.n_fits * a.p, ctx->stream));
        PSK_HIP(ctx, icpt.download(a.icpt_out, a.n_fits, ctx->stream));
        if (a.iters_out) PSK_HIP(ctx, iters.download(a.iters_out, a.n_fits, ctx->stream));
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return PSK_OK;
    }
};

// presence/absence design: every entry 0 or 1
inline bool design_is_binary(const float *X, size_t count)
{
    return std::all_of(X, X + count, [](float v) { return v == 0.0f || v == 1.0f; });
}

inline std::vector<int8_t> labels_pm1(const int32_t *y01, int n)
{
    std::vector<int8_t> ypm(n);
    for (int i = 0; i < n; i++) ypm[i] = y01[i] ? 1 : -1;
    return ypm;
}

// X[n][p] -> XT[p][n], or XT[p + 1][n] with a last row of ones (the intercept as a feature)
inline std::vector<float> transpose_f32(const float *X, int n, int p, bool ones_row)
{
    std::vector<float> XT((size_t)(p + (ones_row ? 1 : 0)) * n, 1.0f);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < p; j++) XT[(size_t)j * n + i] = X[(size_t)i * p + j];
    return XT;
}

// [rows][W] column bit words: sample i of column j = bit i & 63 of word i >> 6 of row j; rows p.. are zero, or row p is
// the constant-1 intercept column (`intercept`, rows > p)
inline std::vector<uint64_t> pack_sample_bits(const float *X, int n, int p, int W, int rows, bool intercept)
{
    std::vector<uint64_t> bits((size_t)rows * W, 0);
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < p; j++)
            if (X[(size_t)i * p + j] != 0.0f) bits[(size_t)j * W + (i >> 6)] |= 1ull << (i & 63);
        if (intercept) bits[(size_t)p * W + (i >> 6)] |= 1ull << (i & 63);
    }
    return bits;
}

// [cols][64] lane-transposed columns for the register forms of the descent (a column in one register per lane, n <= 4096):
// word l of column j holds sample 64 t + l at bit t; column p is the constant-1 intercept column when `intercept`
inline std::vector<uint64_t> pack_lane_bits(const float *X, int n, int p, bool intercept)
{
    std::vector<uint64_t> bitsT((size_t)(p + (intercept ? 1 : 0)) * 64, 0);
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < p; j++)
            if (X[(size_t)i * p + j] != 0.0f) bitsT[(size_t)j * 64 + (i & 63)] |= 1ull << (i >> 6);
        if (intercept) bitsT[(size_t)p * 64 + (i & 63)] |= 1ull << (i >> 6);
    }
    return bitsT;
}

}  // namespace
