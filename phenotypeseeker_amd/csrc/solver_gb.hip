// Gradient-boosted regression trees for `-bc XGBC` / `-reg XGBR`.  The reference offers both names and completes neither:
// get_model_name, set_model, set_hyperparameters and get_best_model (modeling.py:186-207, :994-1103) have no case for them.
// The yardstick is scikit-learn 1.7.2's GradientBoostingClassifier() / GradientBoostingRegressor() with their defaults
// (n_estimators 100, learning_rate 0.1, max_depth 3, criterion 'friedman_mse', subsample 1.0, min_samples_split 2,
// min_samples_leaf 1, every feature considered, init None; loss log_loss / squared_error), fitted directly, no search.  THIS IS
// SCIKIT-LEARN'S GRADIENT BOOSTING, NOT XGBOOST'S REGULARISED OBJECTIVE.  The design is 0/1, so a node is a bit-mask over the
// samples and a split evaluation is a sum of residuals over the set bits of a column.  What is restated
// (sklearn/ensemble/_gb.py::_fit_stage, _update_terminal_regions; sklearn/tree/_criterion.pyx::FriedmanMSE.
// proxy_impurity_improvement; sklearn/tree/_tree.pyx::DepthFirstTreeBuilder; DESIGN.md section 5 and include/psk.h, f16):
//   * per stage the residuals r = y - F (squared error) or y - gb_expit(F) (log loss; gb_expit is this project's own function,
//     solver_gb_math.h), a regression tree on them, then F += learning_rate * value[leaf] for EVERY sample
//   * EVERY SUM OVER SAMPLES IS TAKEN IN A TWO-LEVEL ORDER: within a word of 64 samples ascending sample index from 0.0, then
//     the word partials in ascending word index from 0.0.  (scikit-learn adds in the order its introsort leaves the samples:
//     another order of the same terms.)
//   * a node with in-bag samples S: w = |S|, sum = sum r, sq = sum r r, value = sum / w, impurity = sq / w - (sum / w)(sum / w);
//     a leaf at max_depth, with w < 2, with impurity <= DBL_EPSILON, WHEN ALL r OF S ARE BIT-EQUAL (our rule: the case
//     scikit-learn's leaf rule means and its rounding decides at random), or without a non-constant column
//   * a split on column j: w_r / sum_r over the set bits, w_l = w - w_r, sum_l = sum - sum_r, diff = w_r sum_l - w_l sum_r,
//     proxy = diff diff / (w_l w_r); the largest proxy wins, THE LOWEST COLUMN INDEX among bit-equal maxima (our rule; the
//     reduction runs over (value, index) pairs as in tree_fit_kernel); nodes in pre-order, the left child (bit clear) first
//   * log loss replaces a leaf's value by the Newton step: num = sum / w, den = (sum of prob (1 - prob)) / w with
//     prob = y - r, value = 0 if |den| < 1e-150 else num / den
// Held-out samples (fold == the fit's fit_fold) are routed and updated but never counted.
// Kernels: tree_pack_kernel (solver_tree_common.h) packs the design; gb_fit_kernel runs one workgroup per fit through all
// stages, with the stage's residuals (f64, 4096 samples = 32 KB) and the routing masks of the current path in LDS and F in
// global memory; gb_decision_kernel walks a fitted model with one thread per sample.
// COUNT DESIGNS (psk_gb_fit_counts / psk_gb_decision_counts, include/psk.h f16): the columns above become the threshold planes of
// tree_pack_counts (solver_tree_common.h), scanned in plane order, each plane's sum of residuals taken on its own in the
// two-level order; the node record gets the winning plane's column, the threshold comes from the node's in-bag values
// (tree_node_threshold) and the children are routed by the plane of tree_route_plane.  gb_decision_counts_kernel reads the
// float design itself: x <= threshold goes left.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_gb_math.h"
#include "solver_host.h"
#include "solver_tree_common.h"

namespace {

constexpr int GB_THREADS = 1024;
constexpr int GB_WAVES = GB_THREADS / 64;
constexpr int GB_MAX_N = 4096;
constexpr int GB_MAX_W = GB_MAX_N / 64;
constexpr int GB_MAX_DEPTH = 10;
constexpr int GB_MAX_STAGES = 1000;
constexpr int GB_NODE_FIELDS = 4;   // feature (-2: leaf), left, right (-1: leaf), n_node_samples

__device__ __forceinline__ bool gb_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

struct GbRec { int parent, depth, is_left; };

// the totals of a node, made by one lane over the word partials
struct GbNode { double sum, sq, hess; int w, all_equal; };

// COUNTS: `bits` holds the P threshold planes of a count design and p is P, so the scan below is the lowest column, then the
// lowest threshold (tree_build of solver_tree.hip does the same); thr_out gets scikit-learn's threshold, -2.0 at a leaf.
template <int LOSS, bool COUNTS>
__global__ __launch_bounds__(GB_THREADS) void gb_fit_kernel(
    const uint64_t *__restrict__ bits, const double *__restrict__ y, const int32_t *__restrict__ fold, int n, int p, int W,
    const int32_t *__restrict__ fit_fold, const double *__restrict__ init_raw, int n_estimators, double learning_rate, int max_depth,
    int cap, int32_t *__restrict__ node_count, int32_t *__restrict__ nodes, double *__restrict__ value_out,
    double *__restrict__ imp_out, double *__restrict__ raw, double *__restrict__ staged, const TreePlaneView<COUNTS> pv,
    double *__restrict__ thr_out)
{
    __shared__ double r[GB_MAX_N];
    __shared__ uint64_t mask[GB_MAX_DEPTH + 1][GB_MAX_W];
    __shared__ uint64_t T[GB_MAX_W], MT[GB_MAX_W], w_first[GB_MAX_W];
    __shared__ double w_sum[GB_MAX_W], w_sq[GB_MAX_W], w_hess[GB_MAX_W];
    __shared__ int w_equal[GB_MAX_W];
    __shared__ GbRec stack[GB_MAX_DEPTH + 2];
    __shared__ int path_feat[GB_MAX_DEPTH + 1];
    __shared__ double red_v[GB_WAVES];
    __shared__ int red_i[GB_WAVES];
    __shared__ GbNode node;
    __shared__ int gap[2];   // (COUNTS: the two values around a split, tree_node_threshold)

    const int fit = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tf = fit_fold[fit];
    // the in-bag mask and the mask of existing samples, a word per wave ballot (n <= 4096 = 4 x 1024)
    for (int s0 = 0; s0 < W * 64; s0 += GB_THREADS) {
        const int s = s0 + tid;
        const uint64_t live = __ballot(s < n), train = __ballot(s < n && fold[min(s, n - 1)] != tf);
        if (lane == 0 && s < W * 64) {
            mask[0][s >> 6] = live;
            T[s >> 6] = train;
        }
    }
    double *F = raw + (size_t)fit * n;
    for (int s = tid; s < n; s += GB_THREADS) F[s] = init_raw[fit];   // (thread s % 1024 owns F[s] throughout)

    for (int stage = 0; stage < n_estimators; stage++) {
        const size_t tree = (size_t)fit * n_estimators + stage;
        int32_t *nd = nodes + tree * cap * GB_NODE_FIELDS;
        double *vo = value_out + tree * cap, *io = imp_out + tree * cap;
        double *to = COUNTS ? thr_out + tree * cap : nullptr;
        __syncthreads();   // every read of the stage before
        for (int s = tid; s < n; s += GB_THREADS) r[s] = LOSS == 0 ? y[s] - F[s] : y[s] - gb_expit(F[s]);
        if (tid == 0) stack[0] = GbRec{-1, 0, 0};
        int sp = 1, next_id = 0;
        while (sp > 0) {
            __syncthreads();   // the residuals, the stack, the path and everything the node before wrote
            const GbRec rec = stack[--sp];
            const int d = rec.depth;
            if (tid < W) {
                // one lane per word: the routing mask of the node, then the word's partial sums in ascending sample order
                uint64_t m = mask[0][tid];
                if (d > 0) {
                    const uint64_t col = bits[tree_bit_at(path_feat[d - 1], tid, p)];
                    m = mask[d - 1][tid] & (rec.is_left ? ~col : col);
                    mask[d][tid] = m;
                }
                uint64_t v = m & T[tid];
                MT[tid] = v;
                double ps = 0.0, pq = 0.0, ph = 0.0;
                uint64_t first = 0;
                int eq = 1;
                bool have = false;
                while (v) {
                    const int s = tid * 64 + __builtin_ctzll(v);
                    v &= v - 1;
                    const double g = r[s];
                    ps += g;
                    pq += g * g;
                    if (LOSS == 1) {
                        const double prob = y[s] - g;
                        ph += prob * (1.0 - prob);
                    }
                    const uint64_t gb = (uint64_t)__double_as_longlong(g);
                    if (!have) { first = gb; have = true; }
                    else if (gb != first) eq = 0;
                }
                w_sum[tid] = ps; w_sq[tid] = pq; w_hess[tid] = ph; w_first[tid] = first; w_equal[tid] = eq;
            }
            __syncthreads();
            if (tid == 0) {
                // one lane over the words, ascending
                GbNode t{0.0, 0.0, 0.0, 0, 1};
                uint64_t first = 0;
                bool have = false;
                for (int w = 0; w < W; w++) {
                    t.sum += w_sum[w]; t.sq += w_sq[w]; t.hess += w_hess[w];
                    if (!MT[w]) continue;
                    t.w += __popcll(MT[w]);
                    if (!w_equal[w]) t.all_equal = 0;
                    if (!have) { first = w_first[w]; have = true; }
                    else if (w_first[w] != first) t.all_equal = 0;
                }
                node = t;
            }
            __syncthreads();
            const GbNode t = node;
            const double nw = (double)t.w;
            const double mean = t.sum / nw;
            const double imp = t.sq / nw - mean * mean;
            bool is_leaf = d >= max_depth || t.w < 2 || imp <= DBL_EPSILON || t.all_equal;
            int feat = -2;
            if (!is_leaf) {
                double bv = -INFINITY;
                int bi = INT_MAX;
                for (int j = tid; j < p; j += GB_THREADS) {
                    int c = 0;
                    double sr = 0.0;
                    for (int w = 0; w < W; w++) {
                        const uint64_t m = MT[w];
                        if (!m) continue;   // (uniform: the mask words are the workgroup's)
                        uint64_t v = bits[tree_bit_at(j, w, p)] & m;
                        if (!v) continue;   // (a partial of +0.0: adding it changes nothing)
                        c += __popcll(v);
                        double ps = 0.0;
                        while (v) {
                            ps += r[w * 64 + __builtin_ctzll(v)];
                            v &= v - 1;
                        }
                        sr += ps;
                    }
                    if (c == 0 || c == t.w) continue;   // constant in this node
                    const double wr = (double)c, wl = (double)(t.w - c);
                    const double sl = t.sum - sr;
                    const double diff = wr * sl - wl * sr;
                    const double proxy = diff * diff / (wl * wr);
                    if (proxy > bv) { bv = proxy; bi = j; }   // j ascends: the first maximum stays
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const double ov = psk_shfl_xor_f64(bv, s);
                    const int oi = __shfl_xor(bi, s, 64);
                    if (gb_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                }
                if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
                __syncthreads();
                bv = red_v[0]; bi = red_i[0];
                for (int w = 1; w < GB_WAVES; w++)
                    if (gb_better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
                if (bi == INT_MAX) is_leaf = true;
                else feat = bi;
            }
            const int id = next_id++;
            int route = feat;
            if constexpr (COUNTS) {
                // (is_leaf is the workgroup's: every thread takes the same side, so the barriers inside are met by all)
                double thr = -2.0;
                if (!is_leaf) {
                    const int col = pv.plane_col[feat];
                    thr = tree_node_threshold(pv.X, n, pv.p, col, pv.plane_val[feat], MT, gap);
                    route = tree_route_plane(pv.col_first, pv.plane_val, col, thr);
                    feat = col;
                }
                if (tid == 0) to[id] = thr;
            }
            double val = mean;
            if (LOSS == 1 && is_leaf) {
                // _gb.py::_update_terminal_regions, compute_update of the binomial loss, with _safe_divide
                const double num = t.sum / nw, den = t.hess / nw;
                val = fabs(den) < 1e-150 ? 0.0 : num / den;
            }
            if (tid == 0) {
                int32_t *k = nd + (size_t)id * GB_NODE_FIELDS;
                k[0] = feat;
                k[1] = is_leaf ? -1 : id + 1;
                k[2] = -1;
                k[3] = t.w;
                vo[id] = val;
                io[id] = imp;
                if (rec.parent >= 0 && !rec.is_left) nd[(size_t)rec.parent * GB_NODE_FIELDS + 2] = id;
            }
            if (is_leaf) {
                const double step = learning_rate * val;
                for (int s = tid; s < n; s += GB_THREADS)
                    if ((mask[d][s >> 6] >> (s & 63)) & 1ull) F[s] += step;
            } else {
                // (the barrier of the reduction lies between every thread's read of `rec` and these writes)
                if (tid == 0) {
                    path_feat[d] = route;
                    stack[sp] = GbRec{id, d + 1, 0};       // the right child, taken after the whole left subtree
                    stack[sp + 1] = GbRec{id, d + 1, 1};
                }
                sp += 2;
            }
        }
        if (tid == 0) node_count[tree] = next_id;
        if (staged)
            for (int s = tid; s < n; s += GB_THREADS) staged[tree * n + s] = F[s];
    }
}

// One thread per sample: init + the stages' learning_rate * value[leaf] added in stage order.  The host has checked that a
// split's column lies in 0 .. p - 1 and its children behind it and inside the tree, so the walk ends and stays in bounds.
__global__ __launch_bounds__(256) void gb_decision_kernel(const uint64_t *__restrict__ bits, int n, int p, int n_estimators, int cap,
                                                          const int32_t *__restrict__ nodes, const double *__restrict__ value,
                                                          double init_raw, double learning_rate, double *__restrict__ out)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int w = s >> 6, k = s & 63;
    double F = init_raw;
    for (int t = 0; t < n_estimators; t++) {
        const int32_t *nd = nodes + (size_t)t * cap * GB_NODE_FIELDS;
        int node = 0;
        for (int step = 0; step < cap; step++) {
            const int f = nd[(size_t)node * GB_NODE_FIELDS];
            if (f < 0) break;
            const uint64_t bit = (bits[tree_bit_at(f, w, p)] >> k) & 1ull;
            node = nd[(size_t)node * GB_NODE_FIELDS + (bit ? 2 : 1)];
        }
        F += learning_rate * value[(size_t)t * cap + node];
    }
    out[s] = F;
}

// The same walk on a count design: the float design itself, x <= threshold goes left (a count is exact in f32 and in f64).
// The host has also checked that a split's threshold is finite.
__global__ __launch_bounds__(256) void gb_decision_counts_kernel(const float *__restrict__ X, int n, int p, int n_estimators, int cap,
                                                                 const int32_t *__restrict__ nodes, const double *__restrict__ value,
                                                                 const double *__restrict__ threshold, double init_raw,
                                                                 double learning_rate, double *__restrict__ out)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float *x = X + (size_t)s * p;
    double F = init_raw;
    for (int t = 0; t < n_estimators; t++) {
        const int32_t *nd = nodes + (size_t)t * cap * GB_NODE_FIELDS;
        const double *th = threshold + (size_t)t * cap;
        int node = 0;
        for (int step = 0; step < cap; step++) {
            const int f = nd[(size_t)node * GB_NODE_FIELDS];
            if (f < 0) break;
            node = nd[(size_t)node * GB_NODE_FIELDS + ((double)x[f] <= th[node] ? 1 : 2)];
        }
        F += learning_rate * value[(size_t)t * cap + node];
    }
    out[s] = F;
}

int gb_check_model_shape(psk_ctx *ctx, const char *who, int n_estimators, int max_depth)
{
    if (max_depth < 1 || max_depth > GB_MAX_DEPTH)
        return psk_fail(ctx, PSK_EINVAL, "%s: max_depth must be 1..%d, got %d", who, GB_MAX_DEPTH, max_depth);
    if (n_estimators < 1 || n_estimators > GB_MAX_STAGES)
        return psk_fail(ctx, PSK_EINVAL, "%s: n_estimators must be 1..%d, got %d", who, GB_MAX_STAGES, n_estimators);
    return PSK_OK;
}

// What both decision calls check before the kernel walks the model: the walk trusts that a split's column exists, that its
// children lie behind it (pre-order) and inside the tree and, with thresholds, that a split's threshold is finite.
int gb_check_model(psk_ctx *ctx, const char *who, const float *X, int n, int p, int n_estimators, int max_depth, const int32_t *node_count,
                   const int32_t *nodes, const double *value, const double *threshold, bool counts, const double *raw_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !node_count || !nodes || !value || !raw_out || (counts && !threshold)) return psk_fail(ctx, PSK_EINVAL, "%s: null buffer", who);
    if (n < 1 || p < 1) return psk_fail(ctx, PSK_EINVAL, "%s: bad problem shape n=%d p=%d", who, n, p);
    if (const int rc = gb_check_model_shape(ctx, who, n_estimators, max_depth)) return rc;
    const int cap = (2 << max_depth) - 1;
    for (int t = 0; t < n_estimators; t++) {
        const int count = node_count[t];
        if (count < 1 || count > cap)
            return psk_fail(ctx, PSK_EINVAL, "%s: stage %d has %d nodes, a tree of depth %d has 1..%d", who, t, count, max_depth, cap);
        for (int k = 0; k < count; k++) {
            const int32_t *nd = nodes + ((size_t)t * cap + k) * GB_NODE_FIELDS;
            if (nd[0] < 0) continue;
            if (nd[0] >= p || nd[1] <= k || nd[1] >= count || nd[2] <= k || nd[2] >= count)
                return psk_fail(ctx, PSK_EINVAL, "%s: node %d of stage %d is not a split of a pre-order tree on %d columns", who, k, t, p);
            if (counts && !std::isfinite(threshold[(size_t)t * cap + k]))
                return psk_fail(ctx, PSK_EINVAL, "%s: node %d of stage %d splits at a threshold that is not finite", who, k, t);
        }
    }
    return PSK_OK;
}

// psk_gb_fit (COUNTS false: threshold_out unused) and psk_gb_fit_counts; `who` names the entry point in messages
template <bool COUNTS>
int gb_fit_call(psk_ctx *ctx, const char *who, const float *X, const double *y, int n, int p, const int32_t *fold, const int32_t *fit_fold,
                int n_fits, int loss, int n_estimators, double learning_rate, int max_depth, const double *init_raw,
                int32_t *node_count_out, int32_t *nodes_out, double *value_out, double *impurity_out, double *threshold_out,
                double *raw_out, double *staged_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !y || !fold || !fit_fold || !init_raw || !node_count_out || !nodes_out || !value_out || !impurity_out || !raw_out ||
        (COUNTS && !threshold_out))
        return psk_fail(ctx, PSK_EINVAL, "%s: null buffer", who);
    if (n < 1 || p < 1 || n_fits < 1 || n_fits > 65535)
        return psk_fail(ctx, PSK_EINVAL, "%s: bad problem shape n=%d p=%d fits=%d", who, n, p, n_fits);
    if (n > GB_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s keeps a stage's residuals and a node's sample mask in LDS: at most %d samples, got %d",
                        who, GB_MAX_N, n);
    if (const int rc = gb_check_model_shape(ctx, who, n_estimators, max_depth)) return rc;
    if (!(learning_rate > 0.0) || !std::isfinite(learning_rate))
        return psk_fail(ctx, PSK_EINVAL, "%s: learning_rate must be a finite number above 0, got %g", who, learning_rate);
    if (loss != 0 && loss != 1)
        return psk_fail(ctx, PSK_EINVAL, "%s: loss must be 0 (squared error) or 1 (log loss), got %d", who, loss);
    for (int i = 0; i < n; i++) {
        if (loss == 1 && y[i] != 0.0 && y[i] != 1.0)
            return psk_fail(ctx, PSK_EINVAL, "%s: the log loss takes labels 0 and 1, sample %d holds %g", who, i, y[i]);
        if (!std::isfinite(y[i])) return psk_fail(ctx, PSK_EINVAL, "%s: sample %d has no finite target", who, i);
    }
    for (int f = 0; f < n_fits; f++) {
        if (!std::isfinite(init_raw[f])) return psk_fail(ctx, PSK_EINVAL, "%s: fit %d has no finite init_raw", who, f);
        int in_bag = 0;
        bool has0 = false, has1 = false;
        for (int i = 0; i < n; i++)
            if (fold[i] != fit_fold[f]) {
                in_bag++;
                (y[i] != 0.0 ? has1 : has0) = true;
            }
        if (!in_bag) return psk_fail(ctx, PSK_EINVAL, "%s: fit %d has no in-bag sample", who, f);
        if (loss == 1 && !(has0 && has1))
            return psk_fail(ctx, PSK_EINVAL, "%s: the in-bag samples of fit %d are of one class", who, f);
    }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64, cap = (2 << max_depth) - 1;
    const size_t trees = (size_t)n_fits * n_estimators, slots = trees * cap;
    FitArr<uint64_t> bits, ymask;
    FitArr<int32_t> d_fold, d_fit_fold, count, d_nodes;
    FitArr<double> d_y, d_init, d_val, d_imp, d_raw, d_staged, d_thr;
    const std::vector<int32_t> no_labels((size_t)n, 0);   // (the packing kernel takes 0/1 labels; nothing reads their mask here)
    TreePlanes pl;
    TreePlaneView<COUNTS> pv;
    if constexpr (COUNTS) {
        if (const int rc = tree_pack_counts(ctx, who, X, no_labels.data(), n, p, pl, ymask)) return rc;
        pv = TreePlaneView<true>{pl.x, pl.col_first, pl.plane_col, pl.col_order, pl.plane_val, p};
    } else {
        if (const int rc = tree_pack_design(ctx, who, X, no_labels.data(), n, p, bits, ymask)) return rc;
    }
    PSK_HIP(ctx, d_y.upload(y, n, ctx->stream));
    PSK_HIP(ctx, d_fold.upload(fold, n, ctx->stream));
    PSK_HIP(ctx, d_fit_fold.upload(fit_fold, n_fits, ctx->stream));
    PSK_HIP(ctx, d_init.upload(init_raw, n_fits, ctx->stream));
    PSK_HIP(ctx, count.alloc(trees));
    PSK_HIP(ctx, d_nodes.alloc(slots * GB_NODE_FIELDS));
    PSK_HIP(ctx, d_val.alloc(slots));
    PSK_HIP(ctx, d_imp.alloc(slots));
    PSK_HIP(ctx, d_raw.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, d_staged.alloc(staged_out ? trees * n : 0));
    PSK_HIP(ctx, d_thr.alloc(COUNTS ? slots : 0));
    // (slots behind a tree's node_count read as zeros)
    PSK_HIP(ctx, d_nodes.zero(ctx->stream));
    PSK_HIP(ctx, d_val.zero(ctx->stream));
    PSK_HIP(ctx, d_imp.zero(ctx->stream));
    if (COUNTS) PSK_HIP(ctx, d_thr.zero(ctx->stream));
    double *staged = staged_out ? (double *)d_staged : nullptr;
    // (the count kernel scans the P planes where the 0/1 kernel scans the p columns)
    const uint64_t *d_bits = COUNTS ? (const uint64_t *)pl.bits : (const uint64_t *)bits;
    const int cols = COUNTS ? pl.P : p;
    if (loss == 0)
        gb_fit_kernel<0, COUNTS><<<n_fits, GB_THREADS, 0, ctx->stream>>>(d_bits, d_y, d_fold, n, cols, W, d_fit_fold, d_init, n_estimators,
                                                                         learning_rate, max_depth, cap, count, d_nodes, d_val, d_imp, d_raw,
                                                                         staged, pv, d_thr);
    else
        gb_fit_kernel<1, COUNTS><<<n_fits, GB_THREADS, 0, ctx->stream>>>(d_bits, d_y, d_fold, n, cols, W, d_fit_fold, d_init, n_estimators,
                                                                         learning_rate, max_depth, cap, count, d_nodes, d_val, d_imp, d_raw,
                                                                         staged, pv, d_thr);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, count.download(node_count_out, trees, ctx->stream));
    PSK_HIP(ctx, d_nodes.download(nodes_out, slots * GB_NODE_FIELDS, ctx->stream));
    PSK_HIP(ctx, d_val.download(value_out, slots, ctx->stream));
    PSK_HIP(ctx, d_imp.download(impurity_out, slots, ctx->stream));
    PSK_HIP(ctx, d_raw.download(raw_out, (size_t)n_fits * n, ctx->stream));
    if (staged_out) PSK_HIP(ctx, d_staged.download(staged_out, trees * n, ctx->stream));
    if (COUNTS) PSK_HIP(ctx, d_thr.download(threshold_out, slots, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (COUNTS)   // a slot behind a tree's node_count holds what a leaf holds
        for (size_t t = 0; t < trees; t++)
            for (int k = node_count_out[t]; k < cap; k++) threshold_out[t * cap + k] = -2.0;
    return PSK_OK;
}

}  // namespace

extern "C" int psk_gb_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold, const int32_t *fit_fold,
                          int n_fits, int loss, int n_estimators, double learning_rate, int max_depth, const double *init_raw,
                          int32_t *node_count_out, int32_t *nodes_out, double *value_out, double *impurity_out, double *raw_out,
                          double *staged_out)
{
    return gb_fit_call<false>(ctx, "psk_gb_fit", X, y, n, p, fold, fit_fold, n_fits, loss, n_estimators, learning_rate, max_depth, init_raw,
                              node_count_out, nodes_out, value_out, impurity_out, nullptr, raw_out, staged_out);
}

extern "C" int psk_gb_fit_counts(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                                 const int32_t *fit_fold, int n_fits, int loss, int n_estimators, double learning_rate, int max_depth,
                                 const double *init_raw, int32_t *node_count_out, int32_t *nodes_out, double *value_out,
                                 double *impurity_out, double *threshold_out, double *raw_out, double *staged_out)
{
    return gb_fit_call<true>(ctx, "psk_gb_fit_counts", X, y, n, p, fold, fit_fold, n_fits, loss, n_estimators, learning_rate, max_depth,
                             init_raw, node_count_out, nodes_out, value_out, impurity_out, threshold_out, raw_out, staged_out);
}

extern "C" int psk_gb_decision(psk_ctx *ctx, const float *X, int n, int p, int n_estimators, int max_depth, const int32_t *node_count,
                               const int32_t *nodes, const double *value, double init_raw, double learning_rate, double *raw_out)
{
    if (const int rc = gb_check_model(ctx, "psk_gb_decision", X, n, p, n_estimators, max_depth, node_count, nodes, value, nullptr, false, raw_out))
        return rc;
    const int cap = (2 << max_depth) - 1;

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t slots = (size_t)n_estimators * cap;
    FitArr<uint64_t> bits, ymask;
    FitArr<int32_t> d_nodes;
    FitArr<double> d_val, d_out;
    const std::vector<int32_t> no_labels((size_t)n, 0);
    if (const int rc = tree_pack_design(ctx, "psk_gb_decision", X, no_labels.data(), n, p, bits, ymask)) return rc;
    PSK_HIP(ctx, d_nodes.upload(nodes, slots * GB_NODE_FIELDS, ctx->stream));
    PSK_HIP(ctx, d_val.upload(value, slots, ctx->stream));
    PSK_HIP(ctx, d_out.alloc(n));
    gb_decision_kernel<<<div_up(n, 256), 256, 0, ctx->stream>>>(bits, n, p, n_estimators, cap, d_nodes, d_val, init_raw, learning_rate, d_out);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, d_out.download(raw_out, n, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

extern "C" int psk_gb_decision_counts(psk_ctx *ctx, const float *X, int n, int p, int n_estimators, int max_depth, const int32_t *node_count,
                                      const int32_t *nodes, const double *value, const double *threshold, double init_raw,
                                      double learning_rate, double *raw_out)
{
    const char *who = "psk_gb_decision_counts";
    if (const int rc = gb_check_model(ctx, who, X, n, p, n_estimators, max_depth, node_count, nodes, value, threshold, true, raw_out)) return rc;
    const int cap = (2 << max_depth) - 1;
    // (the words of tree_pack_counts: the rows of a count design, whichever call takes them)
    for (int i = 0; i < n; i++)
        for (int j = 0; j < p; j++) {
            const float v = X[(size_t)i * p + j];
            if (!(v >= 0.0f && v <= TREE_COUNT_MAX && v == floorf(v)))
                return psk_fail(ctx, PSK_EINVAL, "%s takes a count design (integers in 0 .. 2^24): sample %d, column %d holds %g", who, i, j,
                                (double)v);
        }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t slots = (size_t)n_estimators * cap;
    FitArr<float> x;
    FitArr<int32_t> d_nodes;
    FitArr<double> d_val, d_thr, d_out;
    PSK_HIP(ctx, x.upload(X, (size_t)n * p, ctx->stream));
    PSK_HIP(ctx, d_nodes.upload(nodes, slots * GB_NODE_FIELDS, ctx->stream));
    PSK_HIP(ctx, d_val.upload(value, slots, ctx->stream));
    PSK_HIP(ctx, d_thr.upload(threshold, slots, ctx->stream));
    PSK_HIP(ctx, d_out.alloc(n));
    gb_decision_counts_kernel<<<div_up(n, 256), 256, 0, ctx->stream>>>(x, n, p, n_estimators, cap, d_nodes, d_val, d_thr, init_raw,
                                                                       learning_rate, d_out);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, d_out.download(raw_out, n, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}
