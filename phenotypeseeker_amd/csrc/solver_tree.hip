// Decision-tree fits of the reference's `-bc DT` branch: GridSearchCV(DecisionTreeClassifier(), {'max_depth': 1..10,
// 'criterion': ['gini', 'entropy']}) (set_model / fit_model, modeling.py:1032-1033, :1069-1073, :1100-1103).  The design is
// 0/1, so a node is a bit-mask over the samples and a split evaluation is two popcounts per column word.  This is
// scikit-learn's DepthFirstTreeBuilder over its BestSplitter with the default settings (min_samples_split 2,
// min_samples_leaf 1, min_impurity_decrease 0, every feature considered, unit sample weights) restated:
//   * nodes are numbered in pre-order, the left subtree (bit clear, x <= 0.5) before the right one
//   * a node is a leaf at max_depth, with fewer than 2 samples, with impurity <= DBL_EPSILON, without a non-constant column,
//     or when the improvement of the best split + DBL_EPSILON < 0 (rounding only: a zero improvement is taken, the best proxy
//     starts at -inf)
//   * the split of a node is the column with the largest proxy  -n_right I_right - n_left I_left  (Criterion::
//     proxy_impurity_improvement over children_impurity), in f64 with scikit-learn's expressions in their order and no FMA
//     fusion (the unit is compiled -ffp-contract=off); gini I = 1 - (c0^2 + c1^2) / (n n), entropy I = -sum c/n (ln(c/n) / ln 2)
//   * scikit-learn visits the columns in an unseeded random order and keeps the first of equally good ones; HERE THE LOWEST
//     COLUMN INDEX WINS among bit-equal maxima.  The reduction runs over (value, index) pairs, a total
//     order, so the order in which lanes and waves are combined cannot matter
//   * a child's impurity is the children_impurity value its parent's split computed; the root's is node_impurity
// Two kernels: tree_pack_kernel (solver_tree_common.h, with the impurity expressions and the node record) turns the float
// design into bit words (W x p u64, W = ceil(n / 64), word-major) plus the label mask and flags any value other than 0 or 1;
// tree_fit_kernel runs one workgroup per fit with the routing masks of
// the current root-to-node path in LDS (11 levels x 64 words = 5.6 KB at 4096 samples) and the pending right children on a
// 12-entry stack.  The routing masks carry every sample, held-out ones included, so each sample's leaf is known when the
// leaf is made; counts are taken under the fit's training mask.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_host.h"
#include "solver_tree_common.h"

namespace {

// A grid search is 20 x (folds + 1) = 220 workgroups on 256 compute units, and the model stage keeps ~1000 columns
// (--n_kmers): one workgroup per compute unit with one column per thread.  LDS per workgroup is 8 KB, no limit here.
constexpr int TREE_THREADS = 1024;
constexpr int TREE_WAVES = TREE_THREADS / 64;
constexpr int TREE_MAX_N = 4096;
constexpr int TREE_MAX_W = TREE_MAX_N / 64;
constexpr int TREE_MAX_DEPTH = 10;

// (value, column) maximum, the LOWEST column winning among equal values
__device__ __forceinline__ bool tree_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

struct TreeRec { int parent, depth, is_left, n, n1; double imp; };

// COUNTS: `bits` holds the P threshold planes of a count design and p is P (solver_tree_common.h), so the scan below is the
// lowest column, then the lowest threshold; the node record gets the plane's column, thr_out scikit-learn's threshold, and the
// path the plane that routes by it.
template <int CRIT, bool COUNTS>
__device__ void tree_build(const uint64_t *__restrict__ bits, int n, int p, int W, int max_depth, int32_t *__restrict__ nodes,
                           double *__restrict__ imp_out, int32_t *__restrict__ leaf_out, double *__restrict__ frac_out,
                           int32_t *__restrict__ node_count, int32_t *__restrict__ depth_out,
                           uint64_t (*mask)[TREE_MAX_W], const uint64_t *T, const uint64_t *Y, uint64_t *MT, uint64_t *MTY,
                           TreeRec *stack, int *path_feat, double *red_v, int *red_i, int *red_c, const TreePlaneView<COUNTS> &pv,
                           double *__restrict__ thr_out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n_tot = 0, n1_tot = 0;
    for (int w = 0; w < W; w++) { n_tot += __popcll(T[w]); n1_tot += __popcll(T[w] & Y[w]); }
    if (tid == 0)
        stack[0] = TreeRec{-1, 0, 0, n_tot, n1_tot, tree_impurity<CRIT>((double)(n_tot - n1_tot), (double)n1_tot, (double)n_tot)};
    int sp = 1, next_id = 0, deepest = 0;
    while (sp > 0) {
        __syncthreads();   // the stack, the path and everything the node before wrote
        const TreeRec rec = stack[--sp];
        const int d = rec.depth;
        if (tid < W) {
            uint64_t m = mask[0][tid];
            if (d > 0) {
                const uint64_t col = bits[tree_bit_at(path_feat[d - 1], tid, p)];
                m = mask[d - 1][tid] & (rec.is_left ? ~col : col);
                mask[d][tid] = m;
            }
            MT[tid] = m & T[tid];
            MTY[tid] = m & T[tid] & Y[tid];
        }
        __syncthreads();
        const double nn = (double)rec.n, c1n = (double)rec.n1, c0n = (double)(rec.n - rec.n1);
        bool is_leaf = d >= max_depth || rec.n < 2 || rec.imp <= DBL_EPSILON;
        int feat = -2, cr = 0, cr1 = 0;
        double imp_l = 0.0, imp_r = 0.0;
        if (!is_leaf) {
            double bv = -INFINITY;
            int bi = INT_MAX, bc = 0;
            for (int j = tid; j < p; j += TREE_THREADS) {
                int c = 0, c1 = 0;
                for (int w = 0; w < W; w++) {
                    const uint64_t m = MT[w];
                    if (!m) continue;   // (uniform: the mask words are the workgroup's)
                    const uint64_t v = bits[tree_bit_at(j, w, p)];
                    c += __popcll(v & m);
                    c1 += __popcll(v & MTY[w]);
                }
                if (c == 0 || c == rec.n) continue;   // constant in this node
                const double wr = (double)c, wl = (double)(rec.n - c);
                const double ir = tree_impurity<CRIT>((double)(c - c1), (double)c1, wr);
                const double il = tree_impurity<CRIT>(c0n - (double)(c - c1), c1n - (double)c1, wl);
                const double proxy = -wr * ir - wl * il;
                if (proxy > bv) { bv = proxy; bi = j; bc = c | (c1 << 16); }   // j ascends: the first maximum stays
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const double ov = psk_shfl_xor_f64(bv, s);
                const int oi = __shfl_xor(bi, s, 64), oc = __shfl_xor(bc, s, 64);
                if (tree_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bc = oc; }
            }
            if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_c[wave] = bc; }
            __syncthreads();
            bv = red_v[0]; bi = red_i[0]; bc = red_c[0];
            for (int w = 1; w < TREE_WAVES; w++)
                if (tree_better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; bc = red_c[w]; }
            if (bi == INT_MAX) {
                is_leaf = true;
            } else {
                cr = bc & 0xffff;
                cr1 = bc >> 16;
                const double wr = (double)cr, wl = (double)(rec.n - cr);
                imp_r = tree_impurity<CRIT>((double)(cr - cr1), (double)cr1, wr);
                imp_l = tree_impurity<CRIT>(c0n - (double)(cr - cr1), c1n - (double)cr1, wl);
                const double improvement = (nn / (double)n_tot) * (rec.imp - (wr / nn * imp_r) - (wl / nn * imp_l));
                if (improvement + DBL_EPSILON < 0.0) is_leaf = true;
                else feat = bi;
            }
        }
        const int id = next_id++;
        deepest = max(deepest, d);
        int route = feat;
        if constexpr (COUNTS) {
            double thr = -2.0;
            if (!is_leaf) {
                const int col = pv.plane_col[feat];
                thr = tree_node_threshold(pv.X, n, pv.p, col, pv.plane_val[feat], MT, red_i);
                route = tree_route_plane(pv.col_first, pv.plane_val, col, thr);
                feat = col;
            }
            if (tid == 0) thr_out[id] = thr;
        }
        if (tid == 0) tree_write_node(nodes, imp_out, id, rec.parent, rec.is_left, feat, is_leaf, rec.n, rec.n - rec.n1, rec.n1, rec.imp);
        if (is_leaf) {
            const double f1 = c1n / nn;
            for (int s = tid; s < n; s += TREE_THREADS)
                if ((mask[d][s >> 6] >> (s & 63)) & 1ull) { leaf_out[s] = id; frac_out[s] = f1; }
        } else {
            // (the barrier of the reduction lies between every thread's read of `rec` and these writes)
            if (tid == 0) {
                path_feat[d] = route;
                stack[sp] = TreeRec{id, d + 1, 0, cr, cr1, imp_r};
                stack[sp + 1] = TreeRec{id, d + 1, 1, rec.n - cr, rec.n1 - cr1, imp_l};
            }
            sp += 2;
        }
    }
    if (tid == 0) { *node_count = next_id; *depth_out = deepest; }
}

template <bool COUNTS>
__global__ __launch_bounds__(TREE_THREADS) void tree_fit_kernel(
    const uint64_t *__restrict__ bits, const uint64_t *__restrict__ ymask, const int32_t *__restrict__ fold, int n, int p, int W,
    const int32_t *__restrict__ fit_max_depth, const int32_t *__restrict__ fit_criterion, const int32_t *__restrict__ fit_fold,
    int32_t *__restrict__ node_count, int32_t *__restrict__ depth_out, int32_t *__restrict__ nodes, double *__restrict__ imp_out,
    int32_t *__restrict__ leaf_out, double *__restrict__ frac_out, const int32_t *__restrict__ fit_off, const TreePlaneView<COUNTS> pv,
    double *__restrict__ thr_out)
{
    __shared__ uint64_t mask[TREE_MAX_DEPTH + 1][TREE_MAX_W];
    __shared__ uint64_t T[TREE_MAX_W], Y[TREE_MAX_W], MT[TREE_MAX_W], MTY[TREE_MAX_W];
    __shared__ TreeRec stack[TREE_MAX_DEPTH + 2];
    __shared__ int path_feat[TREE_MAX_DEPTH + 1];
    __shared__ double red_v[TREE_WAVES];
    __shared__ int red_i[TREE_WAVES], red_c[TREE_WAVES];

    const int fit = blockIdx.x, tid = threadIdx.x;
    const int tf = fit_fold[fit];
    // the training mask and the mask of existing samples, a word per wave ballot (n <= 4096 = 4 x 1024)
    for (int s0 = 0; s0 < W * 64; s0 += TREE_THREADS) {
        const int s = s0 + tid;
        const uint64_t live = __ballot(s < n), train = __ballot(s < n && fold[s] != tf);
        if ((tid & 63) == 0 && s < W * 64) {
            mask[0][s >> 6] = live;
            T[s >> 6] = train;
            Y[s >> 6] = ymask[s >> 6];
        }
    }
    __syncthreads();
    int32_t *nd = nodes + (size_t)fit_off[fit] * TREE_NODE_FIELDS;
    double *io = imp_out + (size_t)fit_off[fit];
    int32_t *lo = leaf_out + (size_t)fit * n;
    double *fo = frac_out + (size_t)fit * n;
    double *to = COUNTS ? thr_out + (size_t)fit_off[fit] : nullptr;
    if (fit_criterion[fit] == 0)
        tree_build<0, COUNTS>(bits, n, p, W, fit_max_depth[fit], nd, io, lo, fo, node_count + fit, depth_out + fit, mask, T, Y, MT, MTY,
                              stack, path_feat, red_v, red_i, red_c, pv, to);
    else
        tree_build<1, COUNTS>(bits, n, p, W, fit_max_depth[fit], nd, io, lo, fo, node_count + fit, depth_out + fit, mask, T, Y, MT, MTY,
                              stack, path_feat, red_v, red_i, red_c, pv, to);
}

// psk_tree_fit (COUNTS false: threshold_out unused) and psk_tree_fit_counts; `who` names the entry point in messages
template <bool COUNTS>
int tree_fit_call(psk_ctx *ctx, const char *who, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                  const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                  int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out, int32_t *leaf_out,
                  double *frac_out, double *threshold_out)
{
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !fold || !fit_max_depth || !fit_criterion || !fit_fold || !node_count_out || !max_depth_out || !nodes_out ||
        !impurity_out || !leaf_out || !frac_out || (COUNTS && !threshold_out))
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (n < 1 || p < 1 || n_fits < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d", n, p, n_fits);
    if (n > TREE_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s keeps a node's sample mask in LDS: at most %d samples, got %d", who, TREE_MAX_N, n);
    for (int f = 0; f < n_fits; f++) {
        if (fit_max_depth[f] < 1 || fit_max_depth[f] > TREE_MAX_DEPTH)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: max_depth must be 1..%d, got %d", f, TREE_MAX_DEPTH, fit_max_depth[f]);
        if (fit_criterion[f] != 0 && fit_criterion[f] != 1)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: criterion must be 0 (gini) or 1 (entropy), got %d", f, fit_criterion[f]);
        int tr = 0;
        for (int i = 0; i < n && !tr; i++) tr = fold[i] != fit_fold[f];
        if (!tr) return psk_fail(ctx, PSK_EINVAL, "fit %d has no training sample", f);
    }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    FitArr<uint64_t> bits, ymask;
    FitArr<int32_t> d_fold, depth, crit, d_fit_fold, d_off, count, dout, d_nodes, leaf;
    FitArr<double> d_imp, frac, d_thr;
    TreePlanes pl;
    TreePlaneView<COUNTS> pv;
    if constexpr (COUNTS) {
        if (const int rc = tree_pack_counts(ctx, who, X, y01, n, p, pl, ymask)) return rc;
        pv = TreePlaneView<true>{pl.x, pl.col_first, pl.plane_col, pl.col_order, pl.plane_val, p};
    } else {
        if (const int rc = tree_pack_design(ctx, who, X, y01, n, p, bits, ymask)) return rc;
    }

    // a tree of max_depth d has at most 2^(d+1) - 1 nodes: fit f's nodes start at off[f] of one packed buffer (a depth-1 fit
    // takes 3 slots, not PSK_TREE_NODE_CAP), and only the node_count[f] nodes it made go back into the caller's strided arrays
    std::vector<int32_t> off((size_t)n_fits + 1, 0);
    for (int f = 0; f < n_fits; f++) off[f + 1] = off[f] + (2 << fit_max_depth[f]) - 1;
    const size_t total = (size_t)off[n_fits];
    PSK_HIP(ctx, d_fold.upload(fold, n, ctx->stream));
    PSK_HIP(ctx, depth.upload(fit_max_depth, n_fits, ctx->stream));
    PSK_HIP(ctx, crit.upload(fit_criterion, n_fits, ctx->stream));
    PSK_HIP(ctx, d_fit_fold.upload(fit_fold, n_fits, ctx->stream));
    PSK_HIP(ctx, d_off.upload(off.data(), n_fits, ctx->stream));
    PSK_HIP(ctx, count.alloc(n_fits));
    PSK_HIP(ctx, dout.alloc(n_fits));
    PSK_HIP(ctx, d_nodes.alloc(total * TREE_NODE_FIELDS));
    PSK_HIP(ctx, d_imp.alloc(total));
    PSK_HIP(ctx, leaf.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, frac.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, d_thr.alloc(COUNTS ? total : 0));
    // (the count kernel scans the P planes where the 0/1 kernel scans the p columns)
    const uint64_t *d_bits = COUNTS ? (const uint64_t *)pl.bits : (const uint64_t *)bits;
    tree_fit_kernel<COUNTS><<<n_fits, TREE_THREADS, 0, ctx->stream>>>(d_bits, ymask, d_fold, n, COUNTS ? pl.P : p, W, depth,
                                                                      crit, d_fit_fold, count, dout, d_nodes, d_imp, leaf, frac, d_off,
                                                                      pv, d_thr);
    PSK_HIP(ctx, hipGetLastError());
    std::vector<int32_t> nodes(total * TREE_NODE_FIELDS);
    std::vector<double> imp(total), thr(COUNTS ? total : 0);
    if (COUNTS) PSK_HIP(ctx, d_thr.download(thr.data(), thr.size(), ctx->stream));
    PSK_HIP(ctx, count.download(node_count_out, n_fits, ctx->stream));
    PSK_HIP(ctx, dout.download(max_depth_out, n_fits, ctx->stream));
    PSK_HIP(ctx, d_nodes.download(nodes.data(), nodes.size(), ctx->stream));
    PSK_HIP(ctx, d_imp.download(imp.data(), imp.size(), ctx->stream));
    PSK_HIP(ctx, leaf.download(leaf_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, frac.download(frac_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < n_fits; f++) {
        const size_t k = (size_t)node_count_out[f];
        tree_report_impurities(fit_criterion[f], nodes.data() + (size_t)off[f] * TREE_NODE_FIELDS, (int)k, imp.data() + off[f]);
        memcpy(nodes_out + (size_t)f * PSK_TREE_NODE_CAP * TREE_NODE_FIELDS, nodes.data() + (size_t)off[f] * TREE_NODE_FIELDS,
               k * TREE_NODE_FIELDS * 4);
        memcpy(impurity_out + (size_t)f * PSK_TREE_NODE_CAP, imp.data() + off[f], k * 8);
        if (COUNTS) memcpy(threshold_out + (size_t)f * PSK_TREE_NODE_CAP, thr.data() + off[f], k * 8);
    }
    return PSK_OK;
}

}  // namespace

extern "C" int psk_tree_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                            const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                            int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                            int32_t *leaf_out, double *frac_out)
{
    return tree_fit_call<false>(ctx, "psk_tree_fit", X, y01, n, p, fold, fit_max_depth, fit_criterion, fit_fold, n_fits, node_count_out,
                                max_depth_out, nodes_out, impurity_out, leaf_out, frac_out, nullptr);
}

extern "C" int psk_tree_fit_counts(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                                   const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                                   int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                                   int32_t *leaf_out, double *frac_out, double *threshold_out)
{
    return tree_fit_call<true>(ctx, "psk_tree_fit_counts", X, y01, n, p, fold, fit_max_depth, fit_criterion, fit_fold, n_fits,
                               node_count_out, max_depth_out, nodes_out, impurity_out, leaf_out, frac_out, threshold_out);
}
