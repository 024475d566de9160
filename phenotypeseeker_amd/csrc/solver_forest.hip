// Random-forest fits of the reference's `-bc RF` branch: RandomizedSearchCV(RandomForestClassifier(), grid, n_iter, cv) over
// the seven-key grid of set_model (modeling.py:1030-1031, :1057-1068, :1096-1099).  The contract is scikit-learn 1.7.2's forest
// for a GIVEN seed, to the node: the host draws everything NumPy's RandomState draws (tree seeds, the
// bootstrap multiplicities, the splitter's generator state) and this unit builds the trees, running only the 32-bit xorshift
// of sklearn/utils/_random.pxd::our_rand_r.  The packed design, the impurity expressions and the node record are the decision
// tree's (solver_tree_common.h).  What differs from its tree:
//   * a sample carries an integer weight (its bootstrap multiplicity; 0 = not in the tree, which is also how a held-out fold is
//     expressed).  n_node_samples counts DISTINCT in-bag samples, class counts / impurities / proxies use the weights
//   * a node visits a random subset of the columns: _splitter.pyx::node_split_best's Fisher-Yates walk over features[] with its
//     n_known / n_drawn / n_found constant bookkeeping and the two memcpy's through constant_features[]; both arrays persist
//     across the nodes of a tree, a node hands its n_total_constants to both children.  The best split is the FIRST in visit
//     order with a strictly larger proxy (no lowest-index rule).  The generator advances only in nodes that reach the search
//   * min_samples_leaf (on distinct in-bag samples: a column whose split leaves fewer on a side is visited but offers no
//     split), min_samples_split, and no bound on the depth
// Leaf rules and pre-order numbering are the decision tree's, with weighted counts in place of counts;
// improvement = (w_node / w_tree) (I - w_r / w_node I_r - w_l / w_node I_l).  f64, no FMA fusion.
//
// One workgroup builds one tree at a time (a persistent grid strides over the trees).  In LDS (all of it in the dynamic region,
// laid out by the host, ForestLds): the weights as bit planes (as many as the call's largest weight needs, so a weighted count
// is sum_b 2^b popcount(column & node & plane_b [& label])), a 16-bit label per sample naming the pending node it belongs to --
// the node's slot on the depth-first stack, so memory does not grow with depth -- from which the current node's masks are
// rebuilt by ballots, and per column the walk's inputs (distinct / weighted / weighted class-1 right counts, proxy) next to
// features[] / constant_features[]; past FOREST_LDS_COLS columns those per-column arrays live in global memory instead (the
// same code through generic pointers).  Per node every thread fills the per-column results, one column per thread and
// round, then ONE lane walks scikit-learn's draw loop over them: each draw's range depends on what the draws before it found,
// so the walk is sequential by construction.  The stack itself (a record per pending node, at most in-bag samples + 1) is in
// global memory, written and read by that one lane.
// Per tree, every sample's two leaf fractions go to scratch; forest_sum_kernel adds them per fit IN TREE ORDER (the order of a
// f64 sum is part of the contract: no atomics).  Node arrays are written only for the trees the caller flags.
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

// 4 waves: a search is tens of thousands of trees and the one-lane walk leaves the other lanes idle, so residency comes from
// several small workgroups per compute unit (LDS: ~35 KB at 2,048 x 1,000 with 3 planes -> 4 per compute unit) rather than
// from a wide one.
constexpr int FOREST_THREADS = 256;
constexpr int FOREST_MAX_N = 4096;
constexpr int FOREST_LDS_COLS = 1024;      // per-column arrays stay in LDS up to this many columns
constexpr int FOREST_COL_BYTES = 28;       // proxy f64, features / constant_features / state / w_r / w_r1 i32
constexpr int FOREST_COL_BYTES_COUNTS = 32;   // on a count design also the column's best plane, i32
constexpr int FOREST_LDS_BYTES = 64 << 10;    // what a launch may ask for without opting in to more
constexpr int FOREST_GRID_PER_CU = 4;
constexpr uint32_t FOREST_NO_LABEL = 0xffff;
constexpr int COL_CONSTANT = -1, COL_NO_SPLIT = -2;

// a pending node: its parent, level, side, distinct / weighted / weighted class-1 in-bag samples, the constants known on the
// way down, and the impurity its parent's split computed for it
struct ForestRec { int parent, depth, is_left, n, wn, w1, n_const, pad; double imp; };

// byte offsets into the dynamic LDS region (every one a multiple of 16) and the region's size
struct ForestLds { int label, planes, mp, mpy, T, Y, MT, cur, walk, cols, total; };

struct ForestArgs {
    const uint64_t *bits, *ymask;
    int n, p, W, B, n_trees, cols_in_lds;
    const uint16_t *tree_weight;
    const uint32_t *tree_state;
    const int32_t *tree_fit, *fit_crit, *fit_depth, *fit_mf, *fit_msl, *fit_mss;
    const int64_t *tree_node_off;      // first slot of the tree in the node pool, -1: not exported
    const int32_t *tree_node_cap, *tree_leaf_row;
    int32_t *node_count, *depth_out, *nodes, *leaf_out;
    double *imp_out, *frac0, *frac1;
    ForestRec *stack;                  // [grid][n + 2]
    char *cols_global;                 // [grid][FOREST_COL_BYTES * p_pad] when the columns do not fit LDS
    ForestLds lds;
};

// what forest_fit_kernel<true> takes besides: on a count design ForestArgs::bits holds the P threshold planes
// (solver_tree_common.h).  Empty for the 0/1 kernel, whose arguments and code stay what they were.
template <bool COUNTS> struct ForestCountArgs {};
template <> struct ForestCountArgs<true> {
    TreePlaneView<true> pv;
    int P;
    double *thr_out;                   // by node slot, as imp_out
};

__device__ __forceinline__ void swap_int(int *a, int i, int j) { const int t = a[i]; a[i] = a[j]; a[j] = t; }

// COUNTS: a thread walks the planes of its column in ascending order and keeps the first strictly larger proxy among the gaps
// between the values present in the node (a plane whose right count equals the plane's before it repeats that partition), so
// the one-lane walk sees per column what it saw on a 0/1 design: constant, no split, or one best split.
template <bool COUNTS> __global__ __launch_bounds__(FOREST_THREADS) void forest_fit_kernel(const ForestArgs a,
                                                                                           const ForestCountArgs<COUNTS> ca)
{
    constexpr int COL_BYTES = COUNTS ? FOREST_COL_BYTES_COUNTS : FOREST_COL_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = a.n, p = a.p, W = a.W, B = a.B, Wn = W * 64;
    uint16_t *label = (uint16_t *)(smem + a.lds.label);
    uint64_t *planes = (uint64_t *)(smem + a.lds.planes), *MP = (uint64_t *)(smem + a.lds.mp), *MPY = (uint64_t *)(smem + a.lds.mpy);
    uint64_t *T = (uint64_t *)(smem + a.lds.T), *Y = (uint64_t *)(smem + a.lds.Y), *MT = (uint64_t *)(smem + a.lds.MT);
    ForestRec *cur = (ForestRec *)(smem + a.lds.cur);
    int *walk = (int *)(smem + a.lds.walk);     // best column, n_known, n_found of the node's walk
    const int p_pad = (p + 3) & ~3;
    char *cols = a.cols_in_lds ? smem + a.lds.cols : a.cols_global + (size_t)blockIdx.x * COL_BYTES * p_pad;
    double *proxy = (double *)cols;
    int *features = (int *)(cols + 8 * (size_t)p_pad), *constant = features + p_pad, *col_state = constant + p_pad;
    int *col_wr = col_state + p_pad, *col_wr1 = col_wr + p_pad;
    int *col_plane = COUNTS ? col_wr1 + p_pad : nullptr;   // the column's best plane
    int bit_cols = p;                   // the second dimension of a.bits
    if constexpr (COUNTS) bit_cols = ca.P;
    ForestRec *stack = a.stack + (size_t)blockIdx.x * (n + 2);

    for (int tree = blockIdx.x; tree < a.n_trees; tree += gridDim.x) {
        const int fit = a.tree_fit[tree];
        const int crit = a.fit_crit[fit], max_depth = a.fit_depth[fit] > 0 ? a.fit_depth[fit] : INT_MAX, max_features = a.fit_mf[fit];
        const int msl = a.fit_msl[fit], mss = a.fit_mss[fit];
        const int64_t node_off = a.tree_node_off[tree];
        const int node_cap = a.tree_node_cap[tree], leaf_row = a.tree_leaf_row[tree];
        const uint16_t *wt = a.tree_weight + (size_t)tree * n;
        uint32_t rng = a.tree_state[tree];   // lane 0's copy is the one that advances
        __syncthreads();                      // the tree before is done with LDS
        for (int s0 = 0; s0 < Wn; s0 += FOREST_THREADS) {
            const int s = s0 + tid;
            const uint32_t wv = s < n ? wt[s] : 0u;
            const uint64_t inbag = __ballot(wv != 0);
            if (s < Wn) label[s] = s < n ? 0 : FOREST_NO_LABEL;
            for (int b = 0; b < B; b++) {
                const uint64_t pl = __ballot((wv >> b) & 1u);
                if (lane == 0 && s < Wn) planes[b * W + (s >> 6)] = pl;
            }
            if (lane == 0 && s < Wn) { T[s >> 6] = inbag; Y[s >> 6] = a.ymask[s >> 6]; }
        }
        for (int j = tid; j < p; j += FOREST_THREADS) { features[j] = j; constant[j] = 0; }
        __syncthreads();
        int n_tot = 0, w_tot = 0, w1_tot = 0;
        for (int w = 0; w < W; w++) {
            n_tot += __popcll(T[w]);
            for (int b = 0; b < B; b++) {
                w_tot += __popcll(planes[b * W + w]) << b;
                w1_tot += __popcll(planes[b * W + w] & Y[w]) << b;
            }
        }
        const double w_tree = (double)w_tot;
        if (tid == 0)
            stack[0] = ForestRec{-1, 0, 0, n_tot, w_tot, w1_tot, 0, 0, tree_impurity(crit, (double)(w_tot - w1_tot), (double)w1_tot, w_tree)};
        int sp = 1, next_id = 0, deepest = 0;
        while (sp > 0) {
            __syncthreads();   // labels, per-column arrays and `cur` of the node before
            --sp;
            if (tid == 0) *cur = stack[sp];
            __syncthreads();
            const ForestRec rec = *cur;
            const uint32_t slot = (uint32_t)sp;
            for (int s0 = 0; s0 < Wn; s0 += FOREST_THREADS) {
                const int s = s0 + tid;
                const uint64_t m = __ballot(s < Wn && label[s] == slot);
                if (lane == 0 && s < Wn) {
                    const int w = s >> 6;
                    MT[w] = m & T[w];
                    for (int b = 0; b < B; b++) {
                        const uint64_t mp = m & planes[b * W + w];
                        MP[b * W + w] = mp;
                        MPY[b * W + w] = mp & Y[w];
                    }
                }
            }
            __syncthreads();
            const double wn = (double)rec.wn, c1n = (double)rec.w1, c0n = (double)(rec.wn - rec.w1);
            bool is_leaf = rec.depth >= max_depth || rec.n < mss || rec.n < 2 * msl || rec.imp <= DBL_EPSILON;
            int feat = -2, nr = 0, wr = 0, wr1 = 0, n_const = rec.n_const;
            double imp_l = 0.0, imp_r = 0.0;
            if (!is_leaf) {
                if constexpr (COUNTS) {
                    for (int i = tid; i < p; i += FOREST_THREADS) {
                        const int j = ca.pv.col_order[i];
                        int st = COL_CONSTANT, prev = rec.n, bq = -1, bcw = 0, bcw1 = 0;
                        double bp = -INFINITY;
                        for (int q = ca.pv.col_first[j]; q < ca.pv.col_first[j + 1]; q++) {
                            int c = 0;
                            for (int w = 0; w < W; w++)
                                if (MT[w]) c += __popcll(a.bits[tree_bit_at(q, w, bit_cols)] & MT[w]);
                            if (c == 0) break;   // (the planes above hold no sample of the node either)
                            if (c == prev) continue;
                            prev = c;
                            if (st == COL_CONSTANT) st = COL_NO_SPLIT;
                            if (rec.n - c < msl || c < msl) continue;
                            int cw = 0, cw1 = 0;
                            for (int w = 0; w < W; w++) {
                                if (!MT[w]) continue;
                                const uint64_t v = a.bits[tree_bit_at(q, w, bit_cols)];
                                for (int b = 0; b < B; b++) {
                                    cw += __popcll(v & MP[b * W + w]) << b;
                                    cw1 += __popcll(v & MPY[b * W + w]) << b;
                                }
                            }
                            const double dwr = (double)cw, dwl = (double)(rec.wn - cw);
                            const double ir = tree_impurity(crit, (double)(cw - cw1), (double)cw1, dwr);
                            const double il = tree_impurity(crit, c0n - (double)(cw - cw1), c1n - (double)cw1, dwl);
                            const double v = -dwr * ir - dwl * il;
                            if (v > bp) { bp = v; bq = q; st = c; bcw = cw; bcw1 = cw1; }
                        }
                        if (bq >= 0) proxy[j] = bp;
                        col_state[j] = st;
                        col_wr[j] = bcw;
                        col_wr1[j] = bcw1;
                        col_plane[j] = bq;
                    }
                } else {
                    for (int j = tid; j < p; j += FOREST_THREADS) {
                        int c = 0, cw = 0, cw1 = 0;
                        for (int w = 0; w < W; w++) {
                            const uint64_t m = MT[w];
                            if (!m) continue;   // (uniform: the mask words are the workgroup's)
                            const uint64_t v = a.bits[tree_bit_at(j, w, p)];
                            c += __popcll(v & m);
                            for (int b = 0; b < B; b++) {
                                cw += __popcll(v & MP[b * W + w]) << b;
                                cw1 += __popcll(v & MPY[b * W + w]) << b;
                            }
                        }
                        int st = c;
                        if (c == 0 || c == rec.n) st = COL_CONSTANT;
                        else if (rec.n - c < msl || c < msl) st = COL_NO_SPLIT;
                        else {
                            const double dwr = (double)cw, dwl = (double)(rec.wn - cw);
                            const double ir = tree_impurity(crit, (double)(cw - cw1), (double)cw1, dwr);
                            const double il = tree_impurity(crit, c0n - (double)(cw - cw1), c1n - (double)cw1, dwl);
                            proxy[j] = -dwr * ir - dwl * il;
                        }
                        col_state[j] = st;
                        col_wr[j] = cw;
                        col_wr1[j] = cw1;
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    // node_split_best's draw loop, statement for statement
                    int f_i = p, n_visited = 0, n_found = 0, n_drawn = 0;
                    const int n_known = rec.n_const;
                    int n_total = n_known, best = -1;
                    double best_proxy = -INFINITY;
                    while (f_i > n_total && (n_visited < max_features || n_visited <= n_found + n_drawn)) {
                        n_visited++;
                        if (rng == 0) rng = 1;
                        rng ^= rng << 13;
                        rng ^= rng >> 17;
                        rng ^= rng << 5;
                        int f_j = n_drawn + (int)((rng & 0x7fffffffu) % (uint32_t)(f_i - n_found - n_drawn));
                        if (f_j < n_known) {
                            swap_int(features, n_drawn, f_j);
                            n_drawn++;
                            continue;
                        }
                        f_j += n_found;
                        const int col = features[f_j], st = col_state[col];
                        if (st == COL_CONSTANT) {
                            swap_int(features, f_j, n_total);
                            n_found++;
                            n_total++;
                            continue;
                        }
                        f_i--;
                        swap_int(features, f_i, f_j);
                        if (st == COL_NO_SPLIT) continue;
                        const double v = proxy[col];
                        if (v > best_proxy) { best_proxy = v; best = col; }
                    }
                    walk[0] = best;
                    walk[1] = n_known;
                    walk[2] = n_found;
                }
                __syncthreads();
                const int best = walk[0], n_known = walk[1], n_found = walk[2];
                // the two memcpy's: features[:n_known] = constant[:n_known]; constant[n_known:+n_found] = features[n_known:+n_found]
                // (disjoint ranges of both arrays, so the copies may run side by side)
                for (int k = tid; k < n_known; k += FOREST_THREADS) features[k] = constant[k];
                for (int k = tid; k < n_found; k += FOREST_THREADS) constant[n_known + k] = features[n_known + k];
                n_const = n_known + n_found;
                if (best < 0) {
                    is_leaf = true;
                } else {
                    nr = col_state[best];
                    wr = col_wr[best];
                    wr1 = col_wr1[best];
                    const double dwr = (double)wr, dwl = (double)(rec.wn - wr);
                    imp_r = tree_impurity(crit, (double)(wr - wr1), (double)wr1, dwr);
                    imp_l = tree_impurity(crit, c0n - (double)(wr - wr1), c1n - (double)wr1, dwl);
                    const double improvement = (wn / w_tree) * (rec.imp - (dwr / wn * imp_r) - (dwl / wn * imp_l));
                    if (improvement + DBL_EPSILON < 0.0) is_leaf = true;
                    else feat = best;
                }
            }
            const int id = next_id++;
            deepest = max(deepest, rec.depth);
            int route = feat;
            if constexpr (COUNTS) {
                double thr = -2.0;
                if (!is_leaf) {
                    thr = tree_node_threshold(ca.pv.X, n, p, feat, ca.pv.plane_val[col_plane[feat]], MT, walk);
                    route = tree_route_plane(ca.pv.col_first, ca.pv.plane_val, feat, thr);
                }
                if (tid == 0 && node_off >= 0 && id < node_cap) ca.thr_out[node_off + id] = thr;
            }
            if (tid == 0 && node_off >= 0 && id < node_cap)
                tree_write_node(a.nodes + (size_t)node_off * TREE_NODE_FIELDS, a.imp_out + node_off, id, rec.parent, rec.is_left, feat, is_leaf,
                                rec.n, rec.wn - rec.w1, rec.w1, rec.imp);
            if (is_leaf) {
                const double f0 = c0n / wn, f1 = c1n / wn;
                for (int s = tid; s < n; s += FOREST_THREADS)
                    if (label[s] == slot) {
                        a.frac0[(size_t)tree * n + s] = f0;
                        a.frac1[(size_t)tree * n + s] = f1;
                        if (leaf_row >= 0) a.leaf_out[(size_t)leaf_row * n + s] = id;
                        label[s] = FOREST_NO_LABEL;
                    }
            } else {
                // the right child takes this node's slot, the left one the slot above it: popped first
                for (int s = tid; s < n; s += FOREST_THREADS)
                    if (label[s] == slot && !((a.bits[tree_bit_at(route, s >> 6, bit_cols)] >> (s & 63)) & 1ull)) label[s] = (uint16_t)(slot + 1);
                if (tid == 0) {
                    stack[sp] = ForestRec{id, rec.depth + 1, 0, nr, wr, wr1, n_const, 0, imp_r};
                    stack[sp + 1] = ForestRec{id, rec.depth + 1, 1, rec.n - nr, rec.wn - wr, rec.w1 - wr1, n_const, 0, imp_l};
                }
                sp += 2;
            }
        }
        if (tid == 0) { a.node_count[tree] = next_id; a.depth_out[tree] = deepest; }
    }
}

// sum0[f][s], sum1[f][s]: the leaf fractions of fit f's trees added one after the other in tree order
__global__ __launch_bounds__(256) void forest_sum_kernel(const double *__restrict__ frac0, const double *__restrict__ frac1, int n,
                                                         const int32_t *__restrict__ fit_ptr, const int32_t *__restrict__ fit_trees,
                                                         double *__restrict__ sum0, double *__restrict__ sum1)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (s >= n) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = fit_ptr[f]; k < fit_ptr[f + 1]; k++) {
        const size_t at = (size_t)fit_trees[k] * n + s;
        s0 += frac0[at];
        s1 += frac1[at];
    }
    sum0[(size_t)f * n + s] = s0;
    sum1[(size_t)f * n + s] = s1;
}

int align16(int v) { return (v + 15) & ~15; }

// the LDS region for a call of W words, B planes and p columns; the per-column arrays go last and are left out (cols_in_lds
// = 0) past FOREST_LDS_COLS columns, or where they would take the region past FOREST_LDS_BYTES
ForestLds forest_lds_layout(int W, int B, int p, int col_bytes, int *cols_in_lds)
{
    ForestLds l{};
    int at = 0;
    l.label = at; at = align16(at + 2 * 64 * W);
    l.planes = at; at = align16(at + 8 * B * W);
    l.mp = at; at = align16(at + 8 * B * W);
    l.mpy = at; at = align16(at + 8 * B * W);
    l.T = at; at = align16(at + 8 * W);
    l.Y = at; at = align16(at + 8 * W);
    l.MT = at; at = align16(at + 8 * W);
    l.cur = at; at = align16(at + (int)sizeof(ForestRec));
    l.walk = at; at = align16(at + 16);
    l.cols = at;
    const int with_cols = align16(at + col_bytes * ((p + 3) & ~3));
    *cols_in_lds = p <= FOREST_LDS_COLS && with_cols <= FOREST_LDS_BYTES;
    if (*cols_in_lds) at = with_cols;
    l.total = at;
    return l;
}

// psk_forest_fit (COUNTS false: threshold_out unused) and psk_forest_fit_counts; `who` names the entry point in messages
template <bool COUNTS>
int forest_fit_call(psk_ctx *ctx, const char *who, const float *X, const int32_t *y01, int n, int p, int n_trees,
                    const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit, const int32_t *tree_export,
                    int n_fits, const int32_t *fit_criterion, const int32_t *fit_max_depth, const int32_t *fit_max_features,
                    const int32_t *fit_min_samples_leaf, const int32_t *fit_min_samples_split, double *sum0_out, double *sum1_out,
                    int32_t *node_count_out, int32_t *max_depth_out, int64_t node_pool, int64_t *tree_node_off_out, int32_t *nodes_out,
                    double *impurity_out, int32_t *leaf_out, double *threshold_out)
{
    constexpr int COL_BYTES = COUNTS ? FOREST_COL_BYTES_COUNTS : FOREST_COL_BYTES;
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !tree_weight || !tree_state || !tree_fit || !tree_export || !fit_criterion || !fit_max_depth ||
        !fit_max_features || !fit_min_samples_leaf || !fit_min_samples_split || !sum0_out || !sum1_out || !node_count_out ||
        !max_depth_out || !tree_node_off_out)
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (n < 1 || p < 1 || n_fits < 1 || n_trees < 1)
        return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d trees=%d", n, p, n_fits, n_trees);
    if (n > FOREST_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s keeps a label per sample in LDS: at most %d samples, got %d", who, FOREST_MAX_N, n);
    for (int f = 0; f < n_fits; f++) {
        if (fit_criterion[f] != 0 && fit_criterion[f] != 1)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: criterion must be 0 (gini) or 1 (entropy), got %d", f, fit_criterion[f]);
        if (fit_max_depth[f] < 0 || fit_max_features[f] < 1 || fit_max_features[f] > p || fit_min_samples_leaf[f] < 1 ||
            fit_min_samples_split[f] < 2)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: max_depth %d (0 = none), max_features %d (1..%d), min_samples_leaf %d (>= 1), "
                            "min_samples_split %d (>= 2)", f, fit_max_depth[f], fit_max_features[f], p, fit_min_samples_leaf[f],
                            fit_min_samples_split[f]);
    }
    // per fit its trees in ascending order; per exported tree its share of the node pool: at most 2 (in-bag samples) - 1 nodes
    std::vector<int32_t> fit_ptr((size_t)n_fits + 1, 0), fit_trees(n_trees), node_cap(n_trees, 0), leaf_row(n_trees, -1);
    std::vector<int64_t> node_off(n_trees, -1);
    int64_t pool = 0;
    int n_export = 0;
    uint32_t w_max = 0;
    for (int t = 0; t < n_trees; t++) {
        if (tree_fit[t] < 0 || tree_fit[t] >= n_fits) return psk_fail(ctx, PSK_EINVAL, "tree %d: fit %d of %d", t, tree_fit[t], n_fits);
        fit_ptr[tree_fit[t] + 1]++;
        int inbag = 0;
        int64_t w_sum = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t w = tree_weight[(size_t)t * n + i];
            inbag += w != 0;
            w_sum += w;
            w_max = std::max(w_max, w);
        }
        if (!inbag) return psk_fail(ctx, PSK_EINVAL, "tree %d has no training sample", t);
        if (w_sum > INT32_MAX) return psk_fail(ctx, PSK_ERANGE, "tree %d: the weights add up to more than 2^31 - 1", t);
        if (tree_export[t]) {
            node_off[t] = pool;
            node_cap[t] = 2 * inbag - 1;
            leaf_row[t] = n_export++;
            pool += node_cap[t];
        }
    }
    if (n_export && (!nodes_out || !impurity_out || !leaf_out || (COUNTS && !threshold_out))) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (pool > node_pool)
        return psk_fail(ctx, PSK_ERANGE, "the exported trees may need %lld node slots (2 x in-bag samples - 1 each), the pool has %lld",
                        (long long)pool, (long long)node_pool);
    for (int f = 0; f < n_fits; f++) fit_ptr[f + 1] += fit_ptr[f];
    {
        std::vector<int32_t> at(fit_ptr.begin(), fit_ptr.end() - 1);
        for (int t = 0; t < n_trees; t++) fit_trees[at[tree_fit[t]]++] = t;
    }
    int B = 1;
    while ((w_max >> B) != 0) B++;

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    FitArr<uint64_t> bits, ymask;
    TreePlanes pl;
    if constexpr (COUNTS) {
        if (const int rc = tree_pack_counts(ctx, who, X, y01, n, p, pl, ymask)) return rc;
    } else {
        if (const int rc = tree_pack_design(ctx, who, X, y01, n, p, bits, ymask)) return rc;
    }

    const int grid = std::min(n_trees, FOREST_GRID_PER_CU * (ctx->n_cu > 0 ? ctx->n_cu : 256));
    ForestArgs a{};
    a.lds = forest_lds_layout(W, B, p, COL_BYTES, &a.cols_in_lds);
    const size_t p_pad = ((size_t)p + 3) & ~(size_t)3;
    FitArr<uint16_t> d_weight;
    FitArr<uint32_t> d_state;
    FitArr<int32_t> d_tree_fit, d_crit, d_depth, d_mf, d_msl, d_mss, d_cap, d_leaf_row, d_count, d_deepest, d_nodes, d_leaf, d_fit_ptr,
        d_fit_tree_ids;
    FitArr<int64_t> d_off;
    FitArr<double> d_imp, d_thr, frac0, frac1, sum0, sum1;
    FitArr<ForestRec> d_stack;
    FitArr<char> d_cols;
    PSK_HIP(ctx, d_weight.upload(tree_weight, (size_t)n_trees * n, ctx->stream));
    PSK_HIP(ctx, d_state.upload(tree_state, n_trees, ctx->stream));
    PSK_HIP(ctx, d_tree_fit.upload(tree_fit, n_trees, ctx->stream));
    PSK_HIP(ctx, d_crit.upload(fit_criterion, n_fits, ctx->stream));
    PSK_HIP(ctx, d_depth.upload(fit_max_depth, n_fits, ctx->stream));
    PSK_HIP(ctx, d_mf.upload(fit_max_features, n_fits, ctx->stream));
    PSK_HIP(ctx, d_msl.upload(fit_min_samples_leaf, n_fits, ctx->stream));
    PSK_HIP(ctx, d_mss.upload(fit_min_samples_split, n_fits, ctx->stream));
    PSK_HIP(ctx, d_off.upload(node_off, ctx->stream));
    PSK_HIP(ctx, d_cap.upload(node_cap, ctx->stream));
    PSK_HIP(ctx, d_leaf_row.upload(leaf_row, ctx->stream));
    PSK_HIP(ctx, d_fit_ptr.upload(fit_ptr, ctx->stream));
    PSK_HIP(ctx, d_fit_tree_ids.upload(fit_trees, ctx->stream));
    PSK_HIP(ctx, d_count.alloc(n_trees));
    PSK_HIP(ctx, d_deepest.alloc(n_trees));
    PSK_HIP(ctx, d_nodes.alloc((size_t)pool * TREE_NODE_FIELDS));
    PSK_HIP(ctx, d_imp.alloc((size_t)pool));
    PSK_HIP(ctx, d_leaf.alloc((size_t)n_export * n));
    PSK_HIP(ctx, frac0.alloc((size_t)n_trees * n));
    PSK_HIP(ctx, frac1.alloc((size_t)n_trees * n));
    PSK_HIP(ctx, sum0.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, sum1.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, d_stack.alloc((size_t)grid * (n + 2)));
    PSK_HIP(ctx, d_cols.alloc(a.cols_in_lds ? 0 : (size_t)grid * COL_BYTES * p_pad));
    PSK_HIP(ctx, d_thr.alloc(COUNTS ? (size_t)pool : 0));
    a.bits = COUNTS ? (const uint64_t *)pl.bits : (const uint64_t *)bits; a.ymask = ymask;
    ForestCountArgs<COUNTS> ca;
    if constexpr (COUNTS) ca = ForestCountArgs<true>{{pl.x, pl.col_first, pl.plane_col, pl.col_order, pl.plane_val, p}, pl.P, d_thr};
    a.n = n; a.p = p; a.W = W; a.B = B; a.n_trees = n_trees;
    a.tree_weight = d_weight; a.tree_state = d_state; a.tree_fit = d_tree_fit;
    a.fit_crit = d_crit; a.fit_depth = d_depth; a.fit_mf = d_mf; a.fit_msl = d_msl; a.fit_mss = d_mss;
    a.tree_node_off = d_off; a.tree_node_cap = d_cap; a.tree_leaf_row = d_leaf_row;
    a.node_count = d_count; a.depth_out = d_deepest; a.nodes = d_nodes; a.leaf_out = d_leaf;
    a.imp_out = d_imp; a.frac0 = frac0; a.frac1 = frac1;
    a.stack = d_stack; a.cols_global = d_cols;
    forest_fit_kernel<COUNTS><<<grid, FOREST_THREADS, a.lds.total, ctx->stream>>>(a, ca);
    PSK_HIP(ctx, hipGetLastError());
    forest_sum_kernel<<<dim3(div_up(n, 256), n_fits), 256, 0, ctx->stream>>>(frac0, frac1, n, d_fit_ptr, d_fit_tree_ids, sum0, sum1);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, sum0.download(sum0_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, sum1.download(sum1_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, d_count.download(node_count_out, n_trees, ctx->stream));
    PSK_HIP(ctx, d_deepest.download(max_depth_out, n_trees, ctx->stream));
    if (n_export) {
        PSK_HIP(ctx, d_nodes.download(nodes_out, (size_t)pool * TREE_NODE_FIELDS, ctx->stream));
        PSK_HIP(ctx, d_imp.download(impurity_out, (size_t)pool, ctx->stream));
        PSK_HIP(ctx, d_leaf.download(leaf_out, (size_t)n_export * n, ctx->stream));
        if (COUNTS) PSK_HIP(ctx, d_thr.download(threshold_out, (size_t)pool, ctx->stream));
    }
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n_trees; t++)
        if (node_off[t] >= 0)
            tree_report_impurities(fit_criterion[tree_fit[t]], nodes_out + (size_t)node_off[t] * TREE_NODE_FIELDS,
                                   std::min(node_count_out[t], node_cap[t]), impurity_out + node_off[t]);
    memcpy(tree_node_off_out, node_off.data(), (size_t)n_trees * sizeof(int64_t));
    return PSK_OK;
}

}  // namespace

extern "C" int psk_forest_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                              const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                              const int32_t *tree_export, int n_fits, const int32_t *fit_criterion, const int32_t *fit_max_depth,
                              const int32_t *fit_max_features, const int32_t *fit_min_samples_leaf,
                              const int32_t *fit_min_samples_split, double *sum0_out, double *sum1_out, int32_t *node_count_out,
                              int32_t *max_depth_out, int64_t node_pool, int64_t *tree_node_off_out, int32_t *nodes_out,
                              double *impurity_out, int32_t *leaf_out)
{
    return forest_fit_call<false>(ctx, "psk_forest_fit", X, y01, n, p, n_trees, tree_weight, tree_state, tree_fit, tree_export, n_fits,
                                  fit_criterion, fit_max_depth, fit_max_features, fit_min_samples_leaf, fit_min_samples_split, sum0_out,
                                  sum1_out, node_count_out, max_depth_out, node_pool, tree_node_off_out, nodes_out, impurity_out, leaf_out,
                                  nullptr);
}

extern "C" int psk_forest_fit_counts(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                                     const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                                     const int32_t *tree_export, int n_fits, const int32_t *fit_criterion,
                                     const int32_t *fit_max_depth, const int32_t *fit_max_features,
                                     const int32_t *fit_min_samples_leaf, const int32_t *fit_min_samples_split, double *sum0_out,
                                     double *sum1_out, int32_t *node_count_out, int32_t *max_depth_out, int64_t node_pool,
                                     int64_t *tree_node_off_out, int32_t *nodes_out, double *impurity_out, int32_t *leaf_out,
                                     double *threshold_out)
{
    return forest_fit_call<true>(ctx, "psk_forest_fit_counts", X, y01, n, p, n_trees, tree_weight, tree_state, tree_fit, tree_export,
                                 n_fits, fit_criterion, fit_max_depth, fit_max_features, fit_min_samples_leaf, fit_min_samples_split,
                                 sum0_out, sum1_out, node_count_out, max_depth_out, node_pool, tree_node_off_out, nodes_out, impurity_out,
                                 leaf_out, threshold_out);
}
