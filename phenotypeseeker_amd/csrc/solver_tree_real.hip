// Tree and forest fits on a REAL-VALUED design (psk_tree_fit_real, psk_forest_fit_real): the reference fits its `-bc DT` / `-bc RF`
// models on whatever ML_df holds, and under --pca that is the matrix of kept principal-component scores (modeling.py:1204, then
// set_model :1030-1033).  The contract is the count calls' (solver_tree.hip, solver_forest.hip: scikit-learn 1.7.2 to the node),
// with the search inside a column restated for columns whose values are nearly all distinct:
//   * any two float32 values that compare different are different values: a column is constant in a node when its in-bag values
//     all compare equal, and a candidate is every place where the sorted in-bag values change (hi > lo as floats).  -0.0 and +0.0
//     compare equal and make no gap (the sort key is taken of x with -0.0 replaced by +0.0, and the gap test compares floats)
//   * the threshold is (double)lo / 2.0 + (double)hi / 2.0, replaced by (double)lo if that equals (double)hi or is infinite;
//     (float32)x <= threshold goes left for every sample of the design, held-out and weight-0 ones included
//   * inside a column the first strictly larger proxy in ascending order wins
// A score column has about n distinct values, so the threshold planes of the count calls (one per gap) would cost about n x p
// planes.  Here every column is sorted ONCE per call (real_sort_kernel: a bitonic network over (value, sample) keys in LDS, one
// workgroup per column) into order[r][j], the sample of rank r in column j (u16), and sval[r][j], its value; both rank-major, so
// the threads of a wave, which hold consecutive columns, read contiguous memory (the point of tree_bit_at's layout).  Device
// memory besides the float design is 6 n p bytes, whatever the values.  Per node a thread walks its column's order from the
// lowest rank, keeps the samples that are in the node and in the bag, and accumulates distinct / weighted / class-1 sums on the
// left side; it stops at the node's last sample.  The walk's trip count is up to n whatever the node's size;
// where the columns are fewer than half the threads (--pca keeps a few components) a column's ranks are cut into segments, a
// thread each, so that the trip count is n over the number of segments, taken twice.
// The impurity and proxy expressions, the node record and the leaf rules are solver_tree_common.h's; f64, no FMA fusion.
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

constexpr int REAL_MAX_N = 4096;
constexpr int REAL_MAX_W = REAL_MAX_N / 64;
constexpr int REAL_SORT_THREADS = 256;

// ---- the sort of every column, once per call ----

// a key that orders as the float does: sign-magnitude to biased; x is finite and -0.0 has been replaced by +0.0
__device__ __forceinline__ uint32_t real_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float real_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// One workgroup sorts column blockIdx.x: keys (value << 16 | sample) in LDS, n2 = the power of two at or above n, the tail
// padded with the largest key.  The sample in the low bits makes the order total, so the result does not depend on the network.
__global__ __launch_bounds__(REAL_SORT_THREADS) void real_sort_kernel(const float *__restrict__ X, int n, int p, int n2,
                                                                      uint16_t *__restrict__ order, float *__restrict__ sval)
{
    __shared__ uint64_t key[REAL_MAX_N];
    const int j = blockIdx.x, tid = threadIdx.x;
    for (int s = tid; s < n2; s += REAL_SORT_THREADS) {
        uint64_t k = ~0ull;
        if (s < n) {
            float x = X[(size_t)s * p + j];
            if (x == 0.0f) x = 0.0f;   // -0.0 and +0.0 are one value
            k = ((uint64_t)real_key(x) << 16) | (uint64_t)s;
        }
        key[s] = k;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int i = tid; i < n2; i += REAL_SORT_THREADS) {
                const int o = i ^ d;
                if (o > i) {
                    const uint64_t a = key[i], b = key[o];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[o] = a; }
                }
            }
            __syncthreads();
        }
    for (int r = tid; r < n; r += REAL_SORT_THREADS) {
        order[(size_t)r * p + j] = (uint16_t)(key[r] & 0xffffu);
        sval[(size_t)r * p + j] = real_unkey((uint32_t)(key[r] >> 16));
    }
}

// label words as tree_pack_kernel writes them
__global__ __launch_bounds__(64) void real_ymask_kernel(const int32_t *__restrict__ y01, int n, uint64_t *__restrict__ ymask)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    const uint64_t b = __ballot(s < n && y01[s] != 0);
    if (threadIdx.x == 0) ymask[blockIdx.x] = b;
}

struct RealDesign {
    FitArr<float> x, sval;        // [n][p] the design; [n][p] rank-major sorted values
    FitArr<uint16_t> order;       // [n][p] rank-major: the sample of rank r in column j
    FitArr<uint64_t> ymask;       // [W]
};

// The prologue of both entry points: every value must be finite (PSK_EINVAL in the name of the caller, `who`); the design goes
// to the device and every column is sorted there.  Returns with the stream idle.
int real_prepare(psk_ctx *ctx, const char *who, const float *X, const int32_t *y01, int n, int p, RealDesign &d)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < p; j++)
            if (!std::isfinite(X[(size_t)i * p + j]))
                return psk_fail(ctx, PSK_EINVAL, "%s takes a finite float32 design: sample %d, column %d holds %g", who, i, j,
                                (double)X[(size_t)i * p + j]);
    const int W = (n + 63) / 64;
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    FitArr<int32_t> y;
    PSK_HIP(ctx, d.x.upload(X, (size_t)n * p, ctx->stream));
    PSK_HIP(ctx, y.upload(y01, n, ctx->stream));
    PSK_HIP(ctx, d.order.alloc((size_t)n * p));
    PSK_HIP(ctx, d.sval.alloc((size_t)n * p));
    PSK_HIP(ctx, d.ymask.alloc(W));
    real_sort_kernel<<<p, REAL_SORT_THREADS, 0, ctx->stream>>>(d.x, n, p, n2, d.order, d.sval);
    PSK_HIP(ctx, hipGetLastError());
    real_ymask_kernel<<<W, 64, 0, ctx->stream>>>(y, n, d.ymask);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

// scikit-learn's threshold between the in-bag values lo < hi around a split
__device__ __forceinline__ double real_threshold(float lo, float hi)
{
    double thr = (double)lo / 2.0 + (double)hi / 2.0;
    if (thr == (double)hi || isinf(thr)) thr = (double)lo;
    return thr;
}

// ---- the walk inside a column ----
// A thread walks the ranks r0 .. r1 - 1 of column j.  With fewer columns than half a workgroup's threads a column's ranks are cut
// into G SEGMENTS of L ranks, one thread each (thread = segment * p + column: the threads of a wave still read consecutive
// columns of one rank); a segment first adds up its in-node samples (real_seg_sum), takes the sums and the last value of the
// segments before it from LDS, and then walks its candidates from there (real_seg_walk).  Candidates keep their order: segments
// of a column are compared in ascending order, the first strictly larger proxy staying.
struct RealSeg { int c, cw, cw1; float last; };   // distinct in-node samples, their weight, their class-1 weight, the last value

// segments per column for a workgroup of `threads`: at least 16 ranks each, at most 64, one when the columns fill the threads
inline int real_segments(int n, int p, int threads)
{
    if (2 * p > threads) return 1;
    return std::max(1, std::min(std::min(threads / p, 64), (n + 15) / 16));
}

// member(s, y): the weight of sample s in the node (0: not in it) and, through y, its label
template <class Member>
__device__ __forceinline__ RealSeg real_seg_sum(const uint16_t *__restrict__ order, const float *__restrict__ sval, int p, int j, int r0,
                                                int r1, const Member &member)
{
    RealSeg t{0, 0, 0, 0.0f};
    int last_r = -1;
    for (int r = r0; r < r1; r++) {
        int y = 0;
        const int w = member(order[(size_t)r * p + j], y);
        if (!w) continue;
        t.c++;
        t.cw += w;
        if (y) t.cw1 += w;
        last_r = r;
    }
    if (last_r >= 0) t.last = sval[(size_t)last_r * p + j];
    return t;
}

// the sums of the segments of column j before segment g (seg[g'][j], g' < g) and the last value among them
__device__ __forceinline__ RealSeg real_seg_before(const RealSeg *seg, int p, int j, int g)
{
    RealSeg b{0, 0, 0, 0.0f};
    for (int k = 0; k < g; k++) {
        const RealSeg t = seg[k * p + j];
        if (!t.c) continue;
        b.c += t.c;
        b.cw += t.cw;
        b.cw1 += t.cw1;
        b.last = t.last;
    }
    return b;
}

// cand(cl, cwl, cwl1, lo, hi) at every place where the in-node values change: the left side's sums and the two values
template <class Member, class Cand>
__device__ __forceinline__ void real_seg_walk(const uint16_t *__restrict__ order, const float *__restrict__ sval, int p, int j, int r0,
                                              int r1, const RealSeg &before, int n_node, const Member &member, Cand &&cand)
{
    int cl = before.c, cwl = before.cw, cwl1 = before.cw1;
    float prev = before.last;
    if (cl == n_node) return;
    for (int r = r0; r < r1; r++) {
        int y = 0;
        const int w = member(order[(size_t)r * p + j], y);
        if (!w) continue;
        const float v = sval[(size_t)r * p + j];
        if (cl > 0 && v > prev) cand(cl, cwl, cwl1, prev, v);
        cl++;
        cwl += w;
        if (y) cwl1 += w;
        prev = v;
        if (cl == n_node) break;   // the node's last sample
    }
}

// ---- one tree per workgroup (psk_tree_fit_real): solver_tree.hip's builder with the walk in place of the popcounts ----

constexpr int RTREE_THREADS = 1024;
constexpr int RTREE_WAVES = RTREE_THREADS / 64;
constexpr int RTREE_MAX_DEPTH = 10;

__device__ __forceinline__ bool rtree_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

struct RTreeRec { int parent, depth, is_left, n, n1; double imp; };

// the node's training samples, unit weights
struct RTreeMember {
    const uint64_t *MT, *MTY;
    __device__ __forceinline__ int operator()(int s, int &y) const
    {
        const uint64_t bit = 1ull << (s & 63);
        if (!(MT[s >> 6] & bit)) return 0;
        y = (MTY[s >> 6] & bit) != 0;
        return 1;
    }
};

struct RTreeLds {
    uint64_t mask[RTREE_MAX_DEPTH + 1][REAL_MAX_W];   // the routing masks of the root-to-node path, every sample
    uint64_t T[REAL_MAX_W], Y[REAL_MAX_W], MT[REAL_MAX_W], MTY[REAL_MAX_W];
    RTreeRec stack[RTREE_MAX_DEPTH + 2];
    int path_feat[RTREE_MAX_DEPTH + 1];
    double path_thr[RTREE_MAX_DEPTH + 1];
    double red_v[RTREE_WAVES];
    int red_i[RTREE_WAVES], red_c[RTREE_WAVES];
    float red_lo[RTREE_WAVES], red_hi[RTREE_WAVES];
    RealSeg seg[RTREE_THREADS];                       // [segment][column] when a column's ranks are cut into segments
};

template <int CRIT>
__device__ void rtree_build(const float *__restrict__ X, const uint16_t *__restrict__ order, const float *__restrict__ sval, int n, int p,
                            int W, int G, int max_depth, int32_t *__restrict__ nodes, double *__restrict__ imp_out, double *__restrict__ thr_out,
                            int32_t *__restrict__ leaf_out, double *__restrict__ frac_out, int32_t *__restrict__ node_count,
                            int32_t *__restrict__ depth_out, RTreeLds &L)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Wn = W * 64;
    int n_tot = 0, n1_tot = 0;
    for (int w = 0; w < W; w++) { n_tot += __popcll(L.T[w]); n1_tot += __popcll(L.T[w] & L.Y[w]); }
    if (tid == 0)
        L.stack[0] = RTreeRec{-1, 0, 0, n_tot, n1_tot, tree_impurity<CRIT>((double)(n_tot - n1_tot), (double)n1_tot, (double)n_tot)};
    int sp = 1, next_id = 0, deepest = 0;
    while (sp > 0) {
        __syncthreads();   // the stack, the path and everything the node before wrote
        const RTreeRec rec = L.stack[--sp];
        const int d = rec.depth;
        if (d == 0) {
            if (tid < W) { L.MT[tid] = L.mask[0][tid] & L.T[tid]; L.MTY[tid] = L.mask[0][tid] & L.T[tid] & L.Y[tid]; }
        } else {
            // x <= threshold goes left, for every sample the parent's mask holds
            const int col = L.path_feat[d - 1];
            const double thr = L.path_thr[d - 1];
            for (int s0 = 0; s0 < Wn; s0 += RTREE_THREADS) {
                const int s = s0 + tid;
                const uint64_t right = __ballot(s < n && !((double)X[(size_t)s * p + col] <= thr));
                if (lane == 0 && s < Wn) {
                    const int w = s >> 6;
                    const uint64_t m = L.mask[d - 1][w] & (rec.is_left ? ~right : right);
                    L.mask[d][w] = m;
                    L.MT[w] = m & L.T[w];
                    L.MTY[w] = m & L.T[w] & L.Y[w];
                }
            }
        }
        __syncthreads();
        const double nn = (double)rec.n, c1n = (double)rec.n1, c0n = (double)(rec.n - rec.n1);
        bool is_leaf = d >= max_depth || rec.n < 2 || rec.imp <= DBL_EPSILON;
        int feat = -2, cr = 0, cr1 = 0;
        double imp_l = 0.0, imp_r = 0.0, thr = -2.0;
        if (!is_leaf) {
            double bv = -INFINITY;
            int bi = INT_MAX, bc = 0;
            float blo = 0.0f, bhi = 0.0f;
            // item = segment * p + column; with G > 1 there is one round.  bi orders (column, segment): the lowest column among
            // bit-equal proxies, then the lowest threshold
            const RTreeMember member{L.MT, L.MTY};
            const int SL = (n + G - 1) / G;
            for (int item0 = 0; item0 < p * G; item0 += RTREE_THREADS) {
                const int item = item0 + tid, g = item / p, j = item - g * p;
                const bool active = item < p * G;
                const int r0 = g * SL, r1 = min(n, r0 + SL);
                RealSeg before{0, 0, 0, 0.0f};
                if (G > 1) {
                    if (active) L.seg[item] = real_seg_sum(order, sval, p, j, r0, r1, member);
                    __syncthreads();
                    if (active) before = real_seg_before(L.seg, p, j, g);
                }
                if (!active) continue;
                real_seg_walk(order, sval, p, j, r0, r1, before, rec.n, member, [&](int cl, int, int cl1, float lo, float hi) {
                    const int c = rec.n - cl, c1 = rec.n1 - cl1;   // the right side, as the other tree calls count it
                    const double wr = (double)c, wl = (double)cl;
                    const double ir = tree_impurity<CRIT>((double)(c - c1), (double)c1, wr);
                    const double il = tree_impurity<CRIT>(c0n - (double)(c - c1), c1n - (double)c1, wl);
                    const double proxy = -wr * ir - wl * il;
                    if (proxy > bv) { bv = proxy; bi = j * G + g; bc = c | (c1 << 16); blo = lo; bhi = hi; }   // ascending: the first maximum stays
                });
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const double ov = psk_shfl_xor_f64(bv, s);
                const int oi = __shfl_xor(bi, s, 64), oc = __shfl_xor(bc, s, 64);
                const float olo = __shfl_xor(blo, s, 64), ohi = __shfl_xor(bhi, s, 64);
                if (rtree_better(ov, oi, bv, bi)) { bv = ov; bi = oi; bc = oc; blo = olo; bhi = ohi; }
            }
            if (lane == 0) { L.red_v[wave] = bv; L.red_i[wave] = bi; L.red_c[wave] = bc; L.red_lo[wave] = blo; L.red_hi[wave] = bhi; }
            __syncthreads();
            bv = L.red_v[0]; bi = L.red_i[0]; bc = L.red_c[0]; blo = L.red_lo[0]; bhi = L.red_hi[0];
            for (int w = 1; w < RTREE_WAVES; w++)
                if (rtree_better(L.red_v[w], L.red_i[w], bv, bi)) {
                    bv = L.red_v[w]; bi = L.red_i[w]; bc = L.red_c[w]; blo = L.red_lo[w]; bhi = L.red_hi[w];
                }
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
                else { feat = bi / G; thr = real_threshold(blo, bhi); }
            }
        }
        const int id = next_id++;
        deepest = max(deepest, d);
        if (tid == 0) {
            thr_out[id] = thr;
            tree_write_node(nodes, imp_out, id, rec.parent, rec.is_left, feat, is_leaf, rec.n, rec.n - rec.n1, rec.n1, rec.imp);
        }
        if (is_leaf) {
            const double f1 = c1n / nn;
            for (int s = tid; s < n; s += RTREE_THREADS)
                if ((L.mask[d][s >> 6] >> (s & 63)) & 1ull) { leaf_out[s] = id; frac_out[s] = f1; }
        } else {
            // (the barrier of the reduction lies between every thread's read of `rec` and these writes)
            if (tid == 0) {
                L.path_feat[d] = feat;
                L.path_thr[d] = thr;
                L.stack[sp] = RTreeRec{id, d + 1, 0, cr, cr1, imp_r};
                L.stack[sp + 1] = RTreeRec{id, d + 1, 1, rec.n - cr, rec.n1 - cr1, imp_l};
            }
            sp += 2;
        }
    }
    if (tid == 0) { *node_count = next_id; *depth_out = deepest; }
}

__global__ __launch_bounds__(RTREE_THREADS) void rtree_fit_kernel(
    const float *__restrict__ X, const uint16_t *__restrict__ order, const float *__restrict__ sval, const uint64_t *__restrict__ ymask,
    const int32_t *__restrict__ fold, int n, int p, int W, int G, const int32_t *__restrict__ fit_max_depth,
    const int32_t *__restrict__ fit_criterion, const int32_t *__restrict__ fit_fold, const int32_t *__restrict__ fit_off,
    int32_t *__restrict__ node_count, int32_t *__restrict__ depth_out, int32_t *__restrict__ nodes, double *__restrict__ imp_out,
    double *__restrict__ thr_out, int32_t *__restrict__ leaf_out, double *__restrict__ frac_out)
{
    __shared__ RTreeLds L;
    const int fit = blockIdx.x, tid = threadIdx.x;
    const int tf = fit_fold[fit];
    // the training mask and the mask of existing samples, a word per wave ballot
    for (int s0 = 0; s0 < W * 64; s0 += RTREE_THREADS) {
        const int s = s0 + tid;
        const uint64_t live = __ballot(s < n), train = __ballot(s < n && fold[s] != tf);
        if ((tid & 63) == 0 && s < W * 64) {
            L.mask[0][s >> 6] = live;
            L.T[s >> 6] = train;
            L.Y[s >> 6] = ymask[s >> 6];
        }
    }
    __syncthreads();
    const size_t off = (size_t)fit_off[fit];
    int32_t *nd = nodes + off * TREE_NODE_FIELDS;
    int32_t *lo = leaf_out + (size_t)fit * n;
    double *fo = frac_out + (size_t)fit * n;
    if (fit_criterion[fit] == 0)
        rtree_build<0>(X, order, sval, n, p, W, G, fit_max_depth[fit], nd, imp_out + off, thr_out + off, lo, fo, node_count + fit,
                       depth_out + fit, L);
    else
        rtree_build<1>(X, order, sval, n, p, W, G, fit_max_depth[fit], nd, imp_out + off, thr_out + off, lo, fo, node_count + fit,
                       depth_out + fit, L);
}

// ---- one tree at a time per workgroup (psk_forest_fit_real): solver_forest.hip's builder with the walk ----

constexpr int RFOREST_THREADS = 256;
constexpr int RFOREST_LDS_COLS = 1024;        // per-column arrays stay in LDS up to this many columns (FOREST_LDS_COLS)
constexpr int RFOREST_COL_BYTES = 36;         // proxy f64, features / constant_features / state / w_r / w_r1 i32, lo / hi f32
constexpr int RFOREST_LDS_BYTES = 64 << 10;   // what a launch may ask for without opting in to more
constexpr int RFOREST_GRID_PER_CU = 4;
constexpr uint32_t RFOREST_NO_LABEL = 0xffff;
constexpr int RCOL_CONSTANT = -1, RCOL_NO_SPLIT = -2;

struct RForestRec { int parent, depth, is_left, n, wn, w1, n_const, pad; double imp; };

// byte offsets into the dynamic LDS region (every one a multiple of 16) and the region's size
struct RForestLds { int label, weight, Y, cur, walk, seg, segbest, cols, total; };

// what a segment of a column found: the column's state as far as the segment saw it, its best proxy and that split
struct RForestBest { double bp; int st, cw, cw1; float lo, hi; int pad; };

// the in-bag samples of the pending node `slot`, their weights in the tree
struct RForestMember {
    const uint16_t *label, *weight;
    const uint64_t *Y;
    uint32_t slot;
    __device__ __forceinline__ int operator()(int s, int &y) const
    {
        if (label[s] != slot) return 0;
        y = (int)((Y[s >> 6] >> (s & 63)) & 1ull);
        return weight[s];
    }
};

struct RForestArgs {
    const float *X, *sval;
    const uint16_t *order;
    const uint64_t *ymask;
    int n, p, W, G, n_trees, cols_in_lds;   // G: segments per column (real_segments)
    const uint16_t *tree_weight;
    const uint32_t *tree_state;
    const int32_t *tree_fit, *fit_crit, *fit_depth, *fit_mf, *fit_msl, *fit_mss;
    const int64_t *tree_node_off;      // first slot of the tree in the node pool, -1: not exported
    const int32_t *tree_node_cap, *tree_leaf_row;
    int32_t *node_count, *depth_out, *nodes, *leaf_out;
    double *imp_out, *thr_out, *frac0, *frac1;
    RForestRec *stack;                 // [grid][n + 2]
    char *cols_global;                 // [grid][RFOREST_COL_BYTES * p_pad] when the columns do not fit LDS
    RForestLds lds;
};

__device__ __forceinline__ void rswap_int(int *a, int i, int j) { const int t = a[i]; a[i] = a[j]; a[j] = t; }

// In LDS per sample: a 16-bit label naming the pending node it belongs to (its slot on the depth-first stack) and its 16-bit
// weight in the tree; the label words of Y; per column the walk's inputs next to features[] / constant_features[].
__global__ __launch_bounds__(RFOREST_THREADS) void rforest_fit_kernel(const RForestArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int n = a.n, p = a.p, Wn = a.W * 64;
    uint16_t *label = (uint16_t *)(smem + a.lds.label), *weight = (uint16_t *)(smem + a.lds.weight);
    uint64_t *Y = (uint64_t *)(smem + a.lds.Y);
    RForestRec *cur = (RForestRec *)(smem + a.lds.cur);
    int *walk = (int *)(smem + a.lds.walk);     // best column, n_known, n_found of the node's walk; the root's three totals
    RealSeg *seg = (RealSeg *)(smem + a.lds.seg);                    // [segment][column], G > 1 only
    RForestBest *segbest = (RForestBest *)(smem + a.lds.segbest);    // the same
    const int G = a.G, SL = (n + G - 1) / G;
    const int p_pad = (p + 3) & ~3;
    char *cols = a.cols_in_lds ? smem + a.lds.cols : a.cols_global + (size_t)blockIdx.x * RFOREST_COL_BYTES * p_pad;
    double *proxy = (double *)cols;
    int *features = (int *)(cols + 8 * (size_t)p_pad), *constant = features + p_pad, *col_state = constant + p_pad;
    int *col_wr = col_state + p_pad, *col_wr1 = col_wr + p_pad;
    float *col_lo = (float *)(col_wr1 + p_pad), *col_hi = col_lo + p_pad;
    RForestRec *stack = a.stack + (size_t)blockIdx.x * (n + 2);

    for (int tree = blockIdx.x; tree < a.n_trees; tree += gridDim.x) {
        const int fit = a.tree_fit[tree];
        const int crit = a.fit_crit[fit], max_depth = a.fit_depth[fit] > 0 ? a.fit_depth[fit] : INT_MAX, max_features = a.fit_mf[fit];
        const int msl = a.fit_msl[fit], mss = a.fit_mss[fit];
        const int64_t node_off = a.tree_node_off[tree];
        const int node_cap = a.tree_node_cap[tree], leaf_row = a.tree_leaf_row[tree];
        const uint16_t *wt = a.tree_weight + (size_t)tree * n;
        uint32_t rng = a.tree_state[tree];   // lane 0's copy is the one that advances
        __syncthreads();                      // the tree before is done with LDS
        if (tid < 3) walk[tid] = 0;
        for (int w = tid; w < a.W; w += RFOREST_THREADS) Y[w] = a.ymask[w];
        __syncthreads();
        for (int s = tid; s < Wn; s += RFOREST_THREADS) {
            const uint32_t wv = s < n ? wt[s] : 0u;
            label[s] = s < n ? 0 : RFOREST_NO_LABEL;
            weight[s] = (uint16_t)wv;
            if (wv) {   // (integer sums: the order of the lanes cannot matter)
                atomicAdd(&walk[0], 1);
                atomicAdd(&walk[1], (int)wv);
                if ((Y[s >> 6] >> (s & 63)) & 1ull) atomicAdd(&walk[2], (int)wv);
            }
        }
        for (int j = tid; j < p; j += RFOREST_THREADS) { features[j] = j; constant[j] = 0; }
        __syncthreads();
        const int n_tot = walk[0], w_tot = walk[1], w1_tot = walk[2];
        const double w_tree = (double)w_tot;
        if (tid == 0)
            stack[0] = RForestRec{-1, 0, 0, n_tot, w_tot, w1_tot, 0, 0, tree_impurity(crit, (double)(w_tot - w1_tot), (double)w1_tot, w_tree)};
        int sp = 1, next_id = 0, deepest = 0;
        while (sp > 0) {
            __syncthreads();   // labels, per-column arrays, `walk` and `cur` of the node before
            --sp;
            if (tid == 0) *cur = stack[sp];
            __syncthreads();
            const RForestRec rec = *cur;
            const uint32_t slot = (uint32_t)sp;
            const double wn = (double)rec.wn, c1n = (double)rec.w1, c0n = (double)(rec.wn - rec.w1);
            bool is_leaf = rec.depth >= max_depth || rec.n < mss || rec.n < 2 * msl || rec.imp <= DBL_EPSILON;
            int feat = -2, nr = 0, wr = 0, wr1 = 0, n_const = rec.n_const;
            double imp_l = 0.0, imp_r = 0.0, thr = -2.0;
            if (!is_leaf) {
                // item = segment * p + column; with G > 1 there is one round
                const RForestMember member{label, weight, Y, slot};
                for (int item0 = 0; item0 < p * G; item0 += RFOREST_THREADS) {
                    const int item = item0 + tid, g = item / p, j = item - g * p;
                    const bool active = item < p * G;
                    const int r0 = g * SL, r1 = min(n, r0 + SL);
                    RealSeg before{0, 0, 0, 0.0f};
                    if (G > 1) {
                        if (active) seg[item] = real_seg_sum(a.order, a.sval, p, j, r0, r1, member);
                        __syncthreads();
                        if (active) before = real_seg_before(seg, p, j, g);
                    }
                    RForestBest b{-INFINITY, RCOL_CONSTANT, 0, 0, 0.0f, 0.0f, 0};
                    if (active)
                        real_seg_walk(a.order, a.sval, p, j, r0, r1, before, rec.n, member, [&](int cl, int cwl, int cwl1, float lo, float hi) {
                            const int c = rec.n - cl;   // distinct in-bag samples on the right
                            if (b.st == RCOL_CONSTANT) b.st = RCOL_NO_SPLIT;
                            if (cl < msl || c < msl) return;
                            const int cw = rec.wn - cwl, cw1 = rec.w1 - cwl1;
                            const double dwr = (double)cw, dwl = (double)cwl;
                            const double ir = tree_impurity(crit, (double)(cw - cw1), (double)cw1, dwr);
                            const double il = tree_impurity(crit, c0n - (double)(cw - cw1), c1n - (double)cw1, dwl);
                            const double pv = -dwr * ir - dwl * il;
                            if (pv > b.bp) { b.bp = pv; b.st = c; b.cw = cw; b.cw1 = cw1; b.lo = lo; b.hi = hi; }
                        });
                    if (G > 1) {
                        // the column's segments in ascending order: the first strictly larger proxy stays
                        if (active) segbest[item] = b;
                        __syncthreads();
                        if (!active || g != 0) continue;
                        for (int k = 1; k < G; k++) {
                            const RForestBest o = segbest[k * p + j];
                            if (o.st == RCOL_CONSTANT) continue;
                            if (b.st == RCOL_CONSTANT) b.st = RCOL_NO_SPLIT;
                            if (o.st >= 0 && o.bp > b.bp) b = o;
                        }
                    }
                    if (!active) continue;
                    if (b.st >= 0) proxy[j] = b.bp;
                    col_state[j] = b.st;
                    col_wr[j] = b.cw;
                    col_wr1[j] = b.cw1;
                    col_lo[j] = b.lo;
                    col_hi[j] = b.hi;
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
                            rswap_int(features, n_drawn, f_j);
                            n_drawn++;
                            continue;
                        }
                        f_j += n_found;
                        const int col = features[f_j], st = col_state[col];
                        if (st == RCOL_CONSTANT) {
                            rswap_int(features, f_j, n_total);
                            n_found++;
                            n_total++;
                            continue;
                        }
                        f_i--;
                        rswap_int(features, f_i, f_j);
                        if (st == RCOL_NO_SPLIT) continue;
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
                for (int k = tid; k < n_known; k += RFOREST_THREADS) features[k] = constant[k];
                for (int k = tid; k < n_found; k += RFOREST_THREADS) constant[n_known + k] = features[n_known + k];
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
                    else { feat = best; thr = real_threshold(col_lo[best], col_hi[best]); }
                }
            }
            const int id = next_id++;
            deepest = max(deepest, rec.depth);
            if (tid == 0 && node_off >= 0 && id < node_cap) {
                a.thr_out[node_off + id] = thr;
                tree_write_node(a.nodes + (size_t)node_off * TREE_NODE_FIELDS, a.imp_out + node_off, id, rec.parent, rec.is_left, feat, is_leaf,
                                rec.n, rec.wn - rec.w1, rec.w1, rec.imp);
            }
            if (is_leaf) {
                const double f0 = c0n / wn, f1 = c1n / wn;
                for (int s = tid; s < n; s += RFOREST_THREADS)
                    if (label[s] == slot) {
                        a.frac0[(size_t)tree * n + s] = f0;
                        a.frac1[(size_t)tree * n + s] = f1;
                        if (leaf_row >= 0) a.leaf_out[(size_t)leaf_row * n + s] = id;
                        label[s] = RFOREST_NO_LABEL;
                    }
            } else {
                // the right child takes this node's slot, the left one the slot above it: popped first
                for (int s = tid; s < n; s += RFOREST_THREADS)
                    if (label[s] == slot && (double)a.X[(size_t)s * p + feat] <= thr) label[s] = (uint16_t)(slot + 1);
                if (tid == 0) {
                    stack[sp] = RForestRec{id, rec.depth + 1, 0, nr, wr, wr1, n_const, 0, imp_r};
                    stack[sp + 1] = RForestRec{id, rec.depth + 1, 1, rec.n - nr, rec.wn - wr, rec.w1 - wr1, n_const, 0, imp_l};
                }
                sp += 2;
            }
        }
        if (tid == 0) { a.node_count[tree] = next_id; a.depth_out[tree] = deepest; }
    }
}

// sum0[f][s], sum1[f][s]: the leaf fractions of fit f's trees added one after the other in tree order (the order of a f64 sum
// is part of the contract: no atomics)
__global__ __launch_bounds__(256) void rforest_sum_kernel(const double *__restrict__ frac0, const double *__restrict__ frac1, int n,
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

int ralign16(int v) { return (v + 15) & ~15; }

// the LDS region for a call of W words, p columns and G segments a column; the per-column arrays go last and are left out (cols_in_lds = 0) past
// RFOREST_LDS_COLS columns, or where they would take the region past RFOREST_LDS_BYTES
RForestLds rforest_lds_layout(int W, int p, int G, int *cols_in_lds)
{
    RForestLds l{};
    int at = 0;
    l.label = at; at = ralign16(at + 2 * 64 * W);
    l.weight = at; at = ralign16(at + 2 * 64 * W);
    l.Y = at; at = ralign16(at + 8 * W);
    l.cur = at; at = ralign16(at + (int)sizeof(RForestRec));
    l.walk = at; at = ralign16(at + 16);
    l.seg = at; at = ralign16(at + (G > 1 ? RFOREST_THREADS * (int)sizeof(RealSeg) : 0));
    l.segbest = at; at = ralign16(at + (G > 1 ? RFOREST_THREADS * (int)sizeof(RForestBest) : 0));
    l.cols = at;
    const int with_cols = ralign16(at + RFOREST_COL_BYTES * ((p + 3) & ~3));
    *cols_in_lds = p <= RFOREST_LDS_COLS && with_cols <= RFOREST_LDS_BYTES;
    if (*cols_in_lds) at = with_cols;
    l.total = at;
    return l;
}

}  // namespace

extern "C" int psk_tree_fit_real(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                                 const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                                 int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                                 int32_t *leaf_out, double *frac_out, double *threshold_out)
{
    const char *who = "psk_tree_fit_real";
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !fold || !fit_max_depth || !fit_criterion || !fit_fold || !node_count_out || !max_depth_out || !nodes_out ||
        !impurity_out || !leaf_out || !frac_out || !threshold_out)
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (n < 1 || p < 1 || n_fits < 1) return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d", n, p, n_fits);
    if (n > REAL_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s keeps a node's sample mask in LDS: at most %d samples, got %d", who, REAL_MAX_N, n);
    for (int f = 0; f < n_fits; f++) {
        if (fit_max_depth[f] < 1 || fit_max_depth[f] > RTREE_MAX_DEPTH)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: max_depth must be 1..%d, got %d", f, RTREE_MAX_DEPTH, fit_max_depth[f]);
        if (fit_criterion[f] != 0 && fit_criterion[f] != 1)
            return psk_fail(ctx, PSK_EINVAL, "fit %d: criterion must be 0 (gini) or 1 (entropy), got %d", f, fit_criterion[f]);
        int tr = 0;
        for (int i = 0; i < n && !tr; i++) tr = fold[i] != fit_fold[f];
        if (!tr) return psk_fail(ctx, PSK_EINVAL, "fit %d has no training sample", f);
    }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    RealDesign d;
    if (const int rc = real_prepare(ctx, who, X, y01, n, p, d)) return rc;

    // a tree of max_depth d has at most 2^(d+1) - 1 nodes: fit f's nodes start at off[f] of one packed buffer, and only the
    // node_count[f] nodes it made go back into the caller's strided arrays
    std::vector<int32_t> off((size_t)n_fits + 1, 0);
    for (int f = 0; f < n_fits; f++) off[f + 1] = off[f] + (2 << fit_max_depth[f]) - 1;
    const size_t total = (size_t)off[n_fits];
    FitArr<int32_t> d_fold, depth, crit, d_fit_fold, d_off, count, dout, d_nodes, leaf;
    FitArr<double> d_imp, frac, d_thr;
    PSK_HIP(ctx, d_fold.upload(fold, n, ctx->stream));
    PSK_HIP(ctx, depth.upload(fit_max_depth, n_fits, ctx->stream));
    PSK_HIP(ctx, crit.upload(fit_criterion, n_fits, ctx->stream));
    PSK_HIP(ctx, d_fit_fold.upload(fit_fold, n_fits, ctx->stream));
    PSK_HIP(ctx, d_off.upload(off.data(), n_fits, ctx->stream));
    PSK_HIP(ctx, count.alloc(n_fits));
    PSK_HIP(ctx, dout.alloc(n_fits));
    PSK_HIP(ctx, d_nodes.alloc(total * TREE_NODE_FIELDS));
    PSK_HIP(ctx, d_imp.alloc(total));
    PSK_HIP(ctx, d_thr.alloc(total));
    PSK_HIP(ctx, leaf.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, frac.alloc((size_t)n_fits * n));
    rtree_fit_kernel<<<n_fits, RTREE_THREADS, 0, ctx->stream>>>(d.x, d.order, d.sval, d.ymask, d_fold, n, p, W, real_segments(n, p, RTREE_THREADS),
                                                                depth, crit, d_fit_fold,
                                                                d_off, count, dout, d_nodes, d_imp, d_thr, leaf, frac);
    PSK_HIP(ctx, hipGetLastError());
    std::vector<int32_t> nodes(total * TREE_NODE_FIELDS);
    std::vector<double> imp(total), thr(total);
    PSK_HIP(ctx, d_thr.download(thr.data(), thr.size(), ctx->stream));
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
        memcpy(threshold_out + (size_t)f * PSK_TREE_NODE_CAP, thr.data() + off[f], k * 8);
    }
    return PSK_OK;
}

extern "C" int psk_forest_fit_real(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                                   const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                                   const int32_t *tree_export, int n_fits, const int32_t *fit_criterion, const int32_t *fit_max_depth,
                                   const int32_t *fit_max_features, const int32_t *fit_min_samples_leaf,
                                   const int32_t *fit_min_samples_split, double *sum0_out, double *sum1_out, int32_t *node_count_out,
                                   int32_t *max_depth_out, int64_t node_pool, int64_t *tree_node_off_out, int32_t *nodes_out,
                                   double *impurity_out, int32_t *leaf_out, double *threshold_out)
{
    const char *who = "psk_forest_fit_real";
    if (!ctx) return PSK_EINVAL;
    if (!X || !y01 || !tree_weight || !tree_state || !tree_fit || !tree_export || !fit_criterion || !fit_max_depth ||
        !fit_max_features || !fit_min_samples_leaf || !fit_min_samples_split || !sum0_out || !sum1_out || !node_count_out ||
        !max_depth_out || !tree_node_off_out)
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (n < 1 || p < 1 || n_fits < 1 || n_trees < 1)
        return psk_fail(ctx, PSK_EINVAL, "bad problem shape n=%d p=%d fits=%d trees=%d", n, p, n_fits, n_trees);
    if (n > REAL_MAX_N)
        return psk_fail(ctx, PSK_ERANGE, "%s keeps a label per sample in LDS: at most %d samples, got %d", who, REAL_MAX_N, n);
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
    for (int t = 0; t < n_trees; t++) {
        if (tree_fit[t] < 0 || tree_fit[t] >= n_fits) return psk_fail(ctx, PSK_EINVAL, "tree %d: fit %d of %d", t, tree_fit[t], n_fits);
        fit_ptr[tree_fit[t] + 1]++;
        int inbag = 0;
        int64_t w_sum = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t w = tree_weight[(size_t)t * n + i];
            inbag += w != 0;
            w_sum += w;
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
    if (n_export && (!nodes_out || !impurity_out || !leaf_out || !threshold_out)) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (pool > node_pool)
        return psk_fail(ctx, PSK_ERANGE, "the exported trees may need %lld node slots (2 x in-bag samples - 1 each), the pool has %lld",
                        (long long)pool, (long long)node_pool);
    for (int f = 0; f < n_fits; f++) fit_ptr[f + 1] += fit_ptr[f];
    {
        std::vector<int32_t> at(fit_ptr.begin(), fit_ptr.end() - 1);
        for (int t = 0; t < n_trees; t++) fit_trees[at[tree_fit[t]]++] = t;
    }

    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int W = (n + 63) / 64;
    RealDesign d;
    if (const int rc = real_prepare(ctx, who, X, y01, n, p, d)) return rc;

    const int grid = std::min(n_trees, RFOREST_GRID_PER_CU * (ctx->n_cu > 0 ? ctx->n_cu : 256));
    RForestArgs a{};
    a.G = real_segments(n, p, RFOREST_THREADS);
    a.lds = rforest_lds_layout(W, p, a.G, &a.cols_in_lds);
    const size_t p_pad = ((size_t)p + 3) & ~(size_t)3;
    FitArr<uint16_t> d_weight;
    FitArr<uint32_t> d_state;
    FitArr<int32_t> d_tree_fit, d_crit, d_depth, d_mf, d_msl, d_mss, d_cap, d_leaf_row, d_count, d_deepest, d_nodes, d_leaf, d_fit_ptr,
        d_fit_tree_ids;
    FitArr<int64_t> d_off;
    FitArr<double> d_imp, d_thr, frac0, frac1, sum0, sum1;
    FitArr<RForestRec> d_stack;
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
    PSK_HIP(ctx, d_thr.alloc((size_t)pool));
    PSK_HIP(ctx, d_leaf.alloc((size_t)n_export * n));
    PSK_HIP(ctx, frac0.alloc((size_t)n_trees * n));
    PSK_HIP(ctx, frac1.alloc((size_t)n_trees * n));
    PSK_HIP(ctx, sum0.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, sum1.alloc((size_t)n_fits * n));
    PSK_HIP(ctx, d_stack.alloc((size_t)grid * (n + 2)));
    PSK_HIP(ctx, d_cols.alloc(a.cols_in_lds ? 0 : (size_t)grid * RFOREST_COL_BYTES * p_pad));
    a.X = d.x; a.sval = d.sval; a.order = d.order; a.ymask = d.ymask;
    a.n = n; a.p = p; a.W = W; a.n_trees = n_trees;
    a.tree_weight = d_weight; a.tree_state = d_state; a.tree_fit = d_tree_fit;
    a.fit_crit = d_crit; a.fit_depth = d_depth; a.fit_mf = d_mf; a.fit_msl = d_msl; a.fit_mss = d_mss;
    a.tree_node_off = d_off; a.tree_node_cap = d_cap; a.tree_leaf_row = d_leaf_row;
    a.node_count = d_count; a.depth_out = d_deepest; a.nodes = d_nodes; a.leaf_out = d_leaf;
    a.imp_out = d_imp; a.thr_out = d_thr; a.frac0 = frac0; a.frac1 = frac1;
    a.stack = d_stack; a.cols_global = d_cols;
    rforest_fit_kernel<<<grid, RFOREST_THREADS, a.lds.total, ctx->stream>>>(a);
    PSK_HIP(ctx, hipGetLastError());
    rforest_sum_kernel<<<dim3(div_up(n, 256), n_fits), 256, 0, ctx->stream>>>(frac0, frac1, n, d_fit_ptr, d_fit_tree_ids, sum0, sum1);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, sum0.download(sum0_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, sum1.download(sum1_out, (size_t)n_fits * n, ctx->stream));
    PSK_HIP(ctx, d_count.download(node_count_out, n_trees, ctx->stream));
    PSK_HIP(ctx, d_deepest.download(max_depth_out, n_trees, ctx->stream));
    if (n_export) {
        PSK_HIP(ctx, d_nodes.download(nodes_out, (size_t)pool * TREE_NODE_FIELDS, ctx->stream));
        PSK_HIP(ctx, d_imp.download(impurity_out, (size_t)pool, ctx->stream));
        PSK_HIP(ctx, d_leaf.download(leaf_out, (size_t)n_export * n, ctx->stream));
        PSK_HIP(ctx, d_thr.download(threshold_out, (size_t)pool, ctx->stream));
    }
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < n_trees; t++)
        if (node_off[t] >= 0)
            tree_report_impurities(fit_criterion[tree_fit[t]], nodes_out + (size_t)node_off[t] * TREE_NODE_FIELDS,
                                   std::min(node_count_out[t], node_cap[t]), impurity_out + node_off[t]);
    memcpy(tree_node_off_out, node_off.data(), (size_t)n_trees * sizeof(int64_t));
    return PSK_OK;
}
