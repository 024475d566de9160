// What the two tree units (solver_tree.hip: one tree of `-bc DT`; solver_forest.hip: the trees of `-bc RF`) have in common:
// the bit layout of the packed 0/1 design and the kernel that packs it, scikit-learn's impurity expressions, the node
// record, and the host prologue that brings the design to the device.  The fit kernels are each unit's own: they
// parallelise differently on purpose.  Both units are compiled -ffp-contract=off; the f64 expressions here are
// scikit-learn's in its order, and this is their one statement.  solver_nb.hip (`-bc NB`) takes the bit layout, the packing
// kernel and the host prologue from here and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "psk_internal.h"
#include "solver_host.h"

namespace {

constexpr int TREE_NODE_FIELDS = 6;   // feature, left, right, n_node_samples, (weighted) class-0 and class-1 counts

// Word w of column j.  Word-major (W x p, W = ceil(n / 64)): the threads of a wave hold consecutive columns, so a wave's 64
// loads of one word are 512 contiguous bytes.  Column-major (p x W) put them W x 8 B apart, a cache line per lane: the
// 220-fit grid at 2,048 x 1,000 took 3.89 ms in that layout and 2.85 ms in this one (profiles/tree_grid_*; 0.36 ms either way
// at n = 256).
__device__ __forceinline__ size_t tree_bit_at(int j, int w, int p) { return (size_t)w * p + j; }

// bits[w][j]: bit k = X[64 w + k][j]; threads of a workgroup take consecutive columns, so the reads of a sample's row and the
// writes of a word coalesce.  ymask[w]: the same for the labels.  Any value other than 0 or 1 raises bad_flag.
__global__ __launch_bounds__(256) void tree_pack_kernel(const float *__restrict__ X, const int32_t *__restrict__ y01, int n, int p,
                                                        uint64_t *__restrict__ bits, uint64_t *__restrict__ ymask,
                                                        int32_t *__restrict__ bad_flag)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    const int s0 = w * 64, s1 = min(n, s0 + 64);
    if (j < p) {
        uint64_t b = 0;
        bool bad = false;
        for (int s = s0; s < s1; s++) {
            const float x = X[(size_t)s * p + j];
            if (x == 1.0f) b |= 1ull << (s - s0);
            else if (!(x == 0.0f)) bad = true;
        }
        bits[tree_bit_at(j, w, p)] = b;
        if (bad) atomicOr(bad_flag, 1);
    }
    if (j == 0) {
        uint64_t b = 0;
        for (int s = s0; s < s1; s++)
            if (y01[s] != 0) b |= 1ull << (s - s0);
        ymask[w] = b;
    }
}

// scikit-learn's entropy is in bits: sklearn/tree/_utils.pyx defines log(x) as ln(x) / ln(2.0).  (Host and device: the kernels
// search with the device's log; the impurities a call REPORTS are taken again on the host, tree_report_impurities below.)
__host__ __device__ __forceinline__ double tree_log2(double x) { return log(x) / log(2.0); }

// The impurity of a node with (weighted) class counts c0, c1 and nn = c0 + c1: CRIT 0 gini, 1 entropy
template <int CRIT> __host__ __device__ __forceinline__ double tree_impurity(double c0, double c1, double nn)
{
    if (CRIT == 0) {
        double sq = 0.0;
        sq += c0 * c0;
        sq += c1 * c1;
        return 1.0 - sq / (nn * nn);
    }
    double e = 0.0;
    if (c0 > 0.0) { const double c = c0 / nn; e -= c * tree_log2(c); }
    if (c1 > 0.0) { const double c = c1 / nn; e -= c * tree_log2(c); }
    return e;
}

// the same with the criterion known only at run time
__host__ __device__ __forceinline__ double tree_impurity(int crit, double c0, double c1, double nn)
{
    if (crit == 0) return tree_impurity<0>(c0, c1, nn);
    return tree_impurity<1>(c0, c1, nn);
}

// The impurities a call reports, on the host: a node's impurity is tree_impurity of its own (weighted) class counts, whether
// it was made as the root's node_impurity or as its parent's children_impurity, and the counts are exact integers.  Taken
// here they go through the C library's log, the one scikit-learn's Cython calls, so an entropy is scikit-learn's to the bit;
// the device's log differs from it in the last place on some arguments (measured: 32 of 19,509 recorded nodes, one ulp each).
// The kernels keep their own values for the leaf rules and the search.  Only a mixed node's entropy is taken again: gini is
// IEEE +, *, / on both sides, and a pure node's entropy is 1 * log(1) = 0 on both.
inline void tree_report_impurities(int crit, const int32_t *nodes, int count, double *imp)
{
    if (crit == 0) return;
    for (int k = 0; k < count; k++) {
        const int32_t c0 = nodes[(size_t)k * TREE_NODE_FIELDS + 4], c1 = nodes[(size_t)k * TREE_NODE_FIELDS + 5];
        if (c0 > 0 && c1 > 0) imp[k] = tree_impurity<1>((double)c0, (double)c1, (double)c0 + (double)c1);
    }
}

// Node `id` of the tree whose records start at nodes / imp_out (one lane calls this).  Pre-order: a split node's left child
// is the next node; its right child writes its own number into the parent's record when it is made.
__device__ __forceinline__ void tree_write_node(int32_t *__restrict__ nodes, double *__restrict__ imp_out, int id, int parent,
                                                bool is_left, int feat, bool is_leaf, int n, int c0, int c1, double imp)
{
    int32_t *nd = nodes + (size_t)id * TREE_NODE_FIELDS;
    nd[0] = feat;
    nd[1] = is_leaf ? -1 : id + 1;
    nd[2] = -1;
    nd[3] = n;
    nd[4] = c0;
    nd[5] = c1;
    imp_out[id] = imp;
    if (parent >= 0 && !is_left) nodes[(size_t)parent * TREE_NODE_FIELDS + 2] = id;
}

// The prologue of both entry points: X[n][p] and y01[n] go to the device and are packed into bits (W x p words) and ymask
// (W words).  A design that holds anything but 0 and 1 fails in the name of the caller, `who`.  Returns with the stream
// idle, so the float design is freed here.
inline int tree_pack_design(psk_ctx *ctx, const char *who, const float *X, const int32_t *y01, int n, int p,
                            FitArr<uint64_t> &bits, FitArr<uint64_t> &ymask)
{
    const int W = (n + 63) / 64;
    FitArr<float> x;
    FitArr<int32_t> bad_flag, y;
    PSK_HIP(ctx, x.upload(X, (size_t)n * p, ctx->stream));
    PSK_HIP(ctx, y.upload(y01, n, ctx->stream));
    PSK_HIP(ctx, bits.alloc((size_t)p * W));
    PSK_HIP(ctx, ymask.alloc(W));
    PSK_HIP(ctx, bad_flag.alloc(1));
    PSK_HIP(ctx, bad_flag.zero(ctx->stream));
    tree_pack_kernel<<<dim3(div_up(p, 256), W), 256, 0, ctx->stream>>>(x, y, n, p, bits, ymask, bad_flag);
    PSK_HIP(ctx, hipGetLastError());
    int32_t bad = 0;
    PSK_HIP(ctx, bad_flag.download(&bad, 1, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad) return psk_fail(ctx, PSK_EINVAL, "%s takes a 0/1 design (k-mer presence): the matrix holds another value", who);
    return PSK_OK;
}

// ---- count designs (psk_tree_fit_counts, psk_forest_fit_counts) ----
// A column with the distinct values g_0 < g_1 < ... (over all n samples) becomes one THRESHOLD PLANE per gap: plane k has bit
// s = (x_s >= g_(k+1)), in the layout of the 0/1 design (tree_bit_at over P planes in place of p columns); planes are ordered
// by (column, k), a constant column has none.  A 0/1 column is its own single plane.  Inside a node, planes of one column
// that lie between the same two values present in the node give the same partition, so "the first strictly larger proxy over
// the planes in index order" is scikit-learn's walk over the gaps between the values present in the node.
constexpr int TREE_PLANE_CAP = 1 << 20;           // planes per call (PSK_TREE_PLANE_CAP): 8 MB of plane words per 64 samples
constexpr float TREE_COUNT_MAX = 16777216.0f;     // 2^24: every integer up to it is a float

struct TreePlanes {
    FitArr<uint64_t> bits;        // [W][P]
    FitArr<float> x;              // the float design [n][p]: a node's threshold is taken from the values present in it
    FitArr<int32_t> col_first;    // [p + 1]: the planes of column j are col_first[j] .. col_first[j + 1] - 1
    FitArr<int32_t> plane_col;    // [P]
    FitArr<int32_t> col_order;    // [p]: the columns by falling number of planes (a kernel that walks a column per thread takes
                                  //      them in this order, so the threads of a round have about the same work)
    FitArr<float> plane_val;      // [P]: g_(k+1), the smallest value on the plane's right side
    int P = 0;
};

// what a fit kernel reads of them; empty in the 0/1 instantiations, whose arguments and code stay what they were
template <bool COUNTS> struct TreePlaneView {};
template <> struct TreePlaneView<true> {
    const float *X;
    const int32_t *col_first, *plane_col, *col_order;
    const float *plane_val;
    int p;                        // columns of the design (the kernels' own p counts planes)
};

// bits[w][q]: bit k = (X[64 w + k][plane_col[q]] >= plane_val[q]); ymask as tree_pack_kernel writes it.  Threads of a wave
// take consecutive planes, mostly of one column: their reads of a sample fall into one or two cache lines.
__global__ __launch_bounds__(256) void tree_pack_planes_kernel(const float *__restrict__ X, const int32_t *__restrict__ y01, int n, int p,
                                                               int P, const int32_t *__restrict__ plane_col,
                                                               const float *__restrict__ plane_val, uint64_t *__restrict__ bits,
                                                               uint64_t *__restrict__ ymask)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    const int s0 = w * 64, s1 = min(n, s0 + 64);
    if (q < P) {
        const int col = plane_col[q];
        const float v = plane_val[q];
        uint64_t b = 0;
        for (int s = s0; s < s1; s++)
            if (X[(size_t)s * p + col] >= v) b |= 1ull << (s - s0);
        bits[tree_bit_at(q, w, P)] = b;
    }
    if (q == 0) {
        uint64_t b = 0;
        for (int s = s0; s < s1; s++)
            if (y01[s] != 0) b |= 1ull << (s - s0);
        ymask[w] = b;
    }
}

// scikit-learn's threshold of a split of column `col` whose right side starts at `val`, in the node whose in-bag samples are
// the mask words MT (LDS): lo / 2.0 + hi / 2.0 of the largest value on the left and the smallest on the right among THOSE
// samples.  Values are integers up to 2^24, so the two extremes are integer atomics on gap[0..1] (LDS; the order of the
// lanes cannot matter).  Called by every thread of the workgroup; the first barrier lets the caller reuse words it has read.
__device__ __forceinline__ double tree_node_threshold(const float *__restrict__ X, int n, int p, int col, float val,
                                                      const uint64_t *MT, int *gap)
{
    __syncthreads();
    if (threadIdx.x == 0) { gap[0] = -1; gap[1] = INT_MAX; }
    __syncthreads();
    for (int s = threadIdx.x; s < n; s += blockDim.x)
        if ((MT[s >> 6] >> (s & 63)) & 1ull) {
            const float x = X[(size_t)s * p + col];
            if (x < val) atomicMax(&gap[0], (int)x);
            else atomicMin(&gap[1], (int)x);
        }
    __syncthreads();
    return (double)gap[0] / 2.0 + (double)gap[1] / 2.0;
}

// The plane that routes by that threshold: k with g_k <= threshold < g_(k+1) over ALL samples' values, not the plane that won
// the search -- values absent from the node (held-out samples, other branches) may lie between lo and hi, and x <= threshold
// decides their side.  It exists: hi is one of the column's values and lies above the threshold.
__device__ __forceinline__ int tree_route_plane(const int32_t *__restrict__ col_first, const float *__restrict__ plane_val, int col,
                                                double thr)
{
    int lo = col_first[col], hi = col_first[col + 1] - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)plane_val[mid] > thr) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The prologue of the two count entry points: checks the values (integers in 0 .. 2^24), finds every column's distinct values
// on the host, and brings the design, the plane tables, the planes and ymask to the device.  Returns with the stream idle.
inline int tree_pack_counts(psk_ctx *ctx, const char *who, const float *X, const int32_t *y01, int n, int p, TreePlanes &pl,
                            FitArr<uint64_t> &ymask)
{
    constexpr int CHUNK = 16, TABLE = 4096;   // columns gathered per pass over the rows; values below TABLE are marked, not sorted
    std::vector<int32_t> col_first((size_t)p + 1, 0), plane_col;
    std::vector<float> plane_val, buf((size_t)CHUNK * n);
    std::vector<uint8_t> seen(TABLE);
    for (int j0 = 0; j0 < p; j0 += CHUNK) {
        const int jc = std::min(CHUNK, p - j0);
        for (int i = 0; i < n; i++)
            for (int c = 0; c < jc; c++) {
                const float v = X[(size_t)i * p + j0 + c];
                if (!(v >= 0.0f && v <= TREE_COUNT_MAX && v == floorf(v)))
                    return psk_fail(ctx, PSK_EINVAL, "%s takes a count design (integers in 0 .. 2^24): sample %d, column %d holds %g", who,
                                    i, j0 + c, (double)v);
                buf[(size_t)c * n + i] = v;
            }
        for (int c = 0; c < jc; c++) {
            float *v = buf.data() + (size_t)c * n;
            const float top = *std::max_element(v, v + n);
            const size_t first = plane_val.size();
            if (top < (float)TABLE) {
                std::fill(seen.begin(), seen.end(), 0);
                for (int i = 0; i < n; i++) seen[(int)v[i]] = 1;
                bool lowest = true;
                for (int g = 0; g <= (int)top; g++)
                    if (seen[g]) {
                        if (!lowest) plane_val.push_back((float)g);
                        lowest = false;
                    }
            } else {
                std::sort(v, v + n);
                for (int i = 1; i < n; i++)
                    if (v[i] != v[i - 1]) plane_val.push_back(v[i]);
            }
            plane_col.insert(plane_col.end(), plane_val.size() - first, j0 + c);
            if (plane_val.size() > (size_t)TREE_PLANE_CAP)
                return psk_fail(ctx, PSK_ERANGE, "%s: the design needs more than %d threshold planes (one per gap between the distinct "
                                "values of a column; PSK_TREE_PLANE_CAP)", who, TREE_PLANE_CAP);
            col_first[j0 + c + 1] = (int32_t)plane_val.size();
        }
    }
    std::vector<int32_t> col_order(p);
    for (int j = 0; j < p; j++) col_order[j] = j;
    std::stable_sort(col_order.begin(), col_order.end(), [&](int32_t a, int32_t b) {
        return col_first[a + 1] - col_first[a] > col_first[b + 1] - col_first[b];
    });
    const int W = (n + 63) / 64, P = pl.P = (int)plane_val.size();
    FitArr<int32_t> y;
    PSK_HIP(ctx, pl.x.upload(X, (size_t)n * p, ctx->stream));
    PSK_HIP(ctx, y.upload(y01, n, ctx->stream));
    PSK_HIP(ctx, pl.col_first.upload(col_first, ctx->stream));
    PSK_HIP(ctx, pl.plane_col.upload(plane_col, ctx->stream));
    PSK_HIP(ctx, pl.col_order.upload(col_order, ctx->stream));
    PSK_HIP(ctx, pl.plane_val.upload(plane_val, ctx->stream));
    PSK_HIP(ctx, pl.bits.alloc((size_t)P * W));
    PSK_HIP(ctx, ymask.alloc(W));
    tree_pack_planes_kernel<<<dim3(div_up(std::max(P, 1), 256), W), 256, 0, ctx->stream>>>(pl.x, y, n, p, P, pl.plane_col, pl.plane_val,
                                                                                       pl.bits, ymask);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

}  // namespace
