// What the two tree units (solver_tree.hip: one tree of `-bc DT`; solver_forest.hip: the trees of `-bc RF`) have in common:
// the bit layout of the packed 0/1 design and the kernel that packs it, scikit-learn's impurity expressions, the node
// record, and the host prologue that brings the design to the device.  The fit kernels are each unit's own: they
// parallelise differently on purpose.  Both units are compiled -ffp-contract=off; the f64 expressions here are
// scikit-learn's in its order, and this is their one statement.  solver_nb.hip (`-bc NB`) takes the bit layout, the packing
// kernel and the host prologue from here and nothing else.
#pragma once
#include <hip/hip_runtime.h>

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

// scikit-learn's entropy is in bits: sklearn/tree/_utils.pyx defines log(x) as ln(x) / ln(2.0)
__device__ __forceinline__ double tree_log2(double x) { return log(x) / log(2.0); }

// The impurity of a node with (weighted) class counts c0, c1 and nn = c0 + c1: CRIT 0 gini, 1 entropy
template <int CRIT> __device__ __forceinline__ double tree_impurity(double c0, double c1, double nn)
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
__device__ __forceinline__ double tree_impurity(int crit, double c0, double c1, double nn)
{
    if (crit == 0) return tree_impurity<0>(c0, c1, nn);
    return tree_impurity<1>(c0, c1, nn);
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

}  // namespace
