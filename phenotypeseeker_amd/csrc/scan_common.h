// What the association scans share (assoc_scan.hip, chi2_driver.hip: chi2; ttest_scan.hip: Welch; scan_results.hip: their result sets):
// the kernel arguments, the result-segment protocol, the row stream both scan kernels are built on, the lane-per-row
// moment forms, and the host's dispatch over the lanes-per-row constant.  Templates and inline device code only: a
// kernel is instantiated by the one unit that launches it.
#pragma once
#include "dev_utils.h"
#include "psk_internal.h"
#include "chi2_plan.h"
#include "scan_stamps.h"

#include <hip/hip_ext.h>
#include <type_traits>

// tuning knobs (overridable at build time for A/B runs: make EXTRA=-DPSK_SC_UNROLL=...)
#ifndef PSK_SC_UNROLL
#define PSK_SC_UNROLL 4
#endif
#ifndef PSK_SC_GRID_MULT
#define PSK_SC_GRID_MULT 16
#endif
#ifndef PSK_SC_NT
#define PSK_SC_NT 1
#endif
constexpr int SC_THREADS = 256;
#ifndef PSK_LUT_THREADS
#define PSK_LUT_THREADS 1024
#endif
constexpr int SC_LUT_THREADS = PSK_LUT_THREADS;   // workgroup of the moment scans that keep their nibble tables in LDS (one per CU)
constexpr size_t SC_LUT_MAX_BYTES = 132 * 1024;
constexpr int SC_UNROLL = PSK_SC_UNROLL;
// Survivors are appended to SC_NSEG independent segments (segment = blockIdx % SC_NSEG), each with its
// own counter on its own 128-byte line: one shared counter serialises at ~11 ns per append (r01: a
// matrix with 1 % survivors ran 15x slower than the stream rate).
constexpr int SC_NSEG = 256;
constexpr int SC_CNT_STRIDE = 32;  // u32 per counter slot
constexpr int SC_INL_WORDS = 16;   // mask words carried inside ScanArgs
static_assert(CX_WAVES * 64 == SC_THREADS && CX_NSEG == SC_NSEG, "chi2_plan.h restates the launch constants");
static_assert(STAMP_NSEG == SC_NSEG, "scan_stamps.h restates the number of segments");
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ScanArgs {
    const u32x4 *bits;
    uint64_t M;
    int cpr;  // 16-byte chunks per row = wpr / 2 (1 when half)
    int half; // rows are ONE u64 (<= 64 samples): row r sits at byte 8 r; masks / tables as for one chunk
    // chi2
    const uint64_t *m1, *m0;   // phenotype == 1 / == 0 masks (wpr words each)
    const double *tab;         // per-sample table of the lane-per-row pass: [wpr*64][NM] doubles (see row_moments)
    const double *lut;         // the same table summed over every subset of each group of 4 samples (row_moments_lut)
    int c_lut;                 // ... for the first c_lut chunks of a row; the rest of the row takes the per-sample form
    const double *raw;         // Welch: {weight (0 for NA), phenotype value (0 for NA)} per sample, for the exact second pass
    const float *lut6;         // f32 six-bit table of the same moments (row_moments_f32) -- candidate selection only
    double e0, e1, e2;         // ... and what its sums may be off by: |sum w| <= e0, |sum w u| <= e1, |sum w u^2| <= e2 (chi2: e0 = class 1, e1 = class 0)
    double eref;               // Welch: what the REFERENCE's own arithmetic may be off by in a group mean (it sums the raw, unshifted values)
    double W1, W0;             // weight totals of the two phenotype classes
    // t-test
    const uint64_t *mvalid;    // non-NA mask
    int nvalid;
    double tcrit;              // t-test: |t| a row must exceed to be a candidate
    ScanCuts cut;              // class sizes, filters, cut-offs
    ScanSink sink;             // output
    // phenotype masks of up to 1024 samples travel in the kernel arguments (no upload per scan)
    int inline_masks;
    uint64_t m1_inl[SC_INL_WORDS], m0_inl[SC_INL_WORDS];
};

__device__ __forceinline__ uint64_t reserve_slot(const ScanSink &S)
{
    const uint32_t seg = blockIdx.x & (SC_NSEG - 1);
    const uint32_t idx = atomicAdd(&S.counter[seg * SC_CNT_STRIDE], 1u);
    return (uint64_t)seg * S.seg_cap + (idx < S.seg_cap ? idx : S.seg_cap - 1);
}

// a candidate of a moment scan: (row, n_with) only -- the scan's second pass computes its statistic and decides
__device__ __forceinline__ void append_candidate(const ScanSink &S, uint64_t row, int n_w)
{
    const uint64_t idx = reserve_slot(S);
    S.res_row[idx] = row;
    S.res_nw[idx] = n_w;
}

// ---- stamps: what the host learns of a scan straight from its kernels (scan_stamps.h) ------------------------------------
// One relaxed system-scope store of an aligned 8-byte word into pinned, coherent host memory: value and tag arrive
// together, so no fence and no second atomic go with it.
__device__ __forceinline__ void stamp_store(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void stamp_clock(const ScanSink &S, int slot) { stamp_store(S.host_counts + STAMP_NSEG + slot, stamp_clock_word(S.seq, (uint64_t)wall_clock64())); }
// a segment's count (the finalize kernels of the two-kernel scans: they are waited for and timed by events)
__device__ __forceinline__ void stamp_count(const ScanSink &S, uint32_t seg, uint32_t c) { stamp_store(S.host_counts + seg, stamp_count_word(S.seq, c)); }
// The ticket line of the single-kernel chi2 scans (scan_stamps.h: stamp_ticket_*): one more 128-byte counter line behind
// the two sets' final_counts, part of the same allocation and of its one memset (bind_results), shared by both result
// sets as the segment counters are -- the scans of a context run one after the other on its stream.
constexpr int SC_TICKET_OFFSET = SC_NSEG * SC_CNT_STRIDE + 2 * SC_NSEG;   // u32 from ScanSink::counter
constexpr int SC_COUNTER_WORDS = SC_TICKET_OFFSET + SC_CNT_STRIDE;        // u32 of the whole counter block
static_assert(SC_TICKET_OFFSET % SC_CNT_STRIDE == 0, "the ticket line starts a 128-byte line");
// Called by the one thread that has just published segment count c (a segment some workgroup maps to: the unowned
// segments of a short launch take no ticket).  One 64-bit atomic adds the count and a ticket and returns the scan's sum
// so far; whoever draws the last ticket therefore holds n_pass -- every other publisher added its count in the same
// atomic that took its ticket, so, as in publish_segment_once, no fence is needed -- and writes the summary line the
// host polls: the end clock and n_pass in two words, each tagged.  It re-arms the line for the next scan with one store,
// at device scope and not a plain one as publish_segment_once's: a segment's workgroups need not share an L2 with this
// line's other writers.  Nothing waits here: a publisher that is not the last simply ends.
__device__ __forceinline__ void publish_summary(const ScanSink &S, uint32_t c)
{
    unsigned long long *line = reinterpret_cast<unsigned long long *>(S.counter + SC_TICKET_OFFSET);
    const uint64_t add = stamp_ticket_addend(c, S.seg_cap);
    const uint64_t before = atomicAdd(line, (unsigned long long)add);
    if (!stamp_ticket_is_last(before, stamp_ticket_publishers(gridDim.x))) return;
    __hip_atomic_store(line, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t after = before + add;
    stamp_store(S.host_counts + STAMP_SUM_END, stamp_clock_word(S.seq, (uint64_t)wall_clock64()));
    stamp_store(S.host_counts + STAMP_SUM_LO, stamp_sum_lo_word(S.seq, stamp_ticket_total(after)));
    stamp_store(S.host_counts + STAMP_SUM_HI, stamp_sum_hi_word(S.seq, stamp_ticket_total(after), stamp_ticket_overflow(after)));
}
// a published segment of a single-kernel chi2 scan: its count word, and in a launch small enough for the summary
// (stamp_summary_used) its ticket; in a larger one the clock just before the count, as until r31
__device__ __forceinline__ void stamp_segment(const ScanSink &S, uint32_t seg, uint32_t c)
{
    if (stamp_summary_used(gridDim.x)) {
        stamp_count(S, seg, c);
        publish_summary(S, c);
    } else {
        stamp_clock(S, (int)seg);
        stamp_count(S, seg, c);
    }
}
// first thing in a single-kernel chi2 scan: the start clock
__device__ __forceinline__ void stamp_scan_start(const ScanSink &S)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) stamp_clock(S, STAMP_START);
}

// Called by every thread at the very end of a chi2 scan workgroup: the LAST workgroup of a segment to get here
// publishes the segment's count and re-arms the counter (ticket = second word of the counter's 128-byte line).
__device__ __forceinline__ void publish_segment(const ScanSink &S)
{
    // No fence: the count lives in device-scope atomics only, and every append of this workgroup has returned
    // its slot index (it was needed for the stores) before the barrier.  A __threadfence() here is an L2
    // write-back + invalidate per workgroup on this multi-XCD part and tripled the kernel time (r01).
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t seg = blockIdx.x & (SC_NSEG - 1);
    const uint32_t n_blocks = (gridDim.x - seg + SC_NSEG - 1) / SC_NSEG;  // workgroups that map to this segment
    uint32_t *slot = &S.counter[seg * SC_CNT_STRIDE];
    if (atomicAdd(slot + 1, 1u) == n_blocks - 1) {
        const uint32_t c = atomicExch(slot, 0u);
        slot[1] = 0;
        S.final_counts[seg] = c;
        stamp_segment(S, seg, c);
    }
}

// The same for a kernel whose workgroups end one atomic round trip sooner: the slot's two words are one aligned u64 (count
// low, tickets high), and adding 1 << 32 returns both -- every append of the scan was counted before the last ticket,
// so the last workgroup has the segment's count with its ticket and re-arms the slot with a plain store.  (The count
// stays below 2^32: a scan has fewer rows.)  Interchangeable with publish_segment from launch to launch.
__device__ __forceinline__ void publish_segment_once(const ScanSink &S)
{
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t seg = blockIdx.x & (SC_NSEG - 1);
    const uint32_t n_blocks = (gridDim.x - seg + SC_NSEG - 1) / SC_NSEG;  // workgroups that map to this segment
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(&S.counter[seg * SC_CNT_STRIDE]);
    const unsigned long long old = atomicAdd(slot, 1ull << 32);
    if ((uint32_t)(old >> 32) == n_blocks - 1) {
        const uint32_t c = (uint32_t)old;
        *slot = 0ull;
        S.final_counts[seg] = c;
        stamp_segment(S, seg, c);
    }
}

// A launch of fewer than SC_NSEG workgroups (chi2_scan_kernel_cx_side_idx) has segments that no workgroup maps to:
// [gridDim.x, SC_NSEG).  Nothing is appended to them, so their counter lines stand at zero as the last scan's publish left
// them; every thread of ONE workgroup calls this and thread i publishes segments gridDim.x + i, + blockDim.x, ... as
// empty -- the compact count and the count word -- so a wave's stores are consecutive 8-byte words.  They take no ticket
// (publish_summary counts min(gridDim.x, SC_NSEG) publishers); in a launch too large for the summary they get their clock
// word as well.  With the owned segments' publish_segment_once this leaves a result set exactly as a launch of SC_NSEG
// workgroups does.
__device__ __forceinline__ void publish_unowned_segments(const ScanSink &S)
{
    const bool clocks = !stamp_summary_used(gridDim.x);
    for (uint32_t seg = gridDim.x + threadIdx.x; seg < (uint32_t)SC_NSEG; seg += blockDim.x) {
        S.final_counts[seg] = 0;
        if (clocks) stamp_clock(S, (int)seg);
        stamp_count(S, seg, 0);
    }
}

// ---- host functions that cross the units ----------------------------------------------------------------------------
// scan_results.hip
int mask_words(const psk_ctx *ctx);
int group_lanes(const ScanArgs &a);
uint64_t scan_grid_cap(const psk_ctx *ctx);
dim3 scan_grid(const psk_ctx *ctx, uint64_t M, int G, int unroll, bool lut = false);
uint64_t result_seg_cap(dim3 grid, uint64_t rows_per_block);   // chi2_plan.h's arithmetic on grid.x
int bind_results(psk_ctx *ctx, ScanSink &s, uint64_t seg_cap, int set);
int setup_results_rows(psk_ctx *ctx, ScanSink &s, dim3 grid, uint64_t rows_per_block, int set);
int setup_results(psk_ctx *ctx, ScanArgs &a, dim3 grid, int G, int unroll, int set, int threads = SC_THREADS);
int pick_result_set(psk_ctx *ctx, int *set_out, bool keep_results = false);
int fetch_counts(psk_ctx *ctx, int set);
void hold_results_unread(psk_ctx *ctx, int set, uint64_t n_pass);
int held_seg_counts(psk_ctx *ctx, const std::vector<uint32_t> **counts);
const volatile uint64_t *scan_stamp_words(const psk_ctx *ctx, int set);
// chi2_driver.hip: the bounded wait for words of result set `set` that its scan's kernel stamps
enum StampWait {
    STAMP_WAIT_SUMMARY,   // the summary line: the scan has ended, n_pass and its time are there
    STAMP_WAIT_COUNTS,    // the STAMP_NSEG count words
    STAMP_WAIT_ALL,       // both (PSK_SCAN_SUMMARY=0: the counts are summed by the host, the time is the summary's)
    STAMP_WAIT_SEGMENTS,  // the count words and the STAMP_CLOCKS clock words of a launch too large for the summary: as until r31
};
int wait_stamps(psk_ctx *ctx, int set, StampWait what);
// ttest_scan.hip: the moment tables (their two building kernels live there, for both scans)
struct ScanShape {   // what a scan launches with
    dim3 grid;
    int unroll, threads;
};
int setup_table_scan(psk_ctx *ctx, ScanArgs &a, const double *tab, int nm, double s0, double s1, double s2, bool build, ScanShape *sh);

// ---- rows -----------------------------------------------------------------------------------------
// G = 0 stands for "half a lane per row" (8-byte rows, two per 16-byte load)
constexpr int sc_rpw(int G) { return G == 0 ? 128 : 64 / G; }   // rows per wave step
constexpr int sc_lanes(int G) { return G == 0 ? 1 : G; }        // lanes that share a load group
template <bool HALF>
__device__ __forceinline__ const u32x4 *sc_row_ptr(const ScanArgs &P, uint64_t r)
{
    if (HALF) return reinterpret_cast<const u32x4 *>(reinterpret_cast<const uint2 *>(P.bits) + r);
    return P.bits + r * (uint64_t)P.cpr;
}
// chunk ch of the row at rp; an 8-byte row is its chunk 0 with an empty upper half
template <bool HALF>
__device__ __forceinline__ u32x4 sc_ld_chunk(const u32x4 *__restrict__ rp, int ch)
{
    if (HALF) {
        const uint2 v = *reinterpret_cast<const uint2 *>(rp);
        return (u32x4){v.x, v.y, 0u, 0u};
    }
    return rp[ch];
}

// ---- lane-per-row moments -----------------------------------------------------------------------
// Rows that pass the popcount frequency filter need f64 sums over their present samples (class weight
// sums for the weighted chi2, weighted moments for Welch).  They are queued per wave and handled 64 at a
// time, ONE ROW PER LANE: every lane walks its own row while all lanes visit the same sample s at the
// same time, so the per-sample table entries tab[s][0..NM) are wave-uniform and come through the scalar
// data cache into SGPRs (constant address space => s_load), not through LDS or the vector pipe.  A cell
// costs 2 + NM VALU ops: the presence bit becomes 0.0 / 1.0 (v_bfe_i32 + v_and 0x3FF00000 on the high
// word), then one v_fma_f64 per moment with the table entry as an SGPR operand -- no cross-lane
// reduction at all.  The sums associate differently from the reference's sample-order loops (two interleaved
// accumulators here, groups of four samples in the table form below): ~1e-15 relative from the reference.  The Welch
// statistics are used as they come (compared at 1e-8); the weighted chi2 uses these sums for its pre-test only and
// re-sums the candidates in the reference's order (chi2w_finalize_kernel; DESIGN.md "Exactness strategy").
// (r01: the previous whole-wave-per-row form spent ~1000 cycles per row in LDS latency and three DPP wave
// sums: 11.1 ms for 16 M x 1024 with a third of the rows passing.)
typedef const __attribute__((address_space(4))) double *cdptr;
// queue entries per wave: < 64 carried over + <= 64 / G appended per step of an unrolled batch
constexpr int rq_cap(int G, int unroll = SC_UNROLL) { return 64 + (G == 0 ? 128 : 64 / G) * unroll; }
#ifndef PSK_LUT_UNROLL
#define PSK_LUT_UNROLL 8
#endif
#ifndef PSK_LUT_NT
#define PSK_LUT_NT 1     // streaming loads of the table-in-LDS kernels carry the nontemporal hint
#endif
// rows in flight per lane group of the table-in-LDS kernels (half the waves per CU of the plain ones); fewer where a
// wave step covers many rows, so that the waves' queues stay small beside the table
constexpr int lut_unroll(int G) { return G == 0 ? (PSK_LUT_UNROLL < 2 ? PSK_LUT_UNROLL : 2) : G == 1 ? (PSK_LUT_UNROLL < 4 ? PSK_LUT_UNROLL : 4) : G == 2 ? (PSK_LUT_UNROLL < 8 ? PSK_LUT_UNROLL : 8) : PSK_LUT_UNROLL; }

template <int NM, bool HALF = false>
__device__ __forceinline__ void row_moments(const u32x4 *__restrict__ rp, int cpr, cdptr tab, double *acc)
{
    double a0[NM], a1[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) { a0[m] = 0.0; a1[m] = 0.0; }
    u32x4 y = sc_ld_chunk<HALF>(rp, 0);
    for (int ch = 0; ch < cpr; ch++) {
        const uint32_t w4[4] = {y.x, y.y, y.z, y.w};
        if (ch + 1 < cpr) y = rp[ch + 1];
        cdptr tp = tab + (size_t)ch * 128 * NM;
#pragma unroll
        for (int h = 0; h < (HALF ? 2 : 4); h++) {
#pragma unroll
            for (int b = 0; b < 32; b += 2) {
                const uint32_t h0 = (uint32_t)(((int32_t)(w4[h] << (31 - b))) >> 31) & 0x3FF00000u;
                const uint32_t h1 = (uint32_t)(((int32_t)(w4[h] << (30 - b))) >> 31) & 0x3FF00000u;
                const double f0 = __hiloint2double((int)h0, 0), f1 = __hiloint2double((int)h1, 0);
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    a0[m] = fma(f0, tp[(h * 32 + b) * NM + m], a0[m]);
                    a1[m] = fma(f1, tp[(h * 32 + b + 1) * NM + m], a1[m]);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < NM; m++) acc[m] = a0[m] + a1[m];
}

// The same sums from a nibble table: lut[g][p][0..NM) = sum of tab[4 g + b] over the bits b set in p (ascending b), for
// every group g of 4 samples and every 4-bit pattern p, held in LDS.  A lane then spends one nibble extract, one
// address and ONE LDS read + NM adds per FOUR samples instead of (2 + NM) VALU instructions per sample: the lanes of
// a wave (64 different rows) look up the same group at the same time, so their 16 possible addresses are 16 x NM x 8
// consecutive bytes -- for NM = 2 exactly the 64 banks, without a conflict; equal patterns are broadcast.
// (r01: the per-sample form was f64-VALU bound, 0.76 ms for 16 M x 1024 with 20 % of the rows passing.)
// The sums associate differently from the reference's sample-order loops: a group's members are added first, then
// the groups in order (two interleaved accumulators, as before) -- 1e-15 relative, see DESIGN.md "Exactness".
// (the table is built by moment_lut_kernel, ttest_scan.hip)
// bytes of the nibble table of row_moments_lut for `chunks` 16-byte chunks of a row and NM moments
inline size_t lut_bytes(int chunks, int nm) { return (size_t)chunks * 32 * 16 * nm * 8; }

// The row itself is read SC_LUT_PF chunks at a time, all loads issued before the first lookup: read one chunk ahead
// (r02 at first) every chunk paid a global-load latency of its own, and THAT, not the LDS pipe, set the time of the pass
// (~8 us per 64 rows of 1024 samples against 1.7 us of lookups).
constexpr int SC_LUT_PF = 8;
template <int NM, bool HALF = false>
__device__ __forceinline__ void row_moments_lut(const u32x4 *__restrict__ rp, int cpr, const double *lut, double *acc)
{
    double a0[NM], a1[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) { a0[m] = 0.0; a1[m] = 0.0; }
    for (int c0 = 0; c0 < cpr; c0 += SC_LUT_PF) {
        u32x4 y[SC_LUT_PF];
#pragma unroll
        for (int i = 0; i < SC_LUT_PF; i++) y[i] = c0 + i < cpr ? sc_ld_chunk<HALF>(rp, c0 + i) : (u32x4)(0u);
#pragma unroll
        for (int i = 0; i < SC_LUT_PF; i++) {
            if (c0 + i >= cpr) break;
            const uint32_t w4[4] = {y[i].x, y[i].y, y[i].z, y[i].w};
            // 32 groups of 4 samples per 16-byte chunk.  NM = 3: entries of 24 bytes were read as ds_read2_b64 + ds_read_b64
            // (8 + 2 LDS cycles, banks mod 32); pairs {m0, m1} and a separate table of m2 are a ds_read_b128 and a
            // ds_read_b64 (4 + 2 cycles, both conflict-free: 16 entries = 64 resp. 32 of the 64 banks)
            const double *lp = lut + (size_t)(c0 + i) * 32 * 16 * (NM == 3 ? 2 : NM);
            const double *lp2 = lut + (size_t)cpr * 32 * 16 * 2 + (size_t)(c0 + i) * 32 * 16;   // NM = 3 only
#pragma unroll
            for (int h = 0; h < (HALF ? 2 : 4); h++) {
#pragma unroll
                for (int k = 0; k < 8; k += 2) {
                    const uint32_t i0 = (h * 8 + k) * 16 + ((w4[h] >> (4 * k)) & 15u), i1 = (h * 8 + k + 1) * 16 + ((w4[h] >> (4 * k + 4)) & 15u);
                    const double *e0 = lp + i0 * (NM == 3 ? 2 : NM);
                    const double *e1 = lp + i1 * (NM == 3 ? 2 : NM);
                    if (NM == 3) {
                        const double2 v0 = *reinterpret_cast<const double2 *>(__builtin_assume_aligned(e0, 16));
                        const double2 v1 = *reinterpret_cast<const double2 *>(__builtin_assume_aligned(e1, 16));
                        a0[0] += v0.x; a0[1] += v0.y; a1[0] += v1.x; a1[1] += v1.y;
                        a0[NM - 1] += lp2[i0]; a1[NM - 1] += lp2[i1];
                    } else if (NM == 2) {
                        // ONE 16-byte read per entry (ds_read_b128: 4 LDS cycles, banks mod 64, the 16 entries of a
                        // group = the 64 banks).  Read as two doubles it became ds_read2_b64 -- 8 cycles, banks mod 32,
                        // every group 2-way conflicted: 41 % of the LDS cycles of the pass (SQ_LDS_BANK_CONFLICT, r02)
                        const double2 v0 = *reinterpret_cast<const double2 *>(__builtin_assume_aligned(e0, 16));
                        const double2 v1 = *reinterpret_cast<const double2 *>(__builtin_assume_aligned(e1, 16));
                        a0[0] += v0.x; a0[NM - 1] += v0.y; a1[0] += v1.x; a1[NM - 1] += v1.y;
                    } else {
#pragma unroll
                        for (int m = 0; m < NM; m++) { a0[m] += e0[m]; a1[m] += e1[m]; }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < NM; m++) acc[m] = a0[m] + a1[m];
}

// ---- six-bit tables in f32: candidate selection at a third of the cost ------------------------------------------------
// Since r03 every moment scan decides in a second kernel that re-sums its candidates exactly (chi2w_finalize_kernel,
// ttest_finalize_kernel), so the sums of the streaming kernel only have to be good enough to not MISS a candidate.  They are
// therefore taken in f32 from a table over groups of SIX samples: a 16-byte chunk of a row is 21 six-bit groups + one
// two-bit group, i.e. 22 lookups instead of 32; an entry of two moments is 8 bytes (one ds_read_b64, 4 LDS cycles
// instead of 8) and is accumulated by ONE v_pk_add_f32 (4 VALU cycles instead of two v_add_f64 = 16).  The kernel turns
// the f32 sums into an UPPER bound of the statistic with the rounding-error bounds the host derives from the table
// itself (e0, e1, e2: (additions per accumulator + 3) x 2^-24 x the sum of the absolute terms over all samples, which
// bounds the error of any subset's f32 sum), and every row whose bound reaches the threshold is a candidate.
// Layout: per chunk 21 x 64 + 4 = SC_L6_ENTRIES entries; float2 {m0, m1} per entry, then -- three moments -- one float
// per entry in a second table behind the first.  1,024 samples: 86 KB (two moments), 129 KB (three).
constexpr int SC_L6_ENTRIES = 21 * 64 + 4;
__host__ __device__ inline size_t lut6_bytes(int chunks, int nm) { return (size_t)chunks * SC_L6_ENTRIES * (nm == 3 ? 12 : 8); }
// (built by moment_lut6_kernel, ttest_scan.hip)

typedef float sc_f32x2 __attribute__((ext_vector_type(2)));

// f32 sums of NM moments over the present samples of one row (one row per lane), from the six-bit tables in LDS
template <int NM, bool HALF = false>
__device__ __forceinline__ void row_moments_f32(const u32x4 *__restrict__ rp, int cpr, const float *lut, double *acc)
{
    sc_f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
    float c0 = 0.f, c1 = 0.f;
    const float *lut3 = lut + (size_t)cpr * SC_L6_ENTRIES * 2;   // NM = 3 only
    for (int g0 = 0; g0 < cpr; g0 += SC_LUT_PF) {
        u32x4 y[SC_LUT_PF];
#pragma unroll
        for (int i = 0; i < SC_LUT_PF; i++) y[i] = g0 + i < cpr ? sc_ld_chunk<HALF>(rp, g0 + i) : (u32x4)(0u);
#pragma unroll
        for (int i = 0; i < SC_LUT_PF; i++) {
            if (g0 + i >= cpr) break;
            const uint32_t w4[5] = {y[i].x, y[i].y, y[i].z, y[i].w, 0u};
            const sc_f32x2 *lp = reinterpret_cast<const sc_f32x2 *>(lut) + (size_t)(g0 + i) * SC_L6_ENTRIES;
            const float *lp3 = lut3 + (size_t)(g0 + i) * SC_L6_ENTRIES;
#pragma unroll
            for (int j = 0; j < (HALF ? 11 : 22); j++) {   // an 8-byte row: samples 0 ... 63 lie in groups 0 ... 10
                const int o = 6 * j, wi = o >> 5, sh = o & 31;
                uint32_t idx;
                if (j == 21) idx = w4[3] >> 30;
                else if (sh <= 26) idx = (w4[wi] >> sh) & 63u;
                else idx = __builtin_amdgcn_alignbit(w4[wi + 1], w4[wi], sh) & 63u;
                const uint32_t e = (uint32_t)j * 64u + idx;
                const sc_f32x2 v = lp[e];
                if (j & 1) a1 += v; else a0 += v;
                if (NM == 3) { if (j & 1) c1 += lp3[e]; else c0 += lp3[e]; }
            }
        }
    }
    const sc_f32x2 a = a0 + a1;
    acc[0] = (double)a.x;
    acc[1] = (double)a.y;
    if (NM == 3) acc[2] = (double)(c0 + c1);
}

// Both forms in one row, for rows whose table does not fit the LDS: the first c_lut chunks through the nibble table, the
// others per sample.  (Splitting a row that does fit in halves, to keep the LDS pipe and the f64 VALU busy at the same
// time, did not pay: 16 M x 1024 with a fifth of the rows passing took 0.66 ms against 0.63 ms with the whole row in
// the table and 0.75 ms per sample, r02.  8 M x 2048, where half the row fits: 0.67 ms against 0.95 ms per sample.)
template <int NM, bool HALF = false>
__device__ __forceinline__ void row_moments_mixed(const u32x4 *__restrict__ rp, int cpr, int c_lut, const double *lut, cdptr tab,
                                                  double *acc)
{
    double a[NM], b[NM];
    row_moments_lut<NM, HALF>(rp, c_lut, lut, a);
#pragma unroll
    for (int m = 0; m < NM; m++) b[m] = 0.0;
    if (c_lut < cpr) row_moments<NM, HALF>(rp + c_lut, cpr - c_lut, tab + (size_t)c_lut * 128 * NM, b);   // (half: c_lut is 0 or 1 = cpr)
#pragma unroll
    for (int m = 0; m < NM; m++) acc[m] = a[m] + b[m];
}

// the workgroup's copy of the nibble table: global -> LDS, 16 bytes per thread and step
__device__ __forceinline__ void load_lut(double *lds, const double *__restrict__ g, int n_doubles, int threads)
{
    const double2 *src = reinterpret_cast<const double2 *>(g);
    double2 *dst = reinterpret_cast<double2 *>(lds);
    for (int i = threadIdx.x; i < n_doubles / 2; i += threads) dst[i] = src[i];
    __syncthreads();
}

// appends the rows flagged in this step (one flag per lane group leader) to the wave's queue
__device__ __forceinline__ int queue_rows(bool flag, uint64_t row, int2 v, uint64_t *q_row, int2 *q_val, int q, int lane)
{
    const uint64_t todo = __ballot(flag);
    if (!todo) return q;
    if (flag) {
        const int pos = q + __popcll(todo & ((1ull << lane) - 1ull));
        q_row[pos] = row;
        q_val[pos] = v;
    }
    return __builtin_amdgcn_readfirstlane(q + __popcll(todo));  // keep the count in an SGPR
}

// drops the first 64 entries of the wave's queue (the rest moves down 64 places, 64 entries at a time)
__device__ __forceinline__ int queue_pop64(uint64_t *q_row, int2 *q_val, int q, int lane)
{
    const int rest = q - 64;
    for (int base = 0; base < rest; base += 64) {
        uint64_t r = 0;
        int2 n = make_int2(0, 0);
        const bool mv = base + lane < rest;
        if (mv) { r = q_row[64 + base + lane]; n = q_val[64 + base + lane]; }
        __builtin_amdgcn_wave_barrier();
        if (mv) { q_row[base + lane] = r; q_val[base + lane] = n; }
        __builtin_amdgcn_wave_barrier();
    }
    return __builtin_amdgcn_readfirstlane(rest > 0 ? rest : 0);
}

// ---- the row stream --------------------------------------------------------------------------------------------------
// What both scan kernels do with the matrix: every lane group streams its rows (UNR steps of loads in flight), popcounts
// them against N masks and reduces over the group; the kernel says what becomes of a row's counts (`on_row`) and of 64
// queued rows (`process`; NoQueue: nothing is queued).
template <int N>
struct RowMasks {
    uint64_t a[N], b[N];      // this lane's two words of each mask (zero where the lane has no chunk of the row)
    const uint64_t *all[N];   // the whole masks, for the chunks beyond the group's lanes (rows wider than 64 chunks)
};
struct RowQueue {
    uint64_t *row;
    int2 *val;
    int n;   // queued rows (wave-uniform)
};
struct NoQueue {};
template <int G, bool LUT> constexpr int sc_threads() { return LUT ? SC_LUT_THREADS : SC_THREADS; }
template <int G, bool LUT> constexpr int sc_unroll() { return LUT ? lut_unroll(G) : SC_UNROLL; }

template <int G, bool LUT, int N, class Row, class Process>
__device__ __forceinline__ void stream_rows(const ScanArgs &P, const RowMasks<N> &mk, RowQueue &Q, Row on_row, Process process)
{
    constexpr bool QUEUED = !std::is_same<Process, NoQueue>::value;
    constexpr bool HALF = G == 0;          // 8-byte rows, two per load
    constexpr int GL = sc_lanes(G), NSUB = HALF ? 2 : 1;
    constexpr int THREADS = sc_threads<G, LUT>(), UNR = sc_unroll<G, LUT>();
    constexpr int RPW = sc_rpw(G);  // rows per wave step
    const int lane = threadIdx.x & 63;
    const int g = lane & (GL - 1);
    const int rsub = HALF ? 2 * lane : lane / GL;
    const uint64_t n_steps = (P.M + RPW - 1) / RPW;
    const uint64_t wave_global = (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    const uint64_t total_waves = (uint64_t)gridDim.x * (THREADS / 64);
    const bool has_chunk = g < P.cpr;
    // one copy of process(): the queue is drained after each unrolled batch and, once the rows run out,
    // down to empty (keeps its registers and code out of the streaming part)
    for (uint64_t s0 = wave_global * UNR;; s0 += total_waves * UNR) {
        const bool more = s0 < n_steps;
        if constexpr (QUEUED) {
            while (Q.n >= 64 || (!more && Q.n > 0)) {
                process(Q.n < 64 ? Q.n : 64);
                Q.n = queue_pop64(Q.row, Q.val, Q.n, lane);
            }
        }
        if (!more) break;
        u32x4 x[UNR];
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const uint64_t row = (s0 + u) * RPW + rsub;
            x[u] = (u32x4)(0u);
            if (HALF) {   // rows `row` and `row + 1` in one 16-byte load (the matrix starts 16-byte aligned and `row` is even)
                const u32x4 *pp = reinterpret_cast<const u32x4 *>(reinterpret_cast<const uint2 *>(P.bits) + row);
                if (row + 1 < P.M) x[u] = __builtin_nontemporal_load(pp);
                else if (row < P.M) { const uint2 v = *reinterpret_cast<const uint2 *>(pp); x[u].x = v.x; x[u].y = v.y; }   // the odd last row
            } else if (row < P.M && has_chunk) {
#if PSK_SC_NT
                if (LUT && !PSK_LUT_NT) x[u] = P.bits[row * (uint64_t)P.cpr + g];
                else x[u] = __builtin_nontemporal_load(&P.bits[row * (uint64_t)P.cpr + g]);
#else
                x[u] = P.bits[row * (uint64_t)P.cpr + g];
#endif
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
          for (int sub = 0; sub < NSUB; sub++) {
            const uint64_t row = (s0 + u) * RPW + rsub + sub;
            const uint64_t xa = sub ? (((uint64_t)x[u].w << 32) | x[u].z) : (((uint64_t)x[u].y << 32) | x[u].x);
            const uint64_t xb = HALF ? 0ull : (((uint64_t)x[u].w << 32) | x[u].z);
            uint32_t cnt[N];
#pragma unroll
            for (int i = 0; i < N; i++) cnt[i] = __popcll(xa & mk.a[i]) + (HALF ? 0u : (uint32_t)__popcll(xb & mk.b[i]));
            if (!HALF && P.cpr > GL) {  // rows wider than 64 chunks (more than 8192 samples)
                if (row < P.M)
                    for (int ch = g + GL; ch < P.cpr; ch += GL) {
                        const u32x4 y = P.bits[row * (uint64_t)P.cpr + ch];
                        const uint64_t ya = ((uint64_t)y.y << 32) | y.x, yb = ((uint64_t)y.w << 32) | y.z;
#pragma unroll
                        for (int i = 0; i < N; i++) cnt[i] += __popcll(ya & mk.all[i][2 * ch]) + __popcll(yb & mk.all[i][2 * ch + 1]);
                    }
            }
#pragma unroll
            for (int d = GL / 2; d > 0; d >>= 1) {
#pragma unroll
                for (int i = 0; i < N; i++) cnt[i] += __shfl_xor(cnt[i], d, 64);
            }
            on_row(row, cnt, g == 0);
        }
    }
}

// the second passes (chi2w_finalize_kernel, ttest_finalize_kernel): one workgroup per result segment
constexpr int SC_FIN_THREADS = 1024;
constexpr int SC_FIN_BLK = 16;         // chunks (of 128 samples) of the weight table staged in LDS at a time: 32 KB

// The run-time G as a compile-time constant: f(std::integral_constant<int, G>).  G is 0 or a power of two up to 64; the
// forms that keep a table in LDS exist up to MAX_G = 16 lanes per row (lut_chunks), the plain ones up to 64.
template <int MAX_G, class F>
void dispatch_G(int G, F &&f)
{
    switch (G) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, (MAX_G < 32 ? MAX_G : 32)>()); break;
    default: f(std::integral_constant<int, MAX_G>()); break;
    }
}

// The event pair of a timed launch; either may be null.  The events ride on the kernel's own dispatch: nothing is queued
// before or after the kernel for them, hipEventSynchronize(stop) waits for the kernel, and hipEventElapsedTime(start, stop)
// is the dispatch's start to its end.  A scan of several kernels puts start on the first and stop on the last.  TimedBy{}:
// no events at all -- the dispatch carries no completion signal, and whoever launched it learns of its end and its time
// from the kernel's stamps (the unweighted chi2 scans of psk_chi2_scan_begin; psk_scan_end, chi2_driver.hip).
struct TimedBy {
    hipEvent_t start = nullptr, stop = nullptr;
    TimedBy first() const { return {start, nullptr}; }
    TimedBy last() const { return {nullptr, stop}; }
};

// The one way a scan kernel is launched: on `st`, timed by `ev` or, with both events null, by nothing (r19: a plain
// hipLaunchKernelGGL in that case cost the host the same, 7.1-7.4 us per step of the native ring either way, so there
// is one call); lds > 0: the kernel keeps `lds` bytes of tables in dynamic LDS (beyond the 64 KB a kernel gets unasked).
template <class... KA, class... A>
void launch_timed(void (*kern)(KA...), dim3 grid, int threads, size_t lds, hipStream_t st, TimedBy ev, const A &...args)
{
    if (lds) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipExtLaunchKernelGGL(kern, grid, dim3(threads), (uint32_t)lds, st, ev.start, ev.stop, 0, KA(args)...);
}
