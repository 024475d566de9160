// One chi2 scan as the host launches it: the arguments of the exception-coded kernels, the launch that chi2_driver.hip fills
// from the plan (chi2_plan.h), and the one function through which another unit reaches the kernels.  The kernels
// themselves are instantiated only in assoc_scan.hip.
#pragma once
#include "scan_common.h"

struct CxScanArgs {
    ScanArgs s;                  // the scan: unit weights, masks inline
    const u32x4 *slots;          // two slots per 16 bytes
    const u32x4 *ov;             // overflow rows, dense, cpr chunks each, ascending
    const uint32_t *ov_row;      // ... their row ids
    uint64_t n_ov;
    uint32_t slot_blocks;        // workgroups [0, slot_blocks) stream the slots (none when no class is feasible),
    uint32_t ov_blocks;          // the next ov_blocks the overflow rows; any beyond only publish their segment
    uint32_t class_mask;         // bit (header & 15): some reachable table of that e and base is a candidate (cx_plan)
    uint64_t corner[2];          // [base] bit a' * 8 + c': the table (a', c') / (n1 - a', n0 - c') is a candidate
};

struct CxSideArgs {
    const u32x4 *ov;
    const uint32_t *ov_row;
    uint64_t n_ov;
    uint64_t m1[4], m0[4];       // the mask words of the row's (at most two) chunks
    ScanCuts cut;
    ScanSink sink;
};
static_assert(sizeof(CxSideArgs) <= 256, "chi2_scan_kernel_cx_side's arguments are meant to stay small");

struct CxSidePcArgs {
    CxSideArgs s;
    const uint16_t *ov_pc;       // popcount of every side-matrix row over the valid samples
    uint64_t feas[4];            // bit pc: a row of that popcount can be a candidate
};
static_assert(sizeof(CxSidePcArgs) <= 256, "chi2_scan_kernel_cx_side_pc's arguments are meant to stay small");

struct CxSideIdxArgs {
    CxSideArgs s;
    const uint32_t *idx;         // positions of the side-matrix rows, grouped by popcount (cx_pc_index)
    uint32_t run_begin[CX_IDX_RUNS], run_len[CX_IDX_RUNS];   // the ranges of idx that hold the feasible rows (cx_idx_runs); unused: len 0
};
static_assert(sizeof(CxSideIdxArgs) <= 256, "chi2_scan_kernel_cx_side_idx's arguments are meant to stay small");

struct Chi2Launch {
    CxScanArgs x;        // x.s: every form's arguments; the rest: chi2_scan_kernel_cx's (CxMixed)
    CxSidePcArgs side;   // side.s: chi2_scan_kernel_cx_side's (CxSide); all of it: ..._side_pc's (CxSidePc)
    CxSideIdxArgs sidx;  // chi2_scan_kernel_cx_side_idx's (CxSideIdx)
    Chi2Form form = Chi2Form::Dense;
    int mode = 0;        // of the dense kernels (pick_chi2_mode)
    int cpr = 0;
    dim3 grid;
};

void launch_chi2_any(psk_ctx *ctx, const Chi2Launch &L, TimedBy ev);   // assoc_scan.hip: on ctx->stream, timed by ev
