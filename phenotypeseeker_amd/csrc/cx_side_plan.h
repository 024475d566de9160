// The launch shape of chi2_scan_kernel_cx_side (assoc_scan.hip) as plain arithmetic: nothing here touches the device, so
// it can be read, compiled and checked on its own (psk_cx_side_shape; tests/test_cx_side_shape_host.py).
//
// The sweep: a row of the side matrix is cpr 16-byte chunks, one lane each, so a wave step covers 64 / cpr rows and a
// batch -- what a wave loads before it evaluates -- CX_SIDE_UNROLL steps.  Wave w of the launch's W waves takes the
// batches w, w + W, w + 2 W, ... (grid-stride), and W = blocks * CX_SIDE_WAVES: every workgroup of the launch sweeps.
#pragma once
#include <cstdint>

#ifndef PSK_CX_SIDE_UNROLL
#define PSK_CX_SIDE_UNROLL 2
#endif
constexpr int CX_SIDE_UNROLL = PSK_CX_SIDE_UNROLL;   // 16-byte loads in flight per lane and register set
constexpr int CX_SIDE_WAVES = 4;                     // waves per workgroup (SC_THREADS / 64)
constexpr int CX_SIDE_NSEG = 256;                    // SC_NSEG: every result segment needs a workgroup to publish its count

struct cx_side_shape_t {
    uint32_t blocks;          // workgroups of the launch
    uint64_t rows_per_block;  // the most rows one of them visits
    uint32_t batch_rows;      // rows of one wave batch
};

// cap_blocks: the most workgroups the launch may have (CUs x the grid multiple).  blocks = what one batch per wave would
// need, capped, and never below CX_SIDE_NSEG; rows_per_block bounds the rows of the waves' batches, full or not.
inline cx_side_shape_t cx_side_shape(uint64_t n_ov, int cpr, uint64_t cap_blocks)
{
    const uint64_t rpw = 64 / (uint64_t)cpr;
    const uint64_t steps = (n_ov + rpw - 1) / rpw;
    const uint64_t batches = (steps + CX_SIDE_UNROLL - 1) / CX_SIDE_UNROLL;
    uint64_t blocks = (batches + CX_SIDE_WAVES - 1) / CX_SIDE_WAVES;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < CX_SIDE_NSEG) blocks = CX_SIDE_NSEG;
    const uint64_t waves = blocks * CX_SIDE_WAVES;
    const uint64_t passes = (batches + waves - 1) / waves;   // batches of wave 0, the most any wave takes
    cx_side_shape_t s;
    s.blocks = (uint32_t)blocks;
    s.batch_rows = (uint32_t)(CX_SIDE_UNROLL * rpw);
    s.rows_per_block = passes * CX_SIDE_WAVES * s.batch_rows;
    return s;
}

// ---- the popcount-filtered sweep (chi2_scan_kernel_cx_side_pc) -----------------------------------------------------
// A row is one lane: a wave step covers 64 rows and a batch CX_PC_UNROLL steps -- the 2-byte popcounts a wave loads
// before it looks at any row.  Batches are dealt to the waves grid-stride exactly as above.
#ifndef PSK_CX_PC_UNROLL
#define PSK_CX_PC_UNROLL 8
#endif
constexpr int CX_PC_UNROLL = PSK_CX_PC_UNROLL;       // 2-byte loads in flight per lane and register set
static_assert(CX_PC_UNROLL == 4 || CX_PC_UNROLL == 8, "a batch is 256 or 512 rows");

inline cx_side_shape_t cx_pc_shape(uint64_t n_ov, uint64_t cap_blocks)
{
    const uint64_t batch_rows = 64 * (uint64_t)CX_PC_UNROLL;
    const uint64_t batches = (n_ov + batch_rows - 1) / batch_rows;
    uint64_t blocks = (batches + CX_SIDE_WAVES - 1) / CX_SIDE_WAVES;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < CX_SIDE_NSEG) blocks = CX_SIDE_NSEG;
    const uint64_t waves = blocks * CX_SIDE_WAVES;
    const uint64_t passes = (batches + waves - 1) / waves;   // batches of wave 0, the most any wave takes
    cx_side_shape_t s;
    s.blocks = (uint32_t)blocks;
    s.batch_rows = (uint32_t)batch_rows;
    s.rows_per_block = passes * CX_SIDE_WAVES * batch_rows;
    return s;
}
